// bls12-381 pairings through the shim: pairingBatch against the reference's pairing vectors and products, blsVerifyBatch against
// its verify booleans (tests/golden/bls12_381_pairing_kat.json, the inputs rebuilt by tests/pairing_helpers.py into the file named
// by argv[2]).  Run by tests/test_gpu_pairing_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'bls12_381_pairing_kat.json')));
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
// Fp12.toBytes of the reference: the 12 coefficients in tower order, 48 bytes big-endian each
const toBytes = (f) => Buffer.concat([f.c0, f.c1].flatMap((six) => [six.c0, six.c1, six.c2]).flatMap((two) => [two.c0, two.c1])
  .map((c) => Buffer.from(c.toString(16).padStart(96, '0'), 'hex')));
let count = 0;

const vec = inp.vectors.map(([a, b]) => ({ g1: bin(a), g2: bin(b) }));
gpu.pairingBatch(vec, vec.map(() => 1)).forEach((f, i) => { assert.strictEqual(toBytes(f).toString('base64'), kat.vectors[i], 'vector ' + i); count++; });
assert.strictEqual(toBytes(gpu.pairingBatch(vec.slice(0, 1))).toString('base64'), kat.vectors[0]);
assert.ok(Object.isFrozen(gpu.pairingBatch(vec.slice(0, 1)).c0.c1) && typeof gpu.pairingBatch(vec.slice(0, 1)).c1.c2.c1 === 'bigint');
inp.batch.forEach((rows, j) => {
  const f = gpu.pairingBatch(rows.map(([a, b]) => ({ g1: bin(a), g2: bin(b) })));
  assert.strictEqual(toBytes(f).toString('base64'), kat.batch[j], 'batch ' + j);
  count++;
});
const sizes = inp.batch.map((r) => r.length);
const all = [].concat(...inp.batch).map(([a, b]) => ({ g1: bin(a), g2: bin(b) }));
gpu.pairingBatch(all, sizes).forEach((f, j) => assert.strictEqual(toBytes(f).toString('base64'), kat.batch[j]));
assert.deepStrictEqual(gpu.pairingBatch([], []), []);
assert.strictEqual(message(() => gpu.pairingBatch([{ g1: new Uint8Array(96), g2: vec[0].g2 }])), 'pairing is not available for ZERO point');
const off = Uint8Array.from(vec[0].g1); off[48] ^= 1;
assert.strictEqual(message(() => gpu.pairingBatch([{ g1: off, g2: vec[0].g2 }])), 'bad point: equation left != right');
assert.strictEqual(message(() => gpu.pairingBatch([{ g1: bin(inp.torsion_g1), g2: vec[0].g2 }], undefined, { checkSubgroup: true })),
  'bad point: not in prime-order subgroup');
assert.strictEqual(message(() => gpu.pairingBatch(vec, [3])), 'group sizes must be non-negative and sum to the number of pairs');
for (const name of ['long', 'short']) {
  const items = inp.verify[name].map(([s, m, k]) => ({ signature: bin(s), message: bin(m), publicKey: bin(k) }));
  assert.deepStrictEqual(gpu.blsVerifyBatch(items, { short: name === 'short' }), kat.verify[name], name);
  assert.deepStrictEqual(gpu.blsVerifyBatch(items.slice(0, 1).concat([{ signature: bin('00'), message: bin(''), publicKey: bin('00') }]), { short: name === 'short' }), [true, false]);
  count += items.length;
}
console.log('pairing OK', count);
