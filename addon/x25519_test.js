// X25519 and ed25519.utils.toMontgomery through the shim: the reference's own answers and messages (tests/golden/x25519_kat.json).
// Run by tests/test_gpu_x25519_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'x25519_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => (b === null ? null : Buffer.from(b).toString('hex'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
let count = 0;

// scalarMult: the whole fixture as one batch, then every refused row and a few accepted ones through the single-item helper
const rows = kat.scalar_mult;
const got = gpu.x25519ScalarMultBatch(rows.map((c) => ({ scalar: bin(c.scalar), u: bin(c.u) })));
rows.forEach((c, i) => { assert.strictEqual(hex(got[i]), c.out, c.name); count++; });
rows.forEach((c, i) => {
  if (c.out === null) assert.strictEqual(message(() => gpu.x25519ScalarMult(bin(c.scalar), bin(c.u))), c.error, c.name);
  else if (i < 8) assert.strictEqual(hex(gpu.x25519ScalarMult(bin(c.scalar), bin(c.u))), c.out, c.name);
});
// one secret against many peer keys
const alice = bin(kat.public_keys[0].scalar);
const peers = rows.slice(4, 60);
const shared = gpu.x25519ScalarMultBatch({ scalar: alice, us: peers.map((c) => bin(c.u)) });
const perRow = gpu.x25519ScalarMultBatch(peers.map((c) => ({ scalar: alice, u: bin(c.u) })));
assert.deepStrictEqual(shared.map(hex), perRow.map(hex));
assert.ok(shared.some((r) => r === null) && shared.some((r) => r !== null));
// the RFC 7748 chain, 100 steps
let k = bin(kat.scalar_mult[0].scalar).fill(0); k[0] = 9;
for (let i = 1, u = k; i <= 100; i++) [k, u] = [gpu.x25519ScalarMult(k, u), k];
assert.strictEqual(hex(k), kat.iterated['100']);
// getPublicKey
const pubs = gpu.x25519GetPublicKeyBatch(kat.public_keys.map((c) => bin(c.scalar)));
kat.public_keys.forEach((c, i) => { assert.strictEqual(hex(pubs[i]), c.out); count++; });
assert.strictEqual(hex(gpu.x25519GetPublicKey(alice)), kat.public_keys[0].out);
// toMontgomery, messages included
const mont = gpu.ed25519ToMontgomeryBatch(kat.to_montgomery.map((c) => bin(c.publicKey)));
kat.to_montgomery.forEach((c, i) => {
  assert.strictEqual(hex(mont[i]), c.out, c.name);
  if (c.out === null) assert.strictEqual(message(() => gpu.ed25519ToMontgomery(bin(c.publicKey))), c.error, c.name);
  count++;
});
assert.strictEqual(hex(gpu.ed25519ToMontgomery(bin(kat.to_montgomery[0].publicKey))), kat.to_montgomery[0].out);
// argument errors, in the reference's order
const E = kat.errors, good = new Uint8Array(32).fill(1), nine = new Uint8Array(32); nine[0] = 9;
assert.strictEqual(message(() => gpu.x25519ScalarMult(good, new Uint8Array(31))), E.u_length);
assert.strictEqual(message(() => gpu.x25519ScalarMult(good, 'x')), E.u_type);
assert.strictEqual(message(() => gpu.x25519ScalarMult(new Uint8Array(33), nine)), E.scalar_length);
assert.strictEqual(message(() => gpu.x25519ScalarMult(new Uint8Array(33), new Uint8Array(31))), E.both_bad);
assert.strictEqual(message(() => gpu.x25519ScalarMult(new Uint8Array(33), new Uint8Array(32))), E.low_order_before_scalar);
assert.strictEqual(message(() => gpu.x25519GetPublicKey(new Uint8Array(31))), E.public_key_length);
assert.strictEqual(message(() => gpu.x25519ScalarMultBatch([{ scalar: new Uint8Array(33), u: new Uint8Array(31) }])), E.both_bad);
assert.deepStrictEqual(gpu.x25519ScalarMultBatch([]), []);
assert.deepStrictEqual(gpu.x25519GetPublicKeyBatch([]), []);
assert.deepStrictEqual(gpu.ed25519ToMontgomeryBatch([]), []);
console.log('x25519 OK: ' + count + ' rows');
