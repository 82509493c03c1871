// X448 and Ed448 verification through the shim: the reference's own answers and messages (tests/golden/ed448_kat.json).
// Run by tests/test_gpu_ed448_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'ed448_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => (b === null ? null : Buffer.from(b).toString('hex'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
let count = 0;

// scalarMult: the whole fixture as one batch
const rows = kat.scalar_mult;
const got = gpu.x448ScalarMultBatch(rows.map((c) => ({ scalar: bin(c.scalar), u: bin(c.u) })));
rows.forEach((c, i) => { assert.strictEqual(hex(got[i]), c.out, c.name); count++; });
assert.ok(got.some((r) => r === null) && got.some((r) => r !== null));
// one secret against many peer keys
const alice = bin(kat.public_keys[0].scalar);
const peers = rows.slice(2, 40);
const shared = gpu.x448ScalarMultBatch({ scalar: alice, us: peers.map((c) => bin(c.u)) });
const perRow = gpu.x448ScalarMultBatch(peers.map((c) => ({ scalar: alice, u: bin(c.u) })));
assert.deepStrictEqual(shared.map(hex), perRow.map(hex));
assert.ok(shared.some((r) => r === null) && shared.some((r) => r !== null));
// getPublicKey
const pubs = gpu.x448GetPublicKeyBatch(kat.public_keys.map((c) => bin(c.scalar)));
kat.public_keys.forEach((c, i) => { assert.strictEqual(hex(pubs[i]), c.out); count++; });
// verify: the reference's verdicts, grouped by (prehash, context)
const groups = new Map();
kat.verify.forEach((c) => {
  const base = kat.signatures[c.row];
  const key = (c.ph ? '1' : '0') + (c.context || '');
  if (!groups.has(key)) groups.set(key, { ph: c.ph, context: c.context, items: [], want: [] });
  const g = groups.get(key);
  g.items.push({ sig: bin(base.sig), msg: bin(c.msg === null ? base.msg : c.msg), publicKey: bin(base.publicKey) });
  g.want.push(c.ok);
});
let accepted = 0, refused = 0;
for (const g of groups.values()) {
  const opts = { prehash: g.ph };
  if (g.context !== null) opts.context = bin(g.context);
  const v = gpu.ed448VerifyBatch(g.items, opts);
  assert.deepStrictEqual(v, g.want);
  v.forEach((x) => { if (x) accepted++; else refused++; count++; });
}
assert.ok(accepted > 20 && refused > 10);
// a flipped bit of s, and of the key
const s0 = kat.signatures[0], sig = bin(s0.sig), pk = bin(s0.publicKey), msg = bin(s0.msg);
const badSig = Uint8Array.from(sig); badSig[60] ^= 1;
const badPk = Uint8Array.from(pk); badPk[5] ^= 1;
assert.deepStrictEqual(gpu.ed448VerifyBatch([{ sig, msg, publicKey: pk }, { sig: badSig, msg, publicKey: pk }, { sig, msg, publicKey: badPk }]),
  [true, false, false]);
// argument errors, in the reference's order
const E = kat.errors, good = new Uint8Array(56).fill(1), five = new Uint8Array(56); five[0] = 5;
const one = (scalar, u) => gpu.x448ScalarMultBatch([{ scalar, u }]);
assert.strictEqual(message(() => one(good, new Uint8Array(55))), E.u_length);
assert.strictEqual(message(() => one(good, 'x')), E.u_type);
assert.strictEqual(message(() => one(new Uint8Array(57), five)), E.scalar_length);
assert.strictEqual(message(() => one(new Uint8Array(57), new Uint8Array(55))), E.both_bad);
assert.strictEqual(message(() => gpu.x448GetPublicKeyBatch([new Uint8Array(55)])), E.public_key_length);
assert.strictEqual(message(() => gpu.ed448VerifyBatch([{ sig: new Uint8Array(113), msg, publicKey: pk }])), E.signature_length);
assert.strictEqual(message(() => gpu.ed448VerifyBatch([{ sig, msg, publicKey: new Uint8Array(56) }])), E.verify_public_key_length);
assert.strictEqual(message(() => gpu.ed448VerifyBatch([{ sig, msg: 'x', publicKey: pk }])), E.message_type);
assert.strictEqual(message(() => gpu.ed448VerifyBatch([{ sig, msg, publicKey: pk }], { context: new Uint8Array(256) })), E.context_too_long);
// ... but only a row that got past decoding, s < n and the small-order test looks at the context (edwards.ts:964-984)
const notOnCurve = Uint8Array.from(pk); notOnCurve.fill(0xff, 0, 56); notOnCurve[56] = 0;
assert.deepStrictEqual(gpu.ed448VerifyBatch([{ sig, msg, publicKey: notOnCurve }, { sig, msg, publicKey: bin(kat.torsion[2]) }],
  { context: new Uint8Array(256) }), [false, false]);
assert.deepStrictEqual(gpu.x448ScalarMultBatch([]), []);
assert.deepStrictEqual(gpu.x448GetPublicKeyBatch([]), []);
assert.deepStrictEqual(gpu.ed448VerifyBatch([]), []);
console.log('ed448 OK: ' + count + ' rows');
