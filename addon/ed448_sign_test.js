// Ed448 signing and verification from messages through the shim: the reference's own answers and messages
// (tests/golden/ed448_sign_kat.json).  Run by tests/test_gpu_ed448_sign_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'ed448_sign_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => (b === null ? null : Buffer.from(b).toString('hex'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
let count = 0;

// getPublicKey: the whole fixture as one batch, a few rows through the single-item form
const pubs = gpu.ed448GetPublicKeyBatch(kat.keys.map((k) => bin(k.secretKey)));
kat.keys.forEach((k, i) => { assert.strictEqual(hex(pubs[i]), k.publicKey); count++; });
kat.keys.slice(0, 3).forEach((k) => assert.strictEqual(hex(gpu.ed448GetPublicKey(bin(k.secretKey))), k.publicKey));
const pubOf = new Map(kat.keys.map((k) => [k.secretKey, bin(k.publicKey)]));

// sign: the rows grouped by what a call shares (variant and context), each group as one batch with per-row keys; the signatures then
// verify with the challenge hashed on the host and on the device, and a changed message does not
const optsOf = (c) => ({ prehash: c.variant === 'ed448ph', context: bin(c.context) });
const groups = new Map();
kat.sign.forEach((c) => {
  const key = c.variant + '/' + c.context;
  if (!groups.has(key)) groups.set(key, []);
  groups.get(key).push(c);
});
assert.ok(groups.size >= 6);
for (const rows of groups.values()) {
  const opts = optsOf(rows[0]);
  const got = gpu.ed448SignBatch(rows.map((c) => ({ msg: bin(c.msg), secretKey: bin(c.secretKey) })), opts);
  assert.strictEqual(got.length, rows.length);
  rows.forEach((c, i) => { assert.strictEqual(hex(got[i]), c.sig, c.variant + ' ' + c.msg.length / 2); count++; });
  assert.strictEqual(hex(gpu.ed448Sign(bin(rows[0].msg), bin(rows[0].secretKey), opts)), rows[0].sig);
  const items = rows.map((c, i) => ({ sig: got[i], msg: bin(c.msg), publicKey: pubOf.get(c.secretKey) }));
  items.push({ sig: got[0], msg: Uint8Array.from([...bin(rows[0].msg), 1]), publicKey: pubOf.get(rows[0].secretKey) });
  const want = rows.map(() => true).concat([false]);
  assert.deepStrictEqual(gpu.ed448VerifyBatch(items, opts), want);
  assert.deepStrictEqual(gpu.ed448VerifyBatch(items, Object.assign({ deviceHash: true }, opts)), want);
}
// one key signing many messages equals the same key per row
const plain = kat.sign.filter((c) => c.variant === 'ed448' && c.context === '');
const sk = bin(plain[0].secretKey), msgs = plain.map((c) => bin(c.msg));
const shared = gpu.ed448SignBatch({ msgs, secretKey: sk }, { oneKey: true });
const perRow = gpu.ed448SignBatch(msgs.map((msg) => ({ msg, secretKey: sk })));
assert.strictEqual(shared.length, perRow.length);
assert.deepStrictEqual(shared.map(hex), perRow.map(hex));
assert.strictEqual(hex(shared[0]), plain[0].sig);
// the thrown messages
const E = kat.errors, m = new Uint8Array(3), good = new Uint8Array(57);
assert.strictEqual(message(() => gpu.ed448GetPublicKey(new Uint8Array(56))), E.secret_key_length_56);
assert.strictEqual(message(() => gpu.ed448Sign(m, new Uint8Array(58))), E.secret_key_length_58);
assert.strictEqual(message(() => gpu.ed448Sign(m, new Uint8Array(114), { context: m, prehash: true })), E.secret_key_length_114);
assert.strictEqual(message(() => gpu.ed448GetPublicKeyBatch([good, new Uint8Array(56)])), E.secret_key_length_56);
assert.strictEqual(message(() => gpu.ed448Sign(m, good, { context: new Uint8Array(256) })), E.context_256);
assert.strictEqual(message(() => gpu.ed448Sign(m, good, { context: new Uint8Array(256), prehash: true })), E.context_256_ph);
assert.strictEqual(message(() => gpu.ed448SignBatch({ msgs: [m], secretKey: new Uint8Array(56) })), E.secret_key_length_56);
assert.strictEqual(message(() => gpu.ed448Sign(m, good, { context: new Uint8Array(255) })), E.context_255);
assert.deepStrictEqual(gpu.ed448GetPublicKeyBatch([]), []);
assert.deepStrictEqual(gpu.ed448SignBatch([]), []);
console.log('ed448 sign OK: ' + count + ' rows');
