// Ed25519 signing through the shim: the reference's own answers and messages (tests/golden/ed25519_sign_kat.json).
// Run by tests/test_gpu_ed25519_sign_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'ed25519_sign_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => (b === null ? null : Buffer.from(b).toString('hex'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
let count = 0;

// getPublicKey: the whole fixture as one batch, a few rows through the single-item form
const pubs = gpu.ed25519GetPublicKeyBatch(kat.keys.map((k) => bin(k.secretKey)));
kat.keys.forEach((k, i) => { assert.strictEqual(hex(pubs[i]), k.publicKey); count++; });
kat.keys.slice(0, 3).forEach((k) => assert.strictEqual(hex(gpu.ed25519GetPublicKey(bin(k.secretKey))), k.publicKey));

// sign: the rows grouped by what a call shares (variant and context), each group as one batch with per-row keys
const optsOf = (c) => Object.assign(c.variant === 'ed25519ph' ? { prehash: true } : {},
                                    c.variant !== 'ed25519' && (c.context !== null || c.variant === 'ed25519ctx') ? { context: bin(c.context || '') } : {});
const groups = new Map();
kat.sign.forEach((c) => {
  const key = c.variant + '/' + c.context;
  if (!groups.has(key)) groups.set(key, []);
  groups.get(key).push(c);
});
assert.ok(groups.size >= 7);
for (const rows of groups.values()) {
  const got = gpu.ed25519SignBatch(rows.map((c) => ({ msg: bin(c.msg), secretKey: bin(c.secretKey) })), optsOf(rows[0]));
  assert.strictEqual(got.length, rows.length);
  rows.forEach((c, i) => { assert.strictEqual(hex(got[i]), c.sig, c.variant + ' ' + c.msg.length / 2); count++; });
  assert.strictEqual(hex(gpu.ed25519Sign(bin(rows[0].msg), bin(rows[0].secretKey), optsOf(rows[0]))), rows[0].sig);
}
// one key signing many messages equals the same key per row; plain signatures verify through the batch verifier
const plain = kat.sign.filter((c) => c.variant === 'ed25519');
const sk = bin(plain[0].secretKey), msgs = plain.map((c) => bin(c.msg));
const shared = gpu.ed25519SignBatch({ msgs, secretKey: sk });
const perRow = gpu.ed25519SignBatch(msgs.map((msg) => ({ msg, secretKey: sk })));
assert.strictEqual(shared.length, perRow.length);
assert.deepStrictEqual(shared.map(hex), perRow.map(hex));
assert.strictEqual(hex(shared[0]), plain[0].sig);
const pk = gpu.ed25519GetPublicKey(sk);
const verdicts = gpu.ed25519VerifyBatch(msgs.map((msg, i) => ({ sig: shared[i], msg, publicKey: pk })), false);
assert.strictEqual(verdicts.length, msgs.length);
assert.ok(verdicts.every((v) => v === true));
// the thrown messages
const E = kat.errors, m = new Uint8Array(3), good = new Uint8Array(32);
assert.strictEqual(message(() => gpu.ed25519GetPublicKey(new Uint8Array(31))), E.secret_key_length_31);
assert.strictEqual(message(() => gpu.ed25519Sign(m, new Uint8Array(33))), E.secret_key_length_33);
assert.strictEqual(message(() => gpu.ed25519Sign(m, new Uint8Array(64), { context: m })), E.secret_key_length_64);
assert.strictEqual(message(() => gpu.ed25519GetPublicKeyBatch([good, new Uint8Array(31)])), E.secret_key_length_31);
assert.strictEqual(message(() => gpu.ed25519Sign(m, good, { context: new Uint8Array(256) })), E.context_256);
assert.strictEqual(message(() => gpu.ed25519Sign(m, good, { context: new Uint8Array(256), prehash: true })), E.context_256_ph);
assert.strictEqual(message(() => gpu.ed25519SignBatch({ msgs: [m], secretKey: new Uint8Array(31) })), E.secret_key_length_31);
assert.deepStrictEqual(gpu.ed25519GetPublicKeyBatch([]), []);
assert.deepStrictEqual(gpu.ed25519SignBatch([]), []);
console.log('ed25519 sign OK: ' + count + ' rows');
