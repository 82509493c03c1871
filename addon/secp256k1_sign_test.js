// secp256k1 signing through the shim: the reference's own answers and messages (tests/golden/secp256k1_sign_kat.json).
// Run by tests/test_gpu_secp256k1_sign_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'secp256k1_sign_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => (b === null ? null : Buffer.from(b).toString('hex'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const be = (v) => bin(v.toString(16).padStart(64, '0'));
const N = BigInt('0xfffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141');
let count = 0;

// public keys: the whole fixture as one batch per form, a few rows through the single-item forms
const sks = kat.keys.map((k) => bin(k.secretKey));
const comp = gpu.secp256k1GetPublicKeyBatch(sks), unc = gpu.secp256k1GetPublicKeyBatch(sks, false), xo = gpu.schnorrGetPublicKeyBatch(sks);
kat.keys.forEach((k, i) => {
  assert.strictEqual(hex(comp[i]), k.compressed);
  assert.strictEqual(hex(unc[i]), k.uncompressed);
  assert.strictEqual(hex(xo[i]), k.xonly);
  count++;
});
kat.keys.slice(0, 3).forEach((k) => {
  assert.strictEqual(hex(gpu.secp256k1GetPublicKey(bin(k.secretKey))), k.compressed);
  assert.strictEqual(hex(gpu.schnorrGetPublicKey(bin(k.secretKey))), k.xonly);
});
const pubOf = new Map(kat.keys.map((k) => [k.secretKey, bin(k.compressed)]));

// ECDSA: the rows grouped by what a call shares (prehash, lowS), one batch per group and format; extra entropy rides per row
for (const prehash of [true, false]) {
  for (const lowS of [true, false]) {
    const rows = kat.ecdsa.filter((c) => c.prehash === prehash && c.lowS === lowS);
    assert.strictEqual(rows.length, 18);
    const items = rows.map((c) => Object.assign({ msg: bin(c.msg), secretKey: bin(c.secretKey) }, c.extraEntropy === null ? {} : { extraEntropy: bin(c.extraEntropy) }));
    const plain = rows.filter((c) => c.extraEntropy === null);
    for (const format of ['compact', 'recovered', 'der']) {
      // a group with extra entropy on some rows only would draw random bytes for the others: sign the two halves separately
      const withX = gpu.ecdsaSignBatch(items.filter((it) => it.extraEntropy), { prehash, lowS, format });
      const without = gpu.ecdsaSignBatch(items.filter((it) => !it.extraEntropy), { prehash, lowS, format });
      rows.filter((c) => c.extraEntropy !== null).forEach((c, i) => { assert.strictEqual(hex(withX[i]), c[format]); count++; });
      plain.forEach((c, i) => { assert.strictEqual(hex(without[i]), c[format]); count++; });
    }
    const c0 = plain[0];
    assert.strictEqual(hex(gpu.secp256k1Sign(bin(c0.msg), bin(c0.secretKey), { prehash, lowS })), c0.compact);
    if (prehash) {
      const sigs = gpu.ecdsaSignBatch(items.filter((it) => !it.extraEntropy), { prehash, lowS });
      const verdicts = gpu.ecdsaVerifyBatchMsgs(plain.map((c, i) => ({ sig: sigs[i], msg: bin(c.msg), publicKey: pubOf.get(c.secretKey) })), lowS);
      assert.ok(verdicts.length === plain.length && verdicts.every((v) => v === true));
    }
  }
}
// one key signing many messages equals the same key per row; random extra entropy changes every signature and still verifies
const msgs = kat.ecdsa.slice(0, 9).map((c) => bin(c.msg)), sk = sks[5];
const shared = gpu.ecdsaSignBatch({ msgs, secretKey: sk });
assert.deepStrictEqual(shared.map(hex), gpu.ecdsaSignBatch(msgs.map((msg) => ({ msg, secretKey: sk }))).map(hex));
const fresh = gpu.ecdsaSignBatch({ msgs, secretKey: sk }, { extraEntropy: true });
assert.ok(fresh.every((s, i) => hex(s) !== hex(shared[i])));
assert.ok(gpu.ecdsaVerifyBatchMsgs(msgs.map((msg, i) => ({ sig: fresh[i], msg, publicKey: comp[5] })), true).every((v) => v === true));

// BIP-340
const sch = gpu.schnorrSignBatch(kat.schnorr.map((c) => ({ msg: bin(c.msg), secretKey: bin(c.secretKey), auxRand: bin(c.auxRand) })));
kat.schnorr.forEach((c, i) => { assert.strictEqual(hex(sch[i]), c.sig); count++; });
const s0 = kat.schnorr[0];
assert.strictEqual(hex(gpu.schnorrSign(bin(s0.msg), bin(s0.secretKey), bin(s0.auxRand))), s0.sig);
const a = gpu.schnorrSign(msgs[1], sk), b = gpu.schnorrSign(msgs[1], sk);          // fresh aux by default
assert.notStrictEqual(hex(a), hex(b));
assert.ok(gpu.schnorrVerifyBatch([a, b].map((sig) => ({ sig, msg: msgs[1], publicKey: xo[5] }))).every((v) => v === true));
// a refused key is a null row and leaves its neighbours alone
const mixed = gpu.ecdsaSignBatch([{ msg: msgs[0], secretKey: be(N) }, { msg: msgs[0], secretKey: sk }]);
assert.strictEqual(mixed[0], null);
assert.strictEqual(hex(mixed[1]), hex(shared[0]));

// the thrown messages
const E = kat.errors, m = new Uint8Array(32), good = be(BigInt(3)), max = be((BigInt(1) << BigInt(256)) - BigInt(1));
assert.strictEqual(message(() => gpu.secp256k1Sign(m, be(BigInt(0)))), E.ecdsa_secret_key_0);
assert.strictEqual(message(() => gpu.secp256k1Sign(m, be(N))), E.ecdsa_secret_key_n);
assert.strictEqual(message(() => gpu.secp256k1Sign(m, max)), E.ecdsa_secret_key_max);
assert.strictEqual(message(() => gpu.secp256k1Sign(m, new Uint8Array(31))), E.ecdsa_secret_key_length_31);
assert.strictEqual(message(() => gpu.secp256k1Sign(m, new Uint8Array(33))), E.ecdsa_secret_key_length_33);
assert.strictEqual(message(() => gpu.secp256k1Sign('abc', good)), E.ecdsa_message_not_bytes);
assert.strictEqual(message(() => gpu.secp256k1GetPublicKey(be(BigInt(0)))), E.public_key_secret_key_0);
assert.strictEqual(message(() => gpu.secp256k1GetPublicKey(be(N))), E.public_key_secret_key_n);
assert.strictEqual(message(() => gpu.secp256k1GetPublicKey(max)), E.public_key_secret_key_max);
assert.strictEqual(message(() => gpu.secp256k1GetPublicKey(new Uint8Array(31))), E.public_key_secret_key_length_31);
assert.strictEqual(message(() => gpu.secp256k1GetPublicKey(new Uint8Array(33))), E.public_key_secret_key_length_33);
assert.strictEqual(message(() => gpu.schnorrSign(m, be(BigInt(0)), m)), E.schnorr_secret_key_0);
assert.strictEqual(message(() => gpu.schnorrSign(m, be(N), m)), E.schnorr_secret_key_n);
assert.strictEqual(message(() => gpu.schnorrSign(m, max, m)), E.schnorr_secret_key_max);
assert.strictEqual(message(() => gpu.schnorrSign(m, new Uint8Array(31), m)), E.schnorr_secret_key_length_31);
assert.strictEqual(message(() => gpu.schnorrSign(m, new Uint8Array(33), m)), E.schnorr_secret_key_length_33);
assert.strictEqual(message(() => gpu.schnorrGetPublicKey(be(BigInt(0)))), E.schnorr_public_key_secret_key_0);
assert.strictEqual(message(() => gpu.schnorrGetPublicKey(new Uint8Array(31))), E.schnorr_public_key_secret_key_length_31);
assert.strictEqual(message(() => gpu.schnorrSign(m, good, new Uint8Array(31))), E.schnorr_aux_rand_length_31);
assert.strictEqual(message(() => gpu.schnorrSign('abc', good, m)), E.schnorr_message_not_bytes);
assert.ok(/only 32-byte extra entropy/.test(message(() => gpu.ecdsaSignBatch([{ msg: m, secretKey: good, extraEntropy: new Uint8Array(31) }]))));
assert.deepStrictEqual(gpu.secp256k1GetPublicKeyBatch([]), []);
assert.deepStrictEqual(gpu.ecdsaSignBatch([]), []);
assert.deepStrictEqual(gpu.schnorrSignBatch([]), []);
console.log('secp256k1 sign OK: ' + count + ' rows');
