// The ristretto255 OPRF through the shim: the reference's own answers and messages (tests/golden/ristretto255_oprf_kat.json), replayed
// with the recorded rng bytes.  The inputs of a batch are indices into the seeded inputs, rebuilt here as tests/oprf_helpers.py does.
// Run by tests/test_gpu_oprf_node.py.
'use strict';
const assert = require('assert');
const crypto = require('crypto');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'ristretto255_oprf_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => Buffer.from(b).toString('hex');
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const seeded = (tag, i, n) => {
  const parts = [];
  for (let c = 0, got = 0; got < n; c++, got += 64) parts.push(crypto.createHash('sha512').update(`ristretto255-oprf-kat/${tag}/${i}/${c}`).digest());
  return Uint8Array.from(Buffer.concat(parts).slice(0, n));
};
const inputs = [bin('00'), new Uint8Array(17).fill(0x5a)].concat([0, 1, 67, 68, 84, 200, 1000].map((n) => seeded('input', n, n)));
const replay = (h) => { const b = bin(h); let at = 0; return (n) => { const r = b.slice(at, at + n); at += n; assert.strictEqual(r.length, n); return r; }; };
const O = gpu.ristretto255_oprf;
let count = 0;

assert.strictEqual(O.name, kat.name);
for (const block of kat.modes) {
  const mode = block.mode;
  const S = mode === 0 ? O.oprf : mode === 1 ? O.voprf : O.poprf(bin(block.info));
  const keys = S.deriveKeyPair(bin(kat.seed), bin(kat.key_info));
  assert.strictEqual(hex(keys.secretKey), block.skS);
  assert.strictEqual(hex(keys.publicKey), block.pkS);
  const sk = keys.secretKey, pk = keys.publicKey;
  for (const b of block.batches.slice(0, 6)) {
    const ins = b.idx.map((i) => inputs[i]), rng = replay(b.rng);
    const bl = mode === 2 ? S.blindBatch(ins, pk, rng) : S.blindBatch(ins, rng);
    assert.deepStrictEqual(bl.blind.map(hex), b.blind);
    assert.deepStrictEqual(bl.blinded.map(hex), b.blinded);
    let evaluated, output;
    if (mode === 0) {
      evaluated = S.blindEvaluateBatch(sk, bl.blinded);
      output = S.finalizeBatch(ins, bl.blind, evaluated);
    } else {
      const res = mode === 1 ? S.blindEvaluateBatch(sk, pk, bl.blinded, rng) : S.blindEvaluateBatch(sk, bl.blinded, rng);
      evaluated = res.evaluated;
      assert.strictEqual(hex(res.proof), b.proof);
      const items = ins.map((input, j) => ({ input, blind: bl.blind[j], evaluated: evaluated[j], blinded: bl.blinded[j] }));
      if (mode === 2) assert.strictEqual(hex(bl.tweakedKey), b.tweakedKey);
      output = mode === 1 ? S.finalizeBatch(items, pk, res.proof) : S.finalizeBatch(items, res.proof, bl.tweakedKey);
      const flipped = Uint8Array.from(res.proof);
      flipped[40] ^= 4;
      assert.strictEqual(message(() => (mode === 1 ? S.finalizeBatch(items, pk, flipped) : S.finalizeBatch(items, flipped, bl.tweakedKey))),
        'proof verification failed');
    }
    assert.deepStrictEqual(evaluated.map(hex), b.evaluated);
    assert.deepStrictEqual(output.map(hex), b.output);
    assert.deepStrictEqual(S.evaluateBatch(sk, ins).map(hex), b.evaluate);
    count += ins.length;
  }
  // the single-item forms on the first row
  const b = block.batches[0], i0 = inputs[b.idx[0]];
  assert.strictEqual(hex(S.evaluate(sk, i0)), b.evaluate[0]);
  const one = mode === 2 ? S.blind(i0, pk, replay(b.rng)) : S.blind(i0, replay(b.rng));
  assert.strictEqual(hex(one.blinded), b.blinded[0]);
}
// RFC 9497 A.1.1 vector 1
const a = kat.anchor[0];
const ab = O.oprf.blind(bin(a.input), replay(a.rng));
assert.strictEqual(hex(ab.blind), a.blind);
assert.strictEqual(hex(ab.blinded), a.blinded);
const aev = O.oprf.blindEvaluate(bin(a.skS), ab.blinded);
assert.strictEqual(hex(aev), a.evaluated);
assert.strictEqual(hex(O.oprf.finalize(bin(a.input), ab.blind, aev)), a.output);

// the reference's messages
const ei = {};
Object.keys(kat.error_inputs).forEach((k) => { ei[k] = bin(kat.error_inputs[k]); });
const V = O.voprf, P2 = O.poprf(new Uint8Array(3));
const zero = new Uint8Array(32), bad = new Uint8Array(32).fill(1), L = (1n << 252n) + 27742317777372353535851937790883648493n;
const le = (n) => { const b = new Uint8Array(32); for (let i = 0; i < 32; i++) { b[i] = Number(n & 255n); n >>= 8n; } return b; };
const cases = {
  input_long: () => O.oprf.blind(new Uint8Array(65536)),
  seed_length: () => O.oprf.deriveKeyPair(new Uint8Array(31), new Uint8Array(0)),
  blind_zero: () => O.oprf.finalize(bin('00'), zero, ei.blinded),
  blind_order: () => O.oprf.finalize(bin('00'), le(L), ei.blinded),
  secret_zero: () => O.oprf.blindEvaluate(zero, ei.blinded),
  bad_encoding: () => O.oprf.blindEvaluate(ei.skS, bad),
  identity_blinded: () => O.oprf.blindEvaluate(ei.skS, zero),
  identity_evaluated: () => O.oprf.finalize(bin('00'), ei.blind, zero),
  identity_public_key: () => V.blindEvaluate(ei.skS, zero, ei.blinded),
  identity_tweaked_key: () => P2.finalize(bin('00'), ei.blind, ei.evaluated, ei.blinded, ei.proof, zero),
  proof_length: () => V.finalize(bin('00'), ei.blind, ei.evaluated, ei.blinded, ei.pkS, new Uint8Array(63)),
  proof_ff: () => V.finalize(bin('00'), ei.blind, ei.evaluated, ei.blinded, ei.pkS, new Uint8Array(64).fill(255)),
  proof_zero: () => V.finalize(bin('00'), ei.blind, ei.evaluated, ei.blinded, ei.pkS, new Uint8Array(64)),
  expected_array: () => V.blindEvaluateBatch(ei.skS, ei.pkS, ei.blinded),
  rng_type: () => O.oprf.blind(bin('00'), 5),
};
Object.keys(cases).forEach((name) => { assert.strictEqual(message(cases[name]), kat.errors[name], name); count++; });
assert.strictEqual(V.finalize(bin('00'), ei.blind, ei.evaluated, ei.blinded, ei.pkS, ei.proof).length, 64);
// a fresh key pair and a round trip with the default rng
const kp = V.generateKeyPair();
const rb = V.blind(bin('c0ffee'));
const re = V.blindEvaluate(kp.secretKey, kp.publicKey, rb.blinded);
assert.strictEqual(hex(V.finalize(bin('c0ffee'), rb.blind, re.evaluated, rb.blinded, kp.publicKey, re.proof)), hex(V.evaluate(kp.secretKey, bin('c0ffee'))));
console.log('ristretto255 OPRF OK: ' + count + ' rows');
