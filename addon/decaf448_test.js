// decaf448 through the shim: the reference's own answers (tests/golden/decaf448_kat.json).
// Run by tests/test_gpu_decaf448_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'decaf448_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => (b === null ? null : Buffer.from(b).toString('hex'));
const big = (h) => BigInt('0x' + h);
const le56 = (v) => { const o = new Uint8Array(56); for (let i = 0; i < 56; i++) { o[i] = Number(v & 255n); v >>= 8n; } return o; };
const affine = (x, y) => { const o = new Uint8Array(112); o.set(le56(big(x)), 0); o.set(le56(big(y)), 56); return o; };
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
let count = 0;

// fromBytes: every decode row of the fixture as one batch, null where the reference throws; then toBytes of what came out
const dec = kat.decode;
const pts = gpu.decaf448FromBytesBatch(dec.map((c) => bin(c.enc)));
dec.forEach((c, i) => {
  assert.strictEqual(pts[i] === null, c.error !== null, c.name);
  if (c.error === null) assert.strictEqual(hex(pts[i]), hex(affine(c.x, c.y)), c.name);
  count++;
});
const good = dec.filter((c) => c.error === null);
assert.ok(good.length > 15 && good.length < dec.length);
assert.deepStrictEqual(gpu.decaf448ToBytesBatch(pts.filter((p) => p !== null)).map(hex), good.map((c) => c.enc));
// toBytes of whole cosets and of the small-order points
assert.deepStrictEqual(gpu.decaf448ToBytesBatch(kat.encode_affine.map((c) => affine(c.x, c.y))).map(hex), kat.encode_affine.map((c) => c.enc));
count += kat.encode_affine.length;
// equals
assert.deepStrictEqual(gpu.decaf448EqualsBatch(kat.equals.map((c) => affine(c.x1, c.y1)), kat.equals.map((c) => affine(c.x2, c.y2))),
  kat.equals.map((c) => c.equal));
count += kat.equals.length;
// multiply: per row, one scalar for all rows, and the base point
const mul = kat.mul.filter((c) => c.multiply.error === null);
assert.deepStrictEqual(gpu.decaf448MultiplyBatch(mul.map((c) => bin(c.enc)), mul.map((c) => big(c.k))).map(hex), mul.map((c) => c.multiply.out));
count += mul.length;
const k7 = 7n, some = kat.multiples.slice(1, 9).map((c) => bin(c.enc)).concat([bin(dec[16 + 14].enc)]);
const oneScalar = gpu.decaf448MultiplyBatch(some, k7);
assert.deepStrictEqual(oneScalar.map(hex), gpu.decaf448MultiplyBatch(some, some.map(() => k7)).map(hex));
assert.ok(oneScalar[8] === null && oneScalar[0] !== null);
assert.strictEqual(hex(oneScalar[0]), kat.multiples[7].enc);                    // 7 * (1 B)
const bm = kat.multiples.filter((c) => big(c.k) >= 1n);
assert.deepStrictEqual(gpu.decaf448MultiplyBaseBatch(bm.map((c) => big(c.k))).map(hex), bm.map((c) => c.enc));
count += bm.length;
// deriveToCurve
assert.deepStrictEqual(gpu.decaf448DeriveToCurveBatch(kat.derive.map((c) => bin(c.uniform))).map(hex), kat.derive.map((c) => c.enc));
count += kat.derive.length;
// argument errors
const E = kat.errors;
assert.strictEqual(message(() => gpu.decaf448FromBytesBatch([new Uint8Array(55)])), E.length);
assert.strictEqual(message(() => gpu.decaf448FromBytesBatch(['00'])), E.type);
assert.strictEqual(message(() => gpu.decaf448DeriveToCurveBatch([new Uint8Array(111)])), E.derive_length);
assert.strictEqual(message(() => gpu.decaf448MultiplyBaseBatch([0n])), E.multiply_zero);
assert.strictEqual(message(() => gpu.decaf448MultiplyBatch([new Uint8Array(56)], [big(kat.multiples[0].k) + (1n << 446n)])), E.multiply_n);
assert.deepStrictEqual(gpu.decaf448FromBytesBatch([]), []);
assert.deepStrictEqual(gpu.decaf448ToBytesBatch([]), []);
assert.deepStrictEqual(gpu.decaf448EqualsBatch([], []), []);
assert.deepStrictEqual(gpu.decaf448MultiplyBatch([], []), []);
assert.deepStrictEqual(gpu.decaf448MultiplyBaseBatch([]), []);
assert.deepStrictEqual(gpu.decaf448DeriveToCurveBatch([]), []);
console.log('decaf448 OK: ' + count + ' rows');
