// ristretto255 through the shim: the reference's own answers and messages (tests/golden/ristretto255_kat.json).
// Run by tests/test_gpu_ristretto_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'ristretto255_kat.json')));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => (b === null ? null : Buffer.from(b).toString('hex'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
let count = 0;

// fromBytes: the whole fixture as one batch; every refused row of the RFC and the edges through the single-item form
const rows = kat.decode;
const pts = gpu.ristrettoFromBytesBatch(rows.map((c) => bin(c.enc)));
rows.forEach((c, i) => { assert.strictEqual(hex(pts[i]), c.affine, c.name); count++; });
rows.forEach((c) => {
  if (c.error !== null && !c.name.startsWith('random')) assert.strictEqual(message(() => gpu.ristrettoFromBytes(bin(c.enc))), c.error, c.name);
});
// toBytes gives the encodings back; equals
const good = rows.filter((c) => c.error === null);
const enc = gpu.ristrettoToBytesBatch(good.map((c) => bin(c.affine)));
good.forEach((c, i) => { assert.strictEqual(hex(enc[i]), c.bytes, c.name); count++; });
assert.strictEqual(hex(gpu.ristrettoToBytes(gpu.ristrettoFromBytes(bin(kat.base)))), kat.base);
kat.equals.forEach((c) => {
  assert.strictEqual(gpu.ristrettoEquals(gpu.ristrettoFromBytes(bin(c.a)), gpu.ristrettoFromBytes(bin(c.b))), c.out);
  count++;
});
const some = good.slice(0, 40).map((c) => bin(c.affine));
assert.ok(gpu.ristrettoEqualsBatch(some, some).every((x) => x === true));
assert.ok(gpu.ristrettoEqualsBatch(some.slice(1, 9), some.slice(2, 10)).every((x) => x === false));
// deriveToCurve
const der = gpu.ristrettoDeriveToCurveBatch(kat.derive.map((c) => bin(c.in)));
kat.derive.forEach((c, i) => { assert.strictEqual(hex(der[i]), c.out); count++; });
assert.strictEqual(hex(gpu.ristrettoDeriveToCurve(bin(kat.derive[0].in))), kat.derive[0].out);
// multiply: per row, one scalar for every row, a rejected row among valid ones, BASE.multiply, messages
const mul = kat.multiply.filter((c) => c.error === null);
const prod = gpu.ristrettoMultiplyBatch(mul.map((c) => bin(c.enc)), mul.map((c) => BigInt(c.k)));
mul.forEach((c, i) => { assert.strictEqual(hex(prod[i]), c.out); count++; });
const badEnc = kat.multiply.filter((c) => c.error !== null && c.error.startsWith('invalid ristretto255')).map((c) => bin(c.enc));
const k = BigInt(mul[3].k);
const mixed = [bin(mul[0].enc), badEnc[0], bin(mul[4].enc), badEnc[1], bin(mul[8].enc)];
const oneScalar = gpu.ristrettoMultiplyBatch(mixed, k), perRow = gpu.ristrettoMultiplyBatch(mixed, mixed.map(() => k));
assert.deepStrictEqual(oneScalar.map(hex), perRow.map(hex));
assert.deepStrictEqual(oneScalar.map((r) => r === null), [false, true, false, true, false]);
assert.strictEqual(hex(gpu.ristrettoMultiply(bin(mul[3].enc), k)), mul[3].out);
kat.multiply.filter((c) => c.error !== null).forEach((c) => {
  assert.strictEqual(message(() => gpu.ristrettoMultiply(bin(c.enc), BigInt(c.k))), c.error);
});
const small = kat.small_multiples;
assert.deepStrictEqual(gpu.ristrettoMultiplyBaseBatch([1n, 2n, 15n]).map(hex), [small[1], small[2], small[15]]);
assert.strictEqual(hex(gpu.ristrettoMultiplyBase(7n)), small[7]);
// msm from encodings: 3 * 2B + 2 * 3B = 12B; a zero sum; a bad encoding
assert.strictEqual(hex(gpu.ristrettoMsm([bin(small[2]), bin(small[3])], [3n, 2n])), small[12]);
const ORDER = (1n << 252n) + 27742317777372353535851937790883648493n;
assert.strictEqual(hex(gpu.ristrettoMsm([bin(small[5]), bin(small[5])], [9n, ORDER - 9n])), small[0]);
assert.strictEqual(message(() => gpu.ristrettoMsm([bin(small[2]), badEnc[1]], [3n, 2n])), 'invalid ristretto255 encoding 2');
assert.strictEqual(message(() => gpu.ristrettoMsm([bin(small[2]), badEnc[0]], [3n, 2n])), 'invalid ristretto255 encoding 1');
// argument errors
const E = kat.errors;
assert.strictEqual(message(() => gpu.ristrettoFromBytes(new Uint8Array(31))), E.length);
assert.strictEqual(message(() => gpu.ristrettoFromBytes('x')), E.type);
assert.strictEqual(message(() => gpu.ristrettoDeriveToCurve(new Uint8Array(63))), E.derive_length);
assert.strictEqual(message(() => gpu.ristrettoMultiplyBase(0n)), E.multiply_zero);
assert.strictEqual(message(() => gpu.ristrettoMultiplyBase(ORDER)), E.multiply_order);
assert.deepStrictEqual(gpu.ristrettoFromBytesBatch([]), []);
assert.deepStrictEqual(gpu.ristrettoToBytesBatch([]), []);
assert.deepStrictEqual(gpu.ristrettoMultiplyBatch([], []), []);
console.log('ristretto255 OK: ' + count + ' rows');
