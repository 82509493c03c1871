// polyFr through the shim: the reference's own answers for poly() over both scalar fields (tests/golden/poly_kat.json), with and
// without "an FFT was passed", and the reference's messages.  Run by tests/test_gpu_poly_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'poly_kat.json')));
const vecs = kat.vectors.map((v) => v.map(BigInt));
const E = kat.errors;
let count = 0;
for (const field of ['bls12_381', 'bn254']) {
  const R = BigInt(kat.fields[field].order);
  const P0 = gpu.polyFr({ field, generator: BigInt(kat.generator) }), P1 = gpu.polyFr({ field, fft: true });
  for (const c of kat.fields[field].cases) {
    const a = c.a === undefined ? undefined : vecs[c.a], b = c.b === undefined ? undefined : vecs[c.b];
    const x = c.x === undefined ? undefined : BigInt(c.x);
    const want = typeof c.out === 'object' ? vecs[c.out.v] : typeof c.out === 'string' ? BigInt(c.out) : c.out;
    for (const P of c.fft ? [P0, P1] : [P0]) {
      let got;
      switch (c.op) {
        case 'add': case 'sub': case 'dot': case 'mul': case 'convolve': case 'eval': got = P[c.op](a, b); break;
        case 'scale': got = P.mul(a, x); break;
        case 'shift': got = P.shift(a, x); break;
        case 'monomial_eval': got = P.monomial.eval(a, x); break;
        case 'lagrange_basis': got = P.lagrange.basis(x, c.n, c.brp); break;
        case 'lagrange_eval': got = P.lagrange.eval(a, x, c.brp); break;
        default: continue;
      }
      assert.deepStrictEqual(got, want, field + ' ' + c.op + ' ' + (a ? a.length : c.n));
      count++;
    }
  }
  const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
  const fixed = gpu.polyFr({ field, length: 4 });
  assert.strictEqual(msg(() => P0.add([1n, 2n], [1n])), E.mismatched);
  assert.strictEqual(msg(() => fixed.add([1n], [1n])), E.fixed_length);
  assert.strictEqual(msg(() => fixed.shift([1n, 2n], 3n)), E.fixed_length_shift);
  assert.strictEqual(msg(() => P0.lagrange.basis(2n, 3)), E.lagrange_basis_length);
  assert.strictEqual(msg(() => P0.lagrange.eval([1n, 2n, 3n], 2n)), E.lagrange_eval_length);
  assert.strictEqual(msg(() => P0.add(5n, [1n])), E.not_poly_bigint);
  assert.strictEqual(msg(() => P0.add('x', [1n])), E.not_poly_string);
  assert.strictEqual(msg(() => P0.add([1n], 5n)), E.not_poly_b);
  assert.strictEqual(msg(() => P0.shift(7n, 3n)), E.not_poly_shift);
  assert.strictEqual(msg(() => P1.mul([1n, 2n, 3n], [1n, 2n, 3n])), E.fft_length);
  assert.strictEqual(msg(() => P0.add([R], [0n])), E.out_of_range);
  assert.strictEqual(msg(() => P0.mul([1n], R)), E.out_of_range);
  assert.strictEqual(msg(() => P0.monomial.eval([1n, 2n], -1n)), E.out_of_range);
}
assert.throws(() => gpu.polyFr({ field: 'secp256k1' }), /unknown field/);
assert.ok(count > 400, 'cases replayed: ' + count);
console.log('poly OK');
