// The bn254 scalar-field transform through the shim (fftFr with opts.field = 'bn254'): the reference's `bn254 roots` /
// `bn254 brp` known answers (tests/golden/fft_kat_bn254.json) as the transform of the delta at 1, round trips in two
// orderings, and the range check against THIS field's order.  Run by tests/test_gpu_ntt_bn254_node.py.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001n;
const BLS_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001n;
const bn = { field: 'bn254' };
const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'fft_kat_bn254.json')));
const roots3 = kat.roots3.map(BigInt), brp3 = kat.brp3.map(BigInt);

// roots(3) = direct(delta at 1); brp(3) = the same with bit-reversed output
const delta = [0n, 1n, 0n, 0n, 0n, 0n, 0n, 0n];
assert.deepStrictEqual(gpu.fftFr(delta, bn), roots3);
assert.deepStrictEqual(gpu.fftFr(delta, Object.assign({ brpOutput: true }, bn)), brp3);
// the default field is untouched: the same delta over bls12-381 Fr gives other roots
assert.notDeepStrictEqual(gpu.fftFr(delta), roots3);

// round trips: natural order, and bit-reversed between the two transforms
let x = 0x9e3779b97f4a7c15n;
const poly = [];
for (let i = 0; i < 1 << 11; i++) { x = (x * x + 0x1234567n * BigInt(i + 1)) % R; poly.push(x); }
poly[0] = 0n; poly[1] = 1n; poly[2] = R - 1n;
const y = gpu.fftFr(poly, bn);
assert.deepStrictEqual(gpu.fftFr(y, Object.assign({ inverse: true }, bn)), poly);
const yb = gpu.fftFr(poly, Object.assign({ brpOutput: true }, bn));
assert.deepStrictEqual(gpu.fftFr(yb, Object.assign({ inverse: true, brpInput: true }, bn)), poly);
assert.strictEqual(y[0], poly.reduce((a, b) => (a + b) % R, 0n));      // y[0] = sum x

// range: r itself and a bls12-381 residue above r are outside, r - 1 is inside
assert.throws(() => gpu.fftFr([R, 0n], bn), /invalid field element: outside of range 0\.\.ORDER/);
assert.throws(() => gpu.fftFr([0n, BLS_R - 1n], bn), /outside of range/);
assert.deepStrictEqual(gpu.fftFr([R - 1n, 0n], bn), [R - 1n, R - 1n]);
assert.deepStrictEqual(gpu.fftFr([BLS_R - 1n, 0n]), [BLS_R - 1n, BLS_R - 1n]);
assert.throws(() => gpu.fftFr([1n, 2n, 3n], bn), /FFT: Polynomial size should be power of two/);
assert.throws(() => gpu.fftFr([1n, 2n], { field: 'secp256k1' }), /unknown field/);
console.log('bn254 fft OK');
