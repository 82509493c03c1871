// RFC 9380 for edwards448 and decaf448 through the shim: the reference's own answers and messages (tests/golden/h2c448_kat.json).
// The inputs of the listed rows are rebuilt here by name, as tests/h2c448_helpers.py does.  Run by tests/test_gpu_h2c448_node.py.
'use strict';
const assert = require('assert');
const crypto = require('crypto');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'h2c448_kat.json')));
const ascii = (s) => Uint8Array.from(Buffer.from(s, 'ascii'));
const hex = (b) => Buffer.from(b).toString('hex');
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const seeded = (tag, i, n) => {
  const parts = [];
  for (let c = 0, got = 0; got < n; c++, got += 64) parts.push(crypto.createHash('sha512').update(`h2c448-kat/${tag}/${i}/${c}`).digest());
  return Uint8Array.from(Buffer.concat(parts).slice(0, n));
};
const RO = 'edwards448_XOF:SHAKE256_ELL2_RO_', NU = 'edwards448_XOF:SHAKE256_ELL2_NU_', QUUX = 'QUUX-V01-CS02-with-';
const DECAF = 'decaf448_XOF:SHAKE256_D448MAP_RO_';
const MESSAGES = [['empty', ascii('')], ['abc', ascii('abc')], ['abcdef', ascii('abcdef0123456789')], ['q133', ascii('q'.repeat(133))],
  ['a512', ascii('a'.repeat(512))]];
function listedRows() {
  const rows = [];
  for (const [mn, msg] of MESSAGES)
    rows.push([`${mn}/rfc/ro`, msg, ascii(QUUX + RO), 2], [`${mn}/rfc/nu`, msg, ascii(QUUX + NU), 1], [`${mn}/default/ro`, msg, ascii(RO), 2],
      [`${mn}/default/nu`, msg, ascii(NU), 1]);
  rows.push(['dst300', ascii('abc'), ascii('x'.repeat(300)), 2], ['dst1', ascii('abc'), ascii('D'), 2], ['dst255', ascii('abc'), ascii('y'.repeat(255)), 1]);
  const fixed = 2 + RO.length + 1;
  [135, 136, 137].forEach((r, k) => rows.push([`boundary${r}`, seeded('boundary', k, (((r - fixed) % 136) + 136) % 136 + 136), ascii(RO), 2]));
  rows.push(['long1000', seeded('long', 0, 1000), ascii(RO), 2]);
  return rows;
}
const decafRows = MESSAGES.map(([n, m]) => [n, m, ascii(DECAF)]).concat([['fill5', new Uint8Array(10).fill(5), ascii(DECAF)],
  ['abc/custom', ascii('abc'), ascii(QUUX + DECAF)], ['abc/dst300', ascii('abc'), ascii('w'.repeat(300))], ['abc/dst255', ascii('abc'), ascii('v'.repeat(255))]]);
const scalarRows = MESSAGES.map(([n, m]) => [n, m, undefined]).concat([['abc/custom', ascii('abc'), ascii(QUUX + RO)],
  ['abc/dst300', ascii('abc'), ascii('z'.repeat(300))]]);
const want = (r) => [BigInt('0x' + r.x), BigInt('0x' + r.y)];
let count = 0;

const rows = listedRows(), h = gpu.ed448_hasher;
assert.deepStrictEqual(rows.map((r) => r[0]), kat.hash.map((r) => r.name));
// one native call per (DST, count) group, and the single-call forms of the hasher object on every row
const groups = new Map();
rows.forEach((r, i) => { const key = hex(r[2]) + '/' + r[3]; groups.set(key, (groups.get(key) || []).concat([i])); });
for (const idx of groups.values()) {
  const [, , dst, cnt] = rows[idx[0]];
  const got = (cnt === 2 ? gpu.ed448HashToCurveBatch : gpu.ed448EncodeToCurveBatch)(idx.map((i) => rows[i][1]), { DST: dst });
  idx.forEach((i, j) => { assert.deepStrictEqual([got[j].x, got[j].y], want(kat.hash[i]), rows[i][0]); count++; });
}
rows.forEach((r, i) => {
  const p = r[3] === 2 ? h.hashToCurve(r[1], { DST: r[2] }) : h.encodeToCurve(r[1], { DST: r[2] });
  assert.deepStrictEqual([p.x, p.y], want(kat.hash[i]), `${r[0]} single`);
});
// the default DSTs, and a string DST read as ASCII
const abc = ascii('abc'), byName = (n) => want(kat.hash.find((r) => r.name === n));
let p = h.hashToCurve(abc);
assert.deepStrictEqual([p.x, p.y], byName('abc/default/ro'));
p = h.encodeToCurve(abc);
assert.deepStrictEqual([p.x, p.y], byName('abc/default/nu'));
p = h.hashToCurveBatch([abc], { DST: QUUX + RO })[0];
assert.deepStrictEqual([p.x, p.y], byName('abc/rfc/ro'));
// hashToScalar of both hashers: the default DST, a custom one, and a 300-byte one (compressed to 56 bytes here, to 64 for decaf448)
assert.deepStrictEqual(scalarRows.map((r) => r[0]), kat.scalar.map((r) => r.name));
scalarRows.forEach(([name, msg, dst], i) => {
  const o = dst === undefined ? undefined : { DST: dst };
  assert.strictEqual(h.hashToScalar(msg, o), BigInt('0x' + kat.scalar[i].out), `scalar ${name}`);
  assert.strictEqual(gpu.decaf448HashToScalarBatch([msg], o)[0], BigInt('0x' + kat.decaf_scalar[i].out), `decaf scalar ${name}`);
  count += 2;
});
assert.deepStrictEqual(h.hashToScalarBatch(MESSAGES.map((m) => m[1])), kat.scalar.slice(0, 5).map((r) => BigInt('0x' + r.out)));
assert.deepStrictEqual(gpu.decaf448HashToScalarBatch(MESSAGES.map((m) => m[1])), kat.decaf_scalar.slice(0, 5).map((r) => BigInt('0x' + r.out)));
// decaf448 hashToCurve: the encoded elements, the reference's inline vector among them
assert.deepStrictEqual(decafRows.map((r) => r[0]), kat.decaf.map((r) => r.name));
decafRows.forEach(([name, msg, dst], i) => {
  assert.strictEqual(hex(gpu.decaf448HashToCurveBatch([msg], { DST: dst })[0]), kat.decaf[i].out, `decaf ${name}`);
  count++;
});
assert.deepStrictEqual(gpu.decaf448HashToCurveBatch(MESSAGES.map((m) => m[1])).map(hex), kat.decaf.slice(0, 5).map((r) => r.out));
assert.strictEqual(hex(gpu.decaf448HashToCurveBatch([new Uint8Array(10).fill(5)])[0]), kat.pins[0].out);
// a Point class of the caller's
const P = { ZERO: 'zero', fromAffine: (a) => ['pt', a.x, a.y] };
assert.deepStrictEqual(gpu.ed448HashToCurveBatch([abc], { Point: P })[0], ['pt'].concat(byName('abc/default/ro')));
// defaults: a fresh copy each time
const d = h.defaults;
assert.deepStrictEqual([d.DST, d.encodeDST, d.p.toString(), d.m, d.k, d.expand],
  [kat.defaults.DST, kat.defaults.encodeDST, kat.defaults.p, kat.defaults.m, kat.defaults.k, kat.defaults.expand]);
d.DST = 'poisoned';
assert.strictEqual(h.defaults.DST, kat.defaults.DST);
// the reference's messages
assert.strictEqual(message(() => h.hashToCurve(new Uint8Array(1), { DST: '' })), kat.errors.empty_dst);
assert.strictEqual(message(() => h.encodeToCurve(new Uint8Array(1), { DST: new Uint8Array(0) })), kat.errors.empty_dst_bytes);
assert.strictEqual(message(() => h.hashToScalar(new Uint8Array(1), { DST: '' })), kat.errors.scalar_empty_dst);
assert.strictEqual(message(() => h.hashToCurve('abc')), kat.errors.msg_string);
assert.strictEqual(message(() => gpu.decaf448HashToCurveBatch([new Uint8Array(1)], { DST: '' })), kat.errors.decaf_empty_dst);
assert.strictEqual(message(() => gpu.decaf448HashToScalarBatch([new Uint8Array(1)], { DST: '' })), kat.errors.decaf_scalar_empty_dst);
assert.deepStrictEqual(gpu.ed448HashToCurveBatch([]), []);
assert.deepStrictEqual(gpu.decaf448HashToCurveBatch([]), []);
assert.deepStrictEqual(gpu.decaf448HashToScalarBatch([]), []);
console.log(`h2c448 OK: ${count} rows`);
