// RFC 9380 for secp256k1 and ed25519 through the shim: the reference's own answers and messages (tests/golden/h2c_suites_kat.json).
// The inputs of the listed rows are rebuilt here by name, as tests/h2c_suites_helpers.py does.  Run by tests/test_gpu_h2c_suites_node.py.
'use strict';
const assert = require('assert');
const crypto = require('crypto');
const fs = require('fs');
const path = require('path');
const gpu = require('./noble_gpu.js');

const kat = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'h2c_suites_kat.json')));
const ascii = (s) => Uint8Array.from(Buffer.from(s, 'ascii'));
const message = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const seeded = (tag, i, n) => {
  const parts = [];
  for (let c = 0, got = 0; got < n; c++, got += 64) parts.push(crypto.createHash('sha512').update(`h2c-suites-kat/${tag}/${i}/${c}`).digest());
  return Uint8Array.from(Buffer.concat(parts).slice(0, n));
};
const SUITES = {
  secp256k1: { hasher: gpu.secp256k1_hasher, hash: gpu.secp256k1HashToCurveBatch, encode: gpu.secp256k1EncodeToCurveBatch, block: 64, lenfield: 8,
    ro: 'secp256k1_XMD:SHA-256_SSWU_RO_', nu: 'secp256k1_XMD:SHA-256_SSWU_NU_', zero: [0n, 0n] },
  ed25519: { hasher: gpu.ed25519_hasher, hash: gpu.ed25519HashToCurveBatch, encode: gpu.ed25519EncodeToCurveBatch, block: 128, lenfield: 16,
    ro: 'edwards25519_XMD:SHA-512_ELL2_RO_', nu: 'edwards25519_XMD:SHA-512_ELL2_NU_', zero: [0n, 1n] },
};
const MESSAGES = [['empty', ascii('')], ['abc', ascii('abc')], ['abcdef', ascii('abcdef0123456789')], ['q133', ascii('q'.repeat(133))],
  ['a512', ascii('a'.repeat(512))]];
function listedRows(name) {
  const s = SUITES[name], quux = 'QUUX-V01-CS02-with-', rows = [];
  for (const [mn, msg] of MESSAGES)
    rows.push([`${mn}/rfc/ro`, msg, ascii(quux + s.ro), 2], [`${mn}/rfc/nu`, msg, ascii(quux + s.nu), 1], [`${mn}/default/ro`, msg, ascii(s.ro), 2],
      [`${mn}/default/nu`, msg, ascii(s.nu), 1]);
  rows.push(['dst300', ascii('abc'), ascii('x'.repeat(300)), 2], ['dst1', ascii('abc'), ascii('D'), 2], ['dst255', ascii('abc'), ascii('y'.repeat(255)), 1]);
  const fixed = s.block + 3 + s.ro.length + 1 + 1 + s.lenfield;
  const at = ((-fixed % s.block) + s.block) % s.block + s.block;
  [at - 1, at, at + 1].forEach((n, k) => rows.push([`boundary${k - 1 >= 0 ? '+' : ''}${k - 1}`, seeded(`boundary-${name}`, k, n), ascii(s.ro), 2]));
  rows.push(['long1000', seeded(`long-${name}`, 0, 1000), ascii(s.ro), 2]);
  return rows;
}
const want = (r) => [BigInt('0x' + r.x), BigInt('0x' + r.y)];
let count = 0;

for (const name of Object.keys(SUITES)) {
  const s = SUITES[name], k = kat[name], rows = listedRows(name);
  assert.deepStrictEqual(rows.map((r) => r[0]), k.hash.map((r) => r.name));
  // one native call per (DST, count) group, and the single-call forms of the hasher objects on every row
  const groups = new Map();
  rows.forEach((r, i) => { const key = Buffer.from(r[2]).toString('hex') + '/' + r[3]; groups.set(key, (groups.get(key) || []).concat([i])); });
  for (const idx of groups.values()) {
    const [, , dst, cnt] = rows[idx[0]];
    const got = (cnt === 2 ? s.hash : s.encode)(idx.map((i) => rows[i][1]), { DST: dst });
    idx.forEach((i, j) => { assert.deepStrictEqual([got[j].x, got[j].y], want(k.hash[i]), `${name} ${rows[i][0]}`); count++; });
  }
  rows.forEach((r, i) => {
    const p = r[3] === 2 ? s.hasher.hashToCurve(r[1], { DST: r[2] }) : s.hasher.encodeToCurve(r[1], { DST: r[2] });
    assert.deepStrictEqual([p.x, p.y], want(k.hash[i]), `${name} ${r[0]} single`);
  });
  // the default DSTs, and a string DST read as ASCII
  const abc = ascii('abc'), byName = (n) => want(k.hash.find((r) => r.name === n));
  let p = s.hasher.hashToCurve(abc);
  assert.deepStrictEqual([p.x, p.y], byName('abc/default/ro'));
  p = s.hasher.encodeToCurve(abc);
  assert.deepStrictEqual([p.x, p.y], byName('abc/default/nu'));
  p = s.hasher.hashToCurve(abc, { DST: 'QUUX-V01-CS02-with-' + s.ro });
  assert.deepStrictEqual([p.x, p.y], byName('abc/rfc/ro'));
  // hashToScalar: the default DST for the five messages, then a custom one
  const sc = gpu.hashToScalarBatch(MESSAGES.map((m) => m[1]), { curve: name });
  assert.deepStrictEqual(sc, k.scalar.slice(0, 5).map((r) => BigInt('0x' + r.out)));
  assert.deepStrictEqual(s.hasher.hashToScalarBatch(MESSAGES.map((m) => m[1])), sc);
  assert.strictEqual(s.hasher.hashToScalar(abc, { DST: ascii('QUUX-V01-CS02-with-' + s.ro) }), BigInt('0x' + k.scalar[5].out));
  count += 6;
  // a Point class of the caller's: fromAffine for a point (ZERO has its own branch, not reachable from a hash)
  const P = { ZERO: 'zero', fromAffine: (a) => ['pt', a.x, a.y] };
  assert.deepStrictEqual(s.hash([abc], { Point: P })[0], ['pt'].concat(byName('abc/default/ro')));
  // defaults: a fresh copy each time
  const d = s.hasher.defaults;
  assert.deepStrictEqual([d.DST, d.encodeDST, d.p.toString(), d.m, d.k, d.expand], [k.defaults.DST, k.defaults.encodeDST, k.defaults.p, 1, 128, 'xmd']);
  d.DST = 'poisoned';
  assert.strictEqual(s.hasher.defaults.DST, k.defaults.DST);
  // the reference's messages
  assert.strictEqual(message(() => s.hasher.hashToCurve(new Uint8Array(1), { DST: '' })), k.errors.empty_dst);
  assert.strictEqual(message(() => s.hasher.encodeToCurve(new Uint8Array(1), { DST: new Uint8Array(0) })), k.errors.empty_dst_bytes);
  assert.strictEqual(message(() => s.hasher.hashToScalar(new Uint8Array(1), { DST: '' })), k.errors.scalar_empty_dst);
  assert.strictEqual(message(() => s.hasher.hashToCurve('abc')), k.errors.msg_string);
  assert.deepStrictEqual(s.hash([]), []);
  assert.deepStrictEqual(gpu.hashToScalarBatch([], { curve: name }), []);
}
assert.strictEqual(gpu.hashToScalarBatch([ascii('abc')])[0], BigInt('0x0afe998ff82d0b7ca5673a6c8dcaf2a0cd1361d1d1b2a4e4f57f4dc9a0305788'));   // secp256k1 by default
console.log(`h2c suites OK: ${count} rows`);
