'use strict';
// JS shim over the N-API addon: keeps the reference's call shapes for the hot path.
//   pippenger(c, points, scalars)          - same signature / validation / messages as
//                                            src/abstract/curve.ts:863-905
//   multiplyUnsafeBatch(c, points, scalars) - array form of Point.multiplyUnsafe
//                                            (src/abstract/weierstrass.ts:915-928)
//   multiplyBaseBatch(c, scalars)          - array form of BASE.multiply (curve.ts:588-606)
//   ed25519VerifyBatch(items, zip215)      - array form of eddsa.verify (edwards.ts:942-989)
//   x25519ScalarMultBatch(items)           - array form of x25519.scalarMult / getSharedSecret (abstract/montgomery.ts:314-331);
//   x25519GetPublicKeyBatch(secretKeys)      x25519.getPublicKey; ed25519ToMontgomeryBatch(publicKeys): ed25519.utils.toMontgomery
//   secp256k1GetPublicKeyBatch(secretKeys, isCompressed), schnorrGetPublicKeyBatch(secretKeys), ecdsaSignBatch(items, opts),
//   schnorrSignBatch(items)                - array forms of secp256k1.getPublicKey / sign (RFC 6979) and schnorr.getPublicKey / sign
//                                            (BIP-340) on the device; secp256k1Sign / schnorrSign: single-item forms with the reference's messages
//   ed25519GetPublicKeyBatch(secretKeys)   - array form of eddsa.getPublicKey (abstract/edwards.ts:870-897);
//   ed25519SignBatch(items | {msgs, secretKey}, { context, prehash }) - eddsa.sign for ed25519, ed25519ctx (context given) and
//                                            ed25519ph (prehash: true) (edwards.ts:908-930, ed25519.ts:146-223), hashes included, on the
//                                            device; ed25519GetPublicKey / ed25519Sign: single-item forms with the reference's messages
//   x448ScalarMultBatch(items), x448GetPublicKeyBatch(secretKeys) - x448.scalarMult / getPublicKey (ed448.ts:284-311);
//   ed448VerifyBatch(items, { context, prehash, deviceHash }) - ed448 / ed448ph verify, the SHAKE256 challenge hashed here on the
//                                            host, or on the device with deviceHash: true
//   ed448GetPublicKeyBatch(secretKeys), ed448SignBatch(items | {msgs, secretKey}, { context, prehash }) - eddsa.getPublicKey / sign
//                                            for ed448 and ed448ph, every hash on the device; ed448GetPublicKey / ed448Sign: single items
//   ristretto255_oprf                      - RFC 9497 OPRF / VOPRF / POPRF over ristretto255-SHA512 in the reference's shape, with
//                                            blindBatch / blindEvaluateBatch / finalizeBatch / evaluateBatch beside the single forms
//   ristrettoFromBytesBatch(encodings) ...  - array forms of ristretto255.Point.fromBytes / toBytes / equals / multiply /
//                                            BASE.multiply, an MSM from encodings and ristretto255_hasher.deriveToCurve
//                                            (src/ed25519.ts:443-668), with single-item forms that throw the reference's messages
//   decaf448FromBytesBatch(encodings) ...   - array forms of decaf448.Point.fromBytes / toBytes / equals / multiply / BASE.multiply
//                                            and decaf448_hasher.deriveToCurve (src/ed448.ts:462-701)
//   fftFr(values, opts)                    - FFT(roots, Fr).direct / .inverse (abstract/fft.ts:518-577)
//   polyFr(opts)                           - poly(Fr, roots, ...) on arrays of bigint (abstract/fft.ts:583-926): add, sub, dot,
//                                            mul, convolve, shift, eval, monomial.eval, lagrange.basis / eval
// `c` is any Point constructor with the reference's CurvePointCons surface (BASE, ZERO, Fp, Fn,
// fromAffine; curve.ts:159-195) that was registered with `register(c, curveId)`; points are
// instances of it (toAffine()).  Plain CommonJS + BigInt so it also loads on old Node.
const native = require('./noble_gpu.node');
const crypto = require('crypto');

const CURVE = { SECP256K1: 0, ED25519: 1, BLS12_381_G1: 2, BLS12_381_G2: 3, BN254_G1: 5 };
const registry = new Map();
let inited = false;
function init(device) { if (!inited) { native.init(device || 0); inited = true; } }
// one process, several GPUs: pippenger shards its points over `deviceIds` (ncg_msm_multi: one RCCL all-gather of
// window sums, combine on the first device); every other call runs on the first device
function initMulti(deviceIds) { if (!inited) { native.initMulti(deviceIds); inited = true; multiDevice = deviceIds.length > 1; } return deviceIds.length; }
function register(c, curveId) { registry.set(c, curveId); }

// BigInt <-> little-endian bytes through hex strings (utils.ts:498 numberToBytesLE / :456
// bytesToNumberLE use the same route): ~15x faster than shifting a BigInt byte by byte, and the
// marshalling is what an end-to-end call from JS spends its time in (SURVEY 8a gotcha 8).
function leBytes(n, len, out, off) {
  const be = Buffer.from(n.toString(16).padStart(2 * len, '0'), 'hex');
  for (let i = 0; i < len; i++) out[off + i] = be[len - 1 - i];
}
function leNumber(buf, off, len) {
  const be = Buffer.allocUnsafe(len);
  for (let i = 0; i < len; i++) be[i] = buf[off + len - 1 - i];
  return BigInt('0x' + be.toString('hex'));
}
function coordsOf(aff, isFp2) { return isFp2 ? [aff.x.c0, aff.x.c1, aff.y.c0, aff.y.c1] : [aff.x, aff.y]; }

// Field.isValid / isValidNot0 of the scalar field (modular.ts:925-936): a non-bigint is a TypeError, not `false`
function isValidScalar(Fn, s) {
  if (typeof s !== 'bigint') throw new TypeError('invalid field element: expected bigint, got ' + typeof s);
  return s >= 0n && s < Fn.ORDER;
}
function isValidScalarNot0(Fn, s) { return s !== 0n && isValidScalar(Fn, s); }
function validateMSMPoints(points, c) {         // curve.ts:390-395 (aarray: utils.ts:134-143)
  if (!Array.isArray(points)) throw new TypeError('"points" expected array, got type=' + typeof points);
  points.forEach((p, i) => { if (!(p instanceof c)) throw new Error('invalid point at index ' + i); });
}
function validateMSMScalars(scalars, field) {   // curve.ts:398-404
  if (!Array.isArray(scalars)) throw new Error('array of scalars expected');
  scalars.forEach((s, i) => { if (!isValidScalar(field, s)) throw new Error('invalid scalar at index ' + i); });
}
// Point.multiply / multiplyUnsafe argument errors: weierstrass.ts:904, :920; edwards.ts:561, :573
function scalarRangeError(id, not0) {
  if (id === CURVE.ED25519) return new RangeError('invalid scalar: expected ' + (not0 ? '1' : '0') + ' <= sc < curve.n');
  return new RangeError('invalid scalar: out of range');
}
// coordinates / scalars cross as packed little-endian bytes; the BigInt -> bytes step runs natively
// (napi_get_value_bigint_words), ~5x faster than the hex-string route it replaces
// Affine coordinates of every point with ONE field inversion (Montgomery's trick over Z, what the reference's own normalizeZ does,
// curve.ts:311-326): a point with Z != 1 - any result of add / double / multiplyUnsafe - costs p.toAffine() a BigInt inversion
// (~400 field products), 4 096 of them seconds.  Needs the reference's surface (p.Z, toAffine(invertedZ), Fp.mul / inv / eql / is0 /
// ONE: weierstrass.ts:768-790, edwards.ts:603-607); any other registered class, and arrays whose points all have Z = 1, take
// the plain path.
function affineAll(c, points) {
  const Fp = c.Fp, n = points.length;
  const plain = () => { const out = new Array(n); for (let i = 0; i < n; i++) out[i] = points[i].toAffine(); return out; };
  if (n < 2 || !Fp || typeof Fp.mul !== 'function' || typeof Fp.inv !== 'function' || typeof Fp.eql !== 'function' ||
      typeof Fp.is0 !== 'function' || Fp.ONE === undefined || points[0].Z === undefined) return plain();
  const pre = new Array(n);
  let acc = Fp.ONE, any = false;
  for (let i = 0; i < n; i++) {
    const z = points[i].Z;
    if (z === undefined || Fp.is0(z)) { pre[i] = undefined; continue; }   // ZERO: toAffine() answers by itself
    if (!any && !Fp.eql(z, Fp.ONE)) any = true;
    pre[i] = acc;
    acc = Fp.mul(acc, z);
  }
  if (!any) return plain();
  let inv = Fp.inv(acc);
  const out = new Array(n);
  for (let i = n - 1; i >= 0; i--) {
    if (pre[i] === undefined) { out[i] = points[i].toAffine(); continue; }
    out[i] = points[i].toAffine(Fp.mul(inv, pre[i]));
    inv = Fp.mul(inv, points[i].Z);
  }
  return out;
}
function marshalPoints(c, id, points) {
  const pb = native.pointBytes(id), isFp2 = id === CURVE.BLS12_381_G2, fb = pb / (isFp2 ? 4 : 2);
  const flat = new Array(points.length * (isFp2 ? 4 : 2));
  const aff = affineAll(c, points);
  let k = 0;
  for (let i = 0; i < aff.length; i++) {
    const a = aff[i];
    if (isFp2) { flat[k++] = a.x.c0; flat[k++] = a.x.c1; flat[k++] = a.y.c0; flat[k++] = a.y.c1; }
    else if (id === CURVE.ED25519) { flat[k++] = a.x % c.Fp.ORDER; flat[k++] = a.y % c.Fp.ORDER; }
    else { flat[k++] = a.x; flat[k++] = a.y; }
  }
  return native.packBigInts(flat, fb);
}
function marshalScalars(scalars) { return native.packBigInts(scalars, 32); }
function unmarshalPoint(c, id, buf, off, inf) {
  if (inf) return c.ZERO;
  const pb = native.pointBytes(id), isFp2 = id === CURVE.BLS12_381_G2, fb = pb / (isFp2 ? 4 : 2);
  const v = [];
  for (let j = 0; j < pb / fb; j++) v.push(leNumber(buf, off + j * fb, fb));
  return isFp2 ? c.fromAffine({ x: { c0: v[0], c1: v[1] }, y: { c0: v[2], c1: v[3] } }) : c.fromAffine({ x: v[0], y: v[1] });
}
// n points at the start of `out` (pb bytes each), their infinity flags at out[infOff + i]; `keep(i)` (optional) filters
function unmarshalPoints(c, id, out, n, infOff, keep) {
  const pb = native.pointBytes(id), isFp2 = id === CURVE.BLS12_381_G2, per = isFp2 ? 4 : 2, fb = pb / per;
  const v = native.unpackBigInts(out.subarray(0, n * pb), fb);     // all coordinates in one native call
  const res = new Array(n);
  for (let i = 0; i < n; i++) {
    if (keep && !keep(i)) { res[i] = null; continue; }
    if (out[infOff + i] === 1) { res[i] = c.ZERO; continue; }
    const o = i * per;
    res[i] = isFp2 ? c.fromAffine({ x: { c0: v[o], c1: v[o + 1] }, y: { c0: v[o + 2], c1: v[o + 3] } }) : c.fromAffine({ x: v[o], y: v[o + 1] });
  }
  return res;
}
function curveId(c) {
  const id = registry.get(c);
  if (id === undefined) throw new Error('noble-gpu: Point class not registered');
  return id;
}

// Packed columns (SURVEY 8a gotcha 8; VERDICT r02 #9): every BigInt that crosses N-API costs ~100 ns
// (napi_get_element + napi_get_value_bigint_words), i.e. 2^16 points + scalars = 196 608 values = most of an
// end-to-end pippenger.  Callers that keep their data in columns skip that entirely:
//   packPoints(c, points)  -> Uint8Array, affine x || y little-endian per point (the wire format of include/ncg.h;
//                             Fp2 as c0 || c1) - marshal ONCE, reuse across calls (or uploadPoints for a resident set)
//   packScalars(scalars)   -> Uint8Array, 32 bytes little-endian each; a BigUint64Array of 4 words per scalar is the
//                             same bytes on a little-endian host and is accepted as is
// pippenger / multiplyUnsafeBatch accept these in place of Point[] / BigInt[]; packed scalars are range-checked on the
// bytes (same 'invalid scalar at index i'), packed points are trusted like fromAffine trusts its caller.
function packPoints(c, points) { const id = curveId(c); validateMSMPoints(points, c); return marshalPoints(c, id, points); }
function packScalars(scalars, Fn) { if (Fn) validateMSMScalars(scalars, Fn); return marshalScalars(scalars); }
function asBytes(x) {
  if (x instanceof Uint8Array) return x;
  if (typeof BigUint64Array !== 'undefined' && x instanceof BigUint64Array) return new Uint8Array(x.buffer, x.byteOffset, x.byteLength);
  return null;
}
// ---- the same Point[] seen again: keep its device copy (VERDICT r04 #7; the reference's own advice for a fixed point set,
// curve.ts:907-918).  `pippenger(c, points, scalars)` with Point OBJECTS spends its time in points.map(toAffine) + BigInt
// packing (2^20 points: ~200 ms against 3.5 ms on the device).  The reference's instances are frozen (weierstrass.ts:703,
// edwards.ts:391) and its own precompute cache is keyed by object identity (curve.ts pointPrecomputes WeakMap), so the same
// rule is used here: an array whose elements are all frozen is uploaded ONCE as a resident set, remembered in a WeakMap keyed by
// the array together with a snapshot of its element references; a later call with the same array is a hit only if every
// element is still the identical object (one tight loop of === over the array, ~1 ns per point) - replacing, adding or removing
// an element is a miss and rebuilds the entry.  At most `maxSets` sets stay on the device (least recently used is freed).
const POINT_CACHE = { enabled: true, minPoints: 1024, maxSets: 4, requireDeepFrozen: false, hits: 0, misses: 0 };
const pointCache = new WeakMap();
let cacheLru = [];
let multiDevice = false;
function setPointCache(opts) { Object.assign(POINT_CACHE, opts || {}); if (!POINT_CACHE.enabled) clearPointCache(); return POINT_CACHE; }
function clearPointCache() { cacheLru.forEach((e) => e.set.free()); cacheLru = []; }
// a HIT only: the resident set of this very array (every element still the identical object), else null.  Nothing is validated,
// marshalled or uploaded here.
function cacheLookup(c, points) {
  if (!POINT_CACHE.enabled || multiDevice || points.length < POINT_CACHE.minPoints) return null;
  const e = pointCache.get(points);
  if (e === undefined) return null;
  if (e.set.handle !== null && e.c === c && e.snap.length === points.length) {
    const snap = e.snap, n = snap.length;
    let i = 0;
    while (i < n && snap[i] === points[i]) i++;
    if (i === n) {
      POINT_CACHE.hits++;
      if (cacheLru[cacheLru.length - 1] !== e) { cacheLru = cacheLru.filter((x) => x !== e); cacheLru.push(e); }
      return e.set;
    }
  }
  e.set.free(); cacheLru = cacheLru.filter((x) => x !== e); pointCache.delete(points);   // stale: the array changed
  return null;
}
// a MISS: upload `points` (already validated by the caller, AFTER the scalars and lengths were - ADVICE r05: a call that is about
// to throw must not pay an upload or leave a set resident) and remember the set.  Retention: the LRU list holds the entries
// strongly (the WeakMap alone would let the device memory outlive nothing, but the list keeps up to `maxSets` sets and a snapshot
// of their point references alive until they are evicted, `clearPointCache()` is called, or the array is seen changed).
// Only arrays of FROZEN instances are cached (the reference's classes: weierstrass.ts:703, edwards.ts:391).  The check is shallow: the
// Fp2 coordinates {c0, c1} of a G2 point are plain objects the reference never mutates (its field ops return new objects) but
// does not freeze either; `setPointCache({ requireDeepFrozen: true })` refuses such points unless their coordinates are frozen too.
function cacheInsert(c, id, points) {
  if (!POINT_CACHE.enabled || multiDevice || points.length < POINT_CACHE.minPoints) return null;
  const deep = POINT_CACHE.requireDeepFrozen;
  for (let i = 0; i < points.length; i++) {
    const p = points[i];
    if (!Object.isFrozen(p)) return null;   // mutable stand-in classes: never cached
    if (deep && p.X !== undefined && typeof p.X === 'object' && !(Object.isFrozen(p.X) && Object.isFrozen(p.Y) && Object.isFrozen(p.Z))) return null;
  }
  POINT_CACHE.misses++;
  init();
  const set = new PointSet(c, id, native.uploadPoints(id, marshalPoints(c, id, points), false, false), points.length);
  const e = { c, snap: points.slice(), set };
  pointCache.set(points, e);
  cacheLru.push(e);
  while (cacheLru.length > POINT_CACHE.maxSets) cacheLru.shift().set.free();
  return set;
}
function msmCall(c, id, points, pBytes, scalars, sBytes, set) {
  init();
  const out = set !== null ? native.msmResident(set.handle, sBytes === null ? scalars : sBytes)
    : native.msm(id, pBytes === null ? marshalPoints(c, id, points) : pBytes, sBytes === null ? marshalScalars(scalars) : sBytes);
  return unmarshalPoint(c, id, out, 0, out[out.length - 1] === 1);
}
function pippenger(c, points, scalars) {
  const id = curveId(c);
  const pb = native.pointBytes(id);
  const pBytes = asBytes(points), sBytes = asBytes(scalars);
  // argument checks in the reference's order (curve.ts:871-875): points, scalars, lengths - all of them before anything is uploaded
  let set = pBytes === null && Array.isArray(points) ? cacheLookup(c, points) : null;    // a hit is an array validated before
  if (pBytes === null) { if (set === null) validateMSMPoints(points, c); }
  else if (pBytes.length % pb) throw new Error('noble-gpu: packed points: expected a multiple of ' + pb + ' bytes');
  if (sBytes === null) validateMSMScalars(scalars, c.Fn);
  else if (sBytes.length % 32) throw new Error('array of scalars expected');
  const np = pBytes === null ? points.length : pBytes.length / pb, ns = sBytes === null ? scalars.length : sBytes.length / 32;
  if (np !== ns) throw new Error('arrays of points and scalars must have equal length');
  if (sBytes !== null) checkPackedScalars(sBytes, c.Fn);
  if (np === 0) return c.ZERO;      // curve.ts:878
  if (set === null && pBytes === null) set = cacheInsert(c, id, points);
  return msmCall(c, id, points, pBytes, scalars, sBytes, set);
}
// ---- the REDIRECT (VERDICT r05 #2; SURVEY 8b "switches to GPU above a size threshold"): with the 12-line patch of INTEGRATION.md in
// src/abstract/curve.ts, the reference's own `pippenger` export hands every call with at least `minPoints` points to the backend
// registered for the Point class - AFTER its own argument checks and its empty-input return - and runs its own loop below that.
//     gpu.install(await import('@noble/curves/abstract/curve.js'), [secp256k1.Point, bls12_381.G1.Point, ...], { minPoints })
// Every caller of the reference's export (its tests, its benchmarks, bls.ts, user code) then runs on the GPU unchanged.
// DEFAULT_MIN_POINTS: the measured crossover of the reference's loop against one redirected call from Point objects
// (profiles/r06_js_threshold.json; EPYC 9575F + MI355X, marshalling included) lies BELOW one point: the reference's loop runs
// ~(Fn.BITS / w) (n + 2^w) BigInt point additions - 4.8 ms (secp256k1) / 2.5 (ed25519) / 5.1 (G1) / 19.3 ms (G2) for ONE point,
// 87 / 52 / 108 / 384 ms for 256 - against 0.20 / 0.21 / 0.25 / 0.37 ms and 0.41 / 0.50 / 0.62 / 1.02 ms redirected.  So the
// default redirects every non-empty call; `minPoints` stays the caller's knob (a process that must not touch the device for
// small inputs, a GPU shared with other work).
const DEFAULT_MIN_POINTS = 1;
const STATS = { msmRedirected: 0, msmPointsRedirected: 0 };
function redirectedMsm(c, points, scalars) {      // arguments already validated by the reference (curve.ts:871-878)
  const id = curveId(c);
  STATS.msmRedirected++;
  STATS.msmPointsRedirected += points.length;
  let set = cacheLookup(c, points);
  if (set === null) set = cacheInsert(c, id, points);
  return msmCall(c, id, points, null, scalars, null, set);
}
function install(curveModule, classes, opts) {
  if (!curveModule || typeof curveModule.setMSMBackend !== 'function')
    throw new Error('noble-gpu: install: this abstract/curve.js has no setMSMBackend (apply the patch of INTEGRATION.md)');
  const minPoints = opts && opts.minPoints !== undefined ? opts.minPoints : DEFAULT_MIN_POINTS;
  if (!Number.isSafeInteger(minPoints) || minPoints < 1) throw new Error('noble-gpu: install: minPoints must be a positive integer');
  for (const c of classes) { curveId(c); curveModule.setMSMBackend(c, { minPoints, msm: redirectedMsm }); }
  return minPoints;
}
function uninstall(curveModule, classes) { for (const c of classes) curveModule.setMSMBackend(c, undefined); }
// ---- resident point sets (interleavedMSMUnsafe's pattern, curve.ts:907-959): upload once, then only the
// scalars cross per call.  `scalars` may be a BigInt[] (validated like the reference, read natively as
// 64-bit words) or a Uint8Array of packed 32-byte little-endian values (no marshalling at all).
class PointSet {
  constructor(c, id, handle, length) { this.c = c; this.id = id; this.handle = handle; this.length = length; }
  free() { if (this.handle !== null) { native.freePoints(this.handle); this.handle = null; } }
  // bls12-381: every point is known to be torsion-free (decoded by fromBytes, or verified at upload): pippengerResident
  // then splits the scalars along the curve endomorphism - same result, half (G1) / a quarter (G2) of the windows
  get inSubgroup() { return this.handle !== null && native.inSubgroup(this.handle); }
}
// opts.checkSubgroup (bls12-381): run p.isTorsionFree() (bls12-381.ts:567-577, :599-601) on every point once, on the
// device; pippenger accepts points outside the subgroup, so a set holding one simply keeps the generic path
function uploadPoints(c, points, opts) {
  const id = curveId(c);
  validateMSMPoints(points, c);
  init();
  const set = new PointSet(c, id, native.uploadPoints(id, marshalPoints(c, id, points), false, false), points.length);
  if (opts && opts.checkSubgroup && (id === CURVE.BLS12_381_G1 || id === CURVE.BLS12_381_G2) && points.length) native.verifySubgroup(set.handle);
  return set;
}
function uploadEncoded(c, bytes, zip215) {      // concatenated compressed encodings; decoded + validated on the device
  const id = curveId(c);
  init();
  const eb = { 0: 33, 1: 32, 2: 48, 3: 96 }[id];
  if (!(bytes instanceof Uint8Array) || bytes.length % eb) throw new Error('noble-gpu: expected a Uint8Array of ' + eb + '-byte encodings');
  return new PointSet(c, id, native.uploadPoints(id, bytes, true, !!zip215), bytes.length / eb);
}
// packed scalars (32 bytes little-endian each) must satisfy the same rule as BigInt ones: 0 <= s < Fn.ORDER
// (validateMSMScalars, curve.ts:398-404 / 'invalid scalar: out of range', weierstrass.ts:920) - checked here, on
// the bytes, so that no entry point can reach the device with an unreduced scalar
function checkPackedScalars(bytes, Fn) {
  const order = Fn.ORDER;
  const ob = new Uint8Array(32);
  for (let i = 0, v = order; i < 32; i++, v >>= 8n) ob[i] = Number(v & 0xffn);
  const n = bytes.length >>> 5;
  // fast path: the top 32-bit word decides for all but ~2^-32 of the scalars of a full-width order
  const top = ((ob[31] << 24) | (ob[30] << 16) | (ob[29] << 8) | ob[28]) >>> 0;
  const u32 = (bytes.byteOffset & 3) === 0 ? new Uint32Array(bytes.buffer, bytes.byteOffset, bytes.length >>> 2) : null;
  for (let i = 0; i < n; i++) {
    if (u32 !== null && u32[8 * i + 7] < top) continue;
    const o = i << 5;
    let k = 31;
    while (k >= 0 && bytes[o + k] === ob[k]) k--;
    if (k < 0 || bytes[o + k] > ob[k]) throw new Error('invalid scalar at index ' + i);
  }
}
function residentScalars(set, scalars) {
  if (scalars instanceof Uint8Array) {
    if (scalars.length !== 32 * set.length) throw new Error('arrays of points and scalars must have equal length');
    checkPackedScalars(scalars, set.c.Fn);
    return scalars;
  }
  validateMSMScalars(scalars, set.c.Fn);
  if (scalars.length !== set.length) throw new Error('arrays of points and scalars must have equal length');
  return scalars;
}
function pippengerResident(set, scalars) {
  const sc = residentScalars(set, scalars);
  if (set.length === 0) return set.c.ZERO;
  const out = native.msmResident(set.handle, sc);
  return unmarshalPoint(set.c, set.id, out, 0, out[out.length - 1] === 1);
}
function multiplyUnsafeBatchResident(set, scalars) {
  const sc = residentScalars(set, scalars);
  if (set.length === 0) return [];
  const n = set.length, pb = native.pointBytes(set.id);
  const out = native.mulVarResident(set.handle, sc);
  return unmarshalPoints(set.c, set.id, out, n, n * pb);
}
// interleavedMSMUnsafe (curve.ts:938-959): MSM over a FIXED point set, returns the closure scalars -> Point.
// Same argument checks and messages; the closure accepts at most points.length scalars, omitted trailing ones
// are zero.  windowSize only sizes the reference's wNAF tables and never changes the result: here the set
// is uploaded once and each call runs the bucket MSM on the resident points.
function interleavedMSMUnsafe(c, points, windowSize) {
  const bits = c.Fn.BITS;
  if (!Number.isSafeInteger(windowSize) || windowSize < 2 || windowSize > bits)
    throw new Error('invalid window size, expected [2..' + bits + '], got W=' + windowSize);
  validateMSMPoints(points, c);
  const n = points.length;
  const set = n ? uploadPoints(c, points) : null;
  if (set) native.precomputePoints(set.handle);   // the reference builds its per-point tables here (curve.ts:948)
  return (scalars) => {
    validateMSMScalars(scalars, c.Fn);
    if (scalars.length > n) throw new Error('array of scalars must not be larger than array of points');
    if (n === 0) return c.ZERO;
    const padded = scalars.length === n ? scalars : scalars.concat(new Array(n - scalars.length).fill(0n));
    const out = native.msmResident(set.handle, padded);
    return unmarshalPoint(c, set.id, out, 0, out[out.length - 1] === 1);
  };
}
// eddsa.verify for a batch from (sig, msg, publicKey): the SHA-512 challenge is computed on the device
function ed25519VerifyBatchDevice(items, zip215) {
  const n = items.length;
  if (n === 0) return [];
  let total = 0;
  items.forEach((it) => { total += it.msg.length; });
  const sig = new Uint8Array(64 * n), pk = new Uint8Array(32 * n), msgs = new Uint8Array(total), offs = new Uint8Array(8 * (n + 1));
  const dv = new DataView(offs.buffer);
  let pos = 0;
  items.forEach((it, i) => {
    if (it.sig.length !== 64) throw new Error('"signature" expected Uint8Array of length 64');
    if (it.publicKey.length !== 32) throw new Error('"publicKey" expected Uint8Array of length 32');
    sig.set(it.sig, 64 * i); pk.set(it.publicKey, 32 * i); msgs.set(it.msg, pos);
    dv.setUint32(8 * i, pos % 4294967296, true); dv.setUint32(8 * i + 4, Math.floor(pos / 4294967296), true);
    pos += it.msg.length;
  });
  dv.setUint32(8 * n, pos % 4294967296, true); dv.setUint32(8 * n + 4, Math.floor(pos / 4294967296), true);
  init();
  return Array.from(native.ed25519VerifyMsgs(sig, pk, msgs, offs, zip215 !== false)).map((x) => x === 1);
}

// secp256k1.verify(sig, msgHash, publicKey, { prehash: false, lowS }) for a batch (weierstrass.ts:1571-1620): compact
// 64-byte signatures, 32-byte message hashes (hash with the reference's own sha256 first for prehash: true), 33-byte
// compressed keys; key decompression, s^-1 mod n, u1 G + u2 P and the comparison run on the device
function ecdsaVerifyBatch(items, lowS) {
  const n = items.length;
  if (n === 0) return [];
  const sig = new Uint8Array(64 * n), hs = new Uint8Array(32 * n), pk = new Uint8Array(33 * n);
  const live = new Array(n).fill(true);
  items.forEach((it, i) => {
    if (!(it.sig instanceof Uint8Array) || it.sig.length !== 64) throw new Error('"signature" expected Uint8Array of length 64');
    if (!(it.msgHash instanceof Uint8Array) || it.msgHash.length !== 32) throw new Error('"msgHash" expected Uint8Array of length 32');
    if (!(it.publicKey instanceof Uint8Array)) throw new Error('"publicKey" expected Uint8Array');
    if (it.publicKey.length !== 33) { live[i] = false; pk[33 * i] = 2; return; }   // other encodings: compress them first
    sig.set(it.sig, 64 * i); hs.set(it.msgHash, 32 * i); pk.set(it.publicKey, 33 * i);
  });
  init();
  return Array.from(native.ecdsaVerify(sig, hs, pk, lowS !== false)).map((x, i) => live[i] && x === 1);
}

function packMsgs(items, n) {
  let total = 0;
  items.forEach((it) => { total += it.msg.length; });
  const msgs = new Uint8Array(total), offs = new Uint8Array(8 * (n + 1));
  const dv = new DataView(offs.buffer);
  let pos = 0;
  items.forEach((it, i) => {
    if (!(it.msg instanceof Uint8Array)) throw new Error('"message" expected Uint8Array');
    msgs.set(it.msg, pos);
    dv.setUint32(8 * i, pos % 4294967296, true); dv.setUint32(8 * i + 4, Math.floor(pos / 4294967296), true);
    pos += it.msg.length;
  });
  dv.setUint32(8 * n, pos % 4294967296, true); dv.setUint32(8 * n + 4, Math.floor(pos / 4294967296), true);
  return [msgs, offs];
}
// secp256k1.verify(sig, msg, publicKey, { lowS }) with the default prehash for a batch: SHA-256 of every message, key
// handling (all keys 33-byte compressed or all 65-byte uncompressed) and the verification run on the device
function ecdsaVerifyBatchMsgs(items, lowS) {
  const n = items.length;
  if (n === 0) return [];
  const kb = items[0].publicKey.length;
  if (kb !== 33 && kb !== 65) throw new Error('noble-gpu: ecdsaVerifyBatchMsgs: 33- or 65-byte public keys');
  const sig = new Uint8Array(64 * n), pk = new Uint8Array(kb * n);
  items.forEach((it, i) => {
    if (!(it.sig instanceof Uint8Array) || it.sig.length !== 64) throw new Error('"signature" expected Uint8Array of length 64');
    if (!(it.publicKey instanceof Uint8Array) || it.publicKey.length !== kb) throw new Error('noble-gpu: ecdsaVerifyBatchMsgs: mixed public-key lengths');
    sig.set(it.sig, 64 * i); pk.set(it.publicKey, kb * i);
  });
  const [msgs, offs] = packMsgs(items, n);
  init();
  return Array.from(native.secpVerifyMsgs(0, sig, pk, msgs, offs, lowS !== false)).map((x) => x === 1);
}
// schnorr.verify(sig, msg, publicKey) (src/secp256k1.ts:228-258) for a batch, tagged challenge hash on the device
function schnorrVerifyBatch(items) {
  const n = items.length;
  if (n === 0) return [];
  const sig = new Uint8Array(64 * n), pk = new Uint8Array(32 * n);
  items.forEach((it, i) => {
    if (!(it.sig instanceof Uint8Array) || it.sig.length !== 64) throw new Error('"signature" expected Uint8Array of length 64');
    if (!(it.publicKey instanceof Uint8Array) || it.publicKey.length !== 32) throw new Error('"publicKey" expected Uint8Array of length 32');
    sig.set(it.sig, 64 * i); pk.set(it.publicKey, 32 * i);
  });
  const [msgs, offs] = packMsgs(items, n);
  init();
  return Array.from(native.secpVerifyMsgs(1, sig, pk, msgs, offs, true)).map((x) => x === 1);
}
// recoverPublicKey for a batch of { sig (65 bytes: recovery id || r || s), msgHash (32 bytes) }: compressed keys, null
// where the reference throws
function ecdsaRecoverBatch(items) {
  const n = items.length;
  if (n === 0) return [];
  const sig = new Uint8Array(65 * n), hs = new Uint8Array(32 * n);
  items.forEach((it, i) => {
    if (!(it.sig instanceof Uint8Array) || it.sig.length !== 65) throw new Error('"signature" expected Uint8Array of length 65');
    if (!(it.msgHash instanceof Uint8Array) || it.msgHash.length !== 32) throw new Error('"msgHash" expected Uint8Array of length 32');
    sig.set(it.sig, 65 * i); hs.set(it.msgHash, 32 * i);
  });
  init();
  const out = native.ecdsaRecover(sig, hs);
  return items.map((_, i) => (out[33 * n + i] === 1 ? out.slice(33 * i, 33 * i + 33) : null));
}

function multiplyUnsafeBatch(c, points, scalars) {
  const id = curveId(c);
  validateMSMPoints(points, c);
  if (points.length !== scalars.length) throw new Error('arrays of points and scalars must have equal length');
  scalars.forEach((s) => { if (!isValidScalar(c.Fn, s)) throw scalarRangeError(id, false); });   // weierstrass.ts:920, edwards.ts:573
  if (points.length === 0) return [];
  init();
  const n = points.length, pb = native.pointBytes(id);
  const out = native.mulVarBatch(id, marshalPoints(c, id, points), marshalScalars(scalars));
  return unmarshalPoints(c, id, out, n, n * pb);
}
function multiplyBaseBatch(c, scalars) {
  const id = curveId(c);
  scalars.forEach((s) => { if (!isValidScalarNot0(c.Fn, s)) throw scalarRangeError(id, true); });   // weierstrass.ts:904, edwards.ts:561
  if (id === CURVE.ED25519) return multiplyUnsafeBatch(c, scalars.map(() => c.BASE), scalars);
  if (scalars.length === 0) return [];
  init();
  const n = scalars.length, pb = native.pointBytes(id);
  const out = native.mulBaseBatch(id, marshalScalars(scalars));
  return unmarshalPoints(c, id, out, n, n * pb);
}
const ED_L = 0x1000000000000000000000000000000014def9dea2f79cd65812631a5cf5d3edn;
function ed25519VerifyBatch(items, zip215) {   // items: [{sig, msg, publicKey}] of Uint8Array
  const n = items.length;
  const sig = new Uint8Array(64 * n), pk = new Uint8Array(32 * n), ks = new Uint8Array(32 * n);
  items.forEach((it, i) => {
    if (it.sig.length !== 64) throw new Error('"signature" expected Uint8Array of length 64');
    if (it.publicKey.length !== 32) throw new Error('"publicKey" expected Uint8Array of length 32');
    sig.set(it.sig, 64 * i); pk.set(it.publicKey, 32 * i);
    const h = crypto.createHash('sha512');     // edwards.ts:900-906 (SHA-512 is @noble/hashes in the reference)
    h.update(it.sig.subarray(0, 32)); h.update(it.publicKey); h.update(it.msg);
    leBytes(leNumber(h.digest(), 0, 64) % ED_L, 32, ks, 32 * i);
  });
  if (n === 0) return [];
  init();
  return Array.from(native.ed25519VerifyBatch(sig, pk, ks, zip215 !== false)).map((x) => x === 1);
}

// ---- X25519 (abstract/montgomery.ts:247-420, ed25519.ts:266-292) and ed25519.utils.toMontgomery (ed25519.ts:128-134) ----------
// Batch forms return arrays of Uint8Array | null: null where the reference throws.  The single-item helpers throw its message.
const X25519_INVALID = 'invalid private or public key received';
function abytes32(b, title) {                   // utils abytes(value, 32, title)
  const bytes = b instanceof Uint8Array;
  if (!bytes || b.length !== 32)
    throw new Error((title && `"${title}" `) + 'expected Uint8Array of length 32, got ' + (bytes ? `length=${b.length}` : `type=${typeof b}`));
  return b;
}
function x25519Rows(packed, n) {
  const out = new Array(n);
  for (let i = 0; i < n; i++) out[i] = packed[32 * n + i] === 1 ? packed.slice(32 * i, 32 * i + 32) : null;
  return out;
}
// items: [{scalar, u}] - or {scalar, us}: ONE secret against many peer keys (the secret crosses once).  The u coordinate of a row is
// checked before its scalar (montgomery.ts:324-326).
function x25519ScalarMultBatch(items) {
  const one = !Array.isArray(items);
  const us = one ? items.us : items.map((it) => it.u);
  const n = us.length;
  const U = new Uint8Array(32 * n), S = new Uint8Array(one ? 32 : 32 * n);
  for (let i = 0; i < n; i++) {
    U.set(abytes32(us[i], 'uCoordinate'), 32 * i);
    if (!one) S.set(abytes32(items[i].scalar, 'scalar'), 32 * i);
  }
  if (one) S.set(abytes32(items.scalar, 'scalar'), 0);
  if (n === 0) return [];
  init();
  // (the native call tells the two forms apart by the length of S; for n = 1 they are the same call)
  return x25519Rows(native.x25519(0, S, U), n);
}
function x25519GetPublicKeyBatch(secretKeys) {
  const n = secretKeys.length, S = new Uint8Array(32 * n);
  secretKeys.forEach((k, i) => S.set(abytes32(k, 'scalar'), 32 * i));
  if (n === 0) return [];
  init();
  return x25519Rows(native.x25519(1, null, S), n);
}
function ed25519ToMontgomeryBatch(publicKeys) {
  const n = publicKeys.length, K = new Uint8Array(32 * n);
  publicKeys.forEach((k, i) => K.set(abytes32(k, 'point'), 32 * i));
  if (n === 0) return [];
  init();
  return x25519Rows(native.x25519(2, null, K), n);
}
// ---- Ed25519 signing (abstract/edwards.ts:870-930, ed25519.ts:146-223): getPublicKey and sign for ed25519 / ed25519ctx / ed25519ph.
// Both hashes, the two fixed-base multiplications and the scalar arithmetic run on the device; only the domain prefix is built here.
// opts.context: a Uint8Array selects ed25519ctx (even an empty one - pass nothing for plain ed25519); opts.prehash: true selects
// ed25519ph.  Batch forms return null for a row the device refused (r = 0 mod L); the single-item forms throw the reference's messages.
function ed25519Dom(opts) {                     // ed25519_domain (ed25519.ts:148-160); plain ed25519 has no prefix (edwards.ts:857-862)
  const prehash = !!(opts && opts.prehash), has = !!(opts && opts.context !== undefined), domain = has || prehash;
  const ctx = has ? opts.context : new Uint8Array(0);
  if (!(ctx instanceof Uint8Array)) throw new Error('"context" expected Uint8Array, got type=' + typeof ctx);
  if (!domain) return { dom: new Uint8Array(0), flags: 0 };
  if (ctx.length > 255) throw new Error('Context is too big');
  const dom = new Uint8Array(34 + ctx.length);
  dom.set(Buffer.from('SigEd25519 no Ed25519 collisions', 'ascii'), 0);
  dom[32] = prehash ? 1 : 0;
  dom[33] = ctx.length;
  dom.set(ctx, 34);
  return { dom, flags: prehash ? 4 : 0 };
}
function ed25519GetPublicKeyBatch(secretKeys) {
  const n = secretKeys.length, S = new Uint8Array(32 * n);
  secretKeys.forEach((k, i) => S.set(abytes32(k, 'secretKey'), 32 * i));
  if (n === 0) return [];
  init();
  const out = native.ed25519Sign(0, S);
  S.fill(0);
  return Array.from({ length: n }, (_, i) => out.slice(32 * i, 32 * i + 32));
}
// items: [{msg, secretKey}] - or {msgs, secretKey}: ONE key signing many messages (the key crosses once)
function ed25519SignBatch(items, opts) {
  const { dom, flags } = ed25519Dom(opts);
  const one = !Array.isArray(items);
  const msgs = one ? items.msgs : items.map((it) => it.msg);
  const n = msgs.length;
  const K = new Uint8Array(one ? 32 : 32 * n), lens = new Uint8Array(4 * n), view = new DataView(lens.buffer);
  let total = 0;
  for (let i = 0; i < n; i++) {
    const m = msgs[i];
    if (!(m instanceof Uint8Array)) throw new Error('"message" expected Uint8Array, got type=' + typeof m);
    if (!one) K.set(abytes32(items[i].secretKey, 'secretKey'), 32 * i);
    view.setUint32(4 * i, m.length, true);
    total += m.length;
  }
  if (one) K.set(abytes32(items.secretKey, 'secretKey'), 0);
  if (n === 0) return [];
  const blob = new Uint8Array(total);
  for (let i = 0, at = 0; i < n; at += msgs[i++].length) blob.set(msgs[i], at);
  init();
  const out = native.ed25519Sign(1, K, flags, dom, blob, lens);
  K.fill(0);
  return Array.from({ length: n }, (_, i) => (out[64 * n + i] === 1 ? out.slice(64 * i, 64 * i + 64) : null));
}
function ed25519GetPublicKey(secretKey) { return ed25519GetPublicKeyBatch([secretKey])[0]; }
function ed25519Sign(msg, secretKey, opts) {
  const r = ed25519SignBatch([{ msg, secretKey }], opts)[0];
  if (r === null) throw new Error('invalid scalar: expected 1 <= sc < curve.n');   // BASE.multiply(0), edwards.ts:920-924
  return r;
}

// ---- secp256k1 signing (abstract/weierstrass.ts:1480-1568, secp256k1.ts:147-221): getPublicKey, ECDSA sign with RFC 6979 nonces and
// BIP-340 sign.  The DRBG, every hash, the fixed-base multiplications and the scalar arithmetic run on the device; DER is encoded here.
// Batch forms return null for a row the device refused; the single-item forms throw the reference's messages.
const SECP_N = BigInt('0xfffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141');
function secpKeyRows(keys, check) {             // the keys packed into one array; nothing of them is left behind when a check throws
  const S = new Uint8Array(32 * keys.length);
  try {
    keys.forEach((k, i) => S.set(check(k), 32 * i));
  } catch (e) {
    S.fill(0);
    throw e;
  }
  return S;
}
function fnBytes32(b) {                        // Fn.fromBytes of the ECDSA side: its own message for a wrong length
  if (!(b instanceof Uint8Array)) throw new Error('"secretKey" expected Uint8Array, got type=' + typeof b);
  if (b.length !== 32) throw new Error('Field.fromBytes: expected 32 bytes, got ' + b.length);
  return b;
}
function secpRefusedKey(sk, zeroMessage) {     // the reference's message for a key outside [1, n), null for a key in range
  const d = BigInt('0x' + Buffer.from(sk).toString('hex'));
  if (d === BigInt(0)) return zeroMessage;
  return d >= SECP_N ? 'invalid field element: outside of range 0..ORDER' : null;
}
function secpPublicKeys(secretKeys, mode, check) {
  const n = secretKeys.length, w = mode === 1 ? 65 : mode === 2 ? 32 : 33;
  const S = secpKeyRows(secretKeys, check);
  if (n === 0) return [];
  let out;
  try {
    init();
    out = native.secpSign(0, S, mode);
  } finally {
    S.fill(0);
  }
  return Array.from({ length: n }, (_, i) => (out[w * n + i] === 1 ? out.slice(w * i, w * i + w) : null));
}
function secp256k1GetPublicKeyBatch(secretKeys, isCompressed) {
  return secpPublicKeys(secretKeys, isCompressed === false ? 1 : 0, fnBytes32);
}
function schnorrGetPublicKeyBatch(secretKeys) { return secpPublicKeys(secretKeys, 2, (k) => abytes32(k, 'secretKey')); }
function secpPackMsgs(msgs) {
  const n = msgs.length, lens = new Uint8Array(4 * n), view = new DataView(lens.buffer);
  let total = 0;
  msgs.forEach((m, i) => {
    if (!(m instanceof Uint8Array)) throw new Error('"message" expected Uint8Array, got type=' + typeof m);
    view.setUint32(4 * i, m.length, true);
    total += m.length;
  });
  const blob = new Uint8Array(total);
  for (let i = 0, at = 0; i < n; at += msgs[i++].length) blob.set(msgs[i], at);
  return { blob, lens };
}
function derOfCompact(sig) {                   // DER.hexFromSig: SEQUENCE of two minimal positive INTEGERs
  const int = (b) => {
    let i = 0;
    while (i < 31 && b[i] === 0) i++;
    const body = b[i] & 0x80 ? [0, ...b.slice(i)] : [...b.slice(i)];
    return [2, body.length, ...body];
  };
  const body = [...int(sig.slice(0, 32)), ...int(sig.slice(32, 64))];
  return Uint8Array.from([0x30, body.length, ...body]);
}
// items: [{msg, secretKey[, extraEntropy]}] - or {msgs, secretKey}: ONE key signing many messages (the key crosses once).
// opts: lowS (true), prehash (true), format 'compact' | 'recovered' | 'der', extraEntropy: true draws 32 random bytes per row (a per-row
// extraEntropy of an item wins); only 32-byte extra entropy is offered in batch.
function ecdsaSignBatch(items, opts) {
  const o = Object.assign({ lowS: true, prehash: true, format: 'compact', extraEntropy: false }, opts || {});
  if (!['compact', 'recovered', 'der'].includes(o.format)) throw new Error('Signature format must be "compact", "recovered", or "der"');
  const one = !Array.isArray(items);
  const msgs = one ? items.msgs : items.map((it) => it.msg);
  const n = msgs.length;
  msgs.forEach((m) => { if (!(m instanceof Uint8Array)) throw new Error('"message" expected Uint8Array, got type=' + typeof m); });
  const K = secpKeyRows(one ? [items.secretKey] : items.map((it) => it.secretKey), fnBytes32);
  let X = new Uint8Array(0), out;
  try {                                           // the packed keys and extra entropy are zeroed on every way out
    const perRow = !one && items.some((it) => it.extraEntropy !== undefined && it.extraEntropy !== false);
    if (perRow || o.extraEntropy === true) {
      X = new Uint8Array(32 * n);
      for (let i = 0; i < n; i++) {
        const e = !one && items[i].extraEntropy instanceof Uint8Array ? items[i].extraEntropy : require('crypto').randomBytes(32);
        if (e.length !== 32) throw new Error('noble-gpu: only 32-byte extra entropy is offered in batch');
        X.set(e, 32 * i);
      }
    } else if (o.extraEntropy) throw new Error('noble-gpu: only 32-byte extra entropy is offered in batch');
    if (n === 0) return [];
    init();
    if (o.prehash) {
      const { blob, lens } = secpPackMsgs(msgs);
      out = native.secpSign(1, K, o.lowS ? 1 : 0, blob, lens, X);
    } else {
      const H = new Uint8Array(32 * n);           // bits2int keeps the leading 32 bytes; a shorter message is left-padded
      msgs.forEach((m, i) => {
        if (m.length > 8192) throw new Error('input is too large');
        if (m.length >= 32) H.set(m.slice(0, 32), 32 * i);
        else H.set(m, 32 * i + 32 - m.length);
      });
      out = native.secpSign(1, K, o.lowS ? 1 : 0, H, new Uint8Array(0), X);
    }
  } finally {
    K.fill(0);
    X.fill(0);
  }
  return Array.from({ length: n }, (_, i) => {
    if (out[65 * n + i] !== 1) return null;
    const sig = out.slice(64 * i, 64 * i + 64);
    if (o.format === 'der') return derOfCompact(sig);
    if (o.format === 'recovered') return Uint8Array.from([out[64 * n + i], ...sig]);
    return sig;
  });
}
// items: [{msg, secretKey[, auxRand]}]: auxRand defaults to 32 fresh random bytes, as in the reference
function schnorrSignBatch(items) {
  const n = items.length;
  const K = secpKeyRows(items.map((it) => it.secretKey), (k) => abytes32(k, 'secretKey'));
  const A = new Uint8Array(32 * n);
  let out;
  try {                                           // the packed keys and aux rows are zeroed on every way out
    items.forEach((it, i) => A.set(it.auxRand === undefined ? require('crypto').randomBytes(32) : abytes32(it.auxRand, 'auxRand'), 32 * i));
    const { blob, lens } = secpPackMsgs(items.map((it) => it.msg));
    if (n === 0) return [];
    init();
    out = native.secpSign(2, K, 0, blob, lens, A);
  } finally {
    K.fill(0);
    A.fill(0);
  }
  return Array.from({ length: n }, (_, i) => (out[64 * n + i] === 1 ? out.slice(64 * i, 64 * i + 64) : null));
}
function secp256k1GetPublicKey(secretKey, isCompressed) {
  const r = secp256k1GetPublicKeyBatch([secretKey], isCompressed)[0];
  if (r === null) throw new Error(secpRefusedKey(secretKey, 'invalid scalar: out of range'));
  return r;
}
function schnorrGetPublicKey(secretKey) {
  const r = schnorrGetPublicKeyBatch([secretKey])[0];
  if (r === null) throw new Error(secpRefusedKey(secretKey, 'invalid scalar: out of range'));
  return r;
}
function secp256k1Sign(msg, secretKey, opts) {
  const item = { msg, secretKey };
  if (opts && opts.extraEntropy instanceof Uint8Array) item.extraEntropy = opts.extraEntropy;
  const r = ecdsaSignBatch([item], opts)[0];
  if (r === null) throw new Error(secpRefusedKey(secretKey, 'invalid private key') || 'drbg: tried max amount of iterations');
  return r;
}
function schnorrSign(msg, secretKey, auxRand) {
  const r = schnorrSignBatch([{ msg, secretKey, auxRand }])[0];
  if (r === null) throw new Error(secpRefusedKey(secretKey, 'invalid scalar: out of range') || 'sign failed: k is zero');
  if (!schnorrVerifyBatch([{ sig: r, msg, publicKey: schnorrGetPublicKey(secretKey) }])[0]) throw new Error('sign: Invalid signature produced');
  return r;
}

// ---- X448 and Ed448 verification (ed448.ts; abstract/montgomery.ts:247-420, abstract/edwards.ts:942-989) ----------------------
// The same buffers-in / buffers-out convention as the X25519 calls.  ed448VerifyBatch hashes on the host by default: the challenge
// k = SHAKE256(dom4(phflag, context) || R || A || PH(M), 114) mod n and the ed448ph prehash use crypto.createHash('shake256');
// opts.deviceHash: true sends the messages and the domain prefix to the device instead (ncg_ed448_verify_batch_msgs).
function abytesT(b, len, title) {               // utils abytes(value, length | undefined, title)
  const bytes = b instanceof Uint8Array;
  if (!bytes || (len !== undefined && b.length !== len))
    throw new Error(`"${title}" expected Uint8Array` + (len !== undefined ? ' of length ' + len : '') + ', got ' +
                    (bytes ? `length=${b.length}` : `type=${typeof b}`));
  return b;
}
function x448Rows(packed, n) {
  const out = new Array(n);
  for (let i = 0; i < n; i++) out[i] = packed[56 * n + i] === 1 ? packed.slice(56 * i, 56 * i + 56) : null;
  return out;
}
// items: [{scalar, u}] - or {scalar, us}: ONE secret against many peer keys.  The u coordinate of a row is checked before its scalar.
function x448ScalarMultBatch(items) {
  const one = !Array.isArray(items);
  const us = one ? items.us : items.map((it) => it.u);
  const n = us.length;
  const U = new Uint8Array(56 * n), S = new Uint8Array(one ? 56 : 56 * n);
  for (let i = 0; i < n; i++) {
    U.set(abytesT(us[i], 56, 'uCoordinate'), 56 * i);
    if (!one) S.set(abytesT(items[i].scalar, 56, 'scalar'), 56 * i);
  }
  if (one) S.set(abytesT(items.scalar, 56, 'scalar'), 0);
  if (n === 0) return [];
  init();
  return x448Rows(native.ed448(0, S, U), n);
}
function x448GetPublicKeyBatch(secretKeys) {
  const n = secretKeys.length, S = new Uint8Array(56 * n);
  secretKeys.forEach((k, i) => S.set(abytesT(k, 56, 'scalar'), 56 * i));
  if (n === 0) return [];
  init();
  return x448Rows(native.ed448(1, null, S), n);
}
const ED448_N = (1n << 446n) - 13818066809895115352007386748515426880336692474882178609894547503885n;
const ED448_P = (1n << 448n) - (1n << 224n) - 1n;
function ed448Decodes(enc) {                    // whether Point.fromBytes (strict) accepts the 57 bytes
  if (enc[56] & 0x7f) return false;
  const P = ED448_P, y = leNumber(enc, 0, 56);
  if (y >= P) return false;
  const y2 = y * y % P, x2 = (y2 - 1n + P) % P * powMod(((P - 39081n) * y2 - 1n + P) % P, P - 2n, P) % P;
  if (x2 !== 0n && powMod(x2, (P - 1n) / 2n, P) !== 1n) return false;
  return !(x2 === 0n && (enc[56] & 0x80));
}
function ed448SmallOrder(enc) {                 // a canonical encoding of one of the four points of order 1, 2, 4 (ed448.ts:738-743)
  const y = leNumber(enc, 0, 56);
  return y === 1n || y === ED448_P - 1n || y === 0n;
}
function shake256(len, ...parts) {
  const h = crypto.createHash('shake256', { outputLength: len });
  for (const p of parts) h.update(p);
  return h.digest();
}
// items: [{sig, msg, publicKey}] -> array of booleans; opts.context (Uint8Array, at most 255 bytes) and opts.prehash (true: ed448ph)
// hold for the whole batch
function ed448VerifyBatch(items, opts = {}) {
  const context = opts.context === undefined ? new Uint8Array(0) : abytesT(opts.context, undefined, 'context');
  const prehash = !!opts.prehash, n = items.length;
  const S = new Uint8Array(114 * n), A = new Uint8Array(57 * n), K = new Uint8Array(56 * n);
  for (let i = 0; i < n; i++) {
    const sig = abytesT(items[i].sig, 114, 'signature');
    let msg = abytesT(items[i].msg, undefined, 'message');
    const pk = abytesT(items[i].publicKey, 57, 'publicKey');
    if (context.length > 255) {
      // edwards.ts:964-984: dom4 refuses the context only for a row that got past the decoding of A and R, s < n and the small-order
      // test; every other row is false without the context being looked at (rare path: host integers)
      if (ed448Decodes(pk) && ed448Decodes(sig.subarray(0, 57)) && leNumber(sig, 57, 57) < ED448_N && !ed448SmallOrder(pk))
        throw new Error('context must be smaller than 255, got: ' + context.length);
      continue;
    }
    S.set(sig, 114 * i);
    A.set(pk, 57 * i);
    if (opts.deviceHash) continue;
    if (prehash) msg = shake256(64, msg);
    const dom = Buffer.concat([Buffer.from('SigEd448'), Buffer.from([prehash ? 1 : 0, context.length]), context]);
    leBytes(leNumber(shake256(114, dom, sig.subarray(0, 57), pk, msg), 0, 114) % ED448_N, 56, K, 56 * i);
  }
  if (n === 0) return [];
  if (context.length > 255) return new Array(n).fill(false);
  init();
  if (opts.deviceHash) {
    const { blob, lens } = ed448Blob(items.map((it) => it.msg));
    return Array.from(native.ed448Sign(2, S, prehash ? 4 : 0, ed448Dom(opts).dom, blob, lens, A), (v) => v === 1);
  }
  return Array.from(native.ed448(2, S, A, K), (v) => v === 1);
}
// ---- Ed448 signing (abstract/edwards.ts:866-930, ed448.ts:190-246): getPublicKey and sign for ed448 / ed448ph.  Every SHAKE256, the two
// multiplications and the scalar arithmetic run on the device; only the domain prefix is built here.  opts.context: at most 255 bytes;
// opts.prehash: true selects ed448ph.  Batch forms return null for a row the device refused (r = 0 mod n); the single-item forms throw
// the reference's messages.
function ed448Dom(opts) {                       // dom4 (ed448.ts:190-201)
  const prehash = !!(opts && opts.prehash);
  const ctx = opts && opts.context !== undefined ? abytesT(opts.context, undefined, 'context') : new Uint8Array(0);
  if (ctx.length > 255) throw new Error('context must be smaller than 255, got: ' + ctx.length);
  const dom = new Uint8Array(10 + ctx.length);
  dom.set(Buffer.from('SigEd448', 'ascii'), 0);
  dom[8] = prehash ? 1 : 0;
  dom[9] = ctx.length;
  dom.set(ctx, 10);
  return { dom, flags: prehash ? 4 : 0 };
}
function ed448Blob(msgs) {                      // the messages back to back and their lengths as LE uint32
  const n = msgs.length, lens = new Uint8Array(4 * n), view = new DataView(lens.buffer);
  let total = 0;
  for (let i = 0; i < n; i++) {
    view.setUint32(4 * i, abytesT(msgs[i], undefined, 'message').length, true);
    total += msgs[i].length;
  }
  const blob = new Uint8Array(total);
  for (let i = 0, at = 0; i < n; at += msgs[i++].length) blob.set(msgs[i], at);
  return { blob, lens };
}
function ed448GetPublicKeyBatch(secretKeys) {
  const n = secretKeys.length, S = new Uint8Array(57 * n);
  secretKeys.forEach((k, i) => S.set(abytesT(k, 57, 'secretKey'), 57 * i));
  if (n === 0) return [];
  init();
  const out = native.ed448Sign(0, S);
  S.fill(0);
  return Array.from({ length: n }, (_, i) => out.slice(57 * i, 57 * i + 57));
}
// items: [{msg, secretKey}] - or {msgs, secretKey}: ONE key signing many messages (opts.oneKey says the same: the key crosses once)
function ed448SignBatch(items, opts) {
  const one = !Array.isArray(items);
  if (opts && opts.oneKey !== undefined && !!opts.oneKey !== one) throw new Error('oneKey goes with {msgs, secretKey}');
  const msgs = one ? items.msgs : items.map((it) => it.msg);
  const n = msgs.length;
  const K = new Uint8Array(one ? 57 : 57 * n);
  const { blob, lens } = ed448Blob(msgs);
  if (one) K.set(abytesT(items.secretKey, 57, 'secretKey'), 0);
  else items.forEach((it, i) => K.set(abytesT(it.secretKey, 57, 'secretKey'), 57 * i));
  const { dom, flags } = ed448Dom(opts);          // the key is checked before the context, as in the reference
  if (n === 0) return [];
  init();
  const out = native.ed448Sign(1, K, flags, dom, blob, lens);
  K.fill(0);
  return Array.from({ length: n }, (_, i) => (out[114 * n + i] === 1 ? out.slice(114 * i, 114 * i + 114) : null));
}
function ed448GetPublicKey(secretKey) { return ed448GetPublicKeyBatch([secretKey])[0]; }
function ed448Sign(msg, secretKey, opts) {
  const r = ed448SignBatch([{ msg, secretKey }], opts)[0];
  if (r === null) throw new Error('invalid scalar: expected 1 <= sc < curve.n');   // BASE.multiply(0), edwards.ts:920-924
  return r;
}

const X25519_P = (1n << 255n) - 19n;
const X25519_LOW = [0n, 1n, X25519_P - 1n, 325606250916557431795983626356110631294008115727848805560023387167927233504n,
                    39382357235489614581723060781553021112529911719440698176882885853963445705823n];
function x25519ScalarMult(scalar, u) {          // montgomery.ts:314-331 with its order of checks: u, low order, then the scalar
  abytes32(u, 'uCoordinate');
  const pu = (leNumber(u, 0, 32) & ((1n << 255n) - 1n)) % X25519_P;
  if (X25519_LOW.includes(pu)) throw new Error(X25519_INVALID);
  const r = x25519ScalarMultBatch([{ scalar, u }])[0];
  if (r === null) throw new Error(X25519_INVALID);
  return r;
}
function x25519GetPublicKey(secretKey) {
  const r = x25519GetPublicKeyBatch([secretKey])[0];
  if (r === null) throw new Error(X25519_INVALID);
  return r;
}
const ED_D = 37095705934669439343138083508754565189542113879843219016388785533085940283555n;
function ed25519ToMontgomery(publicKey) {        // the message of a refused key is re-derived on host integers (rare path)
  const r = ed25519ToMontgomeryBatch([publicKey])[0];
  if (r !== null) return r;
  const P = X25519_P, y = leNumber(publicKey, 0, 32) & ((1n << 255n) - 1n);
  if (y >= P) throw new Error('expected valid point.y: 0 <= n < ' + P + ', got ' + y);
  const x2 = (y * y - 1n + P) % P * powMod((ED_D * y % P * y + 1n) % P, P - 2n, P) % P;
  if (x2 !== 0n && powMod(x2, (P - 1n) / 2n, P) !== 1n) throw new Error('bad point: invalid y coordinate');
  if (x2 === 0n && (publicKey[31] & 0x80)) throw new Error('bad point: x=0 and x_0=1');
  throw new Error('invert: expected non-zero number');
}

// ---- ristretto255 (src/ed25519.ts:443-668, RFC 9496).  An element is its 32-byte encoding on this side; fromBytes hands back the
// Edwards representative as a 64-byte ed25519 wire point (x || y), which the NCG_ED25519 calls take.  Batch forms return null where
// the reference throws; the single-item forms throw its messages ('encoding 1' decided here from canonicity and parity).
const RISTRETTO_ENC1 = 'invalid ristretto255 encoding 1', RISTRETTO_ENC2 = 'invalid ristretto255 encoding 2';
function abytesN(b, len) {                       // utils abytes(value, length) without a title
  const bytes = b instanceof Uint8Array;
  if (!bytes || b.length !== len) throw new Error('expected Uint8Array of length ' + len + ', got ' + (bytes ? `length=${b.length}` : `type=${typeof b}`));
  return b;
}
function ristrettoPack(items, len) {
  const out = new Uint8Array(len * items.length);
  items.forEach((b, i) => out.set(abytesN(b, len), len * i));
  return out;
}
function ristrettoScalars(ks, lo) {              // Point.multiply: 1 <= k < L (the MSM also takes 0)
  const out = new Uint8Array(32 * ks.length);
  ks.forEach((k, i) => {
    if (typeof k !== 'bigint' || k < lo || k >= ED_L) throw new Error('invalid scalar: expected 1 <= sc < curve.n');
    leBytes(k, 32, out, 32 * i);
  });
  return out;
}
function ristrettoSplit(packed, n, len, flags) {
  const out = new Array(n);
  for (let i = 0; i < n; i++) out[i] = !flags || packed[len * n + i] === 1 ? packed.slice(len * i, len * i + len) : null;
  return out;
}
function ristrettoFromBytesBatch(encodings) {    // -> 64-byte wire points (x || y) or null
  const n = encodings.length, E = ristrettoPack(encodings, 32);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.ristretto(0, E, null), n, 64, true);
}
function ristrettoToBytesBatch(points) {         // 64-byte wire points -> encodings
  const n = points.length, A = ristrettoPack(points, 64);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.ristretto(1, A, null), n, 32, false);
}
function ristrettoEqualsBatch(as, bs) {
  if (as.length !== bs.length) throw new Error('arrays of points must have equal length');
  const A = ristrettoPack(as, 64), B = ristrettoPack(bs, 64);
  if (as.length === 0) return [];
  init();
  return Array.from(native.ristretto(2, A, B)).map((x) => x === 1);
}
function ristrettoDeriveToCurveBatch(rows64) {
  const n = rows64.length, A = ristrettoPack(rows64, 64);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.ristretto(3, A, null), n, 32, false);
}
// encodings x scalars (bigint[]), or ONE bigint against every row -> encodings of the products, null where a row does not decode
function ristrettoMultiplyBatch(encodings, scalars) {
  const one = typeof scalars === 'bigint';
  if (!one && scalars.length !== encodings.length) throw new Error('arrays of points and scalars must have equal length');
  const n = encodings.length, E = ristrettoPack(encodings, 32), K = ristrettoScalars(one ? [scalars] : scalars, 1n);
  if (n === 0) return [];
  init();
  // (the native call tells the two forms apart by the length of K; for n = 1 they are the same call)
  return ristrettoSplit(native.ristretto(4, E, K), n, 32, true);
}
function ristrettoMultiplyBaseBatch(scalars) {
  const n = scalars.length, K = ristrettoScalars(scalars, 1n);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.ristretto(5, K, null), n, 32, false);
}
function ristrettoCanonicalEven(b) { return (b[0] & 1) === 0 && leNumber(b, 0, 32) < X25519_P; }
function ristrettoMsm(encodings, scalars) {      // -> the encoding of sum k_i P_i; throws like fromBytes on a bad encoding
  if (scalars.length !== encodings.length) throw new Error('arrays of points and scalars must have equal length');
  const E = ristrettoPack(encodings, 32), K = ristrettoScalars(scalars, 0n);
  encodings.forEach((b) => { if (!ristrettoCanonicalEven(b)) throw new Error(RISTRETTO_ENC1); });
  init();
  try {
    return native.ristretto(6, E, K);
  } catch (e) {
    if (/invalid ristretto255 encoding at index/.test(e.message)) throw new Error(RISTRETTO_ENC2);
    throw e;
  }
}
function ristrettoFromBytes(b) {
  abytesN(b, 32);
  if (!ristrettoCanonicalEven(b)) throw new Error(RISTRETTO_ENC1);
  const r = ristrettoFromBytesBatch([b])[0];
  if (r === null) throw new Error(RISTRETTO_ENC2);
  return r;
}
function ristrettoToBytes(point) { return ristrettoToBytesBatch([point])[0]; }
function ristrettoEquals(a, b) { return ristrettoEqualsBatch([a], [b])[0]; }
function ristrettoMultiply(encoding, k) {
  ristrettoFromBytes(encoding);                  // the reference decodes first: its messages come first
  return ristrettoMultiplyBatch([encoding], [k])[0];
}
function ristrettoMultiplyBase(k) { return ristrettoMultiplyBaseBatch([k])[0]; }
function ristrettoDeriveToCurve(bytes64) { return ristrettoDeriveToCurveBatch([bytes64])[0]; }

// ---- RFC 9497 OPRF over ristretto255-SHA512 (src/abstract/oprf.ts, ristretto255_oprf of src/ed25519.ts:682): an object of the reference's
// shape with batch forms beside it.  The hashes to the group and to scalars, the blinding, evaluation and unblinding multiplies (secret
// scalars: no table lookup by digit), the Finalize hash, the composite scalars and the DLEQ proof run on the device (native.oprf);
// POPRF's m, t = skS + m and the argument checks with the reference's messages are here.  rng: (n) => Uint8Array of n bytes.
const OPRF_NAME = 'ristretto255-SHA512';
const OPRF_BASE = Uint8Array.from(Buffer.from('e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76', 'hex'));
const OPRF_NONE = new Uint8Array(0);
function oprfInput(title, b) {
  abytesT(b, undefined, title);
  if (b.length > 0xffff) throw new Error(`"${title}" expected Uint8Array of length <= 65535, got length=${b.length}`);
  return b;
}
function oprfCtx(mode) { return Buffer.concat([Buffer.from('OPRFV1-', 'ascii'), Buffer.from([mode]), Buffer.from('-' + OPRF_NAME, 'ascii')]); }
function oprfScalar(b) {                          // Fn.fromBytes
  abytesN(b, 32);
  const k = leNumber(b, 0, 32);
  if (k >= ED_L) throw new Error('invalid field element: outside of range 0..ORDER');
  return k;
}
function oprfLe(k) { const out = new Uint8Array(32); leBytes(k, 32, out, 0); return out; }
function oprfRandomScalar(rng) {
  if (typeof rng !== 'function') throw new TypeError('"rng" expected function, got type=' + typeof rng);
  const b = rng(48);
  return leNumber(b, 0, 48) % (ED_L - 1n) + 1n;
}
function oprfBlob(msgs) {
  const n = msgs.length, lens = new Uint8Array(4 * n), view = new DataView(lens.buffer);
  let total = 0;
  msgs.forEach((m, i) => { view.setUint32(4 * i, m.length, true); total += m.length; });
  const blob = new Uint8Array(total);
  for (let i = 0, at = 0; i < n; at += msgs[i++].length) blob.set(msgs[i], at);
  return { blob, lens };
}
function oprfEncError(b) { return ristrettoCanonicalEven(b) ? RISTRETTO_ENC2 : RISTRETTO_ENC1; }
function oprfRows(out, n, width, label, rows, invert) {   // the rows of a native answer, or the reference's message for the first refused one
  for (let i = 0; i < n; i++) {
    const st = out[width * n + i];
    if (st === 3) throw new Error(invert ? 'invert: expected non-zero number' : 'invalid scalar: expected 1 <= sc < curve.n');
    if (st === 2) throw new Error(label + ' point at infinity');
    if (st === 1) throw new Error(oprfEncError(rows[i]));
  }
  return Array.from({ length: n }, (_, i) => out.slice(width * i, width * i + width));
}
function oprfWirePoints(label, rows) {
  rows.forEach((r) => { abytesN(r, 32); if (r.every((x) => x === 0)) throw new Error(label + ' point at infinity'); });
  if (rows.length) ristrettoFromBytesBatch(rows).forEach((p, i) => { if (p === null) throw new Error(oprfEncError(rows[i])); });
  return rows;
}
function oprfArray(a) { if (!Array.isArray(a)) throw new Error('expected array'); return a; }
function oprfRng(n) { return new Uint8Array(crypto.randomBytes(n)); }
function oprfHashToScalar(msg, dst) {
  init();
  const { blob, lens } = oprfBlob([msg]);
  return native.oprf(6, 0, 0, blob, lens, dst, OPRF_NONE);
}
// ---- RFC 9380 for secp256k1 and ed25519: secp256k1_hasher (src/secp256k1.ts:403-428) and ed25519_hasher (src/ed25519.ts:381-405)
// under createHasher (src/abstract/hash-to-curve.ts:441-530), hashed and mapped on the device (ncg_h2c_hash_batch,
// ncg_h2c_hash_to_scalar_batch).  Every batch form makes one native call.  Points come back as affine { x, y } of bigints - ZERO as
// the curve's affine ZERO, (0, 0) or (0, 1) - or through opts.Point.fromAffine when the caller passes the reference's Point class.
const H2C_SUITES = {
  secp256k1: { id: 0, DST: 'secp256k1_XMD:SHA-256_SSWU_RO_', encodeDST: 'secp256k1_XMD:SHA-256_SSWU_NU_', hash: 'sha256',
    p: 0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2fn },
  ed25519: { id: 1, DST: 'edwards25519_XMD:SHA-512_ELL2_RO_', encodeDST: 'edwards25519_XMD:SHA-512_ELL2_NU_', hash: 'sha512',
    p: (1n << 255n) - 19n },
};
function h2cDst(suite, DST) {       // normDST (hash-to-curve.ts:160-167) and the oversize rule of expand_message_xmd (:202)
  if (!(DST instanceof Uint8Array) && typeof DST !== 'string') throw new Error('DST must be Uint8Array or ascii string');
  let dst = typeof DST === 'string' ? Uint8Array.from(Buffer.from(DST, 'ascii')) : DST;
  if (dst.length === 0) throw new Error('DST must be non-empty');
  if (dst.length > 255) dst = new Uint8Array(crypto.createHash(suite.hash).update('H2C-OVERSIZE-DST-', 'ascii').update(dst).digest());
  return dst;
}
function h2cMsgs(msgs) {
  if (!Array.isArray(msgs)) throw new Error('expected array');
  msgs.forEach((m) => { if (!(m instanceof Uint8Array)) throw new Error('expected Uint8Array, got type=' + typeof m); });
  return msgs;
}
function h2cPoints(suite, msgs, opts, count) {
  const dst = h2cDst(suite, opts && opts.DST !== undefined ? opts.DST : (count === 2 ? suite.DST : suite.encodeDST));   // only DST may be overridden
  const n = h2cMsgs(msgs).length;
  if (n === 0) return [];
  init();
  const { blob, lens } = oprfBlob(msgs);
  const out = native.h2c(0, suite.id, count, blob, lens, dst);
  return Array.from({ length: n }, (_, i) => {
    const a = { x: leNumber(out, 64 * i, 32), y: leNumber(out, 64 * i + 32, 32) };
    return opts && opts.Point ? (out[64 * n + i] ? opts.Point.ZERO : opts.Point.fromAffine(a)) : a;
  });
}
function h2cScalars(suite, msgs, opts) {
  const dst = h2cDst(suite, opts && opts.DST !== undefined ? opts.DST : 'HashToScalar-');     // _DST_scalar (:412, :523)
  const n = h2cMsgs(msgs).length;
  if (n === 0) return [];
  init();
  const { blob, lens } = oprfBlob(msgs);
  const out = native.h2c(1, suite.id, 1, blob, lens, dst);
  return Array.from({ length: n }, (_, i) => leNumber(out, 32 * i, 32));
}
const secp256k1HashToCurveBatch = (msgs, opts) => h2cPoints(H2C_SUITES.secp256k1, msgs, opts, 2);
const secp256k1EncodeToCurveBatch = (msgs, opts) => h2cPoints(H2C_SUITES.secp256k1, msgs, opts, 1);
const ed25519HashToCurveBatch = (msgs, opts) => h2cPoints(H2C_SUITES.ed25519, msgs, opts, 2);
const ed25519EncodeToCurveBatch = (msgs, opts) => h2cPoints(H2C_SUITES.ed25519, msgs, opts, 1);
// hashToScalarBatch(msgs, { DST, curve }): curve 'secp256k1' (the default) or 'ed25519'
function hashToScalarBatch(msgs, opts) {
  const suite = H2C_SUITES[(opts && opts.curve) || 'secp256k1'];
  if (!suite) throw new Error('hashToScalarBatch: curve must be secp256k1 or ed25519');
  return h2cScalars(suite, msgs, opts);
}
function h2cHasher(name) {
  const suite = H2C_SUITES[name];
  return Object.freeze({
    get defaults() { return { DST: suite.DST, encodeDST: suite.encodeDST, p: suite.p, m: 1, k: 128, expand: 'xmd', hash: suite.hash }; },
    hashToCurve: (msg, opts) => h2cPoints(suite, [msg], opts, 2)[0],
    encodeToCurve: (msg, opts) => h2cPoints(suite, [msg], opts, 1)[0],
    hashToScalar: (msg, opts) => h2cScalars(suite, [msg], opts)[0],
    hashToCurveBatch: (msgs, opts) => h2cPoints(suite, msgs, opts, 2),
    encodeToCurveBatch: (msgs, opts) => h2cPoints(suite, msgs, opts, 1),
    hashToScalarBatch: (msgs, opts) => h2cScalars(suite, msgs, opts),
  });
}
const secp256k1_hasher = h2cHasher('secp256k1'), ed25519_hasher = h2cHasher('ed25519');

// ---- RFC 9380 for edwards448 and decaf448: ed448_hasher (src/ed448.ts:408-417) under createHasher, and the hash side of
// decaf448_hasher (:662-701), with expand_message_xof over SHAKE256, the maps and the group law on the device (ncg_ed448_h2c_hash_batch,
// ncg_ed448_h2c_hash_to_scalar_batch, ncg_decaf448_hash_to_group_batch, ncg_decaf448_hash_to_scalar_batch).  Every batch form makes one
// native call.  Ed448 points come back as affine { x, y } of bigints, ZERO as (0, 1), or through opts.Point.fromAffine; decaf448
// elements as their 56-byte encodings.
const H2C448 = { DST: 'edwards448_XOF:SHAKE256_ELL2_RO_', encodeDST: 'edwards448_XOF:SHAKE256_ELL2_NU_' };
function h2c448Dst(DST, k) {        // normDST and the oversize rule of expand_message_xof (:263-266): ceil(2 k / 8) bytes of SHAKE256
  if (!(DST instanceof Uint8Array) && typeof DST !== 'string') throw new Error('DST must be Uint8Array or ascii string');
  let dst = typeof DST === 'string' ? Uint8Array.from(Buffer.from(DST, 'ascii')) : DST;
  if (dst.length === 0) throw new Error('DST must be non-empty');
  if (dst.length > 255)
    dst = new Uint8Array(crypto.createHash('shake256', { outputLength: Math.ceil((2 * k) / 8) }).update('H2C-OVERSIZE-DST-', 'ascii').update(dst).digest());
  return dst;
}
function h2c448Call(op, count, msgs, dst, width) {
  const n = h2cMsgs(msgs).length;
  if (n === 0) return [];
  init();
  const { blob, lens } = oprfBlob(msgs);
  const out = native.h2c448(op, count, blob, lens, dst);
  return Array.from({ length: n }, (_, i) => out.subarray(width * i, width * i + width));
}
function h2c448Points(msgs, opts, count) {
  const dst = h2c448Dst(opts && opts.DST !== undefined ? opts.DST : (count === 2 ? H2C448.DST : H2C448.encodeDST), 224);
  return h2c448Call(0, count, msgs, dst, 112).map((row) => {
    const a = { x: leNumber(row, 0, 56), y: leNumber(row, 56, 56) };
    return opts && opts.Point ? (a.x === 0n && a.y === 1n ? opts.Point.ZERO : opts.Point.fromAffine(a)) : a;
  });
}
function h2c448Scalars(msgs, opts) {
  const dst = h2c448Dst(opts && opts.DST !== undefined ? opts.DST : 'HashToScalar-', 224);
  return h2c448Call(1, 1, msgs, dst, 56).map((row) => leNumber(row, 0, 56));
}
const ed448HashToCurveBatch = (msgs, opts) => h2c448Points(msgs, opts, 2);
const ed448EncodeToCurveBatch = (msgs, opts) => h2c448Points(msgs, opts, 1);
// decaf448_hasher.hashToCurve(msg, { DST }).toBytes() for every message
function decaf448HashToCurveBatch(msgs, opts) {
  const dst = h2c448Dst(opts && opts.DST !== undefined ? opts.DST : 'decaf448_XOF:SHAKE256_D448MAP_RO_', 224);
  return h2c448Call(2, 1, msgs, dst, 56).map((row) => Uint8Array.from(row));
}
// decaf448_hasher.hashToScalar: k = 256, so an oversize DST is compressed to 64 bytes (ed448.ts:677)
function decaf448HashToScalarBatch(msgs, opts) {
  const dst = h2c448Dst(opts && opts.DST !== undefined ? opts.DST : 'HashToScalar-', 256);
  return h2c448Call(3, 1, msgs, dst, 56).map((row) => leNumber(row, 0, 56));
}
const ed448_hasher = Object.freeze({
  get defaults() { return { DST: H2C448.DST, encodeDST: H2C448.encodeDST, p: ED448_P, m: 1, k: 224, expand: 'xof', hash: 'shake256' }; },
  hashToCurve: (msg, opts) => h2c448Points([msg], opts, 2)[0],
  encodeToCurve: (msg, opts) => h2c448Points([msg], opts, 1)[0],
  hashToScalar: (msg, opts) => h2c448Scalars([msg], opts)[0],
  hashToCurveBatch: (msgs, opts) => h2c448Points(msgs, opts, 2),
  encodeToCurveBatch: (msgs, opts) => h2c448Points(msgs, opts, 1),
  hashToScalarBatch: (msgs, opts) => h2c448Scalars(msgs, opts),
});

function oprfMode(mode, info) {
  const m = mode === 2 ? leNumber(oprfHashToScalar(Buffer.concat([Buffer.from('Info', 'ascii'), Buffer.from([info.length >> 8, info.length & 255]), info]),
    Buffer.concat([Buffer.from('HashToScalar-', 'ascii'), oprfCtx(2)])), 0, 32) : 0n;
  const inf = mode === 2 ? info : OPRF_NONE;
  const mulOne = (label, elements, k, invert) => {
    elements.forEach((e) => abytesN(e, 32));
    const n = elements.length;
    if (n === 0) return [];
    init();
    const K = oprfLe(k), out = native.oprf(1, mode, invert ? 2 : 0, ristrettoPack(elements, 32), K, OPRF_NONE, OPRF_NONE);
    K.fill(0);
    return oprfRows(out, n, 32, label, elements, invert);
  };
  const blindBatch = (inputs, rng = oprfRng) => {
    inputs.forEach((i) => oprfInput('input', i));
    const blinds = inputs.map(() => oprfLe(oprfRandomScalar(rng))), n = inputs.length;
    if (n === 0) return { blind: [], blinded: [] };
    init();
    const { blob, lens } = oprfBlob(inputs);
    const out = native.oprf(0, mode, 0, blob, lens, ristrettoPack(blinds, 32), OPRF_NONE);
    for (let i = 0; i < n; i++) if (out[32 * n + i] !== 0) throw new Error('Input point at infinity');
    return { blind: blinds, blinded: Array.from({ length: n }, (_, i) => out.slice(32 * i, 32 * i + 32)) };
  };
  const unblind = (inputs, blinds, evaluated) => {
    const n = inputs.length;
    blinds.forEach(oprfScalar);
    evaluated.forEach((e) => abytesN(e, 32));
    if (n === 0) return [];
    init();
    const { blob, lens } = oprfBlob(inputs), C = new Uint8Array(64 * n);
    C.set(ristrettoPack(blinds, 32), 0);
    C.set(ristrettoPack(evaluated, 32), 32 * n);
    const out = native.oprf(2, mode, 0, blob, lens, C, inf);
    C.fill(0);
    return oprfRows(out, n, 64, 'evaluated', evaluated, true);
  };
  const evaluateBatch = (k, invert, inputs) => {
    inputs.forEach((i) => oprfInput('input', i));
    const n = inputs.length;
    if (n === 0) return [];
    init();
    const { blob, lens } = oprfBlob(inputs), K = oprfLe(k);
    const out = native.oprf(3, mode, invert ? 2 : 0, blob, lens, K, inf);
    K.fill(0);
    return oprfRows(out, n, 64, 'Input', inputs, invert);
  };
  const proof = (k, B, C, D, rng) => {
    const A = new Uint8Array(96);
    A.set(oprfLe(k), 0); A.set(B, 32); A.set(oprfLe(oprfRandomScalar(rng)), 64);
    init();
    const out = native.oprf(4, mode, 0, A, ristrettoPack(C, 32), ristrettoPack(D, 32), OPRF_NONE);
    A.fill(0);
    return out;
  };
  const verify = (B, C, D, prf) => {
    abytesN(prf, 64);
    oprfScalar(prf.subarray(0, 32)); oprfScalar(prf.subarray(32));
    const A = new Uint8Array(96);
    A.set(B, 0); A.set(prf, 32);
    init();
    if (native.oprf(5, mode, 0, A, ristrettoPack(C, 32), ristrettoPack(D, 32), OPRF_NONE)[0] !== 1) throw new Error('proof verification failed');
  };
  const common = {
    generateKeyPair() {
      const sk = oprfRandomScalar(oprfRng);
      return { secretKey: oprfLe(sk), publicKey: mulOne('base', [OPRF_BASE], sk, false)[0] };
    },
    deriveKeyPair(seed, keyInfo) {
      abytesT(seed, 32, 'seed');
      oprfInput('keyInfo', keyInfo);
      const dst = Buffer.concat([Buffer.from('DeriveKeyPair', 'ascii'), oprfCtx(mode)]);
      for (let counter = 0; counter <= 255; counter++) {
        const sk = oprfHashToScalar(Buffer.concat([seed, Buffer.from([keyInfo.length >> 8, keyInfo.length & 255]), keyInfo, Buffer.from([counter])]), dst);
        if (sk.every((x) => x === 0)) continue;
        return { secretKey: sk, publicKey: mulOne('base', [OPRF_BASE], leNumber(sk, 0, 32), false)[0] };
      }
      throw new Error('Cannot derive key');
    },
  };
  if (mode !== 2) {
    const S = Object.assign(common, {
      blind(input, rng = oprfRng) { const r = blindBatch([input], rng); return { blind: r.blind[0], blinded: r.blinded[0] }; },
      blindBatch,
      evaluate(secretKey, input) { return evaluateBatch(oprfScalar(secretKey), false, [input])[0]; },
      evaluateBatch(secretKey, inputs) { return evaluateBatch(oprfScalar(secretKey), false, inputs); },
    });
    if (mode === 0) return Object.freeze(Object.assign(S, {
      blindEvaluate(secretKey, blinded) { return mulOne('blinded', [blinded], oprfScalar(secretKey), false)[0]; },
      blindEvaluateBatch(secretKey, blinded) { return mulOne('blinded', oprfArray(blinded), oprfScalar(secretKey), false); },
      finalize(input, blind, evaluated) { return unblind([oprfInput('input', input)], [blind], [evaluated])[0]; },
      finalizeBatch(inputs, blinds, evaluated) { return unblind(inputs.map((i) => oprfInput('input', i)), blinds, evaluated); },
    }));
    return Object.freeze(Object.assign(S, {
      blindEvaluateBatch(secretKey, publicKey, blinded, rng = oprfRng) {
        oprfArray(blinded);
        const sk = oprfScalar(secretKey), pk = oprfWirePoints('public key', [publicKey])[0];
        const evaluated = mulOne('blinded', blinded, sk, false);
        return { evaluated, proof: proof(sk, pk, blinded, evaluated, rng) };
      },
      blindEvaluate(secretKey, publicKey, blinded, rng = oprfRng) {
        const res = this.blindEvaluateBatch(secretKey, publicKey, [blinded], rng);
        return { evaluated: res.evaluated[0], proof: res.proof };
      },
      finalizeBatch(items, publicKey, prf) {
        oprfArray(items);
        const pk = oprfWirePoints('public key', [publicKey])[0];
        const blinded = oprfWirePoints('blinded', items.map((i) => i.blinded)), evaluated = oprfWirePoints('evaluated', items.map((i) => i.evaluated));
        verify(pk, blinded, evaluated, prf);
        return unblind(items.map((i) => oprfInput('input', i.input)), items.map((i) => i.blind), evaluated);
      },
      finalize(input, blind, evaluated, blinded, publicKey, prf) { return this.finalizeBatch([{ input, blind, evaluated, blinded }], publicKey, prf)[0]; },
    }));
  }
  const tOf = (secretKey) => {
    const t = (oprfScalar(secretKey) + m) % ED_L;
    if (t === 0n) throw new Error('invert: expected non-zero number');
    return t;
  };
  return Object.freeze(Object.assign(common, {
    blindBatch(inputs, publicKey, rng = oprfRng) {
      inputs.forEach((i) => oprfInput('input', i));
      const pk = oprfWirePoints('public key', [publicKey])[0];
      // T + pkS, T = m G with the PUBLIC m: the MSM of the ristretto255 exports
      const tweakedKey = ristrettoMsm([OPRF_BASE, pk], [m, 1n]);
      if (tweakedKey.every((x) => x === 0)) throw new Error('tweakedKey point at infinity');
      return Object.assign(blindBatch(inputs, rng), { tweakedKey });
    },
    blind(input, publicKey, rng = oprfRng) {
      const r = this.blindBatch([input], publicKey, rng);
      return { blind: r.blind[0], blinded: r.blinded[0], tweakedKey: r.tweakedKey };
    },
    blindEvaluateBatch(secretKey, blinded, rng = oprfRng) {
      oprfArray(blinded);
      const t = tOf(secretKey);
      const evaluated = mulOne('blinded', blinded, t, true);
      const tweakedKey = mulOne('base', [OPRF_BASE], t, false)[0];
      return { evaluated, proof: proof(t, tweakedKey, evaluated, blinded, rng) };
    },
    blindEvaluate(secretKey, blinded, rng = oprfRng) {
      const res = this.blindEvaluateBatch(secretKey, [blinded], rng);
      return { evaluated: res.evaluated[0], proof: res.proof };
    },
    finalizeBatch(items, prf, tweakedKey) {
      oprfArray(items);
      const inputs = items.map((i) => oprfInput('input', i.input));
      const evaluated = oprfWirePoints('evaluated', items.map((i) => i.evaluated));
      const tw = oprfWirePoints('tweakedKey', [tweakedKey])[0];
      verify(tw, evaluated, oprfWirePoints('blinded', items.map((i) => i.blinded)), prf);
      return unblind(inputs, items.map((i) => i.blind), evaluated);
    },
    finalize(input, blind, evaluated, blinded, prf, tweakedKey) { return this.finalizeBatch([{ input, blind, evaluated, blinded }], prf, tweakedKey)[0]; },
    evaluate(secretKey, input) { return evaluateBatch(tOf(secretKey), true, [input])[0]; },
    evaluateBatch(secretKey, inputs) { return evaluateBatch(tOf(secretKey), true, inputs); },
  }));
}
const ristretto255_oprf = Object.freeze({
  name: OPRF_NAME,
  get oprf() { return oprfMode(0); },
  get voprf() { return oprfMode(1); },
  poprf(info) { return oprfMode(2, Uint8Array.from(oprfInput('info', info))); },
});

// ---- decaf448 (src/ed448.ts:462-701, RFC 9496 section 5), with the argument conventions of the ristretto255 exports.  An element is
// its 56-byte encoding on this side; fromBytes hands back the Edwards representative as a 112-byte Ed448 affine point (x || y).
// Batch forms return null where the reference throws.
function decafScalars(ks) {                       // Point.multiply: 1 <= k < n
  const out = new Uint8Array(56 * ks.length);
  ks.forEach((k, i) => {
    if (typeof k !== 'bigint' || k < 1n || k >= ED448_N) throw new Error('invalid scalar: expected 1 <= sc < curve.n');
    leBytes(k, 56, out, 56 * i);
  });
  return out;
}
function decaf448FromBytesBatch(encodings) {      // -> 112-byte affine representatives (x || y) or null
  const n = encodings.length, E = ristrettoPack(encodings, 56);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.decaf448(0, E, null), n, 112, true);
}
function decaf448ToBytesBatch(points) {           // 112-byte affine points -> encodings
  const n = points.length, A = ristrettoPack(points, 112);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.decaf448(1, A, null), n, 56, false);
}
function decaf448EqualsBatch(as, bs) {
  if (as.length !== bs.length) throw new Error('arrays of points must have equal length');
  const A = ristrettoPack(as, 112), B = ristrettoPack(bs, 112);
  if (as.length === 0) return [];
  init();
  return Array.from(native.decaf448(2, A, B)).map((x) => x === 1);
}
function decaf448DeriveToCurveBatch(rows112) {
  const n = rows112.length, A = ristrettoPack(rows112, 112);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.decaf448(3, A, null), n, 56, false);
}
// encodings x scalars (bigint[]), or ONE bigint against every row -> encodings of the products, null where a row does not decode
function decaf448MultiplyBatch(encodings, scalars) {
  const one = typeof scalars === 'bigint';
  if (!one && scalars.length !== encodings.length) throw new Error('arrays of points and scalars must have equal length');
  const n = encodings.length, E = ristrettoPack(encodings, 56), K = decafScalars(one ? [scalars] : scalars);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.decaf448(4, E, K), n, 56, true);
}
function decaf448MultiplyBaseBatch(scalars) {
  const n = scalars.length, K = decafScalars(scalars);
  if (n === 0) return [];
  init();
  return ristrettoSplit(native.decaf448(5, K, null), n, 56, false);
}


// ---- codecs: array forms of Point.fromBytes / toBytes (compressed) --------------------------------
//   weierstrass.ts:541-605, bls12-381.ts:377-459 (+ subgroup checks :567-577, :599-601), edwards.ts:405-436,620-628
// fromBytesBatch returns null where the reference would throw.
const ENC = [33, 32, 48, 96];
function fromBytesBatch(c, encodings, zip215) {
  const id = curveId(c), eb = ENC[id], pb = native.pointBytes(id), n = encodings.length;
  const buf = new Uint8Array(n * eb);
  encodings.forEach((e, i) => {
    if (!(e instanceof Uint8Array) || e.length !== eb) throw new Error('invalid point encoding at index ' + i + ': expected ' + eb + ' bytes');
    buf.set(e, i * eb);
  });
  if (n === 0) return [];
  init();
  const out = native.decodePoints(id, buf, !!zip215);
  return unmarshalPoints(c, id, out, n, n * pb + n, (i) => out[n * pb + i] === 1);
}
function toBytesBatch(c, points) {
  const id = curveId(c), eb = ENC[id];
  validateMSMPoints(points, c);
  if (points.length === 0) return [];
  init();
  const out = native.encodePoints(id, marshalPoints(c, id, points));
  const n = points.length;
  return points.map((_, i) => {
    if (!out[n * eb + i]) throw new Error('bad point: ZERO');     // weierstrass.ts:545
    return out.slice(i * eb, (i + 1) * eb);
  });
}

// sum of the decoded points: the group part of bls.aggregatePublicKeys on encoded keys (abstract/bls.ts:857-873)
function aggregateFromBytes(c, encodings, zip215) {
  const id = curveId(c), eb = ENC[id], pb = native.pointBytes(id), n = encodings.length;
  if (!Array.isArray(encodings) || n === 0) throw new Error('expected non-empty array');   // bls.ts:426-431 aNonEmpty
  const buf = new Uint8Array(n * eb);
  encodings.forEach((e, i) => {
    if (!(e instanceof Uint8Array) || e.length !== eb) throw new Error('invalid point encoding at index ' + i + ': expected ' + eb + ' bytes');
    buf.set(e, i * eb);
  });
  init();
  const out = native.aggregateEncoded(id, buf, !!zip215);
  return unmarshalPoint(c, id, out, 0, out[pb] === 1);
}

// ---- FFT over the bls12-381 scalar field (the default) or, with opts.field = 'bn254', the bn254 scalar field:
// FFT(roots, Fr).direct / .inverse (fft.ts:518-577) ----------------------------------------------------
const FR = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001n;
const FFT_FIELDS = {                            // ORDER, NCG_FIELD_* id (include/ncg.h), 2-adicity
  bls12_381: { order: FR, id: 0, twoAdicity: 32 },
  bn254: { order: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001n, id: 5, twoAdicity: 28 },
};
function powMod(b, e, m) { let r = 1n; b %= m; while (e > 0n) { if (e & 1n) r = r * b % m; b = b * b % m; e >>= 1n; } return r; }
function fftFr(values, opts) {                  // opts: { inverse, brpInput, brpOutput, generator = 7n, field = 'bls12_381' }
  opts = opts || {};
  const fld = FFT_FIELDS[opts.field || 'bls12_381'];
  if (!fld) throw new Error('noble-gpu: fftFr: unknown field ' + opts.field + ' (bls12_381, bn254)');
  const FR = fld.order;
  const N = values.length;
  if (N === 0 || (N & (N - 1)) !== 0) throw new Error('FFT: Polynomial size should be power of two');
  const bits = 31 - Math.clz32(N);
  if (bits > fld.twoAdicity) throw new Error('rootsOfUnity: wrong bits ' + bits + ' powerOfTwo=' + fld.twoAdicity);   // fft.ts:262-266
  const omega = powMod(opts.generator || 7n, (FR - 1n) >> BigInt(bits), FR);   // rootsOfUnity.omega(bits), fft.ts:238-241
  const data = new Uint8Array(N * 32), om = new Uint8Array(32);
  values.forEach((v, i) => {
    if (typeof v !== 'bigint' || v < 0n || v >= FR) throw new Error('invalid field element: outside of range 0..ORDER');
    leBytes(v, 32, data, 32 * i);
  });
  leBytes(omega, 32, om, 0);
  init();
  const out = native.ntt(bits, om, data, (opts.inverse ? 1 : 0) | (opts.brpInput ? 2 : 0) | (opts.brpOutput ? 4 : 0), fld.id);
  return values.map((_, i) => leNumber(out, 32 * i, 32));
}

// ---- poly(Fr, roots, create?, fft?, length?) of the reference (fft.ts:583-926) over the same two fields, on arrays of bigint:
// polyFr(opts) with opts.field / opts.generator as for fftFr (and opts.length, opts.fft: truthy = "an FFT was passed") returns
// { add, sub, dot, mul, convolve, shift, eval, monomial: { eval }, lagrange: { eval } } with the reference's messages; the vector
// work runs in ncg_poly_* (native.poly).
function polyFr(opts) {
  opts = opts || {};
  const fld = FFT_FIELDS[opts.field || 'bls12_381'];
  if (!fld) throw new Error('noble-gpu: polyFr: unknown field ' + opts.field + ' (bls12_381, bn254)');
  const R = fld.order, length = opts.length, G = opts.generator || 7n;
  const isPow2 = (n) => n > 0 && (n & (n - 1)) === 0;
  const nextPow2 = (n) => { let p = 1; while (p < n) p *= 2; return p; };
  const log2 = (n) => 31 - Math.clz32(n);
  const omegaOf = (bits) => {
    if (bits > fld.twoAdicity) throw new Error('rootsOfUnity: wrong bits ' + bits + ' powerOfTwo=' + fld.twoAdicity);
    return powMod(G, (R - 1n) >> BigInt(bits), R);
  };
  const elem = (v) => {
    if (typeof v !== 'bigint' || v < 0n || v >= R) throw new Error('invalid field element: outside of range 0..ORDER');
    return v;
  };
  const pack = (vals) => { const d = new Uint8Array(vals.length * 32); vals.forEach((v, i) => leBytes(elem(v), 32, d, 32 * i)); return d; };
  const unpack = (buf) => { const out = new Array(buf.length / 32); for (let i = 0; i < out.length; i++) out[i] = leNumber(buf, 32 * i, 32); return out; };
  const checkPoly = (title, v) => { if (!Array.isArray(v)) throw new TypeError(`"${title}" expected polynomial, got type=${typeof v}`); };
  const checkFixed = (L) => { if (length !== undefined && L !== length) throw new Error(`poly: expected fixed length ${length}, got ${L}`); };
  const checkLength = (a, b) => {
    checkPoly('a', a);
    const L = a.length;
    if (b !== undefined) {
      checkPoly('b', b);
      if (b.length !== L) throw new Error(`poly: mismatched lengths ${L} vs ${b.length}`);
    }
    checkFixed(L);
    return L;
  };
  const call = (kind, a, b, small, i1, i2) => { init(); return native.poly(kind, fld.id, a, b, small, i1 || 0, i2 || 0); };
  const pointwise = (op) => (a, b) => {
    const L = checkLength(a, b), A = pack(a), B = pack(b);
    return L ? unpack(call(0, A, B, null, op)) : [];
  };
  const cyclic = (bits, A, B) => call(5, A, B, pack([omegaOf(bits)]), bits);
  const lagrangeBits = (n) => {
    if (!isPow2(n)) throw new Error('poly.lagrange: expected power of two length, got ' + n);
    return log2(n);
  };
  const lagrangeBasis = (x, n, brp) => {
    const bits = lagrangeBits(n);
    return call(4, null, null, pack([omegaOf(bits), elem(x)]), bits, brp ? 1 : 0);
  };
  const api = {
    length,
    add: pointwise(0),
    sub: pointwise(1),
    dot: pointwise(2),
    mul(a, b) {
      if (!Array.isArray(b)) {
        const L = checkLength(a), A = pack(a), s = pack([b]);
        return L ? unpack(call(1, A, null, s, 0)) : [];
      }
      const L = checkLength(a, b);
      if (L && !isPow2(L) && opts.fft) throw new Error('FFT: Polynomial size should be power of two');
      const A = pack(a), B = pack(b);
      if (!L) return [];
      if (isPow2(L)) return unpack(cyclic(log2(L), A, B));
      const full = cyclic(log2(nextPow2(2 * L - 1)), A, B);   // the quadratic product mod x^L - 1 (:816-824): linear product, folded
      return unpack(call(0, full.subarray(0, 32 * L), full.subarray(32 * L, 64 * L), null, 0));
    },
    convolve(a, b) {
      checkPoly('a', a);
      checkPoly('b', b);
      const n = nextPow2(a.length + b.length - 1);
      checkFixed(a.length); checkFixed(b.length); checkFixed(n);
      return unpack(cyclic(log2(n), pack(a), pack(b)));
    },
    shift(p, factor) {
      checkPoly('p', p);
      checkFixed(p.length);
      const P = pack(p), f = pack([factor]);
      return p.length ? unpack(call(1, P, null, f, 1)) : [];
    },
    eval(a, basis) {
      checkLength(a, basis);
      return unpack(call(2, pack(a), pack(basis), null))[0];
    },
    monomial: {
      eval(a, x) {
        checkLength(a);
        return unpack(call(3, pack(a), null, pack([x])))[0];
      },
    },
    lagrange: {
      basis: (x, n, brp) => unpack(lagrangeBasis(x, n, brp)),
      eval(a, x, brp) {
        const L = checkLength(a);
        lagrangeBits(L);
        const A = pack(a);
        const basis = lagrangeBasis(x, L, brp);      // the delta when x is a root: the sum is then a[idx], the reference's fast path
        return unpack(call(2, A, basis, null))[0];
      },
    },
  };
  return api;
}

// ---- hash-to-curve for bls12-381 G1 / G2: createHasher(...).hashToCurve (hash-to-curve.ts:441-548) -
const BLS_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn;
function expandMessageXmd(msg, dst, len) {      // hash-to-curve.ts:189-228 with SHA-256
  const sha = (...parts) => { const h = crypto.createHash('sha256'); parts.forEach((p) => h.update(p)); return h.digest(); };
  if (dst.length > 255) dst = sha(Buffer.from('H2C-OVERSIZE-DST-'), dst);
  const ell = Math.ceil(len / 32);
  if (len > 65535 || ell > 255) throw new Error('expand_message_xmd: invalid lenInBytes');
  const dstPrime = Buffer.concat([dst, Buffer.from([dst.length])]);
  const b0 = sha(Buffer.alloc(64), msg, Buffer.from([len >> 8, len & 255, 0]), dstPrime);
  const b = [sha(b0, Buffer.from([1]), dstPrime)];
  for (let i = 1; i < ell; i++) b.push(sha(Buffer.from(b0.map((x, j) => x ^ b[i - 1][j])), Buffer.from([i + 1]), dstPrime));
  return Buffer.concat(b).slice(0, len);
}
function hashToCurveBatch(c, msgs, DST) {
  const id = curveId(c);
  if (id !== CURVE.BLS12_381_G1 && id !== CURVE.BLS12_381_G2) throw new Error('noble-gpu: hashToCurveBatch: bls12-381 G1 / G2 only');
  const m = id === CURVE.BLS12_381_G2 ? 2 : 1, L = 64, count = 2;
  const dst = Buffer.from(DST || (m === 2 ? 'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_' : 'BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_'));
  const u = new Uint8Array(msgs.length * count * m * 48);
  msgs.forEach((msg, i) => {
    const prb = expandMessageXmd(Buffer.from(msg), dst, count * m * L);       // hash_to_field :312-378
    for (let e = 0; e < count * m; e++) {
      let v = 0n;
      for (let j = 0; j < L; j++) v = (v << 8n) | BigInt(prb[e * L + j]);
      leBytes(v % BLS_P, 48, u, (i * count * m + e) * 48);
    }
  });
  if (msgs.length === 0) return [];
  init();
  const pb = native.pointBytes(id), n = msgs.length;
  const out = native.mapToCurve(id, count, u);
  return unmarshalPoints(c, id, out, n, n * pb);
}

// ---- bls12-381 pairings: bls.pairingBatch for many groups in one call (bls.ts:670-693) and verify per row from bytes (:795-818).
// pairs: [{ g1, g2 }] of registered G1 / G2 points, or of affine wire rows (Uint8Array of 96 / 192 bytes); groups: sizes summing to
// pairs.length (omitted: ONE product, one Fp12 returned; given: an array of Fp12).  The result has the reference's Fp12 object shape
// ({ c0: { c0: { c0, c1 }, c1, c2 }, c1: .. } of bigint, frozen); with registerBls(bls12_381) it goes through fields.Fp12.create.
let blsFields = null, blsG1 = null, blsG2 = null;
function registerBls(bls) {
  blsFields = bls.fields; blsG1 = bls.G1.Point; blsG2 = bls.G2.Point;
  register(blsG1, CURVE.BLS12_381_G1); register(blsG2, CURVE.BLS12_381_G2);
}
const BLS_ERRORS = ['pairing is not available for ZERO point', 'bad point: equation left != right', 'bad point: not in prime-order subgroup'];
function blsWire(p, c, bytes, title) {
  if (p instanceof Uint8Array) {
    if (p.length !== bytes) throw new TypeError('"' + title + '" expected ' + bytes + ' bytes');
    return p;
  }
  if (c === null || !(p instanceof c)) throw new TypeError('"' + title + '" expected ' + (bytes === 96 ? 'G1' : 'G2') + ' point, got type=' + typeof p);
  return marshalPoints(c, curveId(c), [p]).subarray(0, bytes);
}
function fp12FromWire(buf, off) {
  const f2 = (k) => Object.freeze({ c0: leNumber(buf, off + 96 * k, 48), c1: leNumber(buf, off + 96 * k + 48, 48) });
  const f6 = (k) => Object.freeze({ c0: f2(3 * k), c1: f2(3 * k + 1), c2: f2(3 * k + 2) });
  const v = Object.freeze({ c0: f6(0), c1: f6(1) });
  return blsFields ? blsFields.Fp12.create(v) : v;
}
function pairingBatch(pairs, groups, opts) {
  if (!Array.isArray(pairs)) throw new TypeError('"pairs" expected array, got type=' + typeof pairs);
  const n = pairs.length, sizes = groups === undefined ? [n] : Array.from(groups);
  if (sizes.some((x) => !Number.isInteger(x) || x < 0) || sizes.reduce((a, b) => a + b, 0) !== n) throw new Error('group sizes must be non-negative and sum to the number of pairs');
  const g1 = new Uint8Array(n * 96), g2 = new Uint8Array(n * 192), off = new Uint8Array((sizes.length + 1) * 4);
  pairs.forEach((pr, i) => {
    const a = blsWire(pr.g1, blsG1, 96, 'pairs[' + i + '].g1'), b = blsWire(pr.g2, blsG2, 192, 'pairs[' + i + '].g2');
    if (a.every((x) => x === 0) || b.every((x) => x === 0)) throw new Error(BLS_ERRORS[0]);
    g1.set(a, i * 96); g2.set(b, i * 192);
  });
  let acc = 0;
  sizes.forEach((x, g) => { acc += x; new DataView(off.buffer).setUint32(4 * (g + 1), acc, true); });
  if (sizes.length === 0) return [];
  init();
  let out;
  try { out = native.bls(0, g1, g2, off, opts && opts.checkSubgroup ? 1 : 0); } catch (e) {
    const m = BLS_ERRORS.find((t) => e.message.includes(t));
    throw m ? new Error(m) : e;
  }
  const res = sizes.map((_, g) => fp12FromWire(out, g * 576));
  return groups === undefined ? res[0] : res;
}
// items: [{ signature, message, publicKey }] of BYTES (message: the raw message); { short, DST } -> boolean[]; false where the reference's
// verify returns false or its fromBytes throws
function blsVerifyBatch(items, opts) {
  const short = !!(opts && opts.short), pw = short ? 96 : 48, sw = short ? 48 : 96, m = short ? 1 : 2, L = 64, uw = 2 * m * 48;
  const dst = Buffer.from((opts && opts.DST) || (short ? 'BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_' : 'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_'));
  const verdict = items.map(() => false);
  const good = items.map((_, i) => i).filter((i) => items[i].signature.length === sw && items[i].publicKey.length === pw);
  if (good.length === 0) return verdict;
  const pk = new Uint8Array(good.length * pw), sig = new Uint8Array(good.length * sw), u = new Uint8Array(good.length * uw);
  good.forEach((i, k) => {
    pk.set(items[i].publicKey, k * pw); sig.set(items[i].signature, k * sw);
    const prb = expandMessageXmd(Buffer.from(items[i].message), dst, 2 * m * L);
    for (let e = 0; e < 2 * m; e++) {
      let v = 0n;
      for (let j = 0; j < L; j++) v = (v << 8n) | BigInt(prb[e * L + j]);
      leBytes(v % BLS_P, 48, u, k * uw + e * 48);
    }
  });
  init();
  const ok = native.bls(1, pk, sig, u, short ? 1 : 0);
  good.forEach((i, k) => { verdict[i] = ok[k] === 1; });
  return verdict;
}

module.exports = { CURVE, init, initMulti, register, install, uninstall, STATS, DEFAULT_MIN_POINTS, setPointCache, clearPointCache, packPoints, packScalars, pippenger, multiplyUnsafeBatch, multiplyBaseBatch, ed25519VerifyBatch,
                   PointSet, uploadPoints, uploadEncoded, interleavedMSMUnsafe, pippengerResident, multiplyUnsafeBatchResident, ed25519VerifyBatchDevice, ecdsaVerifyBatch, ecdsaVerifyBatchMsgs, schnorrVerifyBatch, ecdsaRecoverBatch,
                   fromBytesBatch, toBytesBatch, aggregateFromBytes, fftFr, polyFr, hashToCurveBatch, registerBls, pairingBatch, blsVerifyBatch,
                   x25519ScalarMultBatch, x25519GetPublicKeyBatch, ed25519ToMontgomeryBatch, x25519ScalarMult, x25519GetPublicKey, ed25519ToMontgomery,
                   ed25519GetPublicKeyBatch, ed25519SignBatch, ed25519GetPublicKey, ed25519Sign,
                   secp256k1GetPublicKeyBatch, ecdsaSignBatch, schnorrGetPublicKeyBatch, schnorrSignBatch, secp256k1GetPublicKey, schnorrGetPublicKey,
                   secp256k1Sign, schnorrSign,
                   x448ScalarMultBatch, x448GetPublicKeyBatch, ed448VerifyBatch,
                   ed448GetPublicKeyBatch, ed448SignBatch, ed448GetPublicKey, ed448Sign,
                   ristrettoFromBytesBatch, ristrettoToBytesBatch, ristrettoEqualsBatch, ristrettoMultiplyBatch, ristrettoMultiplyBaseBatch, ristrettoMsm,
                   ristrettoDeriveToCurveBatch, ristrettoFromBytes, ristrettoToBytes, ristrettoEquals, ristrettoMultiply, ristrettoMultiplyBase,
                   ristrettoDeriveToCurve, ristretto255_oprf,
                   secp256k1HashToCurveBatch, secp256k1EncodeToCurveBatch, ed25519HashToCurveBatch, ed25519EncodeToCurveBatch, hashToScalarBatch,
                   secp256k1_hasher, ed25519_hasher,
                   ed448_hasher, ed448HashToCurveBatch, ed448EncodeToCurveBatch, decaf448HashToCurveBatch, decaf448HashToScalarBatch,
                   decaf448FromBytesBatch, decaf448ToBytesBatch, decaf448EqualsBatch, decaf448MultiplyBatch, decaf448MultiplyBaseBatch,
                   decaf448DeriveToCurveBatch, native };
