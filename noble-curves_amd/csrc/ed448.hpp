// X448 (RFC 7748) and Ed448-Goldilocks (RFC 8032) on Fe448 (fe448.hpp): the lane code of the kernels of ed448.hip and of their
// CPU twins.  Reproduces the values of the reference's src/ed448.ts over src/abstract/montgomery.ts and src/abstract/edwards.ts:
//   x448.scalarMult(scalar, u) = encodeU(montgomeryLadder(decodeU(u), decodeScalar(scalar)))           (montgomery.ts:294-331)
//   decodeScalar = adjustScalarBytes (b[0] &= 252, b[55] |= 128, ed448.ts:122-130) then little-endian
//   decodeU      = mod p, NO masked bit: p .. 2^448 - 1 are accepted                                    (montgomery.ts:277-287)
//   0, 1 and p - 1 are refused before the ladder, a zero result after it                               (:303-330)
//   Point.fromBytes strict (edwards.ts:405-436) with uvRatio (ed448.ts:135-153), Point.toBytes (edwards.ts:620-628),
//   Point.add / double over a = 1, d = -39081, eddsa.verify (edwards.ts:942-989), toMontgomery (ed448.ts:171-179)
// One ladder step is montgomery.ts:366-386 with a24 = 39081 on values with declared limb bounds:
//   A = x2 + z2 (2)   B = x2 - z2 (3)   C = x3 + z3 (2)   D = x3 - z3 (3)
//   AA = A^2          BB = B^2 (B takes the weak pass inside fe448_sqr)
//   DA = D A (3 * 2)  CB = C B (2 * 3)
//   x3' = (DA + CB)^2 (2)       z3' = x1 (DA - CB)^2 (the difference, bound 3, weak pass inside fe448_sqr)
//   x2' = AA BB       E = AA - BB (3)      z2' = E (AA + a24 E): fe448_mulk_add
// Per step 5 products + 4 squares + the chain of AA + a24 E: 5 * 256 + 4 * 136 + 16 = 1840 multiply-adds, 64 selects.
// Nothing in the ladder branches or indexes on a scalar bit: the swap is a per-limb select.
//
// Edwards points are projective (X : Y : Z); the formulas are add-2007-bl and dbl-2007-bl for a = 1, complete because d is not
// a square: the identity (0 : 1 : 1), the point of order 2 (0 : -1 : 1), the points of order 4 (+-1 : 0 : 1), P = Q and P = -Q
// take the same path as everything else.  d = -39081 enters as "+ 39081 ..." with the signs of the formula turned.
#pragma once
#include "fe448.hpp"

namespace ncg {

constexpr uint32_t ED448_K = 39081u;  // a24 of curve448 = (156326 - 2) / 4, and -d of edwards448 (ed448.ts:60-62, montgomery.ts:263)

struct X448State {  // (x2 : z2) and (x3 : z3), bound 1
  F448 x2, z2, x3, z3;
};

NCG_DI void fe448_cswap(uint32_t swap, F448& a, F448& b) {  // swap = 0 / 1: per-limb selects, no branch
  const bool s = swap != 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint32_t x = a.v[i], y = b.v[i];
    a.v[i] = s ? y : x;
    b.v[i] = s ? x : y;
  }
}
NCG_DI F448 fe448_select(bool s, const F448& a, const F448& b) {  // s ? a : b
  F448 r;
#pragma unroll
  for (int i = 0; i < 16; i++) r.v[i] = s ? a.v[i] : b.v[i];
  return r;
}

// cswap(swap) then the ladder step of montgomery.ts:366-386
NCG_DI void x448_step(X448State& st, const F448& x1, uint32_t swap) {
  fe448_cswap(swap, st.x2, st.x3);
  fe448_cswap(swap, st.z2, st.z3);
  const auto A = st.x2 + st.z2;
  const auto B = st.x2 - st.z2;
  const auto C = st.x3 + st.z3;
  const auto D = st.x3 - st.z3;
  const F448 AA = fe448_sqr(A);
  const F448 BB = fe448_sqr(B);
  const F448 DA = D * A;
  const F448 CB = C * B;
  st.x3 = fe448_sqr(DA + CB);
  st.z3 = x1 * fe448_sqr(DA - CB);
  st.x2 = AA * BB;
  const auto E = AA - BB;
  st.z2 = E * fe448_mulk_add<ED448_K>(AA, E);
}

// adjustScalarBytes on 14 LE words (ed448.ts:122-130)
NCG_DI void x448_decode_scalar(uint32_t (&k)[14]) {
  k[0] &= 0xfffffffcu;
  k[13] |= 0x80000000u;
}

NCG_DI void fe448_p_words(uint32_t (&w)[14], uint32_t low) {  // p with its lowest word replaced: p - 1 = (.., 0xfffffffe)
#pragma unroll
  for (int i = 0; i < 14; i++) w[i] = i == 7 ? 0xfffffffeu : 0xffffffffu;
  w[0] = low;
}

// decodeU + the low-order test: w = the 14 LE words of the encoding; on return w = the canonical residue, u = its field form.
// false for 0, 1 and p - 1 (montgomery.ts:303-313)
NCG_DI bool x448_decode_u(uint32_t (&w)[14], F448& u) {
  uint32_t pm[14];
  fe448_p_words(pm, 0xfffffffeu);
  u = fe448_from_words(w);
  fe448_to_words(w, u);
  const bool low = fe448_words_small(w, 0u) || fe448_words_small(w, 1u) || fe448_words_eq(w, pm);
  return !low;
}

// one left shift of a 448-bit register; returns the bit that falls out (bit 447)
NCG_DI uint32_t ed448_shl1(uint32_t (&k)[14]) {
  const uint32_t top = k[13] >> 31;
#pragma unroll
  for (int i = 13; i >= 0; i--) k[i] = (k[i] << 1) | (i > 0 ? k[i - 1] >> 31 : 0u);
  return top;
}

// montgomeryLadder (montgomery.ts:352-393) without the final division.  The swap bit of step t is bit t of k ^ (k >> 1); the
// register is shifted left once per step so that the bit is always the top one - no index depends on t or on the scalar.
NCG_DI X448State x448_ladder(const uint32_t (&k)[14], const F448& x1) {
  uint32_t kx[14];
#pragma unroll
  for (int i = 0; i < 14; i++) kx[i] = k[i] ^ ((k[i] >> 1) | (i < 13 ? k[i + 1] << 31 : 0u));
  X448State st{F448::one(), F448::zero(), x1, F448::one()};
  for (int t = 447; t >= 0; t--) {
    const uint32_t swap = ed448_shl1(kx);
    x448_step(st, x1, swap);
  }
  const uint32_t last = k[0] & 1u;
  fe448_cswap(last, st.x2, st.x3);
  fe448_cswap(last, st.z2, st.z3);
  return st;
}

// One scalarMult: raw 56-byte scalar and u as 14 LE words each, or u = NULL for the base point u = 5; out = the 14 LE words of
// the result, zero where refused.
NCG_DI bool x448_lane(const uint32_t* __restrict__ scalar, const uint32_t* __restrict__ uenc, uint32_t (&out)[14]) {
  uint32_t k[14], w[14];
#pragma unroll
  for (int i = 0; i < 14; i++) {
    k[i] = scalar[i];
    w[i] = uenc ? uenc[i] : (i == 0 ? 5u : 0u);
  }
  x448_decode_scalar(k);
  F448 x1;
  bool ok = x448_decode_u(w, x1);
  const X448State st = x448_ladder(k, x1);
  const F448 r = st.x2 * fe448_inv(st.z2);
  fe448_to_words(out, r);
  ok = ok && !fe448_words_small(out, 0u);  // montgomery.ts:329
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = ok ? out[i] : 0u;
  return ok;
}

// ---- Ed448
struct Ed448Pt {  // projective, bound 1
  F448 X, Y, Z;
};
NCG_DI Ed448Pt ed448_identity() { return Ed448Pt{F448::zero(), F448::one(), F448::one()}; }
NCG_DI Ed448Pt ed448_select(bool s, const Ed448Pt& a, const Ed448Pt& b) {
  return Ed448Pt{fe448_select(s, a.X, b.X), fe448_select(s, a.Y, b.Y), fe448_select(s, a.Z, b.Z)};
}
NCG_DI Ed448Pt ed448_neg(const Ed448Pt& p) { return Ed448Pt{fe448_neg(p.X), p.Y, p.Z}; }

// add-2007-bl, a = 1, d = -39081: 10 products, 1 square, 1 small-constant chain = 2712 multiply-adds
NCG_DI Ed448Pt ed448_add(const Ed448Pt& p, const Ed448Pt& q) {
  const F448 A = p.Z * q.Z;
  const F448 B = fe448_sqr(A);
  const F448 C = p.X * q.X;
  const F448 D = p.Y * q.Y;
  const F448 K = fe448_mulk_add<ED448_K>(F448::zero(), C * D);  // -E = 39081 C D
  const auto F = B + K;                                          // B - E (2)
  const auto G = B - K;                                          // B + E (3)
  const F448 T = (p.X + p.Y) * (q.X + q.Y);
  const F448 AF = A * F, AG = A * G;
  Ed448Pt r;
  r.X = AF * ((T - C) - D);  // 1 * 5
  r.Y = AG * (D - C);        // 1 * 3
  r.Z = F * G;               // 2 * 3
  return r;
}

// dbl-2007-bl, a = 1: 3 products, 4 squares = 1312 multiply-adds
NCG_DI Ed448Pt ed448_dbl(const Ed448Pt& p) {
  const F448 B = fe448_sqr(p.X + p.Y);
  const F448 C = fe448_sqr(p.X);
  const F448 D = fe448_sqr(p.Y);
  const auto F = C + D;  // 2
  const F448 H = fe448_sqr(p.Z);
  const F448 J = fe448_weak(F - (H + H));
  Ed448Pt r;
  r.X = ((B - C) - D) * J;  // 5 * 1
  r.Y = F * (C - D);        // 2 * 3
  r.Z = F * J;
  return r;
}

NCG_DI bool ed448_is_identity(const Ed448Pt& p) { return fe448_is_zero(p.X) && fe448_eq(p.Y, p.Z); }
// isSmallOrder: [4]P is the identity
NCG_DI bool ed448_is_small_order(const Ed448Pt& p) { return ed448_is_identity(ed448_dbl(ed448_dbl(p))); }

// the 57 bytes of an encoding: 14 LE words and the last byte.  Packed rows sit at any address: byte loads.
NCG_DI uint32_t ed448_load57(const uint8_t* __restrict__ e, uint32_t (&w)[14]) {
#pragma unroll
  for (int i = 0; i < 14; i++)
    w[i] = (uint32_t)e[4 * i] | ((uint32_t)e[4 * i + 1] << 8) | ((uint32_t)e[4 * i + 2] << 16) | ((uint32_t)e[4 * i + 3] << 24);
  return e[56];
}
NCG_DI void ed448_store57(uint8_t* __restrict__ e, const uint32_t (&w)[14], uint32_t last) {
#pragma unroll
  for (int i = 0; i < 14; i++) {
    e[4 * i] = (uint8_t)w[i];
    e[4 * i + 1] = (uint8_t)(w[i] >> 8);
    e[4 * i + 2] = (uint8_t)(w[i] >> 16);
    e[4 * i + 3] = (uint8_t)(w[i] >> 24);
  }
  e[56] = (uint8_t)last;
}

// Point.fromBytes, zip215 = false (edwards.ts:405-436): y < p (so every bit of byte 56 but the sign must be clear), x^2 = u / v
// with u = y^2 - 1, v = d y^2 - 1 through uvRatio (ed448.ts:135-153): x = u^3 v (u^5 v^3)^((p - 3) / 4), valid iff v x^2 = u;
// x = 0 with the sign bit is refused; x is negated where its parity differs from the sign bit.
// Here u and v are both taken with the opposite sign (1 - y^2, 39081 y^2 + 1): u^3 v, u^5 v^3 and the test are unchanged by that.
NCG_DI bool ed448_decode(const uint32_t (&w)[14], uint32_t last, F448& x, F448& y) {
  uint32_t c[14];
  y = fe448_from_words(w);
  fe448_to_words(c, y);
  bool ok = (last & 0x7fu) == 0 && fe448_words_eq(c, w);
  const uint32_t sign = (last >> 7) & 1u;
  const F448 y2 = fe448_sqr(y);
  const F448 u = fe448_weak(F448::one() - y2);
  const F448 v = fe448_mulk_add<ED448_K>(F448::one(), y2);
  const F448 u2v = fe448_sqr(u) * v;
  const F448 u3v = u2v * u;
  const F448 u5v3 = (u3v * u2v) * v;
  x = u3v * fe448_pow_pm3d4(u5v3);
  ok = ok && fe448_eq(fe448_sqr(x) * v, u);
  fe448_to_words(c, x);
  const bool x0 = fe448_words_small(c, 0u);
  ok = ok && !(x0 && sign);
  x = fe448_select((c[0] & 1u) != sign, fe448_neg(x), x);
  return ok;
}

// Point.toBytes of an affine point: y in 56 bytes, the parity of x in bit 7 of byte 56
NCG_DI uint32_t ed448_encode(const F448& x, const F448& y, uint32_t (&w)[14]) {
  fe448_to_words(w, y);
  return fe448_parity(x) << 7;
}
NCG_DI uint32_t ed448_encode_proj(const Ed448Pt& p, uint32_t (&w)[14]) {
  const F448 zi = fe448_inv(p.Z);
  return ed448_encode(p.X * zi, p.Y * zi, w);
}

NCG_DI Ed448Pt ed448_base() {  // ed448.ts:63-68 Gx, Gy as LE words
  const uint32_t gx[14] = {0xc70cc05eu, 0x2626a82bu, 0x8b00938eu, 0x433b80e1u, 0x2ab66511u, 0x12ae1af7u, 0xa3d3a464u,
                           0xea6de324u, 0x470f1767u, 0x9e146570u, 0x22bf36dau, 0x221d15a6u, 0x6bed0dedu, 0x4f1970c6u};
  const uint32_t gy[14] = {0xf230fa14u, 0x9808795bu, 0x4ed7c8adu, 0xfdbd132cu, 0xe67c39c4u, 0x3ad3ff1cu, 0x05a0c2d7u,
                           0x87789c1eu, 0x6ca39840u, 0x4bea7373u, 0x56c9c762u, 0x88762037u, 0x6eb6bc24u, 0x693f4671u};
  return Ed448Pt{fe448_from_words(gx), fe448_from_words(gy), F448::one()};
}

// [k]P, k any value below 2^448 (multiplyUnsafe): double, add, keep the sum where the bit is set - a select, the lanes of a wave
// would run both sides of a branch anyway.  448 doublings + 448 additions.
NCG_DI Ed448Pt ed448_mul(const Ed448Pt& p, const uint32_t (&k)[14]) {
  uint32_t kk[14];
#pragma unroll
  for (int i = 0; i < 14; i++) kk[i] = k[i];
  Ed448Pt q = ed448_identity();
  for (int t = 447; t >= 0; t--) {
    const uint32_t bit = ed448_shl1(kk);
    q = ed448_dbl(q);
    q = ed448_select(bit != 0, ed448_add(q, p), q);
  }
  return q;
}

// [s]B + [k]A2 by Straus with one-bit digits: the table {B, A2, B + A2} stays in registers and is read by selects
NCG_DI Ed448Pt ed448_mul2_base(const uint32_t (&s)[14], const Ed448Pt& a2, const uint32_t (&k)[14]) {
  uint32_t ss[14], kk[14];
#pragma unroll
  for (int i = 0; i < 14; i++) {
    ss[i] = s[i];
    kk[i] = k[i];
  }
  const Ed448Pt b = ed448_base();
  const Ed448Pt ba = ed448_add(b, a2);
  Ed448Pt q = ed448_identity();
  for (int t = 447; t >= 0; t--) {
    const uint32_t sb = ed448_shl1(ss), kb = ed448_shl1(kk);
    q = ed448_dbl(q);
    const Ed448Pt addend = ed448_select(kb != 0, ed448_select(sb != 0, ba, a2), b);
    q = ed448_select((sb | kb) != 0, ed448_add(q, addend), q);
  }
  return q;
}

NCG_DI bool ed448_scalar_below_n(const uint32_t (&s)[14]) {  // s < n (ed448.ts:55-57)
  const uint32_t n[14] = {0xab5844f3u, 0x2378c292u, 0x8dc58f55u, 0x216cc272u, 0xaed63690u, 0xc44edb49u, 0x7cca23e9u,
                          0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x3fffffffu};
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    const uint64_t d = (uint64_t)s[i] - n[i] - borrow;
    borrow = (uint32_t)(d >> 63);
  }
  return borrow != 0;
}

// eddsa.verify, strict (edwards.ts:942-989), the challenge k given: sig = R (57) || s (57), pk = A (57), k = 14 LE words
NCG_DI bool ed448_verify_lane(const uint8_t* __restrict__ sig, const uint8_t* __restrict__ pk, const uint32_t* __restrict__ k56) {
  uint32_t aw[14], rw[14], s[14], k[14];
  const uint32_t al = ed448_load57(pk, aw), rl = ed448_load57(sig, rw), sl = ed448_load57(sig + 57, s);
#pragma unroll
  for (int i = 0; i < 14; i++) k[i] = k56[i];
  Ed448Pt A, R;
  A.Z = R.Z = F448::one();
  bool ok = ed448_decode(aw, al, A.X, A.Y);
  ok = ed448_decode(rw, rl, R.X, R.Y) && ok;
  ok = ok && sl == 0 && ed448_scalar_below_n(s);
  ok = ok && !ed448_is_small_order(A);
  // [s]B - [k]A - R, then the cofactor
  Ed448Pt q = ed448_mul2_base(s, ed448_neg(A), k);
  q = ed448_add(q, ed448_neg(R));
  return ok && ed448_is_small_order(q);
}

// fromBytes(enc).multiplyUnsafe(k).toBytes(); a zero row where the encoding is refused
NCG_DI bool ed448_mul_lane(const uint8_t* __restrict__ enc, const uint32_t* __restrict__ k56, uint8_t* __restrict__ out) {
  uint32_t w[14], k[14];
  const uint32_t last = ed448_load57(enc, w);
#pragma unroll
  for (int i = 0; i < 14; i++) k[i] = k56[i];
  Ed448Pt p;
  p.Z = F448::one();
  const bool ok = ed448_decode(w, last, p.X, p.Y);
  const Ed448Pt q = ed448_mul(p, k);
  uint32_t o = ed448_encode_proj(q, w);
#pragma unroll
  for (int i = 0; i < 14; i++) w[i] = ok ? w[i] : 0u;
  o = ok ? o : 0u;
  ed448_store57(out, w, o);
  return ok;
}

NCG_DI void ed448_mul_base_lane(const uint32_t* __restrict__ k56, uint8_t* __restrict__ out) {
  uint32_t w[14], k[14];
#pragma unroll
  for (int i = 0; i < 14; i++) k[i] = k56[i];
  const Ed448Pt q = ed448_mul(ed448_base(), k);
  const uint32_t o = ed448_encode_proj(q, w);
  ed448_store57(out, w, o);
}

// enc -> x || y (28 words), zero where refused
NCG_DI bool ed448_decode_lane(const uint8_t* __restrict__ enc, uint32_t* __restrict__ out) {
  uint32_t w[14], xw[14], yw[14];
  const uint32_t last = ed448_load57(enc, w);
  F448 x, y;
  const bool ok = ed448_decode(w, last, x, y);
  fe448_to_words(xw, x);
  fe448_to_words(yw, y);
#pragma unroll
  for (int i = 0; i < 14; i++) {
    out[i] = ok ? xw[i] : 0u;
    out[14 + i] = ok ? yw[i] : 0u;
  }
  return ok;
}

NCG_DI void ed448_affine_load(const uint32_t* __restrict__ a, Ed448Pt& p) {
  uint32_t xw[14], yw[14];
#pragma unroll
  for (int i = 0; i < 14; i++) {
    xw[i] = a[i];
    yw[i] = a[14 + i];
  }
  p = Ed448Pt{fe448_from_words(xw), fe448_from_words(yw), F448::one()};
}

NCG_DI void ed448_encode_lane(const uint32_t* __restrict__ affine, uint8_t* __restrict__ out) {
  Ed448Pt p;
  ed448_affine_load(affine, p);
  uint32_t w[14];
  const uint32_t o = ed448_encode(p.X, p.Y, w);
  ed448_store57(out, w, o);
}

// Point.add / Point.subtract on affine points, the result affine
NCG_DI void ed448_add_pairs_lane(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int subtract, uint32_t* __restrict__ out) {
  Ed448Pt p, q;
  ed448_affine_load(a, p);
  ed448_affine_load(b, q);
  q.X = fe448_select(subtract != 0, fe448_neg(q.X), q.X);
  const Ed448Pt r = ed448_add(p, q);
  const F448 zi = fe448_inv(r.Z);
  uint32_t xw[14], yw[14];
  fe448_to_words(xw, r.X * zi);
  fe448_to_words(yw, r.Y * zi);
#pragma unroll
  for (int i = 0; i < 14; i++) {
    out[i] = xw[i];
    out[14 + i] = yw[i];
  }
}

// ed448.utils.toMontgomery (ed448.ts:171-179): u = y^2 / x^2 of the strictly decoded key; refused for x = 0 (the reference's
// inversion of zero throws)
NCG_DI bool ed448_to_montgomery_lane(const uint8_t* __restrict__ pk, uint32_t (&out)[14]) {
  uint32_t w[14];
  const uint32_t last = ed448_load57(pk, w);
  F448 x, y;
  bool ok = ed448_decode(w, last, x, y);
  ok = ok && !fe448_is_zero(x);
  const F448 r = fe448_sqr(y * fe448_inv(x));
  fe448_to_words(out, r);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = ok ? out[i] : 0u;
  return ok;
}

// ---- the pieces on raw limbs (ncg_fe448_check, ht_fe448_op).  Words per row (a, b, out), include/ncg.h has the same table:
//   0 mul (16, 16, 16)   1 sqr (16, 0, 16)   2 a + b, a - b, -a (16, 16, 48)   3 a + 39081 b (16, 16, 16)
//   4 canonical store: 16 limbs -> 14 words (16, 0, 14)   5 load: 14 words -> 16 limbs (14, 0, 16)
//   6 x^((p - 3) / 4) (16, 0, 16)   7 inversion (16, 0, 16)   8 x448_step, swap = variant & 1: a = x2 z2 x3 z3, b = x1 (64, 16, 64)
//   9 ed448_add: a, b = X Y Z (48, 48, 48)   10 ed448_dbl (48, 0, 48)
constexpr int FE448_CHECK_OPS = 11;
NCG_DI void fe448_check_widths(int op, int& wa, int& wb, int& wo) {
  const int A[FE448_CHECK_OPS] = {16, 16, 16, 16, 16, 14, 16, 16, 64, 48, 48};
  const int B[FE448_CHECK_OPS] = {16, 0, 16, 16, 0, 0, 0, 0, 16, 48, 0};
  const int O[FE448_CHECK_OPS] = {16, 16, 48, 16, 14, 16, 16, 16, 64, 48, 48};
  const bool known = op >= 0 && op < FE448_CHECK_OPS;
  wa = known ? A[op] : 0;
  wb = known ? B[op] : 0;
  wo = known ? O[op] : 0;
}

template <int B>
NCG_DI Fe448<B> fe448_raw(const uint32_t* __restrict__ p) {
  Fe448<B> r;
#pragma unroll
  for (int i = 0; i < 16; i++) r.v[i] = p[i];
  return r;
}
template <int B>
NCG_DI void fe448_raw_store(uint32_t* __restrict__ p, const Fe448<B>& a) {
#pragma unroll
  for (int i = 0; i < 16; i++) p[i] = a.v[i];
}

// Input bounds: ops 0, 3: a at 3, b at 2 (the widest pair the ladder multiplies); 1: a at 2; 2: both at 1 (out at 2, 3, 1);
// 4: a at 8; 6, 7, 8, 9, 10: every element at 1.  Output elements are at bound 1 unless stated.
NCG_DI int fe448_check_op(int op, int variant, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  switch (op) {
    case 0: fe448_raw_store(out, fe448_raw<3>(a) * fe448_raw<2>(b)); return 0;
    case 1: fe448_raw_store(out, fe448_sqr(fe448_raw<2>(a))); return 0;
    case 2: {
      const F448 x = fe448_raw<1>(a), y = fe448_raw<1>(b);
      fe448_raw_store(out, x + y);
      fe448_raw_store(out + 16, x - y);
      fe448_raw_store(out + 32, fe448_neg(x));
      return 0;
    }
    case 3: fe448_raw_store(out, fe448_mulk_add<ED448_K>(fe448_raw<3>(a), fe448_raw<2>(b))); return 0;
    case 4: {
      uint32_t w[14];
      fe448_to_words(w, fe448_raw<8>(a));
#pragma unroll
      for (int i = 0; i < 14; i++) out[i] = w[i];
      return 0;
    }
    case 5: {
      uint32_t w[14];
#pragma unroll
      for (int i = 0; i < 14; i++) w[i] = a[i];
      fe448_raw_store(out, fe448_from_words(w));
      return 0;
    }
    case 6: fe448_raw_store(out, fe448_pow_pm3d4(fe448_raw<1>(a))); return 0;
    case 7: fe448_raw_store(out, fe448_inv(fe448_raw<1>(a))); return 0;
    case 8: {
      X448State st{fe448_raw<1>(a), fe448_raw<1>(a + 16), fe448_raw<1>(a + 32), fe448_raw<1>(a + 48)};
      x448_step(st, fe448_raw<1>(b), (uint32_t)variant & 1u);
      fe448_raw_store(out, st.x2);
      fe448_raw_store(out + 16, st.z2);
      fe448_raw_store(out + 32, st.x3);
      fe448_raw_store(out + 48, st.z3);
      return 0;
    }
    case 9:
    case 10: {
      const Ed448Pt p{fe448_raw<1>(a), fe448_raw<1>(a + 16), fe448_raw<1>(a + 32)};
      Ed448Pt r;
      if (op == 9) r = ed448_add(p, Ed448Pt{fe448_raw<1>(b), fe448_raw<1>(b + 16), fe448_raw<1>(b + 32)});
      else r = ed448_dbl(p);
      fe448_raw_store(out, r.X);
      fe448_raw_store(out + 16, r.Y);
      fe448_raw_store(out + 32, r.Z);
      return 0;
    }
    default: return -1;
  }
}

}  // namespace ncg
