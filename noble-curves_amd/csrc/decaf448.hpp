// decaf448 (RFC 9496 section 5) on the Ed448 field: the lane code of the kernels of decaf448.hip and of their CPU twins.
//
// Restates the formulas of the reference's _DecafPoint and decaf448_hasher (src/ed448.ts) on F448 values:
//   sqrtRatioM1 / invertSqrt  :462-466   decaf_sqrt_ratio_m1     uvRatio (:135-153) through fe448_pow_pm3d4, then the even one of +-value
//   fromBytes                 :569-595   decaf_decode_lane       one SQRT_RATIO_M1(1, u2 u1^2)
//   toBytes                   :610-621   decaf_encode_ext        one SQRT_RATIO_M1(1, (1 - d) u1 X^2), no inversion
//   equals                    :627-633   decaf_equals            two products: X1 Y2 == Y1 X2 and nothing else
//   calcElligatorDecafMap     :474-510   decaf_elligator         one SQRT_RATIO_M1(1 - 2 d, (r + 1) u1)
//   deriveToCurve             :689-700   decaf_from_uniform      two maps and the complete addition ed448_add
//   DECAF_BASE_X / _Y         :515-520   decaf_base              twice the Ed448 base, not ed448_base()
// The power chain fe448_pow_pm3d4 (445 squarings + 13 products) dominates every function here.
// An element is handled through an Edwards representative: the decoder returns the affine pair (x, y), an Ed448 affine point; the
// encoder takes any point of the curve; P and P + (0, -1) = (-x, -y) give the same 56 bytes, the translates by the points of order 4
// do not (the reference's toBytes does not fold them either: every representative a decaf448 operation produces lies in 2 E, where
// the two-torsion is all that is left).  a = 1 and d = -39081 throughout:
// "- 4 d s^2" is "+ 4 * 39081 s^2" and "d (r - 1)" is "39081 (1 - r)".
// Every intermediate carries its limb bound in its type (Fe448<B>, fe448.hpp); the comments name the bounds where they are not 1.
#pragma once
#include "consts_gen.hpp"
#include "ed448.hpp"

namespace ncg {

NCG_DI F448 decaf_const(const uint32_t (&c)[16]) {
  F448 r;
#pragma unroll
  for (int i = 0; i < 16; i++) r.v[i] = c[i];
  return r;
}
struct DecafConsts {  // src/ed448.ts:446-457, generated from d (tools/gen_consts.py); canonical limbs, bound 1
  static NCG_DI F448 one_minus_d() { return decaf_const(Decaf448Consts::ONE_MINUS_D); }
  static NCG_DI F448 one_minus_two_d() { return decaf_const(Decaf448Consts::ONE_MINUS_TWO_D); }
  static NCG_DI F448 sqrt_minus_d() { return decaf_const(Decaf448Consts::SQRT_MINUS_D); }
  static NCG_DI F448 invsqrt_minus_d() { return decaf_const(Decaf448Consts::INVSQRT_MINUS_D); }
};

struct Decaf448Ext {  // extended (X : Y : Z : T), T Z = X Y, bound 1
  F448 X, Y, Z, T;
};

NCG_DI F448 decaf_abs(const F448& a) {  // the non-negative (even) one of +-a
  return fe448_select(fe448_parity(a) != 0, fe448_neg(a), a);
}

// sqrtRatioM1 (ed448.ts:462-465) over uvRatio (:135-153): out = u^3 v (u^5 v^3)^((p - 3) / 4), made even; true iff v out^2 = u.
// For a non-square u / v the value is the reference's (it has no further meaning); v = 0 gives 0 and false unless u = 0.
// invertSqrt(v) is the u = 1 case.
NCG_DI bool decaf_sqrt_ratio_m1(const F448& u, const F448& v, F448& out) {
  const F448 u2v = fe448_sqr(u) * v;
  const F448 u3v = u2v * u;
  const F448 u5v3 = (u3v * u2v) * v;
  const F448 x = u3v * fe448_pow_pm3d4(u5v3);
  const bool valid = fe448_eq(fe448_sqr(x) * v, u);
  out = decaf_abs(x);
  return valid;
}

// fromBytes (ed448.ts:569-595) on the 14 LE words of an encoding.  false where the reference throws: s >= p or s odd
// ('encoding 1'); the ratio not a square ('encoding 2').  x, y: the affine representative of steps 5-7, meaningful only when the
// result is true.
NCG_DI bool decaf_decode_lane(const uint32_t (&w)[14], F448& x, F448& y) {
  uint32_t c[14];
  const F448 s = fe448_from_words(w);
  fe448_to_words(c, s);
  const bool ok = fe448_words_eq(c, w) && (w[0] & 1u) == 0;  // canonical and even
  const F448 s2 = fe448_sqr(s);                              // 1
  const auto u1 = F448::one() + s2;                          // 2 (bound 2)
  const F448 u1sq = fe448_sqr(u1);
  const F448 u2 = fe448_mulk_add<ED448_K>(u1sq, (s2 + s2) + (s2 + s2));  // 3: u1^2 - 4 d s^2 (the addend at bound 4)
  F448 I;
  const bool valid = decaf_sqrt_ratio_m1(F448::one(), u2 * u1sq, I);     // 4
  const F448 u3 = decaf_abs((((s + s) * I) * u1) * DecafConsts::sqrt_minus_d());  // 5: (2 * 1), (1 * 2)
  x = ((u3 * I) * u2) * DecafConsts::invsqrt_minus_d();                           // 6
  y = ((F448::one() - s2) * I) * u1;                                              // 7: (3 * 1), (1 * 2)
  return ok && valid;
}

// toBytes (ed448.ts:610-621) of an extended point (X : Y : Z : T), T Z = X Y; out = the 14 LE words of the encoding.  Y does not
// enter the formula.  The result does not depend on the projective scale: u1 and X^2 scale by the square, the root by its inverse
// up to sign, and both signs are fixed by the two absolute values.
NCG_DI void decaf_encode_ext(const F448& X, const F448& Y, const F448& Z, const F448& T, uint32_t (&out)[14]) {
  (void)Y;
  const F448 u1 = (X + T) * (X - T);  // 1: (2 * 3)
  const F448 x2 = fe448_sqr(X);
  F448 I;
  (void)decaf_sqrt_ratio_m1(F448::one(), (u1 * DecafConsts::one_minus_d()) * x2, I);  // 2: a square for every point of the curve
  const F448 ratio = decaf_abs((I * u1) * DecafConsts::sqrt_minus_d());               // 3
  const auto u2 = (DecafConsts::invsqrt_minus_d() * ratio) * Z - T;                   // 4 (bound 3)
  const F448 s = decaf_abs(((DecafConsts::one_minus_d() * I) * X) * u2);              // 5: (1 * 3)
  fe448_to_words(out, s);
}
// an affine wire point: Z = 1, T = x y
NCG_DI void decaf_encode_affine(const F448& x, const F448& y, uint32_t (&out)[14]) {
  decaf_encode_ext(x, y, F448::one(), x * y, out);
}
// a projective Ed448Pt through the extended representative (X Z : Y Z : Z^2 : X Y) of the same point: what ed448_mul and
// ed448_add hand over, encoded without the inversion of the affine conversion
NCG_DI void decaf_encode_proj(const Ed448Pt& p, uint32_t (&out)[14]) {
  decaf_encode_ext(p.X * p.Z, p.Y * p.Z, fe448_sqr(p.Z), p.X * p.Y, out);
}

// equals (ed448.ts:627-633): x1 y2 == y1 x2, on affine representatives (the test is homogeneous); no second clause
NCG_DI bool decaf_equals(const F448& x1, const F448& y1, const F448& x2, const F448& y2) { return fe448_eq(x1 * y2, y1 * x2); }

// calcElligatorDecafMap (ed448.ts:474-510, RFC 9496 section 5.3.4 MAP): an extended Edwards representative
NCG_DI Decaf448Ext decaf_elligator(const F448& r0) {
  const F448 one = F448::one();
  const F448 r = fe448_neg(fe448_sqr(r0));                                 // 1
  const F448 u0 = fe448_mulk_add<ED448_K>(F448::zero(), one - r);          // 2: d (r - 1) = 39081 (1 - r) (the factor at bound 3)
  const F448 u1 = (u0 + one) * (u0 - r);                                   // 3: (2 * 3)
  const auto rp1 = r + one;                                                // bound 2
  F448 v;
  const bool sq = decaf_sqrt_ratio_m1(DecafConsts::one_minus_two_d(), rp1 * u1, v);  // 4
  const F448 vp = fe448_select(sq, v, r0 * v);                                        // 5
  const F448 sgn = fe448_select(sq, one, fe448_neg(one));                             // 6
  const F448 s = vp * rp1;                                                            // 7
  const F448 s_abs = decaf_abs(s);
  const F448 s2 = fe448_sqr(s);
  const auto W0 = s_abs + s_abs;  // 8 (bound 2)
  const auto W1 = s2 + one;       // 9 (bound 2)
  const auto W2 = s2 - one;       // 10 (bound 3)
  const auto W3 = (((vp * s) * (r - one)) * DecafConsts::one_minus_two_d()) + sgn;  // 11: (1 * 3), then bound 2
  return Decaf448Ext{W0 * W3, W2 * W1, W1 * W3, W0 * W2};                           // (2 * 2), (3 * 2), (2 * 2), (2 * 3)
}

// deriveToCurve (ed448.ts:689-700) on the 28 LE words of 112 uniform bytes: each half reduced mod p - no bit is masked, the
// values p .. 2^448 - 1 are accepted - mapped, and the two points added by the complete addition.
NCG_DI Ed448Pt decaf_from_uniform(const uint32_t (&w)[28]) {
  uint32_t h[14];
#pragma unroll
  for (int i = 0; i < 14; i++) h[i] = w[i];
  const Decaf448Ext R1 = decaf_elligator(fe448_from_words(h));  // congruent to the residue
#pragma unroll
  for (int i = 0; i < 14; i++) h[i] = w[14 + i];
  const Decaf448Ext R2 = decaf_elligator(fe448_from_words(h));
  return ed448_add(Ed448Pt{R1.X, R1.Y, R1.Z}, Ed448Pt{R2.X, R2.Y, R2.Z});
}

NCG_DI Ed448Pt decaf_base() {  // ed448.ts:515-520: twice the Ed448 base
  return Ed448Pt{decaf_const(Decaf448Consts::BASE_X), decaf_const(Decaf448Consts::BASE_Y), F448::one()};
}

// ---- one row of each batch operation: 56-byte rows are 14 LE words, affine points x || y 28 words
// enc -> x || y (28 words), zero where refused (as ed448_decode_lane leaves a refused row)
NCG_DI bool decaf_decode_row(const uint32_t* __restrict__ enc, uint32_t* __restrict__ out) {
  uint32_t w[14], xw[14], yw[14];
#pragma unroll
  for (int i = 0; i < 14; i++) w[i] = enc[i];
  F448 x, y;
  const bool ok = decaf_decode_lane(w, x, y);
  fe448_to_words(xw, x);
  fe448_to_words(yw, y);
#pragma unroll
  for (int i = 0; i < 14; i++) {
    out[i] = ok ? xw[i] : 0u;
    out[14 + i] = ok ? yw[i] : 0u;
  }
  return ok;
}

NCG_DI void decaf_encode_row(const uint32_t* __restrict__ affine, uint32_t* __restrict__ out) {
  Ed448Pt p;
  ed448_affine_load(affine, p);
  uint32_t w[14];
  decaf_encode_affine(p.X, p.Y, w);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = w[i];
}

NCG_DI bool decaf_equals_row(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b) {
  Ed448Pt p, q;
  ed448_affine_load(a, p);
  ed448_affine_load(b, q);
  return decaf_equals(p.X, p.Y, q.X, q.Y);
}

NCG_DI void decaf_from_uniform_row(const uint32_t* __restrict__ uniform, uint32_t* __restrict__ out) {
  uint32_t u[28], w[14];
#pragma unroll
  for (int i = 0; i < 28; i++) u[i] = uniform[i];
  decaf_encode_proj(decaf_from_uniform(u), w);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = w[i];
}

// fromBytes(enc).multiplyUnsafe(k).toBytes(), k any value below 2^448: decode, ed448_mul and the encoding of the projective result
// in one lane; a zero row where the encoding is refused.  enc = NULL: the decaf base.
NCG_DI bool decaf_mul_row(const uint32_t* __restrict__ enc, const uint32_t* __restrict__ k56, uint32_t* __restrict__ out) {
  uint32_t w[14], k[14];
#pragma unroll
  for (int i = 0; i < 14; i++) {
    w[i] = enc ? enc[i] : 0u;
    k[i] = k56[i];
  }
  Ed448Pt p = decaf_base();
  bool ok = true;
  if (enc) {
    p.Z = F448::one();
    ok = decaf_decode_lane(w, p.X, p.Y);
  }
  decaf_encode_proj(ed448_mul(p, k), w);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = ok ? w[i] : 0u;
  return ok;
}

// ---- the pieces on raw limbs (ncg_decaf448_check, ht_decaf448_op).  Words per row (a, b, out), include/ncg.h has the same table;
// every input element is 16 limbs at bound 1, every output element 16 limbs at bound 1:
//   0 SQRT_RATIO_M1(u, v): a = u, b = v; out[0..16) = the value (even), out[16] = 1 if u / v is a square       (16, 16, 17)
//   1 encode_ext: a = X Y Z T; out = the 14 LE words of the encoding                                            (64,  0, 14)
//   2 the Elligator map: a = r0; out = X Y Z T of the extended representative                                   (16,  0, 64)
constexpr int DECAF448_CHECK_OPS = 3;
NCG_DI void decaf448_check_widths(int op, int& wa, int& wb, int& wo) {
  const int A[DECAF448_CHECK_OPS] = {16, 64, 16};
  const int B[DECAF448_CHECK_OPS] = {16, 0, 0};
  const int O[DECAF448_CHECK_OPS] = {17, 14, 64};
  const bool known = op >= 0 && op < DECAF448_CHECK_OPS;
  wa = known ? A[op] : 0;
  wb = known ? B[op] : 0;
  wo = known ? O[op] : 0;
}

NCG_DI int decaf448_check_op(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  switch (op) {
    case 0: {
      F448 r;
      const bool sq = decaf_sqrt_ratio_m1(fe448_raw<1>(a), fe448_raw<1>(b), r);
      fe448_raw_store(out, r);
      out[16] = sq ? 1u : 0u;
      return 0;
    }
    case 1: {
      uint32_t w[14];
      decaf_encode_ext(fe448_raw<1>(a), fe448_raw<1>(a + 16), fe448_raw<1>(a + 32), fe448_raw<1>(a + 48), w);
#pragma unroll
      for (int i = 0; i < 14; i++) out[i] = w[i];
      return 0;
    }
    case 2: {
      const Decaf448Ext p = decaf_elligator(fe448_raw<1>(a));
      fe448_raw_store(out, p.X);
      fe448_raw_store(out + 16, p.Y);
      fe448_raw_store(out + 32, p.Z);
      fe448_raw_store(out + 48, p.T);
      return 0;
    }
    default: return -1;
  }
}

}  // namespace ncg
