// ristretto255 (RFC 9496) on the ed25519 field: the lane code of the kernels of ristretto.hip and of their CPU twins.
//
// Restates the formulas of the reference's _RistrettoPoint and ristretto255_hasher (src/ed25519.ts) on FEd values:
//   fromBytes                 :510-533   ristretto_decode_lane   one SQRT_RATIO_M1(1, v u2^2): 1 + 8 squarings / 10 products + the chain
//   toBytes                   :548-572   ristretto_encode_ext    one SQRT_RATIO_M1(1, u1 u2^2), no inversion
//   equals                    :578-586   ristretto_equals        four products
//   calcElligatorRistrettoMap :443-461   ristretto_elligator     one SQRT_RATIO_M1(Ns, D)
//   deriveToCurve             :658-666   ristretto_from_uniform  two maps and the unified addition
// SQRT_RATIO_M1 is ed_uv_ratio (ec_te.hpp): for a non-square u / v it already returns the non-negative sqrt(i u / v) RFC 9496
// section 4.2 asks for.  The power chain ed_pow_p58 (250 squarings + 11 products) dominates every function here.
// An element is handled through an Edwards representative: the decoder returns the affine pair (x, y), which is an ed25519 wire
// point (Z = 1, T = x y); the encoder takes any point of the curve and maps its whole coset P + E[4] to the same 32 bytes.
// The a of the curve is -1 throughout: 1 + a s^2 = 1 - s^2, a d u1^2 - u2^2 = -(d u1^2 + u2^2), and c = -1 in the map.
#pragma once
#include "ec_te.hpp"

namespace ncg {

struct RistrettoConsts {  // src/ed25519.ts:410-424, generated from d and sqrt(-1) (tools/gen_consts.py)
  static NCG_DI FEd sqrt_ad_minus_one() { return FEd::from_limbs(Fe9EdPR::SQRT_AD_MINUS_ONE); }
  static NCG_DI FEd invsqrt_a_minus_d() { return FEd::from_limbs(Fe9EdPR::INVSQRT_A_MINUS_D); }
  static NCG_DI FEd one_minus_d_sq() { return FEd::from_limbs(Fe9EdPR::ONE_MINUS_D_SQ); }
  static NCG_DI FEd d_minus_one_sq() { return FEd::from_limbs(Fe9EdPR::D_MINUS_ONE_SQ); }
};

NCG_DI FEd ristretto_select(bool c, const FEd& a, const FEd& b) {  // c ? a : b, per limb
  FEd r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
NCG_DI FEd ristretto_abs(const FEd& a) {  // the non-negative (even) one of +-a
  const FEd n = f_neg(a);
  return ristretto_select(ed_is_odd(a), n, a);
}

// fromBytes (ed25519.ts:510-533) on the 8 LE words of an encoding.  false where the reference throws: s >= p (bit 255 set
// included: the opposite contract of the map's parser) or s odd ('encoding 1'); the ratio not a square, t odd or y = 0
// ('encoding 2').  x, y: the affine representative, meaningful only when the result is true.
NCG_DI bool ristretto_decode_lane(const uint32_t (&w)[8], FEd& x, FEd& y) {
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)__builtin_subc(w[i], (uint32_t)ParamsEdP::P[i], bw, &bw);
  bool ok = bw != 0 && (w[0] & 1u) == 0;  // s < p and s even
  const FEd s = fe9_from_wire<Fe9EdPR>(w);
  const FEd s2 = f_sqr(s);
  const auto u1 = FEd::one() - s2;  // 4
  const auto u2 = FEd::one() + s2;  // 5
  const FEd u1_2 = f_sqr(u1);
  const FEd u2_2 = f_sqr(u2);
  const FEd v = f_neg(EdConsts::d() * u1_2 + u2_2);  // 6
  FEd I;
  const bool valid = ed_uv_ratio(FEd::one(), v * u2_2, I);  // 7
  const FEd Dx = I * u2;                                   // 8
  const FEd Dy = I * Dx * v;                               // 9
  x = ristretto_abs(f_dbl(s) * Dx);                        // 10
  y = u1 * Dy;                                             // 11
  const FEd t = x * y;                                     // 12
  ok = ok && valid && !ed_is_odd(t) && !f_eqz(y);
  return ok;
}

// toBytes (ed25519.ts:548-572) of an extended point (X : Y : Z : T), T Z = X Y; out = the 8 LE words of the encoding.
// The result does not depend on the projective scale of the input.
NCG_DI void ristretto_encode_ext(const FEd& X, const FEd& Y, const FEd& Z, const FEd& T, uint32_t (&out)[8]) {
  const FEd u1 = (Z + Y) * (Z - Y);  // 1
  const FEd u2 = X * Y;              // 2
  FEd inv;
  (void)ed_uv_ratio(FEd::one(), u1 * f_sqr(u2), inv);  // 3: the square root always exists for a point of the curve
  const FEd D1 = inv * u1;                             // 4
  const FEd D2 = inv * u2;                             // 5
  const FEd zInv = D1 * D2 * T;                        // 6
  const bool rot = ed_is_odd(T * zInv);                // 7: the representative rotated by the point of order 4 (i, 0)
  const FEd i = EdConsts::sqrt_m1();
  const FEd Xr = ristretto_select(rot, Y * i, X);
  FEd Yr = ristretto_select(rot, X * i, Y);
  const FEd D = ristretto_select(rot, D1 * RistrettoConsts::invsqrt_a_minus_d(), D2);  // 8
  const FEd Yn = f_neg(Yr);
  Yr = ristretto_select(ed_is_odd(Xr * zInv), Yn, Yr);  // 9
  const FEd s = ristretto_abs((Z - Yr) * D);            // 10
  fe9_to_wire(out, s);                                  // 11
}
// an affine wire point: Z = 1, T = x y
NCG_DI void ristretto_encode_affine(const FEd& x, const FEd& y, uint32_t (&out)[8]) {
  ristretto_encode_ext(x, y, FEd::one(), x * y, out);
}
// a projective (X : Y : Z) triple through the extended representative (X Z : Y Z : Z^2 : X Y) of the same point: what the
// fixed-base table walk hands over, encoded without the inversion of the affine conversion
NCG_DI void ristretto_encode_proj(const FEd& X, const FEd& Y, const FEd& Z, uint32_t (&out)[8]) {
  ristretto_encode_ext(X * Z, Y * Z, f_sqr(Z), X * Y, out);
}

// equals (ed25519.ts:578-586): x1 y2 == y1 x2 or y1 y2 == x1 x2, on affine representatives (the test is homogeneous)
NCG_DI bool ristretto_equals(const FEd& x1, const FEd& y1, const FEd& x2, const FEd& y2) {
  const bool one = f_eq(x1 * y2, y1 * x2);
  const bool two = f_eq(y1 * y2, x1 * x2);
  return one || two;
}

// calcElligatorRistrettoMap (ed25519.ts:443-461, RFC 9496 section 4.3.4 MAP): an extended Edwards representative
NCG_DI EdExt<FEd> ristretto_elligator(const FEd& r0) {
  const FEd one = FEd::one(), d = EdConsts::d();
  const FEd r = EdConsts::sqrt_m1() * r0 * r0;                   // 1
  const FEd Ns = (r + one) * RistrettoConsts::one_minus_d_sq();  // 2
  const FEd D = f_neg((one + d * r) * (r + d));                  // 3, 4: (c - d r)(r + d) with c = -1
  FEd s;
  const bool sq = ed_uv_ratio(Ns, D, s);  // 5
  const FEd sp = s * r0;                  // 6
  const FEd spn = f_neg(sp);
  const FEd s_ = ristretto_select(ed_is_odd(sp), sp, spn);  // the NEGATIVE (odd) one of +-s r0
  s = ristretto_select(sq, s, s_);                          // 7
  const FEd m1 = f_neg(one);
  const FEd c = ristretto_select(sq, m1, r);                              // 8
  const FEd Nt = c * (r - one) * RistrettoConsts::d_minus_one_sq() - D;  // 9
  const FEd s2 = f_sqr(s);
  const FEd W0 = f_dbl(s) * D;                                // 10
  const FEd W1 = Nt * RistrettoConsts::sqrt_ad_minus_one();  // 11
  const auto W2 = one - s2;                                   // 12
  const auto W3 = one + s2;                                   // 13
  return {W0 * W3, W2 * W1, W1 * W3, W0 * W2};
}

// deriveToCurve (ed25519.ts:658-666) on the 16 LE words of 64 uniform bytes: each half with bit 255 MASKED and reduced mod p
// (bytes255ToNumberLE), mapped, and the two points added by the unified addition.
NCG_DI EdExt<FEd> ristretto_from_uniform(const uint32_t (&w)[16]) {
  uint32_t h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = w[i];
  h[7] &= 0x7fffffffu;
  const EdExt<FEd> R1 = ristretto_elligator(fe9_from_wire<Fe9EdPR>(h));  // below 2^255: congruent to the residue
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = w[8 + i];
  h[7] &= 0x7fffffffu;
  const EdExt<FEd> R2 = ristretto_elligator(fe9_from_wire<Fe9EdPR>(h));
  return ed_add_niels(R1, ed_to_niels(R2, EdConsts::d2()), false);
}

NCG_DI void ristretto_load4(const uint32_t* __restrict__ a, FEd& X, FEd& Y, FEd& Z, FEd& T) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    X.v[i] = a[i];
    Y.v[i] = a[9 + i];
    Z.v[i] = a[18 + i];
    T.v[i] = a[27 + i];
  }
}

// The pieces on raw limbs (ncg_field_check field 17, ht_ristretto_op): a 36 words, b 9 words, out 36 words, every input limb
// below the bound stored values have (1: 2^29 + 2^19).
//   op 0  SQRT_RATIO_M1(u, v): a[0..9) = u, b = v; out[0..9) = the value (raw limbs, non-negative), out[9] = 1 if u / v is a square
//   op 1  encode_ext: a = X Y Z T; out[0..8) = the LE words of the encoding
//   op 2  the Elligator map: a[0..9) = r0; out = X Y Z T of the extended representative (raw limbs)
NCG_DI int ristretto_check_op(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  FEd X, Y, Z, T;
  ristretto_load4(a, X, Y, Z, T);
  if (op == 0) {
    FEd v, r;
#pragma unroll
    for (int i = 0; i < 9; i++) v.v[i] = b[i];
    const bool sq = ed_uv_ratio(X, v, r);
#pragma unroll
    for (int i = 0; i < 9; i++) out[i] = r.v[i];
    out[9] = sq ? 1u : 0u;
    return 0;
  }
  if (op == 1) {
    uint32_t w[8];
    ristretto_encode_ext(X, Y, Z, T, w);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = w[i];
    return 0;
  }
  if (op == 2) {
    const EdExt<FEd> p = ristretto_elligator(X);
#pragma unroll
    for (int i = 0; i < 9; i++) {
      out[i] = p.X.v[i];
      out[9 + i] = p.Y.v[i];
      out[18 + i] = p.Z.v[i];
      out[27 + i] = p.T.v[i];
    }
    return 0;
  }
  return -1;
}

}  // namespace ncg
