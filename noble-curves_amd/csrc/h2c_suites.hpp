// RFC 9380 hash-to-curve for secp256k1 and edwards25519, one item per lane: the lane code of the kernels of h2c_suites.hip and of
// their CPU twins.
//
// Restates secp256k1_hasher (src/secp256k1.ts:345-428) and ed25519_hasher (src/ed25519.ts:294-405) under createHasher
// (src/abstract/hash-to-curve.ts:441-530):
//   expand_message_xmd     hash-to-curve.ts:189-228   xmd_sha256_lane (here), xmd_sha512_lane (oprf.hpp)
//   hash_to_field          :312-378                   h2c_hash_to_field_row: m = 1, L = 48, count 48-byte big-endian chunks mod p
//   hashToScalar           :520-528                   h2c_hash_to_scalar_row: one chunk mod n (Fn of secp_fn.hpp) / mod L (mod_l_512)
//   mapToCurveSimpleSWU    :652-717, sqrt_ratio_3mod4 :610-625      secp_swu
//   isogenyMap             :381-405                   secp_iso_jac: evaluated homogeneously, lands in Jacobian coordinates
//   _map_to_curve_elligator2_curve25519 / map_to_curve_elligator2_edwards25519   ed25519.ts:308-379   ed_ell2_map
//   hashToCurve / encodeToCurve / clear                :469-500    secp_sum_row, ed_sum_row (+ the cofactor 8 on edwards25519)
// A map is a function of u alone, so the device is free in how it evaluates it (the same stance as h2c.hip): x of SWU stays a
// fraction over tv4 through the isogeny, the Elligator map keeps (xn : xd), (yn : yd), and no lane inverts anything; the affine
// conversion is the shared batched one.  What IS contractual - sgn0(u) == sgn0(y), the tv1 == 0 branch of SWU, the zero isogeny
// denominator, steps 8-12 of the Edwards map, ZERO staying ZERO - is written out below.
//
// Field form: the radix-2^29 lazy limbs of fe9.hpp for both primes; every named value is kept at bound 1 (a sum or difference
// assigned to F1 / FEd is weakly normalised by the narrowing conversion), so the bound rules never come into play.
#pragma once
#include "curves.hpp"
#include "oprf.hpp"
#include "secp_fn.hpp"
#include "sha256.hpp"

namespace ncg {

enum H2cSuite : int { H2C_SECP256K1_XMD_SHA256_SSWU = 0, H2C_EDWARDS25519_XMD_SHA512_ELL2 = 1 };

// ---- SHA-256 over segments (OSeg of oprf.hpp: bytes in memory, or up to 16 immediate bytes followed by zeros).  PRE: the message
// starts with the 32 bytes of `pre` (8 big-endian words, a chaining value of the xmd) before the segments.
template <int NSEG, bool PRE>
NCG_DI void h2c_sha256(uint32_t (&h)[8], const uint32_t (&pre)[8], const OSeg (&seg)[NSEG]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
  uint64_t end[NSEG];  // end[s]: position after the last byte of segment s
  uint64_t total = PRE ? 32 : 0;
#pragma unroll
  for (int s = 0; s < NSEG; s++) end[s] = total += seg[s].len;
  const uint64_t nblocks = (total + 1 + 8 + 63) / 64;  // 0x80, 64-bit length, padding
  for (uint64_t blk = 0; blk < nblocks; blk++) {
    uint32_t w[16];
#pragma unroll 1
    for (int i = 0; i < 16; i++) {
      uint32_t v = 0;
      for (int j = 0; j < 4; j++) {
        const uint64_t pos = blk * 64 + (uint64_t)i * 4 + j;
        uint32_t byte = pos == total ? 0x80u : 0u;
#pragma unroll
        for (int s = 0; s < NSEG; s++) {
          const uint64_t start = end[s] - seg[s].len;
          if (pos >= start && pos < end[s]) {
            const uint64_t k = pos - start;
            if (seg[s].p) byte = seg[s].p[k];
            else byte = k < 8 ? (uint32_t)(seg[s].imm0 >> (56 - 8 * k)) & 0xffu : (k < 16 ? (uint32_t)(seg[s].imm1 >> (120 - 8 * k)) & 0xffu : 0u);
          }
        }
        v = (v << 8) | byte;
      }
      w[i] = v;
    }
    if (PRE && blk == 0) {
#pragma unroll
      for (int i = 0; i < 8; i++) w[i] = pre[i];
    }
    if (blk == nblocks - 1) {
      w[14] = (uint32_t)(total >> 29);
      w[15] = (uint32_t)(total << 3);
    }
    sha256_block(h, w);
  }
}
// expand_message_xmd over SHA-256 (RFC 9380 section 5.3.1): out_len in 1..256 bytes to `out`.  dstp: DST' = DST || I2OSP(len(DST), 1).
//   b_0 = H(64 zero bytes || msg || I2OSP(out_len, 2) || 0 || DST'),  b_i = H((b_0 ^ b_(i-1)) || I2OSP(i, 1) || DST'), b_0' = 0 for i = 1
NCG_DI void xmd_sha256_lane(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t out_len,
                            uint8_t* __restrict__ out) {
  const uint32_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t b0[8], prev[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cur[8];
  {
    const OSeg seg[4] = {oseg_zero(64), oseg_mem(msg, len), oseg_be((uint64_t)out_len << 8, 3), oseg_mem(dstp, dstp_len)};
    h2c_sha256<4, false>(b0, none, seg);
  }
  const uint32_t ell = (out_len + 31) / 32;
#pragma unroll 1
  for (uint32_t i = 1; i <= ell; i++) {
    uint32_t pre[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pre[j] = b0[j] ^ prev[j];
    const OSeg seg[2] = {oseg_be(i, 1), oseg_mem(dstp, dstp_len)};
    h2c_sha256<2, true>(cur, pre, seg);
    const uint32_t done = 32 * (i - 1), count = out_len - done < 32 ? out_len - done : 32;
#pragma unroll
    for (int j = 0; j < 32; j++)
      if ((uint32_t)j < count) out[done + j] = (uint8_t)(cur[j / 4] >> (24 - 8 * (j % 4)));
#pragma unroll
    for (int j = 0; j < 8; j++) prev[j] = cur[j];
  }
}
template <int SUITE>
NCG_DI void h2c_xmd_lane(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t out_len,
                         uint8_t* __restrict__ out) {
  if constexpr (SUITE == H2C_SECP256K1_XMD_SHA256_SSWU) xmd_sha256_lane(msg, len, dstp, dstp_len, out_len, out);
  else xmd_sha512_lane(msg, len, dstp, dstp_len, out_len, out);
}

// ---- 48 bytes -> a field element.  v = lo + hi 2^256 (lo 8 words, hi 4): 2^256 = K (mod p) with K = 2^32 + 977 (secp256k1) or
// 38 (ed25519), so v = lo + hi K: one product with a linear addend, congruent and of bound 1.  lo below 2^256 has 24 bits in limb 8.
template <class PR>
NCG_DI Fe9<PR, 1> h2c_fold_const() {
  Fe9<PR, 1> k = Fe9<PR, 1>::zero();
  if constexpr (PR::C1 != 0) {  // secp256k1
    k.v[0] = 977u;
    k.v[1] = 8u;  // 2^32 = 8 * 2^29
  } else {
    k.v[0] = 38u;
  }
  return k;
}
template <class PR>
NCG_DI Fe9<PR, 1> h2c_reduce384(const uint32_t (&w)[12]) {
  uint32_t lo[8], hi[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    lo[i] = w[i];
    hi[i] = i < 4 ? w[8 + i] : 0u;
  }
  return f_mul_add(fe9_from_wire<PR>(hi), h2c_fold_const<PR>(), fe9_from_wire<PR>(lo));
}
// an input element of in_words = 12 words (48 bytes, any value) or 8 (a reduced element of hash_to_field)
NCG_DI void h2c_load12(uint32_t (&w)[12], const uint32_t* __restrict__ p, int in_words = 12) {
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = i < in_words ? p[i] : 0u;
}
// 48 big-endian bytes -> 12 LE words
NCG_DI void h2c_be48_words(uint32_t (&w)[12], const uint8_t* p) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint8_t* q = p + 4 * (11 - i);
    w[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
}
// the same value mod n (secp256k1): lo below 2^256 < 2 n takes one subtraction, hi 2^256 = hi R is the Montgomery product of hi and R^2
NCG_DI void h2c_reduce384_mod_n(uint32_t (&r)[8], const uint32_t (&w)[12]) {
  Fn lo, hi = Fn::zero();
#pragma unroll
  for (int i = 0; i < 8; i++) lo.v[i] = w[i];
#pragma unroll
  for (int i = 0; i < 4; i++) hi.v[i] = w[8 + i];
  fp_cond_sub_p<ParamsSecpN>(lo.v, 0u);
  const Fn s = lo + fp_mul<ParamsSecpN>(hi, Fn::from_const(ParamsSecpN::R2));
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = s.v[i];
}
// mod L (ed25519): the 64-byte reduction of the challenge on the value padded with zeros
NCG_DI void h2c_reduce384_mod_l(uint32_t (&r)[8], const uint32_t (&w)[12]) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; i++) x[i] = i < 12 ? w[i] : 0u;
  mod_l_512(r, x);
}

// parity of the canonical residue: sgn0 for m = 1 (RFC 9380 section 4.1; Fp.isOdd)
template <class PR, int A>
NCG_DI bool h2c_sgn0(const Fe9<PR, A>& x) {
  uint32_t c[9];
  fe9_canon_limbs<PR, A>(c, x);
  return (c[0] & 1u) != 0;
}

// ---- hash_to_field rows.  uniform: 48 * count bytes of memory for the xmd output (global memory on the device: a per-lane byte
// array indexed by the loop of the xmd would live in scratch), written and then read back by the same lane; out_u: count canonical elements of 8 LE words.
template <int SUITE>
NCG_DI void h2c_hash_to_field_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len, int count,
                                  uint8_t* uniform, uint32_t* __restrict__ out_u) {
  using PR = typename std::conditional<SUITE == H2C_SECP256K1_XMD_SHA256_SSWU, Fe9SecpPR, Fe9EdPR>::type;
  h2c_xmd_lane<SUITE>(msg, len, dstp, dstp_len, 48u * (uint32_t)count, uniform);
#pragma unroll 1
  for (int j = 0; j < count; j++) {
    uint32_t w[12];
    h2c_be48_words(w, uniform + 48 * j);
    fe9_to_wire(out_u + 8 * j, h2c_reduce384<PR>(w));
  }
}
template <int SUITE>
NCG_DI void h2c_hash_to_scalar_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                   uint8_t* uniform, uint32_t* __restrict__ out8) {
  h2c_xmd_lane<SUITE>(msg, len, dstp, dstp_len, 48u, uniform);
  uint32_t w[12], r[8];
  h2c_be48_words(w, uniform);
  if constexpr (SUITE == H2C_SECP256K1_XMD_SHA256_SSWU) h2c_reduce384_mod_n(r, w);
  else h2c_reduce384_mod_l(r, w);
#pragma unroll
  for (int i = 0; i < 8; i++) out8[i] = r[i];
}

// ------------------------------------------------------------------------------------- secp256k1
using FSecp1 = Fe9<Fe9SecpPR, 1>;
NCG_DI FSecp1 secp_h2c_const(const uint32_t (&k)[9]) { return FSecp1::from_limbs(k); }

// x^((p - 3) / 4): the exponent is [223 ones] 0 [22 ones] 0000 1 0 11 in binary - the chain of the square root (decode.hip,
// secp256k1.ts:73-95) and of the Fermat inverse (fe9.hpp) up to t1, then 00001 and 011: 253 squarings + 13 products
NCG_DI FSecp1 secp_pow_p34(const FSecp1& x) {
  using F = FSecp1;
  F x2 = f_sqr(x) * x;
  F x3 = f_sqr(x2) * x;
  F x6 = fe9_sqr_n(x3, 3) * x3;
  F x9 = fe9_sqr_n(x6, 3) * x3;
  F x11 = fe9_sqr_n(x9, 2) * x2;
  F x22 = fe9_sqr_n(x11, 11) * x11;
  F x44 = fe9_sqr_n(x22, 22) * x22;
  F x88 = fe9_sqr_n(x44, 44) * x44;
  F x176 = fe9_sqr_n(x88, 88) * x88;
  F x220 = fe9_sqr_n(x176, 44) * x44;
  F x223 = fe9_sqr_n(x220, 3) * x3;
  F t = fe9_sqr_n(x223, 23) * x22;
  t = fe9_sqr_n(t, 5) * x;
  return fe9_sqr_n(t, 3) * x2;
}

// mapToCurveSimpleSWU on E' (hash-to-curve.ts:686-716) without step 25: the point is (x / xd, y)
NCG_DI void secp_swu(const FSecp1& u, FSecp1& x_out, FSecp1& xd_out, FSecp1& y_out) {
  using F = FSecp1;
  const F A = secp_h2c_const(SecpH2c::SWU_A), B = secp_h2c_const(SecpH2c::SWU_B), Z = secp_h2c_const(SecpH2c::SWU_Z);
  const F tv1 = f_sqr(u) * Z;                                   // 1-2
  const F tv2 = f_sqr(tv1) + tv1;                               // 3-4
  const F tv3 = (tv2 + F::one()) * B;                           // 5-6
  const F nt2 = f_neg(tv2);
  const F sel = f_eqz(tv2) ? Z : nt2;                           // 7: the exceptional case Z^2 u^4 + Z u^2 = 0 takes Z
  const F tv4 = sel * A;                                        // 8: never zero (A, Z != 0)
  F tv6 = f_sqr(tv4);                                           // 10
  const F gxn = (f_sqr(tv3) + tv6 * A) * tv3;                   // 9, 11-13
  tv6 = tv6 * tv4;                                              // 14
  const F gx = gxn + tv6 * B;                                   // 15-16: g(x1) = gx / tv6
  F x = tv1 * tv3;                                              // 17
  // sqrt_ratio_3mod4(gx, tv6) (:614-625); tv6 = tv4^3 != 0, so isValid = isQR
  const F t2 = gx * tv6;
  const F t1 = f_sqr(tv6) * t2;
  const F y1 = secp_pow_p34(t1) * t2;
  const bool is_qr = f_eq(f_sqr(y1) * tv6, gx);
  const F y1c = y1 * secp_h2c_const(SecpH2c::SWU_C2);
  const F value = is_qr ? y1 : y1c;
  F y = tv1 * u * value;                                        // 19-20
  if (is_qr) {                                                  // 21-22
    x = tv3;
    y = value;
  }
  const F ny = f_neg(y);
  if (h2c_sgn0(u) != h2c_sgn0(y)) y = ny;                       // 23-24
  x_out = x;
  xd_out = tv4;
  y_out = y;
}
// D^(N-1) sum_i k[i] (X / D)^i, coefficients ascending as the reference lists them; every step one fused a b + c d
template <int N>
NCG_DI FSecp1 secp_horner_hom(const uint32_t (&k)[N][9], const FSecp1& X, const FSecp1& D) {
  FSecp1 acc = secp_h2c_const(k[N - 1]);
  FSecp1 dpow = D;
#pragma unroll
  for (int i = N - 2; i >= 0; i--) {
    acc = f_mul_mul(acc, X, secp_h2c_const(k[i]), dpow);
    if (i) dpow = dpow * D;
  }
  return acc;
}
// isoMap (secp256k1.ts:345-390, isogenyMap hash-to-curve.ts:390-404) at (x / D, y), into Jacobian coordinates of E.  With
// XN = D^3 xnum, XD = D^2 xden, YN = D^3 ynum, YD = D^3 yden:  x' = XN / (XD D), y' = y YN / YD, so
//   Z = XD D YD,  X = XN (XD D) YD^2,  Y = y YN YD^2 (XD D)^3;   a zero denominator is ZERO (:394-403).
NCG_DI Jac<FeSecp> secp_iso_jac(const FSecp1& x, const FSecp1& D, const FSecp1& y) {
  using F = FSecp1;
  static_assert(SecpH2c::ISO_XNUM_N == 4 && SecpH2c::ISO_XDEN_N == 3 && SecpH2c::ISO_YNUM_N == 4 && SecpH2c::ISO_YDEN_N == 4,
                "degrees of the homogeneous form");
  const F XN = secp_horner_hom(SecpH2c::ISO_XNUM, x, D), XD = secp_horner_hom(SecpH2c::ISO_XDEN, x, D);
  const F YN = secp_horner_hom(SecpH2c::ISO_YNUM, x, D), YD = secp_horner_hom(SecpH2c::ISO_YDEN, x, D);
  if (f_eqz(XD) || f_eqz(YD)) return Jac<FeSecp>::inf();
  const F Aq = XD * D, YD2 = f_sqr(YD);
  const F A3 = f_sqr(Aq) * Aq;
  return {XN * Aq * YD2, y * YN * YD2 * A3, Aq * YD};
}
NCG_DI Jac<FeSecp> secp_h2c_map(const FSecp1& u) {
  FSecp1 x, xd, y;
  secp_swu(u, x, xd, y);
  return secp_iso_jac(x, xd, y);
}

constexpr int SECP_JAC_WORDS = 27;  // (X, Y, Z) stored, the hand-off to k_jac_batch_affine
NCG_DI void secp_store_jac(uint32_t* __restrict__ o, Jac<FeSecp> R) {
  if (R.is_inf()) R = Jac<FeSecp>::inf();
  FieldIO<FeSecp>::store(o, R.X);
  FieldIO<FeSecp>::store(o + 9, R.Y);
  FieldIO<FeSecp>::store(o + 18, R.Z);
}
NCG_DI Jac<FeSecp> secp_load_jac(const uint32_t* __restrict__ p) {
  return {FieldIO<FeSecp>::load(p), FieldIO<FeSecp>::load(p + 9), FieldIO<FeSecp>::load(p + 18)};
}
// one u (in_words LE words: 12, any value below 2^384, or 8) -> the image on E
NCG_DI void secp_map_row(const uint32_t* __restrict__ u, int in_words, uint32_t* __restrict__ jac_out) {
  uint32_t w[12];
  h2c_load12(w, u, in_words);
  secp_store_jac(jac_out, secp_h2c_map(h2c_reduce384<Fe9SecpPR>(w)));
}
// Q0 [+ Q1]; clearCofactor is the identity (h = 1).  jac_add routes Q1 = Q0 to the doubling and Q1 = -Q0 to ZERO (ec_sw.hpp)
NCG_DI void secp_sum_row(const uint32_t* __restrict__ stage, int count, uint32_t* __restrict__ jac_out) {
  Jac<FeSecp> acc = secp_load_jac(stage);
  if (count == 2) acc = jac_add(acc, secp_load_jac(stage + SECP_JAC_WORDS));
  secp_store_jac(jac_out, acc);
}

// ------------------------------------------------------------------------------------- edwards25519
struct EdH2cConsts {
  static NCG_DI FEd j() { return FEd::from_limbs(EdH2c::ELL2_J); }
  static NCG_DI FEd c2() { return FEd::from_limbs(EdH2c::ELL2_C2); }
  static NCG_DI FEd c1_edwards() { return FEd::from_limbs(EdH2c::ELL2_C1_EDWARDS); }
};
// map_to_curve_elligator2_edwards25519 (ed25519.ts:362-379) over _map_to_curve_elligator2_curve25519 (:308-358), as an extended
// point (X : Y : Z : T) = (xn yd : yn xd : xd yd : xn yn) instead of the two inversions of the reference
NCG_DI EdExt<FEd> ed_ell2_map(const FEd& u) {
  using F = FEd;
  const F J = EdH2cConsts::j(), c3 = EdConsts::sqrt_m1();
  const F tv1 = f_dbl(f_sqr(u));                 // 1-2
  const F xd = tv1 + F::one();                   // 3: non-zero, -1 / 2 is not a square
  const F x1n = f_neg(J);                        // 4
  F tv2 = f_sqr(xd);                             // 5
  const F gxd = tv2 * xd;                        // 6
  F gx1 = tv1 * J * x1n;                         // 7-8
  gx1 = (gx1 + tv2) * x1n;                       // 9-10
  F tv3 = f_sqr(gxd);                            // 11
  tv2 = f_sqr(tv3);                              // 12
  tv3 = tv3 * gxd * gx1;                         // 13-14
  tv2 = tv2 * tv3;                               // 15
  const F y11 = ed_pow_p58(tv2) * tv3;           // 16-17
  const F y12 = y11 * c3;                        // 18
  const bool e1 = f_eq(f_sqr(y11) * gxd, gx1);   // 19-21
  const F y1 = e1 ? y11 : y12;                   // 22
  const F x2n = x1n * tv1;                       // 23
  const F y21 = y11 * u * EdH2cConsts::c2();     // 24-25
  const F y22 = y21 * c3;                        // 26
  const F gx2 = gx1 * tv1;                       // 27
  const bool e2 = f_eq(f_sqr(y21) * gxd, gx2);   // 28-30
  const F y2 = e2 ? y21 : y22;                   // 31
  const bool e3 = f_eq(f_sqr(y1) * gxd, gx1);    // 32-34
  const F xMn = e3 ? x1n : x2n;                  // 35
  F y = e3 ? y1 : y2;                            // 36
  const F ny = f_neg(y);
  if (e3 != h2c_sgn0(y)) y = ny;                 // 37-38
  // to Edwards form: (xMn, xMd, yMn, yMd) = (xMn, xd, y, 1)
  F xn = xMn * EdH2cConsts::c1_edwards();        // 2-3
  F exd = xd * y;                                // 4
  F yn = xMn - xd;                               // 5
  F yd = xMn + xd;                               // 6
  if (f_eqz(exd * yd)) {                         // 7-12: the exceptional case gives (0, 1)
    xn = F::zero();
    exd = F::one();
    yn = F::one();
    yd = F::one();
  }
  return {xn * yd, yn * exd, exd * yd, xn * yn};
}

constexpr int ED_EXT_WORDS = 36;  // (X, Y, Z, T) stored: the hand-off from the map to the sum
NCG_DI void ed_map_row(const uint32_t* __restrict__ u, int in_words, uint32_t* __restrict__ ext_out) {
  uint32_t w[12];
  h2c_load12(w, u, in_words);
  const EdExt<FEd> Q = ed_ell2_map(h2c_reduce384<Fe9EdPR>(w));
  FieldIO<FEd>::store(ext_out, Q.X);
  FieldIO<FEd>::store(ext_out + 9, Q.Y);
  FieldIO<FEd>::store(ext_out + 18, Q.Z);
  FieldIO<FEd>::store(ext_out + 27, Q.T);
}
NCG_DI EdExt<FEd> ed_load_ext(const uint32_t* __restrict__ p) {
  return {FieldIO<FEd>::load(p), FieldIO<FEd>::load(p + 9), FieldIO<FEd>::load(p + 18), FieldIO<FEd>::load(p + 27)};
}
// 8 (Q0 [+ Q1]) as (X, Y, Z): the unified addition (complete on ed25519: Q1 = +-Q0 needs no care) and three doublings without T
NCG_DI void ed_sum_row(const uint32_t* __restrict__ stage, int count, uint32_t* __restrict__ proj_out) {
  EdExt<FEd> acc = ed_load_ext(stage);
  if (count == 2) acc = ed_add_niels(acc, ed_to_niels(ed_load_ext(stage + ED_EXT_WORDS), EdConsts::d2()), false);
#pragma unroll 1
  for (int i = 0; i < 3; i++) acc = ed_dbl_no_t(acc);
  FieldIO<FEd>::store(proj_out, acc.X);
  FieldIO<FEd>::store(proj_out + 9, acc.Y);
  FieldIO<FEd>::store(proj_out + 18, acc.Z);
}

// ---- the pieces on raw words (ncg_h2c_check, ht_h2c_check): a 24 words, out 24 words per row, unused words zero.
//   op 0 / 1   a[0..12) mod p of secp256k1 / ed25519 -> out[0..8)
//   op 2 / 3   a[0..12) mod n of secp256k1 / mod L -> out[0..8)
//   op 4       secp256k1 SWU of u = a[0..12): out = x (8), xd (8), y (8) canonical, the point of E' being (x / xd, y)
//   op 5       secp256k1 isogeny at the affine point (x', y') = a[0..8), a[8..16) of E': out = X, Y, Z canonical (Z = 0: ZERO)
//   op 6       edwards25519 map of u = a[0..12) without the cofactor: out = X, Y, Z canonical
constexpr int H2C_CHECK_OPS = 7, H2C_CHECK_WORDS = 24;
NCG_DI int h2c_check_op(int op, const uint32_t* __restrict__ a, uint32_t* __restrict__ out) {
  uint32_t w[12], r[8];
  if (op < 0 || op >= H2C_CHECK_OPS) return -1;
  h2c_load12(w, a);
  if (op == 0) fe9_to_wire(out, h2c_reduce384<Fe9SecpPR>(w));
  else if (op == 1) fe9_to_wire(out, h2c_reduce384<Fe9EdPR>(w));
  else if (op == 2 || op == 3) {
    if (op == 2) h2c_reduce384_mod_n(r, w);
    else h2c_reduce384_mod_l(r, w);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = r[i];
  } else if (op == 4) {
    FSecp1 x, xd, y;
    secp_swu(h2c_reduce384<Fe9SecpPR>(w), x, xd, y);
    fe9_to_wire(out, x);
    fe9_to_wire(out + 8, xd);
    fe9_to_wire(out + 16, y);
  } else if (op == 5) {
    const Jac<FeSecp> R = secp_iso_jac(fe9_from_wire<Fe9SecpPR>(a), FSecp1::one(), fe9_from_wire<Fe9SecpPR>(a + 8));
    fe9_to_wire(out, R.X);
    fe9_to_wire(out + 8, R.Y);
    fe9_to_wire(out + 16, R.Z);
  } else {
    const EdExt<FEd> Q = ed_ell2_map(h2c_reduce384<Fe9EdPR>(w));
    fe9_to_wire(out, Q.X);
    fe9_to_wire(out + 8, Q.Y);
    fe9_to_wire(out + 16, Q.Z);
  }
  return 0;
}

}  // namespace ncg
