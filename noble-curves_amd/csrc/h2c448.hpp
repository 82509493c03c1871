// RFC 9380 for the 448-bit family: edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_ (the reference's ed448_hasher, src/ed448.ts:313-417) and
// the hash side of decaf448_hasher (:662-701).  Lane code, the same text on the device (h2c448.hip) and on the CPU (hosttest.hip).
//   expand_message_xof           hash-to-curve.ts:252-286   xof448_absorb: SHAKE256(msg || I2OSP(len, 2) || DST || I2OSP(len(DST), 1))
//   hash_to_field, L = 84        :312-378                   h2c448_be84_words, h2c448_mod_p: 84 bytes big-endian mod p
//   hashToScalar, L = 84         :520-528                   h2c448_mod_n_be84: the same 84 bytes mod n through mod_n_912 (keccak.hpp)
//   decaf448 hashToScalar        ed448.ts:674-679           h2c448_mod_n_le64: 64 bytes little-endian mod n
//   map_to_curve_elligator2_curve448    ed448.ts:320-349    h2c448_map_curve448: one power chain, the 27 steps
//   map_to_curve_elligator2_edwards448  ed448.ts:352-394    h2c448_map_edwards448: steps 1-37; the fractions are kept and the lane forms
//                                                           the projective point (xEn yEd : yEn xEd : xEd yEd) instead of inverting twice
//   the hasher tail              hash-to-curve.ts:472-500   h2c448_map_row: Q0 [+ Q1] by the complete ed448_add, two ed448_dbl for h = 4,
//                                                           one fe448_inv for the canonical affine x || y
// Per hashToCurve row: two maps of one power chain each and one inversion - three chains, as decaf_from_uniform_row has.
// The message is one KeccakSeg, the tail `len_be2 || DST || len(DST)` a second one that all rows share (staged once per call).
// The uniform bytes go through memory (shake256_squeeze stores them, the reduction reads them back byte by byte at compile-time
// offsets): on the device that is the workspace row of the lane, never an indexed array in registers.
// Multiply-adds (fe448.hpp: product 256, square 136, small-constant chain 16), the chain fe448_pow_pm3d4 = 445 squares + 13 products:
//   curve448 map:   chain + 10 products + 4 squares          = 63848 + 2560 + 544  = 66952
//   edwards448 map: curve448 map + 14 products + 4 squares   = 66952 + 3584 + 544  = 71080  (with the three products of the point)
//   tail (count 2): add 2712 + 2 dbl 2624 + inversion (chain + 2 squares + 1 product) + 2 products = 70224
//   a hashToCurve row: 2 * 71080 + 70224 = 212384; an encodeToCurve row: 71080 + 67512 = 138592
#pragma once
#include "decaf448.hpp"
#include "keccak.hpp"

namespace ncg {

constexpr int H2C448_L = 84;              // ceil((448 + 224) / 8), and ceil((446 + 224) / 8) for the scalar field
constexpr int H2C448_TAIL_MAX = 2 + 255 + 1;  // len_be2 || DST || len(DST)
constexpr uint32_t ELL2_J448 = 156326u;   // ed448.ts:316

// the tail of expand_message_xof for out_len bytes of output; returns its length
NCG_DI uint32_t xof448_tail(uint8_t* __restrict__ tail, const uint8_t* __restrict__ dst, uint32_t dst_len, uint32_t out_len) {
  tail[0] = (uint8_t)(out_len >> 8);
  tail[1] = (uint8_t)out_len;
  for (uint32_t i = 0; i < dst_len; i++) tail[2 + i] = dst[i];
  tail[2 + dst_len] = (uint8_t)dst_len;
  return dst_len + 3;
}
// expand_message_xof up to the first permutation after the padding: the output is squeezed from st
NCG_DI void xof448_absorb(uint64_t (&st)[25], const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ tail, uint32_t tail_len) {
  const KeccakSeg seg[2] = {{msg, len}, {tail, tail_len}};
  shake256_absorb<2>(st, seg);
}

// 84 bytes big-endian -> 21 LE words
NCG_DI void h2c448_be84_words(uint32_t (&w)[21], const uint8_t* __restrict__ b) {
#pragma unroll
  for (int j = 0; j < 21; j++)
    w[j] = (uint32_t)b[83 - 4 * j] | ((uint32_t)b[82 - 4 * j] << 8) | ((uint32_t)b[81 - 4 * j] << 16) | ((uint32_t)b[80 - 4 * j] << 24);
}
// v < 2^672 mod p, canonical: v = lo + hi 2^448 with hi below 2^224 = eight limbs of the 16 x 2^28 form, and 2^448 = 2^224 + 1, so
// hi is added to the low and to the high eight limbs; fe448_to_words reduces the rest
NCG_DI void h2c448_mod_p(uint32_t (&out)[14], const uint32_t (&v)[21]) {
  uint32_t lo[14], hi[14];
#pragma unroll
  for (int i = 0; i < 14; i++) {
    lo[i] = v[i];
    hi[i] = i < 7 ? v[14 + i] : 0u;
  }
  const F448 l = fe448_from_words(lo), h = fe448_from_words(hi);  // limbs 8..15 of h are zero
  F448 hh;
#pragma unroll
  for (int i = 0; i < 16; i++) hh.v[i] = h.v[i & 7];
  fe448_to_words(out, l + hh);
}
NCG_DI void h2c448_mod_n_be84(uint32_t (&out)[14], const uint32_t (&v)[21]) {
  uint32_t x[29];
#pragma unroll
  for (int i = 0; i < 29; i++) x[i] = i < 21 ? v[i] : 0u;
  mod_n_912(out, x);
}
NCG_DI void h2c448_mod_n_le64(uint32_t (&out)[14], const uint32_t (&v)[16]) {
  uint32_t x[29];
#pragma unroll
  for (int i = 0; i < 29; i++) x[i] = i < 16 ? v[i] : 0u;
  mod_n_912(out, x);
}

// ---- the rows of the hash kernels.  uniform: count * 84 (or 84) bytes of memory of the row
NCG_DI void h2c448_xof_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ tail, uint32_t tail_len, uint32_t out_len,
                           uint8_t* __restrict__ out) {
  uint64_t st[25];
  xof448_absorb(st, msg, len, tail, tail_len);
  shake256_squeeze(st, out, out_len);
}
// hash_to_field: count elements of 14 LE words, reduced
NCG_DI void h2c448_hash_to_field_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ tail, uint32_t tail_len, int count,
                                     uint8_t* __restrict__ uniform, uint32_t* __restrict__ out_u) {
  h2c448_xof_row(msg, len, tail, tail_len, (uint32_t)count * H2C448_L, uniform);
  for (int j = 0; j < count; j++) {
    uint32_t v[21], r[14];
    h2c448_be84_words(v, uniform + j * H2C448_L);
    h2c448_mod_p(r, v);
#pragma unroll
    for (int i = 0; i < 14; i++) out_u[j * 14 + i] = r[i];
  }
}
NCG_DI void h2c448_hash_to_scalar_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ tail, uint32_t tail_len,
                                      uint8_t* __restrict__ uniform, uint32_t* __restrict__ out) {
  h2c448_xof_row(msg, len, tail, tail_len, H2C448_L, uniform);
  uint32_t v[21], r[14];
  h2c448_be84_words(v, uniform);
  h2c448_mod_n_be84(r, v);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = r[i];
}
// decaf448 hashToScalar: 64 bytes of output lie inside the first block, read from the state as words
NCG_DI void decaf448_hash_to_scalar_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ tail, uint32_t tail_len,
                                        uint32_t* __restrict__ out) {
  uint64_t st[25];
  uint32_t v[16], r[14];
  xof448_absorb(st, msg, len, tail, tail_len);
  shake256_words<16>(v, st, 64);
  h2c448_mod_n_le64(r, v);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = r[i];
}

// ---- the maps
struct Curve448Frac {  // (xn / xd, y), yd = 1; bound 1
  F448 xn, xd, y;
};
NCG_DI F448 h2c448_neg_j() {
  F448 j = F448::zero();
  j.v[0] = ELL2_J448;
  return fe448_neg(j);
}
// map_to_curve_elligator2_curve448 (ed448.ts:320-349), the step numbers are the reference's
NCG_DI Curve448Frac h2c448_map_curve448(const F448& u) {
  const F448 one = F448::one(), zero = F448::zero();
  const F448 x1n = h2c448_neg_j();                         // 5
  F448 tv1 = fe448_sqr(u);                                 // 1
  const bool e1 = fe448_eq(tv1, one);                      // 2
  tv1 = fe448_select(e1, zero, tv1);                       // 3
  const F448 xd = fe448_weak(one - tv1);                   // 4
  F448 tv2 = fe448_sqr(xd);                                // 6
  const F448 gxd = tv2 * xd;                               // 7
  F448 gx1 = tv1 * x1n;                                    // 8
  gx1 = gx1 * x1n;                                         // 9
  gx1 = (gx1 + tv2) * x1n;                                 // 10, 11: (2 * 1)
  F448 tv3 = fe448_sqr(gxd);                               // 12
  tv2 = gx1 * gxd;                                         // 13
  tv3 = tv3 * tv2;                                         // 14
  const F448 y1 = fe448_pow_pm3d4(tv3) * tv2;              // 15, 16
  const F448 x2n = x1n * fe448_neg(tv1);                   // 17
  const F448 y2 = fe448_select(e1, zero, y1 * u);          // 18, 19
  tv2 = fe448_sqr(y1) * gxd;                               // 20, 21
  const bool e2 = fe448_eq(tv2, gx1);                      // 22
  const F448 xn = fe448_select(e2, x1n, x2n);              // 23
  F448 y = fe448_select(e2, y1, y2);                       // 24
  const bool e3 = fe448_parity(y) != 0;                    // 25: sgn0 of the canonical value
  y = fe448_select(e2 != e3, fe448_neg(y), y);             // 26
  return Curve448Frac{xn, xd, y};
}
// map_to_curve_elligator2_edwards448 (ed448.ts:352-390) with yd = 1 (steps 6, 10, 14, 30 multiply by one), without the inversions
NCG_DI Ed448Pt h2c448_map_edwards448(const F448& u) {
  const Curve448Frac m = h2c448_map_curve448(u);           // 1
  const F448 one = F448::one();
  const F448 xn2 = fe448_sqr(m.xn);                        // 2
  const F448 xd2 = fe448_sqr(m.xd);                        // 3
  const F448 xd4 = fe448_sqr(xd2);                         // 4
  const F448 yn2 = fe448_sqr(m.y);                         // 5
  const auto d7 = xn2 - xd2;                               // 7 (bound 3)
  const F448 t8 = fe448_weak(d7 - xd2);                    // 8 (bound 5 before the pass)
  const F448 x9 = (d7 * xd2) * m.y;                        // 9, 11: (3 * 1)
  const F448 xEn = fe448_weak((x9 + x9) + (x9 + x9));      // 12
  F448 tv2 = t8 * xn2;                                     // 13
  const auto tv3 = (yn2 + yn2) + (yn2 + yn2);              // 15 (bound 4)
  const F448 tv1 = (tv3 + one) * xd4;                      // 16, 17: (5 * 1)
  const F448 xEd = fe448_weak(tv1 + tv2);                  // 18
  tv2 = tv2 * m.xn;                                        // 19
  const F448 tv4 = m.xn * xd4;                             // 20
  const F448 y22 = (tv3 - one) * tv4;                      // 21, 22: (6 * 1)
  const F448 yEn = fe448_weak(y22 - tv2);                  // 23
  const F448 t27 = (((xn2 + xd2) * xd2) * m.xd) * yn2;     // 24-27
  const F448 t28 = fe448_neg(t27 + t27);                   // 28
  const F448 yEd = fe448_weak((tv2 + t28) + tv4);          // 29, 31
  const bool e = fe448_is_zero(xEd * yEd);                 // 32, 33
  const F448 xEn_ = fe448_select(e, F448::zero(), xEn);    // 34
  const F448 xEd_ = fe448_select(e, one, xEd);             // 35
  const F448 yEn_ = fe448_select(e, one, yEn);             // 36
  const F448 yEd_ = fe448_select(e, one, yEd);             // 37
  return Ed448Pt{xEn_ * yEd_, yEn_ * xEd_, xEd_ * yEd_};
}

NCG_DI F448 h2c448_load_u(const uint32_t* __restrict__ u) {
  uint32_t w[14];
#pragma unroll
  for (int i = 0; i < 14; i++) w[i] = u[i];
  return fe448_from_words(w);  // any value below 2^448, congruent
}
// u: count elements of 14 LE words -> the canonical affine x || y (28 words); the identity comes out as (0, 1)
NCG_DI void h2c448_map_row(const uint32_t* __restrict__ u, int count, uint32_t* __restrict__ out) {
  Ed448Pt q = h2c448_map_edwards448(h2c448_load_u(u));
  if (count == 2) q = ed448_add(q, h2c448_map_edwards448(h2c448_load_u(u + 14)));
  q = ed448_dbl(ed448_dbl(q));  // clearCofactor, h = 4
  const F448 zi = fe448_inv(q.Z);
  uint32_t xw[14], yw[14];
  fe448_to_words(xw, q.X * zi);
  fe448_to_words(yw, q.Y * zi);
#pragma unroll
  for (int i = 0; i < 14; i++) {
    out[i] = xw[i];
    out[14 + i] = yw[i];
  }
}

// ---- the pieces on raw words (ncg_h2c448_check, ht_h2c448_check): rows of 42 words in and out, the words past an op's width are
// not read / left alone.  Every output element is 14 LE words, canonical:
//   0 the 84-byte value (21 LE words) mod p                       (21 -> 14)
//   1 the same value mod n                                         (21 -> 14)
//   2 16 LE words (the 64-byte form) mod n                         (16 -> 14)
//   3 the curve448 map of u (14 words, any value below 2^448): xn, xd, y        (14 -> 42)
//   4 the edwards448 map of u before the cofactor: X, Y, Z of the projective point (xEn yEd : yEn xEd : xEd yEd)   (14 -> 42)
constexpr int H2C448_CHECK_OPS = 5, H2C448_CHECK_WORDS = 42;
NCG_DI void h2c448_store3(uint32_t* __restrict__ out, const F448& a, const F448& b, const F448& c) {
  uint32_t w[14];
  fe448_to_words(w, a);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = w[i];
  fe448_to_words(w, b);
#pragma unroll
  for (int i = 0; i < 14; i++) out[14 + i] = w[i];
  fe448_to_words(w, c);
#pragma unroll
  for (int i = 0; i < 14; i++) out[28 + i] = w[i];
}
NCG_DI int h2c448_check_op(int op, const uint32_t* __restrict__ a, uint32_t* __restrict__ out) {
  switch (op) {
    case 0:
    case 1: {
      uint32_t v[21], r[14];
#pragma unroll
      for (int i = 0; i < 21; i++) v[i] = a[i];
      if (op == 0) h2c448_mod_p(r, v);
      else h2c448_mod_n_be84(r, v);
#pragma unroll
      for (int i = 0; i < 14; i++) out[i] = r[i];
      return 0;
    }
    case 2: {
      uint32_t v[16], r[14];
#pragma unroll
      for (int i = 0; i < 16; i++) v[i] = a[i];
      h2c448_mod_n_le64(r, v);
#pragma unroll
      for (int i = 0; i < 14; i++) out[i] = r[i];
      return 0;
    }
    case 3: {
      const Curve448Frac m = h2c448_map_curve448(h2c448_load_u(a));
      h2c448_store3(out, m.xn, m.xd, m.y);
      return 0;
    }
    case 4: {
      const Ed448Pt p = h2c448_map_edwards448(h2c448_load_u(a));
      h2c448_store3(out, p.X, p.Y, p.Z);
      return 0;
    }
    default: return -1;
  }
}

}  // namespace ncg
