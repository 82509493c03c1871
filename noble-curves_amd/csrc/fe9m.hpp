// The bn254 (alt_bn128, EIP-196) base field in radix 2^29: 9 limbs, Montgomery products with R = 2^261, lazy additions.
// The element type is fe9.hpp's Fe9<Bn254PR, B> (Bn254PR::MONT selects the branches below), so ec_sw.hpp instantiates unchanged.
//
// Why Montgomery here: the two other 9-limb forms lean on their prime - fe9.hpp folds with 2^261 = C0 + C1 2^29 (small C0, C1)
// and fr29.hpp on r = 1 (mod 2^29).  bn254's p has neither, so the product is product-scanning Montgomery: column k
// accumulates a_i b_j and q_i p_j in ONE 64-bit accumulator (v_mad_u64_u32, p's limbs in SGPRs) and the quotient digit is
// q_k = t_k N' mod 2^29 (N' = -p^-1 mod 2^29): one v_mul_lo_u32 and a mask, no carry instruction anywhere.  81 + 81 + 9
// multiply-adds per product, 45 + 81 + 9 per square (fe9_asm_gen-style blocks: fe9m_gen.hpp, tools/gen_fe9m.py).
// The wire <-> Montgomery conversion happens at load and store only.
//
// Bounds.  p < 2^254 leaves 7 bits below 2^261 (2^261 / p = 169.3).  An element of bound B (the type's B, 1 <= B <= 7) has
//   * limbs below B 2^29 (limb 8 included), and
//   * value below 2 B p - so its limb 8 is below 2 B p / 2^232 < B 2^22.6.
// Each op keeps both: a + b adds the bounds; a - b = a + BIAS[B] - b with BIAS[B] = (2B + 1) p, limbs 0..7 in
// [B 2^29, (B + 1) 2^29) and limb 8 above any bound-B limb 8, so the result has bound A + B + 1 (fe9.hpp's rule); the product of
// bounds A, B (A B <= 7) is below A B (2p)^2 / 2^261 + p < 1.17 p with exact limbs 0..7: bound 1.  Column budget: no column
// holds more than 8 products of two large limbs (column 8's a_0 b_8 and a_8 b_0 are small) plus the q p terms, whose limbs
// 0..7 of p sum to 3.01 * 2^29: 8 * 7 * 2^58 + 3.01 * 2^58 + carry < 2^64.  The square doubles one operand: A <= 2.
// The weak normalisation (fe9m_reduce, the narrowing conversion) carries the limbs and subtracts q p for a quotient estimate
// from limb 8: exact limbs, value below 2p.  Canonical residues only at store and compare.
//
// The host twin (same source, hosttest.hip) counts 64-bit column overflows (fe9m_overflows), like fr29.hpp.
#pragma once
#include <stdint.h>

#include "fp.hpp"

namespace ncg {

constexpr uint32_t FE9M_MASK = (1u << 29) - 1u;

// host twin only: counts 64-bit column overflows so the unit tests can assert there are none
inline int& fe9m_overflows() {
  static int n = 0;
  return n;
}

NCG_DI void fe9m_mac(uint64_t& acc, uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b) : "vcc");
#else
  const uint64_t s = acc + (uint64_t)a * b;
  if (s < acc) fe9m_overflows()++;
  acc = s;
#endif
}
// acc += a * k for a wave-uniform constant k (kept in an SGPR)
NCG_DI void fe9m_mac_k(uint64_t& acc, uint32_t a, uint32_t k) {
#ifdef __HIP_DEVICE_COMPILE__
  asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(a), "s"(k) : "vcc");
#else
  fe9m_mac(acc, a, k);
#endif
}

}  // namespace ncg

#include "fe9m_gen.hpp"

namespace ncg {

// r = a * b / 2^261 (mod p): exact limbs 0..7, value below a b / 2^261 + p.  y = b for the product; for the square (SQR) y = 2a
// and the off-diagonal products are taken once.
template <bool SQR>
NCG_DI void fe9m_mont_limbs(uint32_t (&r)[9], const uint32_t (&a)[9], const uint32_t (&y)[9]) {
#ifdef __HIP_DEVICE_COMPILE__  // one asm block per column (fe9m_gen.hpp)
  if constexpr (SQR) {
    NCG_FE9M_SQR_BLOCKS(a, y, r)
  } else {
    NCG_FE9M_MUL_BLOCKS(a, y, r)
  }
  return;
#endif
  uint32_t q[9];
  uint64_t acc = 0;
  for (int k = 0; k < 17; k++) {
    const int lo = k > 8 ? k - 8 : 0, hi = k < 8 ? k : 8;
    for (int i = lo; i <= hi; i++) {
      const int j = k - i;
      if (!SQR) fe9m_mac(acc, a[i], y[j]);
      else if (i < j) fe9m_mac(acc, a[i], y[j]);
      else if (i == j) fe9m_mac(acc, a[i], a[i]);
    }
    for (int i = lo; i < (k < 9 ? k : 9); i++) fe9m_mac(acc, q[i], Bn254PR::P[k - i]);
    if (k < 9) {
      q[k] = ((uint32_t)acc * Bn254PR::NP) & FE9M_MASK;
      fe9m_mac(acc, q[k], Bn254PR::P[0]);  // the low 29 bits cancel
#ifndef __HIP_DEVICE_COMPILE__
      if ((uint32_t)acc & FE9M_MASK) fe9m_overflows()++;
#endif
    } else {
      r[k - 9] = (uint32_t)acc & FE9M_MASK;
    }
    acc >>= 29;
  }
#ifndef __HIP_DEVICE_COMPILE__
  if (acc >> 32) fe9m_overflows()++;
#endif
  r[8] = (uint32_t)acc;
}

// weak normalisation: limbs below 2^32 and a value below 2^261 (any bound <= 7) -> exact limbs, value below 2p.  Carries
// first; q = floor(limb8 * RECIP / 2^40) is floor(value / p) or one less, and value - q p goes through a signed carry chain.
NCG_DI void fe9m_reduce(uint32_t (&r)[9], const uint32_t (&a)[9]) {
  uint32_t t[9];
  uint64_t cy = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    cy += a[i];
    t[i] = (uint32_t)cy & FE9M_MASK;
    cy >>= 29;
  }
  t[8] = a[8] + (uint32_t)cy;
  const uint32_t q = (uint32_t)(((uint64_t)t[8] * Bn254PR::RECIP) >> 40);
  int64_t e = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    e += (int64_t)t[i] - (int64_t)((uint64_t)q * Bn254PR::P[i]);
    r[i] = (uint32_t)e & FE9M_MASK;
    e >>= 29;  // arithmetic: the borrow
  }
  r[8] = (uint32_t)(e + (int64_t)t[8] - (int64_t)((uint64_t)q * Bn254PR::P[8]));
}

// exact limbs, value below 2p -> canonical residue
NCG_DI void fe9m_cond_sub(uint32_t (&o)[9], const uint32_t (&t)[9]) {
  uint32_t s[9];
  int32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int32_t d = (int32_t)t[i] - (int32_t)Bn254PR::P[i] + bw;
    s[i] = (uint32_t)d & FE9M_MASK;
    bw = d >> 29;
  }
  const bool ge = bw == 0;
#pragma unroll
  for (int i = 0; i < 9; i++) o[i] = ge ? s[i] : t[i];
}

// 8 LE words (a value below 2^256) <-> exact limbs
NCG_DI void fe9m_limbs_from_words(uint32_t (&r)[9], const uint32_t* __restrict__ p) {
  uint32_t w[10];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = p[i];
  w[8] = 0;
  w[9] = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, limb = bit >> 5, sh = bit & 31;
    const uint64_t two = ((uint64_t)w[limb + 1] << 32) | w[limb];
    r[i] = (uint32_t)(two >> sh) & FE9M_MASK;
  }
}
NCG_DI void fe9m_words_from_limbs(uint32_t* __restrict__ p, const uint32_t (&c)[9]) {
  uint32_t l[11];
#pragma unroll
  for (int i = 0; i < 9; i++) l[i] = c[i];
  l[9] = 0;
  l[10] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int bit = 32 * k, limb = bit / 29, sh = bit % 29;
    uint64_t acc = (uint64_t)l[limb] >> sh;
    acc |= (uint64_t)l[limb + 1] << (29 - sh);
    acc |= (uint64_t)l[limb + 2] << (58 - sh);
    p[k] = (uint32_t)acc;
  }
}

// canonical residue (plain, not Montgomery) of the Montgomery element a: a / R, then the conditional subtraction
NCG_DI void fe9m_canon_plain(uint32_t (&o)[9], const uint32_t (&a)[9]) {
  uint32_t one[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0}, t[9];
  fe9m_mont_limbs<false>(t, a, one);  // value below a / 2^261 + p < 1.01 p
  fe9m_cond_sub(o, t);
}
// wire (canonical residue, below 2^256) -> Montgomery element of bound 1: x R^2 / R
NCG_DI void fe9m_from_wire(uint32_t (&r)[9], const uint32_t* __restrict__ p) {
  uint32_t x[9], r2[9];
  fe9m_limbs_from_words(x, p);
#pragma unroll
  for (int i = 0; i < 9; i++) r2[i] = Bn254PR::R2[i];
  fe9m_mont_limbs<false>(r, x, r2);
}

}  // namespace ncg
