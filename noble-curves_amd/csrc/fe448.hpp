// GF(p), p = 2^448 - 2^224 - 1 (the field of Ed448-Goldilocks and X448, reference src/ed448.ts:50-52): lane code, the same text
// on the device and on the CPU (hosttest.hip).
//
// Form: 16 limbs in radix 2^28.  224 = 8 * 28, so the Solinas fold 2^448 = 2^224 + 1 (mod p) lands on limb boundaries: a product
// column of weight 2^(28 k), k >= 16, goes to the columns k - 16 and k - 8 with no shift and no multiplication.
//
// Bounds: Fe448<B> holds limbs BELOW B * FE448_U, FE448_U = 2^28 + 2^10; the value is any representative (not reduced mod p).
// Every function states the bound it takes and the bound it gives; the types check them at compile time.
//   a + b              Fe448<A>, Fe448<B> -> Fe448<A + B>                         limb-wise, no carry
//   a - b              Fe448<A>, Fe448<B> -> Fe448<A + 2^k>, 2^k p the bias: k = 1 for B <= 1, 2 for B <= 3, 3 for B <= 7
//   fe448_neg(a)       Fe448<B> -> Fe448<1>                                       bias - a, then one weak pass
//   fe448_weak(a)      Fe448<B>, B <= 15 -> Fe448<1>                              one parallel carry pass, 32-bit
//   a * b              Fe448<A>, Fe448<B>, A * B <= 6 -> Fe448<1>                 256 multiply-adds
//   fe448_sqr(a)       Fe448<A>, A <= 2 (a wider operand takes the weak pass first) -> Fe448<1>     136 multiply-adds
//   fe448_mulk_add<K>(s, e)   s + K e, K < 2^16, Fe448<S <= 4>, Fe448<E <= 4> -> Fe448<1>           16 multiply-adds
//   fe448_to_words     Fe448<B>, B <= 8 -> 14 LE words, the CANONICAL residue (values in [p, 2^448) come out reduced)
//   fe448_from_words   14 LE words (any value below 2^448) -> Fe448<1>, congruent, not reduced
//   fe448_pow_pm3d4    x^((p - 3) / 4) by the reference's chain (ed448.ts:103-118): 445 squarings, 13 products
//   fe448_inv          x^(p - 2) = (x^((p - 3) / 4))^4 x (ed448.ts:286-290); 0 -> 0
//
// The product: with a = a0 + a1 phi, b = b0 + b1 phi, phi = 2^224, phi^2 = phi + 1:
//   a b = (a0 b0 + a1 b1) + (a0 b1 + a1 (b0 + b1)) phi = L + M phi,
// L and M are 15 columns each of 64-bit sums (four 8 x 8 half products, 256 multiply-adds, 8 additions for b0 + b1), and the
// columns 8..14 of M (weights 2^448 and up) come back once more: r_j = L_j + M_(j+8), r_(8+j) = L_(8+j) + M_j + M_(8+j).
// The heaviest column, r_8, sums 38 limb products: 38 * 6 * FE448_U^2 < 2^64 / (1 + 2^-28), hence A * B <= 6.
// (Karatsuba over phi - three half products, 192 multiply-adds - needs the column-wise difference (a0 + a1)(b0 + b1) - a0 b0
// and doubles the operand bound of its middle product; DESIGN.md section 8 has the count and why it is not the form built.)
#pragma once
#include "fp.hpp"

namespace ncg {

constexpr uint32_t FE448_MASK = (1u << 28) - 1;
constexpr uint64_t FE448_U = (1ull << 28) + (1ull << 10);

template <int B>
struct Fe448 {
  static constexpr int BOUND = B;
  uint32_t v[16];
  NCG_DI static Fe448 zero() {
    Fe448 r;
#pragma unroll
    for (int i = 0; i < 16; i++) r.v[i] = 0;
    return r;
  }
  NCG_DI static Fe448 one() {
    Fe448 r = zero();
    r.v[0] = 1;
    return r;
  }
};
using F448 = Fe448<1>;

// bias of a subtraction whose subtrahend has bound B: 2^k p, every limb of it at least B * FE448_U - 1
constexpr int fe448_sub_k(int b) { return b <= 1 ? 1 : b <= 3 ? 2 : 3; }

template <int A, int B>
NCG_DI Fe448<A + B> operator+(const Fe448<A>& a, const Fe448<B>& b) {
  static_assert((uint64_t)(A + B) * FE448_U <= (1ull << 32), "fe448 add: limb overflow");
  Fe448<A + B> r;
#pragma unroll
  for (int i = 0; i < 16; i++) r.v[i] = a.v[i] + b.v[i];
  return r;
}

template <int A, int B>
NCG_DI Fe448<A + (1 << fe448_sub_k(B))> operator-(const Fe448<A>& a, const Fe448<B>& b) {
  constexpr int K = fe448_sub_k(B);
  static_assert(B <= 7, "fe448 sub: subtrahend too wide");
  static_assert(((uint64_t)(FE448_MASK - 1) << K) >= (uint64_t)B * FE448_U - 1, "fe448 sub: bias too small");
  static_assert((uint64_t)(A + (1 << K)) * FE448_U <= (1ull << 32), "fe448 sub: limb overflow");
  Fe448<A + (1 << K)> r;
#pragma unroll
  for (int i = 0; i < 16; i++) r.v[i] = a.v[i] + (((i == 8) ? FE448_MASK - 1 : FE448_MASK) << K) - b.v[i];
  return r;
}

// one carry pass, every carry taken from the incoming limbs: limb i keeps its low 28 bits and takes the carry of limb i - 1
// (below 16); the carry of limb 15 (weight 2^448) goes to limbs 0 and 8.  Result limbs below 2^28 + 32.
template <int B>
NCG_DI F448 fe448_weak(const Fe448<B>& a) {
  static_assert(B <= 15, "fe448_weak: limb overflow");
  F448 r;
  const uint32_t top = a.v[15] >> 28;
#pragma unroll
  for (int i = 0; i < 16; i++) r.v[i] = (a.v[i] & FE448_MASK) + (i ? a.v[i - 1] >> 28 : top);
  r.v[8] += top;
  return r;
}

template <int B>
NCG_DI F448 fe448_neg(const Fe448<B>& a) {
  return fe448_weak(F448::zero() - a);
}

// the 16 columns of 64 bits -> limbs: one carry chain, the carry out of limb 15 (below 2^36) folded into limbs 0, 1 and 8, 9
NCG_DI void fe448_carry_cols(uint32_t (&o)[16], const uint64_t (&r)[16]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    c += r[i];
    o[i] = (uint32_t)c & FE448_MASK;
    c >>= 28;
  }
  const uint64_t f0 = o[0] + c, f8 = o[8] + c;
  o[0] = (uint32_t)f0 & FE448_MASK;
  o[1] += (uint32_t)(f0 >> 28);  // below 2^28 + 2^8 + 1
  o[8] = (uint32_t)f8 & FE448_MASK;
  o[9] += (uint32_t)(f8 >> 28);
}

NCG_DI void fe448_fold_cols(uint64_t (&r)[16], const uint64_t (&L)[15], const uint64_t (&M)[15]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    r[j] = L[j] + (j < 7 ? M[j + 8] : 0);
    r[8 + j] = M[j] + (j < 7 ? L[8 + j] + M[8 + j] : 0);
  }
}

NCG_MULFN void fe448_mul_limbs(uint32_t (&o)[16], const uint32_t (&a)[16], const uint32_t (&b)[16]) {
  uint64_t L[15], M[15], r[16];
  uint32_t bs[8];
#pragma unroll
  for (int i = 0; i < 15; i++) L[i] = M[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) bs[i] = b[i] + b[8 + i];
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      L[i + j] += (uint64_t)a[i] * b[j];
      L[i + j] += (uint64_t)a[8 + i] * b[8 + j];
      M[i + j] += (uint64_t)a[i] * b[8 + j];
      M[i + j] += (uint64_t)a[8 + i] * bs[j];
    }
  }
  fe448_fold_cols(r, L, M);
  fe448_carry_cols(o, r);
}

// a^2: L = a0^2 + a1^2 by the symmetric halves (2 * 36 multiply-adds), M = a1 (2 a0 + a1) (64)
NCG_MULFN void fe448_sqr_limbs(uint32_t (&o)[16], const uint32_t (&a)[16]) {
  uint64_t L[15], M[15], r[16];
  uint32_t ad[16], as[8];
#pragma unroll
  for (int i = 0; i < 15; i++) L[i] = M[i] = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) ad[i] = a[i] << 1;
#pragma unroll
  for (int i = 0; i < 8; i++) as[i] = ad[i] + a[8 + i];
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (j >= i) {
        L[i + j] += (uint64_t)a[i] * (j > i ? ad[j] : a[j]);
        L[i + j] += (uint64_t)a[8 + i] * (j > i ? ad[8 + j] : a[8 + j]);
      }
      M[i + j] += (uint64_t)a[8 + i] * as[j];
    }
  }
  fe448_fold_cols(r, L, M);
  fe448_carry_cols(o, r);
}

template <int A, int B>
NCG_DI F448 operator*(const Fe448<A>& a, const Fe448<B>& b) {
  static_assert(A * B <= 6, "fe448 mul: the heaviest column (38 products) overflows 64 bits");
  F448 r;
  fe448_mul_limbs(r.v, a.v, b.v);
  return r;
}

template <int A>
NCG_DI F448 fe448_sqr(const Fe448<A>& a) {
  F448 r;
  if constexpr (A <= 2) {
    fe448_sqr_limbs(r.v, a.v);
  } else {
    const F448 w = fe448_weak(a);
    fe448_sqr_limbs(r.v, w.v);
  }
  return r;
}

// s + K e for a small constant K, one 64-bit carry chain; the carry out of limb 15 ripples one limb into 1 and 9
template <uint32_t K, int S, int E>
NCG_DI F448 fe448_mulk_add(const Fe448<S>& s, const Fe448<E>& e) {
  static_assert(K < (1u << 16) && S <= 4 && E <= 4, "fe448_mulk_add: bounds");
  F448 r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    c += s.v[i];
    c += (uint64_t)e.v[i] * K;
    r.v[i] = (uint32_t)c & FE448_MASK;
    c >>= 28;
  }
  const uint32_t f0 = r.v[0] + (uint32_t)c, f8 = r.v[8] + (uint32_t)c;  // c below 2^21
  r.v[0] = f0 & FE448_MASK;
  r.v[1] += f0 >> 28;
  r.v[8] = f8 & FE448_MASK;
  r.v[9] += f8 >> 28;
  return r;
}

// ---- wire form: 56 bytes little-endian = 14 LE words
NCG_DI F448 fe448_from_words(const uint32_t (&w)[14]) {
  F448 r;
  uint64_t acc = 0;
  int bits = 0, k = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    if (bits < 28) {
      acc |= (uint64_t)w[k++] << bits;
      bits += 32;
    }
    r.v[i] = (uint32_t)acc & FE448_MASK;
    acc >>= 28;
    bits -= 28;
  }
  return r;
}

// The canonical residue.  Three sequential carry passes leave every limb below 2^28 and the value below 2^448 (the second pass can
// carry out of limb 15 only when limbs 9..15 were all ones and wrapped to zero, so the third cannot); then p is taken off once
// where the value is at least p: v >= p exactly when v + 2^224 + 1 carries out of bit 448.
template <int B>
NCG_DI void fe448_to_words(uint32_t (&w)[14], const Fe448<B>& a) {
  static_assert(B <= 8, "fe448_to_words: limb overflow");
  uint32_t t[16], s[16];
#pragma unroll
  for (int i = 0; i < 16; i++) t[i] = a.v[i];
#pragma unroll
  for (int pass = 0; pass < 3; pass++) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint32_t x = t[i] + c;
      t[i] = x & FE448_MASK;
      c = x >> 28;
    }
    t[0] += c;
    t[8] += c;
  }
  uint32_t c = 1;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint32_t x = t[i] + c + (i == 8 ? 1u : 0u);
    s[i] = x & FE448_MASK;
    c = x >> 28;
  }
  const bool ge = c != 0;
  uint64_t acc = 0;
  int bits = 0, k = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    acc |= (uint64_t)(ge ? s[i] : t[i]) << bits;
    bits += 28;
    if (bits >= 32) {
      w[k++] = (uint32_t)acc;
      acc >>= 32;
      bits -= 32;
    }
  }
}

NCG_DI bool fe448_words_eq(const uint32_t (&a)[14], const uint32_t (&b)[14]) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) d |= a[i] ^ b[i];
  return d == 0;
}
NCG_DI bool fe448_words_small(const uint32_t (&a)[14], uint32_t v) {  // a == v, v one word
  uint32_t d = a[0] ^ v;
#pragma unroll
  for (int i = 1; i < 14; i++) d |= a[i];
  return d == 0;
}
// on canonical values
template <int B>
NCG_DI bool fe448_is_zero(const Fe448<B>& a) {
  uint32_t w[14];
  fe448_to_words(w, a);
  return fe448_words_small(w, 0u);
}
template <int A, int B>
NCG_DI bool fe448_eq(const Fe448<A>& a, const Fe448<B>& b) {
  uint32_t x[14], y[14];
  fe448_to_words(x, a);
  fe448_to_words(y, b);
  return fe448_words_eq(x, y);
}
template <int B>
NCG_DI uint32_t fe448_parity(const Fe448<B>& a) {
  uint32_t w[14];
  fe448_to_words(w, a);
  return w[0] & 1u;
}

NCG_DI F448 fe448_sqr_n(F448 x, int n) {
  for (int i = 0; i < n; i++) x = fe448_sqr(x);
  return x;
}

// x^((p - 3) / 4): the exponent is 223 ones, a zero, 222 ones (ed448.ts:100-118)
NCG_DI F448 fe448_pow_pm3d4(const F448& x) {
  const F448 b2 = fe448_sqr(x) * x;
  const F448 b3 = fe448_sqr(b2) * x;
  const F448 b6 = fe448_sqr_n(b3, 3) * b3;
  const F448 b9 = fe448_sqr_n(b6, 3) * b3;
  const F448 b11 = fe448_sqr_n(b9, 2) * b2;
  const F448 b22 = fe448_sqr_n(b11, 11) * b11;
  const F448 b44 = fe448_sqr_n(b22, 22) * b22;
  const F448 b88 = fe448_sqr_n(b44, 44) * b44;
  const F448 b176 = fe448_sqr_n(b88, 88) * b88;
  const F448 b220 = fe448_sqr_n(b176, 44) * b44;
  const F448 b222 = fe448_sqr_n(b220, 2) * b2;
  const F448 b223 = fe448_sqr(b222) * x;
  return fe448_sqr_n(b223, 223) * b222;
}

NCG_DI F448 fe448_inv(const F448& x) { return fe448_sqr_n(fe448_pow_pm3d4(x), 2) * x; }

}  // namespace ncg
