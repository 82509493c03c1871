// Self-check of the radix-2^29 lazy field form (fe9.hpp) over secp256k1 / ed25519 p on RAW limbs, shared by the device
// (ncg_field_check fields 0 / 1 and 5 / 6, selfcheck.hip) and the host twin (hosttest.hip ht_fe9_op / ht_fe9_fused).  The tests
// feed limbs at the top of what a bound type admits, so the inline-asm multiply-add chains and the bound-typed lazy reduction
// are pinned directly.  Whatever an op does not write stays as the caller left it (zero on the device).
#pragma once
#include "fe9.hpp"

namespace ncg {

// fields 0 / 1.  a, b: 9 raw limbs at the bounds A, B; r: 8 words, the canonical wire value unless noted.
//   op 0 a*b   1 a^2 (normalised first when A > 2)   2 a + b   3 a - b   4 -a   5 1/a   6 normalise   7 r[0] = a is zero mod p
//   op 8 r[0] = largest limb of the normalised a   9 r[0] = largest limb of the raw product, r[1..8) = 0   10 2 a
// An op the bounds do not admit writes nothing.
template <class PR, int A, int B>
NCG_DI void fe9_check_ab(int op, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  Fe9<PR, A> x;
  Fe9<PR, B> y;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    x.v[i] = a[i];
    y.v[i] = b[i];
  }
  auto max_limb = [](const auto& n) {
    uint32_t mx = 0;
    for (int i = 0; i < 9; i++) mx = n.v[i] > mx ? n.v[i] : mx;
    return mx;
  };
  switch (op) {
    case 0: fe9_to_wire(r, x * y); break;
    case 1:
      if constexpr (A <= 2) fe9_to_wire(r, f_sqr(x));
      else fe9_to_wire(r, f_sqr(fe9_norm(x)));
      break;
    case 2: if constexpr (A + B <= 7) fe9_to_wire(r, x + y); break;
    case 3: if constexpr (A + B + 1 <= 7) fe9_to_wire(r, x - y); break;
    case 4: if constexpr (A + 1 <= 7) fe9_to_wire(r, f_neg(x)); break;
    case 5: fe9_to_wire(r, f_inv(x)); break;
    case 6: fe9_to_wire(r, fe9_norm(x)); break;
    case 7: r[0] = f_eqz(x) ? 1u : 0u; break;
    case 8: r[0] = max_limb(fe9_norm(x)); break;  // norm must leave limbs below U
    case 9:                                       // the output bound of the product
      for (int i = 0; i < 8; i++) r[i] = 0;
      r[0] = max_limb(x * y);
      break;
    case 10: if constexpr (2 * A <= 7) fe9_to_wire(r, f_dbl(x)); break;
  }
}
// `variant` = 10 A + B picks the operand bound types; -1 for one that is not instantiated
template <class PR>
NCG_DI int fe9_check(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  switch (variant) {
    case 11: fe9_check_ab<PR, 1, 1>(op, a, b, r); return 0;
    case 12: fe9_check_ab<PR, 1, 2>(op, a, b, r); return 0;
    case 17: fe9_check_ab<PR, 1, 7>(op, a, b, r); return 0;
    case 71: fe9_check_ab<PR, 7, 1>(op, a, b, r); return 0;
    case 23: fe9_check_ab<PR, 2, 3>(op, a, b, r); return 0;
    case 32: fe9_check_ab<PR, 3, 2>(op, a, b, r); return 0;
    case 22: fe9_check_ab<PR, 2, 2>(op, a, b, r); return 0;
    case 15: fe9_check_ab<PR, 1, 5>(op, a, b, r); return 0;
    case 33: fe9_check_ab<PR, 3, 3>(op, a, b, r); return 0;
    case 77: fe9_check_ab<PR, 7, 7>(op, a, b, r); return 0;
    case 46: fe9_check_ab<PR, 4, 6>(op, a, b, r); return 0;
  }
  return -1;
}

// fields 5 / 6: the fused expressions (f_mul_mul / f_mul_sqr / f_mul_add / f_sqr_add / f_half).  a, b, c, d: 9 raw limbs at
// the bounds A, B, C, D; r: the 9 RAW limbs of the result, so that the tests check the output bound as well.
//   op 0 a*b + c*d   1 a*b + c^2   2 a*b + c   3 a^2 + c   4 a / 2
// No combination a fused op rejects is instantiated: such an op writes nothing.
template <class PR, int A, int B, int C, int D>
NCG_DI void fe9_fused_check_abcd(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* r) {
  Fe9<PR, A> x;
  Fe9<PR, B> y;
  Fe9<PR, C> z;
  Fe9<PR, D> w;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    x.v[i] = a[i];
    y.v[i] = b[i];
    z.v[i] = c[i];
    w.v[i] = d[i];
  }
  auto put = [&](const auto& o) {
#pragma unroll
    for (int i = 0; i < 9; i++) r[i] = o.v[i];
  };
  if constexpr (A * B + C * D <= 7) {
    if (op == 0) put(f_mul_mul(x, y, z, w));
  }
  if constexpr (C <= 2 && A * B + C * C <= 7) {
    if (op == 1) put(f_mul_sqr(x, y, z));
  }
  if constexpr (A * B <= 7) {
    if (op == 2) put(f_mul_add(x, y, z));
  }
  if constexpr (A <= 2) {
    if (op == 3) put(f_sqr_add(x, z));
  }
  if constexpr (A == 1) {
    if (op == 4) put(f_half(x));
  }
}
// `variant` = the decimal digits A B C D; -1 for a combination that is not instantiated
template <class PR>
NCG_DI int fe9_fused_check(int op, int variant, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* r) {
  switch (variant) {
    case 1111: fe9_fused_check_abcd<PR, 1, 1, 1, 1>(op, a, b, c, d, r); return 0;
    case 1322: fe9_fused_check_abcd<PR, 1, 3, 2, 2>(op, a, b, c, d, r); return 0;
    case 3211: fe9_fused_check_abcd<PR, 3, 2, 1, 1>(op, a, b, c, d, r); return 0;
    case 2311: fe9_fused_check_abcd<PR, 2, 3, 1, 1>(op, a, b, c, d, r); return 0;
    case 1123: fe9_fused_check_abcd<PR, 1, 1, 2, 3>(op, a, b, c, d, r); return 0;
    case 3121: fe9_fused_check_abcd<PR, 3, 1, 2, 1>(op, a, b, c, d, r); return 0;
    case 1327: fe9_fused_check_abcd<PR, 1, 3, 2, 7>(op, a, b, c, d, r); return 0;
    case 7171: fe9_fused_check_abcd<PR, 7, 1, 7, 1>(op, a, b, c, d, r); return 0;
    case 1771: fe9_fused_check_abcd<PR, 1, 7, 7, 1>(op, a, b, c, d, r); return 0;
    case 2171: fe9_fused_check_abcd<PR, 2, 1, 7, 1>(op, a, b, c, d, r); return 0;
  }
  return -1;
}

}  // namespace ncg
