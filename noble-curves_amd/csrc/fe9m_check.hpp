// Self-check of the bn254 Montgomery form (fe9m.hpp) on RAW limbs, shared by the device (ncg_field_check field 9, selfcheck.hip)
// and the host twin (hosttest.hip).  a, b: 9 raw limbs at the bounds of `variant` (decimal digits A B); r: 9 raw limbs.
//   op 0 a*b   1 a^2   2 a + b   3 a - b   4 -a   5 1/a   6 weak normalisation   7 to wire (plain canonical, 8 words)
//   op 8 from wire (a = 8 LE words of a canonical residue)
#pragma once
#include "fe9.hpp"

namespace ncg {

template <int A, int B>
NCG_DI void fe9m_check_ab(int op, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  Fe9<Bn254PR, A> x;
  Fe9<Bn254PR, B> y;
  for (int i = 0; i < 9; i++) {
    x.v[i] = a[i];
    y.v[i] = b[i];
    r[i] = 0;
  }
  auto put = [&](const auto& z) {
    for (int i = 0; i < 9; i++) r[i] = z.v[i];
  };
  switch (op) {
    case 0: put(x * y); break;
    case 1: put(f_sqr(x)); break;
    case 2:
      if constexpr (A + B <= 7) put(x + y);
      break;
    case 3:
      if constexpr (A + B + 1 <= 7) put(x - y);
      break;
    case 4:
      if constexpr (A + 1 <= 7) put(f_neg(x));
      break;
    case 5: put(f_inv(x)); break;
    case 6: put(fe9_norm(x)); break;
    case 7: fe9_to_wire(r, x); break;
    case 8: put(fe9_from_wire<Bn254PR>(a)); break;
  }
}
NCG_DI int fe9m_check(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  switch (variant) {
    case 11: fe9m_check_ab<1, 1>(op, a, b, r); return 0;
    case 12: fe9m_check_ab<1, 2>(op, a, b, r); return 0;
    case 22: fe9m_check_ab<2, 2>(op, a, b, r); return 0;
    case 23: fe9m_check_ab<2, 3>(op, a, b, r); return 0;
    case 32: fe9m_check_ab<3, 2>(op, a, b, r); return 0;
    case 17: fe9m_check_ab<1, 7>(op, a, b, r); return 0;
    case 71: fe9m_check_ab<7, 1>(op, a, b, r); return 0;
    case 33: fe9m_check_ab<3, 3>(op, a, b, r); return 0;
    case 77: fe9m_check_ab<7, 7>(op, a, b, r); return 0;
  }
  return -1;
}

}  // namespace ncg
