// Self-check of the group law the MSM runs on its buckets, on STORED words (ncg_field_check fields 10-14, selfcheck.hip) and of
// the bls12-381 zero test under its branches (op 7 of fields 3 / 4); shared with the host twin (hosttest.hip ht_group_op /
// ht_fe29_eqz).  Nothing is converted on the way in or out: a, b and out are MsmGroup<C>::ACC_WORDS raw words in the layout
// acc_load / acc_store read and write (Montgomery form included); for ops 0 / 1 b holds AFF_WORDS words in aff_load's layout.
//   op 0 madd(a, b, false)   1 madd(a, b, true)   2 add(a, b)   3 dbl(a)
// The bounds f_eqz is instantiated at by the group law over Fe29 / Fe29x2P (every one reachable through op 7):
//     4   xyzz_add: U2 - U1 and S2 - S1 of two products (ec_sw.hpp; the complete routine of the cooperative form as well)
//    66   xyzz_madd: U2 - X1 and S2 - Y1, a product minus a STORED coordinate (bound 2 + 64) - the bucket accumulation
//   128   CoopXyzz::add: the difference of two values read back from LDS as stored coordinates (msm_coop.hpp FD = F - F)
#pragma once
#include "msm.hpp"

namespace ncg {

template <class C>
NCG_DI void group_check_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  using G = MsmGroup<C>;
  switch (op) {
    case 0:
    case 1: G::acc_store(out, G::madd(G::acc_load(a), G::aff_load(b), op == 1)); break;
    case 2: G::acc_store(out, G::add(G::acc_load(a), G::acc_load(b))); break;
    case 3: G::acc_store(out, G::dbl(G::acc_load(a))); break;
    default: break;
  }
}

// f_eqz of 14 raw limbs taken as FX<A> (FX = Fe29, or Fe29x2P: this lane's half, the verdict is the pair's); -1: unknown bound
template <template <int> class FX>
NCG_DI int fe29_eqz_check(int A, const uint32_t* limbs) {
  const Fe29<4096> h = FieldIO<Fe29<4096>>::load(limbs);
  auto as = [&](auto x) {
#pragma unroll
    for (int i = 0; i < 14; i++) x.v[i] = h.v[i];
    return x;
  };
  switch (A) {
    case 4: return f_eqz(FX<4>(as(Fe29<4>()))) ? 1 : 0;
    case 66: return f_eqz(FX<66>(as(Fe29<66>()))) ? 1 : 0;
    case 128: return f_eqz(FX<128>(as(Fe29<128>()))) ? 1 : 0;
    default: return -1;
  }
}

}  // namespace ncg
