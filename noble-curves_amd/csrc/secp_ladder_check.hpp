// Self-check of the pieces of the secp256k1 fused ladder (CurveSecpI) on RAW limbs, shared by the device (ncg_field_check
// field 7, selfcheck.hip) and the host twin (hosttest.hip ht_jac_neg / ht_glv_split_odd / ht_glv_split_k1_odd; ht_jac_neg_nx
// and ht_glv_split use the load / store helpers).
#pragma once
#include "curves.hpp"
#include "scalar.hpp"

namespace ncg {

// a Jacobian point as 27 raw limbs X, Y, Z (the storage bound 2)
NCG_DI Jac<FeSecp> jac_load_limbs(const uint32_t* p) {
  Jac<FeSecp> P;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    P.X.v[i] = p[i];
    P.Y.v[i] = p[9 + i];
    P.Z.v[i] = p[18 + i];
  }
  return P;
}
NCG_DI void jac_store_limbs(uint32_t* out, const Jac<FeSecp>& R) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    out[i] = R.X.v[i];
    out[9 + i] = R.Y.v[i];
    out[18 + i] = R.Z.v[i];
  }
}
template <int B>
NCG_DI Fe9<Fe9SecpPR, B> fe9_load_limbs(const uint32_t* p) {
  Fe9<Fe9SecpPR, B> x;
#pragma unroll
  for (int i = 0; i < 9; i++) x.v[i] = p[i];
  return x;
}
// the GLV split of the scalar k[0..8)
NCG_DI GlvSplit glv_split_words(const uint32_t* k) {
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kk[i] = k[i];
  return secp_glv_split(kk);
}
// 12 words: k1[5] k2[5] k1neg k2neg
NCG_DI void glv_store(uint32_t* out, const GlvSplit& s) {
#pragma unroll
  for (int i = 0; i < 5; i++) {
    out[i] = s.k1[i];
    out[5 + i] = s.k2[i];
  }
  out[10] = s.k1neg;
  out[11] = s.k2neg;
}

// op 0 jac_dbl_neg(P), op 1 jac_madd_neg(P, qx, qy) (ec_sw.hpp) with P = a (27 limbs), qx at bound 2, qy at bound 3 (a negated
// table entry): out = X, Y, Z.  op 2 secp_glv_split + secp_glv_make_odd, op 3 secp_glv_split + secp_glv_make_k1_odd (the split
// of CurveSecpI's ladder) of the scalar a[0..8): out[0..12) in glv_store's layout; qx and qy are not read.  -1, and nothing
// written, for any other op.
NCG_DI int secp_ladder_check(int op, const uint32_t* a, const uint32_t* qx, const uint32_t* qy, uint32_t* out) {
  if (op == 0 || op == 1) {
    const Jac<FeSecp> P = jac_load_limbs(a);
    jac_store_limbs(out, op == 0 ? jac_dbl_neg(P) : jac_madd_neg(P, fe9_load_limbs<2>(qx), fe9_load_limbs<3>(qy)));
    return 0;
  }
  if (op == 2 || op == 3) {
    GlvSplit s = glv_split_words(a);
    if (op == 2) secp_glv_make_odd(s);
    else secp_glv_make_k1_odd(s);
    glv_store(out, s);
    return 0;
  }
  return -1;
}

}  // namespace ncg
