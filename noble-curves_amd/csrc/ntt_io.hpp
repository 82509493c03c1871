// Element and twiddle-table access shared by the kernels over the two scalar fields (ntt.hip, poly.hip): 16-byte loads /
// stores of canonical residues and the packed 9-limb entries of the twiddle table that ensure_ntt_table (api.hip) caches.
#pragma once
#include "fp.hpp"
#include "fr29.hpp"

namespace ncg {

using Fr = Fp<ParamsBlsR>;  // also the 8-word container of the pass code (loads, stores, word <-> limb conversion) for either field
template <class F>
using FrOf = Fp<typename F::M8>;  // the field the twiddle table is computed in

template <class T = Fr>
NCG_DI T fr_load_g(const uint32_t* __restrict__ p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  T r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
}
template <class T>
NCG_DI void fr_store_g(uint32_t* __restrict__ p, const T& r) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

NCG_DI uint32_t ntt_brev32(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __brev(x);
#else
  uint32_t r = 0;
  for (int i = 0; i < 32; i++) r |= ((x >> i) & 1u) << (31 - i);
  return r;
#endif
}

// twiddle table entry: the 9 limbs of w 2^261 mod r, no conversion on load.  Nine words per entry since the third session of round 6 (36 bytes at
// 4-byte alignment; twelve words = three aligned 16-byte loads before): a 2^22 transform reads its table about twice, a quarter less of it is 1-3 % of
// the transform (profiles/r06_ntt_tw36_ab.txt) and 50 MB less device memory per 2^22 table
constexpr int NTT_TW = 9;   // words per twiddle entry
struct __attribute__((packed, aligned(4))) NttTw9 { uint32_t v[9]; };
NCG_DI Fr29 ntt_load_tw(const uint32_t* __restrict__ p) {
  const NttTw9 t = *reinterpret_cast<const NttTw9*>(p);
  Fr29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = t.v[i];
  return r;
}
template <class T>
NCG_DI void ntt_store_tw(uint32_t* __restrict__ p, const T& canonical) {
  const Fr29 l = fr29_from_words(canonical.v);
  NttTw9 t;
#pragma unroll
  for (int i = 0; i < 9; i++) t.v[i] = l.v[i];
  *reinterpret_cast<NttTw9*>(p) = t;
}

}  // namespace ncg
