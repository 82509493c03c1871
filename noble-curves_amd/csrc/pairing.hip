// bls12-381 pairings for a batch (include/ncg.h "pairings"): one pair, group or Fp12 element per lane PAIR.
//
//   k_pairing_miller   per pair: the checks of pairingBatch (src/abstract/bls.ts:685-688), then the Miller loop; the
//                      value goes to the workspace (168 words per pair, Montgomery limbs)
//   k_pairing_product  the product of each group's Miller values by passes of stride 1, 2, 4, ..: element r of a
//                      group (r a multiple of 2 s) takes in element r + s.  ceil(log2(largest group)) passes, any
//                      group size, groups may straddle blocks: a pass only reads elements no lane of it writes.
//   k_pairing_final    per group: final exponentiation (src/bls12-381.ts:258-276), canonical store, is_one
//   k_fp12_op          bls12_381.fields.Fp12 for a batch
// One wave per block: 32 lane pairs.  Register and scratch figures: DESIGN.md section 8.
#include <vector>

#include "host_api.hpp"
#include "pairing.hpp"

namespace ncg {

using PairP = Pairing<Fe29x2P>;
using TowP = Tower<Fe29x2P>;
constexpr int PAIRING_BLOCK = 64;

__global__ void __launch_bounds__(PAIRING_BLOCK) k_pairing_miller(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2,
                                                                  int subgroup, uint32_t* __restrict__ ws,
                                                                  unsigned long long* __restrict__ first_bad, int n) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // two lanes per pair
  if (i >= n) return;
  Fe29<2> Px, Py;
  TowP::E2 Qx, Qy;
  const uint32_t code = PairP::load_checked(g1 + (size_t)i * 24, g2 + (size_t)i * 48, subgroup != 0, Px, Py, Qx, Qy);  // pair-uniform
  if (code != PAIRING_OK) {  // the call fails: the smallest index wins, nothing of this pair is read again
    if ((threadIdx.x & 1) == 0) atomicMin(first_bad, ((unsigned long long)i << 8) | code);
    return;
  }
  TowP::E12 f;
  PairP::miller_loop(f, Px, Py, Qx, Qy);
  TowP::store_ws(ws + (size_t)i * FP12_WS_WORDS, f);
}

// the group of pair i: the largest g with off[g] <= i (off[n_groups] = n > i; empty groups repeat an offset)
NCG_DI int pairing_group_of(const uint32_t* __restrict__ off, int n_groups, uint32_t i) {
  int lo = 0, hi = n_groups;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(PAIRING_BLOCK) k_pairing_product(uint32_t* __restrict__ ws, const uint32_t* __restrict__ off, int n_groups,
                                                                   int n, uint32_t stride) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (i >= n) return;
  const int g = pairing_group_of(off, n_groups, (uint32_t)i);
  const uint32_t rel = (uint32_t)i - off[g], size = off[g + 1] - off[g];
  if ((rel & (2 * stride - 1)) != 0 || rel + stride >= size) return;
  TowP::E12 a = TowP::load_ws(ws + (size_t)i * FP12_WS_WORDS);
  const TowP::E12 b = TowP::load_ws(ws + ((size_t)i + stride) * FP12_WS_WORDS);
  TowP::mul(a, a, b);
  TowP::store_ws(ws + (size_t)i * FP12_WS_WORDS, a);
}

__global__ void __launch_bounds__(PAIRING_BLOCK) k_pairing_final(const uint32_t* __restrict__ ws, const uint32_t* __restrict__ off, int n_groups,
                                                                 uint32_t* __restrict__ out_gt, uint8_t* __restrict__ out_is_one) {
  const int g = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (g >= n_groups) return;
  TowP::E12 r = TowP::E12::one();  // an empty group
  if (off[g + 1] > off[g]) {
    const TowP::E12 f = TowP::load_ws(ws + (size_t)off[g] * FP12_WS_WORDS);
    TowP::final_exponentiate(r, f);
  }
  if (out_gt) TowP::store_wire(out_gt + (size_t)g * FP12_WIRE_WORDS, r);
  const bool one = f12_is_one(r);
  if ((threadIdx.x & 1) == 0) out_is_one[g] = one ? 1 : 0;
}

// ---- Fp12 for a batch: out = op(a, b).  b: an Fp12 (mul), three Fp2 o0 o1 o4 (mul014), unused otherwise.
// out: an Fp12, or one byte (is_one).  `even` says whether this lane writes the byte.
// RAW (host twin only): a is read in the workspace form, 168 words of Montgomery limbs as they are, so that a test can hand in limbs at
// the top of the storage bound.
template <template <int> class F2, bool RAW = false>
NCG_DI void fp12_op_lane(int op, const uint32_t* a, const uint32_t* b, void* out, size_t row,
                         bool even) {
  using T = Tower<F2>;
  typename T::E12 x = RAW ? T::load_ws(a + row * FP12_WS_WORDS) : T::load_wire(a + row * FP12_WIRE_WORDS), r;
  switch (op) {
    case 0: {
      const typename T::E12 y = T::load_wire(b + row * FP12_WIRE_WORDS);
      T::mul(r, x, y);
      break;
    }
    case 1: T::sqr(r, x); break;
    case 2: T::inv(r, x); break;
    case 3: T::conj(r, x); break;
    case 4: T::frob1(r, x); break;
    case 5: T::frob2(r, x); break;
    case 6: T::frob3(r, x); break;
    case 7: T::cyclotomic_sqr(r, x); break;
    case 8: {
      const uint32_t* o = b + row * 72;
      T::mul014(r, x, T::load2_wire(o), T::load2_wire(o + 24), T::load2_wire(o + 48));
      break;
    }
    case 9: T::final_exponentiate(r, x); break;
    default: {  // 10: Fp12.eql(a, ONE)
      const bool one = f12_is_one(x);
      if (even) ((uint8_t*)out)[row] = one ? 1 : 0;
      return;
    }
  }
  T::store_wire((uint32_t*)out + row * FP12_WIRE_WORDS, r);
}

__global__ void __launch_bounds__(PAIRING_BLOCK) k_fp12_op(int op, const uint32_t* a, const uint32_t* b, void* out, int n) {  // out may be a or b

  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (i >= n) return;
  fp12_op_lane<Fe29x2P>(op, a, b, out, (size_t)i, (threadIdx.x & 1) == 0);
}

static dim3 pairing_grid(int items) { return dim3((unsigned)(((size_t)items * 2 + PAIRING_BLOCK - 1) / PAIRING_BLOCK)); }

hipError_t pairing_miller(const uint32_t* g1, const uint32_t* g2, int subgroup, uint32_t* ws, unsigned long long* first_bad, int n, hipStream_t st) {
  hipError_t e = hipMemsetAsync(first_bad, 0xFF, 8, st);
  if (e != hipSuccess || n <= 0) return e;
  hipLaunchKernelGGL(k_pairing_miller, pairing_grid(n), dim3(PAIRING_BLOCK), 0, st, g1, g2, subgroup, ws, first_bad, n);
  return hipGetLastError();
}
hipError_t pairing_finish(uint32_t* ws, const uint32_t* off, int n_groups, int n, uint32_t largest_group, uint32_t* out_gt,
                          uint8_t* out_is_one, hipStream_t st) {
  if (n_groups <= 0) return hipSuccess;
  for (uint32_t s = 1; s < largest_group; s *= 2) {
    hipLaunchKernelGGL(k_pairing_product, pairing_grid(n), dim3(PAIRING_BLOCK), 0, st, ws, off, n_groups, n, s);
    if (s >= (1u << 31)) break;
  }
  hipLaunchKernelGGL(k_pairing_final, pairing_grid(n_groups), dim3(PAIRING_BLOCK), 0, st, ws, off, n_groups, out_gt, out_is_one);
  return hipGetLastError();
}
hipError_t fp12_batch(int op, const uint32_t* a, const uint32_t* b, void* out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fp12_op, pairing_grid(n), dim3(PAIRING_BLOCK), 0, st, op, a, b, out, n);
  return hipGetLastError();
}

// ---- BLS verification rows (ncg_bls_verify_batch): from the decoded keys and signatures and the mapped messages to two pairs per row,
//   long signatures (scheme 0):  e(-pk, H(m)) e(G1, sig)        short (scheme 1):  e(H(m), -pk) e(sig, G2)
// A row whose key or signature did not decode or is ZERO (or whose message maps to ZERO) verifies false (bls.ts:812-817): it gets the
// generators as pairs, so that the pairing kernels see valid points, and bad[i] = 1.
NCG_DI void bls_copy(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int words) {
  for (int k = 0; k < words; k++) dst[k] = src[k];
}
NCG_DI void bls_copy_neg(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int fw) {  // (x, -y), fw words per coordinate
  bls_copy(dst, src, fw);
  for (int c = 0; c < fw / 12; c++) {
    uint32_t w[12];
    for (int k = 0; k < 12; k++) w[k] = src[fw + 12 * c + k];
    words12_neg_mod_p(w);
    for (int k = 0; k < 12; k++) dst[fw + 12 * c + k] = w[k];
  }
}
__global__ void __launch_bounds__(256) k_bls_pairs(int scheme, const uint32_t* __restrict__ pk, const uint8_t* __restrict__ pk_ok,
                                                   const uint8_t* __restrict__ pk_inf, const uint32_t* __restrict__ sig,
                                                   const uint8_t* __restrict__ sig_ok, const uint8_t* __restrict__ sig_inf,
                                                   const uint32_t* __restrict__ hm, const uint8_t* __restrict__ hm_inf,
                                                   uint32_t* __restrict__ g1, uint32_t* __restrict__ g2, uint8_t* __restrict__ bad, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool b = !pk_ok[i] || pk_inf[i] || !sig_ok[i] || sig_inf[i] || hm_inf[i];
  bad[i] = b ? 1 : 0;
  uint32_t* a1 = g1 + (size_t)2 * i * 24;
  uint32_t* a2 = g2 + (size_t)2 * i * 48;
  if (b) {
    for (int r = 0; r < 2; r++) {
      bls_copy(a1 + 24 * r, BasePoints::G1, 24);
      bls_copy(a2 + 48 * r, BasePoints::G2, 48);
    }
  } else if (scheme == 0) {
    bls_copy_neg(a1, pk + (size_t)i * 24, 12);
    bls_copy(a2, hm + (size_t)i * 48, 48);
    bls_copy(a1 + 24, BasePoints::G1, 24);
    bls_copy(a2 + 48, sig + (size_t)i * 48, 48);
  } else {
    bls_copy(a1, hm + (size_t)i * 24, 24);
    bls_copy_neg(a2, pk + (size_t)i * 48, 24);
    bls_copy(a1 + 24, sig + (size_t)i * 24, 24);
    bls_copy(a2 + 48, BasePoints::G2, 48);
  }
}
__global__ void __launch_bounds__(256) k_bls_verdict(const uint8_t* __restrict__ is_one, const uint8_t* __restrict__ bad,
                                                     uint8_t* __restrict__ out_ok, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out_ok[i] = (is_one[i] && !bad[i]) ? 1 : 0;
}
hipError_t bls_build_pairs(int scheme, const uint32_t* pk, const uint8_t* pk_ok, const uint8_t* pk_inf, const uint32_t* sig,
                           const uint8_t* sig_ok, const uint8_t* sig_inf, const uint32_t* hm, const uint8_t* hm_inf, uint32_t* g1,
                           uint32_t* g2, uint8_t* bad, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bls_pairs, dim3((n + 255) / 256), dim3(256), 0, st, scheme, pk, pk_ok, pk_inf, sig, sig_ok, sig_inf, hm, hm_inf, g1,
                     g2, bad, n);
  return hipGetLastError();
}
hipError_t bls_verdict(const uint8_t* is_one, const uint8_t* bad, uint8_t* out_ok, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bls_verdict, dim3((n + 255) / 256), dim3(256), 0, st, is_one, bad, out_ok, n);
  return hipGetLastError();
}

// ---- host twins (hosttest.hip): the same templates on the unpaired Fp2
void fp12_op_host(int op, const uint32_t* a, const uint32_t* b, void* out, int n, bool raw) {
  for (int i = 0; i < n; i++) {
    if (raw) fp12_op_lane<Fe29x2, true>(op, a, b, out, (size_t)i, true);
    else fp12_op_lane<Fe29x2>(op, a, b, out, (size_t)i, true);
  }
}
// returns -1, or the first refused pair with its PairingBad code in *bad_code (the outputs are then untouched)
int64_t pairing_host(const uint32_t* g1, const uint32_t* g2, int n, const uint32_t* off, int n_groups, int subgroup, uint32_t* out_gt,
                     uint8_t* out_is_one, uint32_t* bad_code) {
  using P = Pairing<Fe29x2>;
  using T = Tower<Fe29x2>;
  std::vector<T::E12> f((size_t)n);
  for (int i = 0; i < n; i++) {
    Fe29<2> Px, Py;
    T::E2 Qx, Qy;
    const uint32_t code = P::load_checked(g1 + (size_t)i * 24, g2 + (size_t)i * 48, subgroup != 0, Px, Py, Qx, Qy);
    if (code != PAIRING_OK) {
      *bad_code = code;
      return i;
    }
    P::miller_loop(f[i], Px, Py, Qx, Qy);
  }
  for (int g = 0; g < n_groups; g++) {
    T::E12 acc = T::E12::one(), r = T::E12::one();
    for (uint32_t i = off[g]; i < off[g + 1]; i++) T::mul(acc, acc, f[i]);
    if (off[g + 1] > off[g]) T::final_exponentiate(r, acc);
    if (out_gt) T::store_wire(out_gt + (size_t)g * FP12_WIRE_WORDS, r);
    out_is_one[g] = f12_is_one(r) ? 1 : 0;
  }
  return -1;
}

}  // namespace ncg
