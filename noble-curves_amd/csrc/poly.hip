// Polynomial arithmetic over the bls12-381 and bn254 scalar fields on resident vectors: the layer the reference puts next to
// its FFT, poly(field, roots, ...) (src/abstract/fft.ts:583-926) - add / sub / dot (:789-806), scalar mul (:826-830), shift
// (:838-850), eval (:857-862), monomial.eval (:873-879), lagrange.basis (:882-901) and the FFT form of mul / convolve
// (:810-814, :832-837).  Elements are canonical residues (32 bytes LE, 16-byte aligned buffers) at both ends, as for the NTT;
// the field is a template parameter F (Fr29Bls / Fr29Bn), of which only F::M8 - the 8 x 32-bit Montgomery parameters - and
// the packed twiddle entries are used here.
//
// Arithmetic: every kernel of this file uses the 8 x 32-bit Montgomery form Fp<F::M8> of fp.hpp (R = 2^256, operands and
// results below r, no lazy bounds to track).  A canonical a times a Montgomery b R is the canonical a b, so data never has
// to be converted on load or store:
//   * add / sub work on the canonical residues themselves;
//   * dot is mont(mont(a, b), R^2) = a b (two products per element);
//   * scale / shift multiply a[i] by a Montgomery-form power of s (one product per element plus the power step);
//   * the sums accumulate mont(a, b) = a b / R and multiply the total by R^2 once;
//   * Horner keeps a canonical accumulator: acc = mont(acc, x R) + a[i].
// fr29.hpp would make a product about 30 % cheaper; the pointwise kernels move 64-96 bytes per one or two products and the
// reductions were not the bottleneck of any caller yet, so the simpler form was taken.
//
// Work assignment of the kernels with per-thread state (shift, sum, Horner, Lagrange): thread t of T owns the indices
// t, t + T, t + 2 T, ... - a run with stride T, so that the lanes of a wavefront read consecutive elements - and gets its start
// power s^t by square-and-multiply (poly_pow) and steps by s^T, which the host computes once per launch and passes as a
// kernel argument.  T = 256 * blocks with blocks = ceil(n / (256 * POLY_RUN)) capped at POLY_MAX_BLOCKS.
//
// Reductions: per-thread sum, wavefront reduction by shuffles, LDS across the four wavefronts, one partial per block into the
// workspace, then a second launch of one block per result.  No atomics; field addition is exact, so the order is immaterial.
#include <vector>

#include "fp.hpp"
#include "fr29.hpp"
#include "ntt_io.hpp"
#include "host_api.hpp"
#include "../../include/ncg.h"

namespace ncg {

constexpr int POLY_THREADS = 256;
constexpr int POLY_MAX_BLOCKS = 1024;   // partials per result in the workspace
constexpr int POLY_RUN = 8;             // elements per thread the strided kernels aim for before the block cap (shift, Horner)
// denominators inverted together by one poly_inv (about 380 products): 16 keeps the prefix products in 128 registers and brings
// the inversion's share to 24 products per element beside the 7 of the run itself
constexpr int POLY_LAG_RUN = 16;
constexpr uint32_t POLY_NO_ROOT = 0xFFFFFFFFu;
// workspace head: the root-index word of the Lagrange basis, then NCG_POLY_MAX_POINTS rows of POLY_MAX_BLOCKS partials
constexpr size_t POLY_WS_PARTIALS = 256;
constexpr size_t POLY_WS_HEAD = POLY_WS_PARTIALS + (size_t)NCG_POLY_MAX_POINTS * POLY_MAX_BLOCKS * 32;

size_t poly_ws_bytes(int log2n_mul) { return POLY_WS_HEAD + (log2n_mul >= 0 ? ((size_t)64 << log2n_mul) : 0); }

// a^e for a Montgomery-form a (0^0 = 1, as the reference's shift copies p[0])
template <class M8>
NCG_DI Fp<M8> poly_pow(Fp<M8> a, uint64_t e) {
  Fp<M8> r = Fp<M8>::one();
  while (e) {
    if (e & 1u) r = fp_mul<M8>(r, a);
    e >>= 1;
    if (e) a = fp_sqr<M8>(a);
  }
  return r;
}

// 1 / a = a^(r - 2) for a Montgomery-form a (0 -> 0), most significant bit first.  fp_inv forms r - 2 in the low word alone, and the low
// word of the bls12-381 r is 1; here the borrow is carried.
template <class M8>
NCG_DI Fp<M8> poly_inv(const Fp<M8>& a) {
  uint32_t e[8], bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) e[i] = __builtin_subc((uint32_t)M8::P[i], i == 0 ? 2u : 0u, bw, &bw);
  Fp<M8> r = Fp<M8>::one();
  bool started = false;
  for (int w = 7; w >= 0; w--) {
    for (int bit = 31; bit >= 0; bit--) {
      if (started) r = fp_sqr<M8>(r);
      if ((e[w] >> bit) & 1u) {
        r = started ? fp_mul<M8>(r, a) : a;
        started = true;
      }
    }
  }
  return r;
}

template <class M8>
NCG_DI Fp<M8> poly_pointwise_elem(int op, const Fp<M8>& a, const Fp<M8>& b) {
  if (op == NCG_POLY_ADD) return a + b;  // fft.ts:792
  if (op == NCG_POLY_SUB) return a - b;  // fft.ts:798
  return fp_mul<M8>(fp_mul<M8>(a, b), Fp<M8>::from_const(M8::R2));  // fft.ts:804
}

// out[i] = a[i] * s (powers = 0) or a[i] * s^i (powers = 1) over the indices of thread t; s_m = s R, sT_m = s^T R
template <class M8>
NCG_DI void poly_scale_run(const uint32_t* a, uint32_t* out, size_t n, size_t t, size_t T, int powers, const Fp<M8>& s_m,
                           const Fp<M8>& sT_m) {
  if (t >= n) return;
  Fp<M8> pw = powers ? poly_pow<M8>(s_m, t) : s_m;
  for (size_t i = t; i < n; i += T) {
    fr_store_g(out + i * 8, fp_mul<M8>(fr_load_g<Fp<M8>>(a + i * 8), pw));
    if (powers && i + T < n) pw = fp_mul<M8>(pw, sT_m);
  }
}

// sum of a[i] b[i] / R over the indices of thread t
template <class M8>
NCG_DI Fp<M8> poly_dot_run(const uint32_t* a, const uint32_t* b, size_t n, size_t t, size_t T) {
  Fp<M8> acc = Fp<M8>::zero();
  for (size_t i = t; i < n; i += T) acc = acc + fp_mul<M8>(fr_load_g<Fp<M8>>(a + i * 8), fr_load_g<Fp<M8>>(b + i * 8));
  return acc;
}

// the points of one monomial evaluation: x R and x^T R
template <class M8>
struct PolyPoints {
  Fp<M8> x[NCG_POLY_MAX_POINTS], xT[NCG_POLY_MAX_POINTS];
};
// acc[k] = sum over the indices i = t + j T of thread t of a[i] x_k^i (canonical): Horner in x_k^T over the run, highest index
// first (fft.ts:877), then times x_k^t
template <class M8, int M>
NCG_DI void poly_horner_run(const uint32_t* a, size_t n, size_t t, size_t T, const PolyPoints<M8>& pts, Fp<M8> (&acc)[M]) {
#pragma unroll
  for (int k = 0; k < M; k++) acc[k] = Fp<M8>::zero();
  if (t >= n) return;
  const size_t cnt = (n - t + T - 1) / T;
  for (size_t j = cnt; j-- > 0;) {
    const Fp<M8> av = fr_load_g<Fp<M8>>(a + (t + j * T) * 8);
#pragma unroll
    for (int k = 0; k < M; k++) acc[k] = fp_mul<M8>(acc[k], pts.xT[k]) + av;
  }
#pragma unroll
  for (int k = 0; k < M; k++) acc[k] = fp_mul<M8>(acc[k], poly_pow<M8>(pts.x[k], t));
}

// Lagrange basis over the table's roots: L_i(x) = c w_i / (x - w_i), c = (x^N - 1) / N canonical (fft.ts:894-899).
// Thread t owns i = t + j T, j < POLY_LAG_RUN (T * POLY_LAG_RUN >= N) and inverts its denominators with Montgomery's trick
// (the reference's invertBatch).  Table entries are w 2^261 (ntt.hip); k251 = 2^251 makes mont(entry, k251) = w R.
// A zero denominator - x is the root i - is replaced by 1 in the products and its index recorded in *root; c is then 0, so
// every output of the launch is 0 and poly_lagrange_fix writes the 1 of the reference's Kronecker shortcut (:889-893).
template <class M8>
NCG_DI Fp<M8> poly_lag_denominator(const uint32_t* tab, size_t idx, const Fp<M8>& x_m, const Fp<M8>& k251, Fp<M8>& w_m) {
  Fp<M8> e;
  fr29_to_words(e.v, ntt_load_tw(tab + idx * NTT_TW));
  w_m = fp_mul<M8>(e, k251);
  return x_m - w_m;
}
NCG_DI size_t poly_lag_index(size_t i, int log2n, int brp) {
  return brp && log2n ? (size_t)(ntt_brev32((uint32_t)i) >> (32 - log2n)) : i;
}
template <class M8>
NCG_DI void poly_lagrange_run(const uint32_t* tab, uint32_t* out, int log2n, int brp, size_t t, size_t T, const Fp<M8>& x_m,
                              const Fp<M8>& c, const Fp<M8>& k251, uint32_t* root) {
  const size_t N = (size_t)1 << log2n;
  if (t >= N) return;
  Fp<M8> pre[POLY_LAG_RUN], run = Fp<M8>::one(), w_m;
#pragma unroll
  for (int j = 0; j < POLY_LAG_RUN; j++) {
    const size_t i = t + (size_t)j * T;
    pre[j] = run;
    if (i < N) {
      const Fp<M8> d = poly_lag_denominator<M8>(tab, poly_lag_index(i, log2n, brp), x_m, k251, w_m);
      if (d.is_zero()) *root = (uint32_t)i;
      else run = fp_mul<M8>(run, d);
    }
  }
  Fp<M8> inv = poly_inv<M8>(run);
#pragma unroll
  for (int j = POLY_LAG_RUN - 1; j >= 0; j--) {
    const size_t i = t + (size_t)j * T;
    if (i < N) {
      const Fp<M8> d = poly_lag_denominator<M8>(tab, poly_lag_index(i, log2n, brp), x_m, k251, w_m);
      const Fp<M8> di = fp_mul<M8>(inv, pre[j]);  // 1 / d_j (Montgomery form)
      if (!d.is_zero()) inv = fp_mul<M8>(inv, d);
      fr_store_g(out + i * 8, fp_mul<M8>(c, fp_mul<M8>(w_m, di)));
    }
  }
}
template <class M8>
NCG_DI void poly_lagrange_fix(const uint32_t* root, uint32_t* out) {
  const uint32_t idx = *root;
  if (idx == POLY_NO_ROOT) return;
  Fp<M8> one = Fp<M8>::zero();
  one.v[0] = 1;
  fr_store_g(out + (size_t)idx * 8, one);
}

// what the host prepares per launch
template <class M8>
static Fp<M8> poly_host_mont(const uint32_t* wire) {
  Fp<M8> x;
  for (int i = 0; i < 8; i++) x.v[i] = wire[i];
  return fp_to_mont<M8>(x);
}
template <class M8>
static Fp<M8> poly_host_k251() {  // (1/2)^5 R = 2^251
  Fp<M8> h = Fp<M8>::from_const(M8::INV2), r = Fp<M8>::one();
  for (int i = 0; i < 5; i++) r = fp_mul<M8>(r, h);
  return r;
}
template <class M8>
static Fp<M8> poly_host_lagrange_c(const Fp<M8>& x_m, int log2n) {  // (x^N - 1) / N, canonical
  Fp<M8> tm = fp_sqr_n<M8>(x_m, log2n), h = Fp<M8>::from_const(M8::INV2), ninv = Fp<M8>::one();
  for (int i = 0; i < log2n; i++) ninv = fp_mul<M8>(ninv, h);
  return fp_from_mont<M8>(fp_mul<M8>(tm - Fp<M8>::one(), ninv));
}
static unsigned poly_blocks(size_t n, size_t per_thread, size_t cap) {
  const size_t per_block = (size_t)POLY_THREADS * per_thread;
  size_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  return (unsigned)(b > cap ? cap : b);
}

#ifdef __HIP_DEVICE_COMPILE__
// sum over the block, valid in thread 0; lds: 4 x 8 words, reusable after the call
template <class M8>
__device__ __forceinline__ Fp<M8> poly_block_sum(Fp<M8> v, uint32_t* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Fp<M8> o;
#pragma unroll
    for (int l = 0; l < 8; l++) o.v[l] = __shfl_down(v.v[l], off, 64);
    v = v + o;
  }
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int l = 0; l < 8; l++) lds[wave * 8 + l] = v.v[l];
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < POLY_THREADS / 64; w++) {
      Fp<M8> o;
#pragma unroll
      for (int l = 0; l < 8; l++) o.v[l] = lds[w * 8 + l];
      v = v + o;
    }
  }
  __syncthreads();
  return v;
}
#endif

template <class F>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, int op) {
  using E = Fp<typename F::M8>;
  const size_t T = (size_t)gridDim.x * POLY_THREADS;
  for (size_t i = (size_t)blockIdx.x * POLY_THREADS + threadIdx.x; i < n; i += T)
    fr_store_g(out + i * 8, poly_pointwise_elem<typename F::M8>(op, fr_load_g<E>(a + i * 8), fr_load_g<E>(b + i * 8)));
}
template <class F>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_scale(const uint32_t* a, uint32_t* out, size_t n, int powers, Fp<typename F::M8> s_m,
                                                             Fp<typename F::M8> sT_m) {
  poly_scale_run<typename F::M8>(a, out, n, (size_t)blockIdx.x * POLY_THREADS + threadIdx.x, (size_t)gridDim.x * POLY_THREADS, powers, s_m, sT_m);
}
template <class F>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_dot_partial(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                                   uint32_t* __restrict__ partials, size_t n) {
#ifdef __HIP_DEVICE_COMPILE__
  __shared__ uint32_t lds[POLY_THREADS / 64 * 8];
  using M8 = typename F::M8;
  Fp<M8> v = poly_dot_run<M8>(a, b, n, (size_t)blockIdx.x * POLY_THREADS + threadIdx.x, (size_t)gridDim.x * POLY_THREADS);
  v = poly_block_sum<M8>(v, lds);
  if (threadIdx.x == 0) fr_store_g(partials + (size_t)blockIdx.x * 8, v);
#endif
}
template <class F, int M>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_horner_partial(const uint32_t* __restrict__ a, uint32_t* __restrict__ partials, size_t n,
                                                                      PolyPoints<typename F::M8> pts) {
#ifdef __HIP_DEVICE_COMPILE__
  __shared__ uint32_t lds[POLY_THREADS / 64 * 8];
  using M8 = typename F::M8;
  Fp<M8> acc[M];
  poly_horner_run<M8, M>(a, n, (size_t)blockIdx.x * POLY_THREADS + threadIdx.x, (size_t)gridDim.x * POLY_THREADS, pts, acc);
#pragma unroll
  for (int k = 0; k < M; k++) {
    const Fp<M8> v = poly_block_sum<M8>(acc[k], lds);
    if (threadIdx.x == 0) fr_store_g(partials + ((size_t)k * POLY_MAX_BLOCKS + blockIdx.x) * 8, v);
  }
#endif
}
// one block per result: out[k] = sum of the `count` partials of row k, times R (from_div_r: the sums of poly_dot_run)
template <class F>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_sum_final(const uint32_t* __restrict__ partials, int count, int from_div_r,
                                                                 uint32_t* __restrict__ out) {
#ifdef __HIP_DEVICE_COMPILE__
  __shared__ uint32_t lds[POLY_THREADS / 64 * 8];
  using M8 = typename F::M8;
  const uint32_t* row = partials + (size_t)blockIdx.x * POLY_MAX_BLOCKS * 8;
  Fp<M8> v = Fp<M8>::zero();
  for (int j = (int)threadIdx.x; j < count; j += POLY_THREADS) v = v + fr_load_g<Fp<M8>>(row + (size_t)j * 8);
  v = poly_block_sum<M8>(v, lds);
  if (threadIdx.x == 0) {
    if (from_div_r) v = fp_mul<M8>(v, Fp<M8>::from_const(M8::R2));
    fr_store_g(out + (size_t)blockIdx.x * 8, v);
  }
#endif
}
template <class F>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_lagrange(const uint32_t* __restrict__ tab, uint32_t* __restrict__ out, int log2n, int brp,
                                                                Fp<typename F::M8> x_m, Fp<typename F::M8> c, Fp<typename F::M8> k251,
                                                                uint32_t* root) {
  poly_lagrange_run<typename F::M8>(tab, out, log2n, brp, (size_t)blockIdx.x * POLY_THREADS + threadIdx.x, (size_t)gridDim.x * POLY_THREADS, x_m, c,
                                    k251, root);
}
template <class F>
__global__ void k_poly_lagrange_fix(const uint32_t* root, uint32_t* out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) poly_lagrange_fix<typename F::M8>(root, out);
}
// ws[0, N) = a zero-extended, ws[N, 2 N) = b zero-extended
__global__ void __launch_bounds__(POLY_THREADS) k_poly_pad2(const uint32_t* __restrict__ a, size_t na, const uint32_t* __restrict__ b, size_t nb,
                                                            uint32_t* __restrict__ ws, size_t N) {
  const size_t T = (size_t)gridDim.x * POLY_THREADS;
  for (size_t i = (size_t)blockIdx.x * POLY_THREADS + threadIdx.x; i < 2 * N; i += T) {
    Fr v = Fr::zero();
    if (i < N) {
      if (i < na) v = fr_load_g(a + i * 8);
    } else if (i - N < nb) {
      v = fr_load_g(b + (i - N) * 8);
    }
    fr_store_g(ws + i * 8, v);
  }
}

#define POLY_FIELD(field, call_bn, call_bls) \
  do {                                       \
    if ((field) == NCG_FIELD_BN254_FR) {     \
      using F = Fr29Bn;                      \
      call_bn;                               \
    } else {                                 \
      using F = Fr29Bls;                     \
      call_bls;                              \
    }                                        \
  } while (0)

hipError_t poly_pointwise(int field, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, hipStream_t st) {
  const dim3 grid(poly_blocks(n, 1, 2048));
  POLY_FIELD(field, hipLaunchKernelGGL(k_poly_pointwise<F>, grid, dim3(POLY_THREADS), 0, st, a, b, out, n, op),
             hipLaunchKernelGGL(k_poly_pointwise<F>, grid, dim3(POLY_THREADS), 0, st, a, b, out, n, op));
  return hipGetLastError();
}

template <class F>
static void poly_scale_t(size_t n, const uint32_t* a, const uint32_t* s_host, int powers, uint32_t* out, hipStream_t st) {
  using M8 = typename F::M8;
  const unsigned blocks = powers ? poly_blocks(n, POLY_RUN, POLY_MAX_BLOCKS) : poly_blocks(n, 1, 2048);
  const Fp<M8> s_m = poly_host_mont<M8>(s_host);
  const Fp<M8> sT_m = powers ? poly_pow<M8>(s_m, (uint64_t)blocks * POLY_THREADS) : s_m;
  hipLaunchKernelGGL(k_poly_scale<F>, dim3(blocks), dim3(POLY_THREADS), 0, st, a, out, n, powers, s_m, sT_m);
}
hipError_t poly_scale(int field, size_t n, const uint32_t* a, const uint32_t* s_host, int powers, uint32_t* out, hipStream_t st) {
  POLY_FIELD(field, poly_scale_t<F>(n, a, s_host, powers, out, st), poly_scale_t<F>(n, a, s_host, powers, out, st));
  return hipGetLastError();
}

template <class F>
static void poly_eval_t(size_t n, const uint32_t* a, const uint32_t* basis, void* ws, uint32_t* out, hipStream_t st) {
  uint32_t* partials = (uint32_t*)((char*)ws + POLY_WS_PARTIALS);
  const unsigned blocks = poly_blocks(n, 1, POLY_MAX_BLOCKS);
  hipLaunchKernelGGL(k_poly_dot_partial<F>, dim3(blocks), dim3(POLY_THREADS), 0, st, a, basis, partials, n);
  hipLaunchKernelGGL(k_poly_sum_final<F>, dim3(1), dim3(POLY_THREADS), 0, st, partials, (int)blocks, 1, out);
}
hipError_t poly_eval(int field, size_t n, const uint32_t* a, const uint32_t* basis, void* ws, uint32_t* out, hipStream_t st) {
  POLY_FIELD(field, poly_eval_t<F>(n, a, basis, ws, out, st), poly_eval_t<F>(n, a, basis, ws, out, st));
  return hipGetLastError();
}

template <class F>
static PolyPoints<typename F::M8> poly_points(int m, const uint32_t* xs_host, uint64_t T) {
  using M8 = typename F::M8;
  PolyPoints<M8> pts;
  for (int k = 0; k < NCG_POLY_MAX_POINTS; k++) {
    pts.x[k] = k < m ? poly_host_mont<M8>(xs_host + 8 * k) : Fp<M8>::zero();
    pts.xT[k] = poly_pow<M8>(pts.x[k], T);
  }
  return pts;
}
template <class F, int M>
static void poly_horner_launch(unsigned blocks, hipStream_t st, const uint32_t* a, uint32_t* partials, size_t n,
                               const PolyPoints<typename F::M8>& pts) {
  hipLaunchKernelGGL((k_poly_horner_partial<F, M>), dim3(blocks), dim3(POLY_THREADS), 0, st, a, partials, n, pts);
}
template <class F>
static void poly_eval_monomial_t(size_t n, const uint32_t* a, int m, const uint32_t* xs_host, void* ws, uint32_t* out, hipStream_t st) {
  uint32_t* partials = (uint32_t*)((char*)ws + POLY_WS_PARTIALS);
  const unsigned blocks = poly_blocks(n, POLY_RUN, POLY_MAX_BLOCKS);
  const PolyPoints<typename F::M8> pts = poly_points<F>(m, xs_host, (uint64_t)blocks * POLY_THREADS);
  switch (m) {
    case 1: poly_horner_launch<F, 1>(blocks, st, a, partials, n, pts); break;
    case 2: poly_horner_launch<F, 2>(blocks, st, a, partials, n, pts); break;
    case 3: poly_horner_launch<F, 3>(blocks, st, a, partials, n, pts); break;
    case 4: poly_horner_launch<F, 4>(blocks, st, a, partials, n, pts); break;
    case 5: poly_horner_launch<F, 5>(blocks, st, a, partials, n, pts); break;
    case 6: poly_horner_launch<F, 6>(blocks, st, a, partials, n, pts); break;
    case 7: poly_horner_launch<F, 7>(blocks, st, a, partials, n, pts); break;
    default: poly_horner_launch<F, 8>(blocks, st, a, partials, n, pts); break;
  }
  hipLaunchKernelGGL(k_poly_sum_final<F>, dim3((unsigned)m), dim3(POLY_THREADS), 0, st, partials, (int)blocks, 0, out);
}
// m in 1..NCG_POLY_MAX_POINTS (the API layer has checked)
hipError_t poly_eval_monomial(int field, size_t n, const uint32_t* a, int m, const uint32_t* xs_host, void* ws, uint32_t* out, hipStream_t st) {
  POLY_FIELD(field, poly_eval_monomial_t<F>(n, a, m, xs_host, ws, out, st), poly_eval_monomial_t<F>(n, a, m, xs_host, ws, out, st));
  return hipGetLastError();
}

template <class F>
static hipError_t poly_lagrange_t(int log2n, const uint32_t* tab, const uint32_t* x_host, int brp, void* ws, uint32_t* out, hipStream_t st) {
  using M8 = typename F::M8;
  uint32_t* root = (uint32_t*)ws;
  const Fp<M8> x_m = poly_host_mont<M8>(x_host);
  const Fp<M8> c = poly_host_lagrange_c<M8>(x_m, log2n);
  hipError_t e = hipMemsetAsync(root, 0xFF, 4, st);  // POLY_NO_ROOT, every call
  if (e != hipSuccess) return e;
  const unsigned blocks = poly_blocks((size_t)1 << log2n, POLY_LAG_RUN, 0xFFFFFFFFu);
  hipLaunchKernelGGL(k_poly_lagrange<F>, dim3(blocks), dim3(POLY_THREADS), 0, st, tab, out, log2n, brp, x_m, c, poly_host_k251<M8>(), root);
  hipLaunchKernelGGL(k_poly_lagrange_fix<F>, dim3(1), dim3(64), 0, st, root, out);
  return hipGetLastError();
}
hipError_t poly_lagrange_basis(int field, int log2n, const uint32_t* tab, const uint32_t* x_host, int brp, void* ws, uint32_t* out,
                               hipStream_t st) {
  if (field == NCG_FIELD_BN254_FR) return poly_lagrange_t<Fr29Bn>(log2n, tab, x_host, brp, ws, out, st);
  return poly_lagrange_t<Fr29Bls>(log2n, tab, x_host, brp, ws, out, st);
}

// out = inverse(direct(a, brpOutput) .* direct(b, brpOutput), brpInput) (fft.ts:810-814) on the 2 N element buffer behind the
// workspace head; na, nb <= N.  a, b are consumed before out is written, so out may alias either.
hipError_t poly_mul(int field, int log2n, const uint32_t* tab, size_t na, const uint32_t* a, size_t nb, const uint32_t* b, void* ws,
                    uint32_t* out, hipStream_t st) {
  const size_t N = (size_t)1 << log2n;
  if (na == 0 || nb == 0) return hipMemsetAsync(out, 0, N * 32, st);
  uint32_t* buf = (uint32_t*)((char*)ws + POLY_WS_HEAD);
  hipLaunchKernelGGL(k_poly_pad2, dim3(poly_blocks(2 * N, 1, 2048)), dim3(POLY_THREADS), 0, st, a, na, b, nb, buf, N);
  hipError_t e = ntt_run(field, log2n, 2, buf, buf, nullptr, tab, log2n, NCG_NTT_BRP_OUTPUT, st);
  if (e != hipSuccess) return e;
  e = poly_pointwise(field, NCG_POLY_DOT, N, buf, buf + N * 8, buf, st);
  if (e != hipSuccess) return e;
  return ntt_run(field, log2n, 1, buf, out, nullptr, tab, log2n, NCG_NTT_INVERSE | NCG_NTT_BRP_INPUT, st);
}

// ---- host twin for the CPU unit tests (hosttest.hip): the same per-element and per-run functions, the T threads of a launch
// executed one after the other, the partial sums added in index order.  T = 0: the thread count the device would launch.
template <class F>
static int poly_host_t(int kind, int op, size_t n, const uint32_t* a, const uint32_t* b, int m, const uint32_t* small, size_t T, uint32_t* out) {
  using M8 = typename F::M8;
  using E = Fp<M8>;
  fr29_overflows() = 0;
  switch (kind) {
    case 0:  // pointwise
      for (size_t i = 0; i < n; i++) fr_store_g(out + i * 8, poly_pointwise_elem<M8>(op, fr_load_g<E>(a + i * 8), fr_load_g<E>(b + i * 8)));
      break;
    case 1: {  // scale (op = powers)
      if (!T) T = (size_t)POLY_THREADS * (op ? poly_blocks(n, POLY_RUN, POLY_MAX_BLOCKS) : poly_blocks(n, 1, 2048));
      const E s_m = poly_host_mont<M8>(small), sT_m = poly_pow<M8>(s_m, T);
      for (size_t t = 0; t < T; t++) poly_scale_run<M8>(a, out, n, t, T, op, s_m, sT_m);
      break;
    }
    case 2: {  // dot-sum
      if (!T) T = (size_t)POLY_THREADS * poly_blocks(n, 1, POLY_MAX_BLOCKS);
      E acc = E::zero();
      for (size_t t = 0; t < T; t++) acc = acc + poly_dot_run<M8>(a, b, n, t, T);
      fr_store_g(out, fp_mul<M8>(acc, E::from_const(M8::R2)));
      break;
    }
    case 3: {  // monomial evaluation at m points (the widest instantiation, unused points are 0)
      if (!T) T = (size_t)POLY_THREADS * poly_blocks(n, POLY_RUN, POLY_MAX_BLOCKS);
      const PolyPoints<M8> pts = poly_points<F>(m, small, T);
      E tot[NCG_POLY_MAX_POINTS], acc[NCG_POLY_MAX_POINTS];
      for (int k = 0; k < NCG_POLY_MAX_POINTS; k++) tot[k] = E::zero();
      for (size_t t = 0; t < T; t++) {
        poly_horner_run<M8, NCG_POLY_MAX_POINTS>(a, n, t, T, pts, acc);
        for (int k = 0; k < m; k++) tot[k] = tot[k] + acc[k];
      }
      for (int k = 0; k < m; k++) fr_store_g(out + (size_t)k * 8, tot[k]);
      break;
    }
    case 4: {  // s^e, e = n (the start power of a run)
      fr_store_g(out, fp_from_mont<M8>(poly_pow<M8>(poly_host_mont<M8>(small), (uint64_t)n)));
      break;
    }
    default: return -1;
  }
  return fr29_overflows();
}
int poly_host(int field, int kind, int op, size_t n, const uint32_t* a, const uint32_t* b, int m, const uint32_t* small, size_t T, uint32_t* out) {
  if (field == NCG_FIELD_BN254_FR) return poly_host_t<Fr29Bn>(kind, op, n, a, b, m, small, T, out);
  return poly_host_t<Fr29Bls>(kind, op, n, a, b, m, small, T, out);
}
// Lagrange basis on the table ntt_build_table would make for omega; root_out: the index word after the launch
template <class F>
static int poly_host_lagrange_t(int log2n, const uint32_t* omega_wire, const uint32_t* x_wire, int brp, size_t T, uint32_t* out, uint32_t* root_out) {
  using M8 = typename F::M8;
  using E = Fp<M8>;
  const size_t N = (size_t)1 << log2n;
  std::vector<uint32_t> tab((N + 1) * NTT_TW);
  const E w = poly_host_mont<M8>(omega_wire), k261 = E::from_const(F::K::K261);
  E acc = E::one();
  for (size_t k = 0; k < N; k++) {
    ntt_store_tw(tab.data() + k * NTT_TW, acc * k261);
    acc = acc * w;
  }
  fr29_overflows() = 0;
  if (!T) T = (size_t)POLY_THREADS * poly_blocks(N, POLY_LAG_RUN, 0xFFFFFFFFu);
  if (T * POLY_LAG_RUN < N) return -1;
  const E x_m = poly_host_mont<M8>(x_wire), c = poly_host_lagrange_c<M8>(x_m, log2n), k251 = poly_host_k251<M8>();
  uint32_t root = POLY_NO_ROOT;
  for (size_t t = 0; t < T; t++) poly_lagrange_run<M8>(tab.data(), out, log2n, brp, t, T, x_m, c, k251, &root);
  poly_lagrange_fix<M8>(&root, out);
  *root_out = root;
  return fr29_overflows();
}
int poly_host_lagrange(int field, int log2n, const uint32_t* omega_wire, const uint32_t* x_wire, int brp, size_t T, uint32_t* out,
                       uint32_t* root_out) {
  if (field == NCG_FIELD_BN254_FR) return poly_host_lagrange_t<Fr29Bn>(log2n, omega_wire, x_wire, brp, T, out, root_out);
  return poly_host_lagrange_t<Fr29Bls>(log2n, omega_wire, x_wire, brp, T, out, root_out);
}

}  // namespace ncg
