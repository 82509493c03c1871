// Field-level self-check on the device (ncg_field_check): out[i] = op(a[i], b[i]) for the device-only code below whole
// operations - the inline-asm multiply-add chains, the bound-typed lazy limbs, the fused expressions, the ladder formulas and the
// bucket group law - so that the tests pin them directly, not only through point operations.  selfcheck.hpp lists the fields and
// their row widths; every family that also runs on the CPU is ONE lane function in a *_check.hpp header, called by the kernel
// here and by the host twin (hosttest.hip).  Built without NCG_MUL_INLINE and NCG_FE29_COLS_PAIRED (DESIGN.md section 2 names
// the product forms this reaches); fields 16 / 17 live in x25519.hip / ristretto.hip, which are built with the inlined multiply.
#include "curves.hpp"
#include "fp29.hpp"
#include "fe9_check.hpp"
#include "fe9m_check.hpp"
#include "fr29_check.hpp"
#include "group_check.hpp"
#include "msm_coop.hpp"
#include "secp_ladder_check.hpp"
#include "selfcheck.hpp"

namespace ncg {

// fields 0 / 1: fe9_check (fe9_check.hpp)
template <class PR>
__global__ void __launch_bounds__(64) k_field_check_fe9(int op, int variant, const uint32_t* __restrict__ a,
                                                        const uint32_t* __restrict__ b, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  (void)fe9_check<PR>(op, variant, a + (size_t)i * 9, b + (size_t)i * 9, out + (size_t)i * 8);
}
// field 2: bls12-381 Fe29 (canonical 12-word operands and results)
__global__ void __launch_bounds__(64) k_field_check_fe29(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe29<2> x = fe29_from_wire(a + (size_t)i * 12), y = fe29_from_wire(b + (size_t)i * 12);
  uint32_t* r = out + (size_t)i * 12;
  switch (op) {
    case 0: fe29_to_wire(r, x * y); break;
    case 1: fe29_to_wire(r, f_sqr(x)); break;
    case 2: fe29_to_wire(r, x + y); break;
    case 3: fe29_to_wire(r, x - y); break;
    case 4: fe29_to_wire(r, f_neg(x)); break;
    case 5: fe29_to_wire(r, f_inv(x)); break;
    default: break;
  }
}
// Fe29 / lane-paired Fp2 on RAW limb arrays at the TOP of their value bounds (the column bounds of the fused products -
// "56 product + 14 reduction terms below 2^64 only because limb 13 of a value below 2^12 p is at most 53256", fe29.hpp -
// are only exercised by operands that generic values never reach).  Inputs per item: a = [a, c], b = [b, d] (each
// element 14 words unpaired / 28 words paired: c0 then c1); ops: 0 a*b, 1 a^2, 6 a*b - c*d; output: canonical wire.
//   unpaired (field 3): a, c < 4096 p;  b, d < 4096 p (mul) / 2048 p (mulsub)
//   paired   (field 4): a, c < 4096 p;  b, d < 2048 p (mul) / 1024 p (mulsub);  a < 2048 p for the square
// These two exist on the device only (pair_odd, Fe29x2P).
template <int B>
__device__ __forceinline__ Fe29<B> fe29_raw(const uint32_t* p) {
  Fe29<B> r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.v[i] = p[i];
  return r;
}
__global__ void __launch_bounds__(64) k_field_check_fe29raw(int op, int variant, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                            uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *pa = a + (size_t)i * 28, *pb = b + (size_t)i * 28;
  uint32_t* r = out + (size_t)i * 12;
  switch (op) {
    case 0: fe29_to_wire(r, fe29_raw<4096>(pa) * fe29_raw<4096>(pb)); break;
    case 1: fe29_to_wire(r, f_sqr(fe29_raw<4096>(pa))); break;
    case 6: fe29_to_wire(r, f_mulsub(fe29_raw<4096>(pa), fe29_raw<2048>(pb), fe29_raw<4096>(pa + 14), fe29_raw<2048>(pb + 14))); break;
    case 7: {  // the zero test at the bounds the group law instantiates (group_check.hpp): variant = A, out[0] = the verdict
      const int z = fe29_eqz_check<Fe29>(variant, pa);
      if (z >= 0) r[0] = (uint32_t)z;
      break;
    }
    default: break;
  }
}
__global__ void __launch_bounds__(64) k_field_check_fe29x2p(int op, int variant, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                            uint32_t* __restrict__ out, int n) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // one Fp2 element per lane pair
  if (i >= n) return;
  const int h = pair_odd() ? 14 : 0;
  const uint32_t *pa = a + (size_t)i * 56 + h, *pb = b + (size_t)i * 56 + h;
  uint32_t* r = out + (size_t)i * 24 + (pair_odd() ? 12 : 0);
  switch (op) {
    case 0: fe29_to_wire(r, (Fe29x2P<4096>(fe29_raw<4096>(pa)) * Fe29x2P<2048>(fe29_raw<2048>(pb))).h); break;
    case 1: fe29_to_wire(r, f_sqr(Fe29x2P<2048>(fe29_raw<2048>(pa))).h); break;
    case 6:
      fe29_to_wire(r, f_mulsub(Fe29x2P<4096>(fe29_raw<4096>(pa)), Fe29x2P<1024>(fe29_raw<1024>(pb)),
                               Fe29x2P<4096>(fe29_raw<4096>(pa + 28)), Fe29x2P<1024>(fe29_raw<1024>(pb + 28))).h);
      break;
    case 7: {  // the pair's verdict on (c0, c1) = a[0..28), written once by the even lane
      const int z = fe29_eqz_check<Fe29x2P>(variant, pa);
      if (z >= 0 && !pair_odd()) out[(size_t)i * 24] = (uint32_t)z;
      break;
    }
    default: break;
  }
}
// fields 5 / 6: fe9_fused_check (fe9_check.hpp); per item a = [a, c], b = [b, d]
template <class PR>
__global__ void __launch_bounds__(64) k_field_check_fused(int op, int variant, const uint32_t* __restrict__ a,
                                                          const uint32_t* __restrict__ b, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *pa = a + (size_t)i * 18, *pb = b + (size_t)i * 18;
  (void)fe9_fused_check<PR>(op, variant, pa, pb, pa + 9, pb + 9, out + (size_t)i * 9);
}
// field 7: secp_ladder_check (secp_ladder_check.hpp); b = qx, qy.  One lane per item, so a wave mixes the generic path and the
// exceptional branch.
__global__ void __launch_bounds__(64) k_field_check_secp_ladder(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                                uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* pb = b + (size_t)i * 18;
  (void)secp_ladder_check(op, a + (size_t)i * 27, pb, pb + 9, out + (size_t)i * 27);
}
// fe9m.hpp (the bn254 base field, Montgomery radix 2^29) on RAW limbs: fe9m_check (fe9m_check.hpp, the host twin's code);
// a, b, out: 9 words per item.
__global__ void __launch_bounds__(64) k_field_check_fe9m(int op, int variant, const uint32_t* __restrict__ a,
                                                         const uint32_t* __restrict__ b, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t x[9], y[9], r[9];
  for (int j = 0; j < 9; j++) {
    x[j] = a[(size_t)i * 9 + j];
    y[j] = b[(size_t)i * 9 + j];
  }
  fe9m_check(op, variant, x, y, r);
  for (int j = 0; j < 9; j++) out[(size_t)i * 9 + j] = r[j];
}
// field 8: fr29_check (fr29_check.hpp), F by `variant`
template <class F>
__global__ void __launch_bounds__(64) k_field_check_fr29(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  (void)fr29_check<F>(op, a + (size_t)i * 9, b + (size_t)i * 9, out + (size_t)i * 9);
}
// The group law of the MSM buckets on STORED words (group_check.hpp: ops 0-3 through MsmGroup<C>::madd / add / dbl, one item
// per row: a lane, or a lane pair of the paired Fp2 form), and the four-lane form of msm_coop.hpp, which exists on the device
// only (ops 8-13, one GROUP of four items per row, the LDS arrangement of k_msm_reduce_level_coop).  a, b, out: ACC_WORDS per
// row.  A row index beyond n drops a whole item / a whole group: the pair exchange and the group broadcasts read their own lanes.
template <class C>
__global__ void __launch_bounds__(64) k_group_check(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                    uint32_t* __restrict__ out, int n) {
  constexpr int XW = MsmGroup<C>::ACC_WORDS;
  const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> LaneShift<C>::value);
  if (i >= n) return;
  group_check_op<C>(op, a + (size_t)i * XW, b + (size_t)i * XW, out + (size_t)i * XW);
}
//   op 8 add(a, b) -> out   9 out = a, then add(out, b) -> out   10 out = b, then add(a, out) -> out
//   op 11 dbl(a) -> out     12 out = a, then dbl(out) -> out     13 copy(a) -> out
#ifdef __HIP_DEVICE_COMPILE__
// between the copy of a row into `out` (global memory here, LDS in the MSM's tail) and the operation that reads it back through
// the other items of the group: the stores are complete before any lane of the wave loads
__device__ __forceinline__ void coop_inplace_sync() {
  __threadfence_block();
  coop_sync();
}
#endif
template <class C>
__global__ void __launch_bounds__(64) k_group_check_coop(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         uint32_t* out, int n) {
#ifdef __HIP_DEVICE_COMPILE__
  using K = CoopXyzz<C>;
  constexpr int XW = MsmGroup<C>::ACC_WORDS;
  extern __shared__ __attribute__((aligned(16))) uint32_t coop_lds[];
  uint32_t* lds = coop_lds + (size_t)K::group_in_block() * K::GROUP_WORDS;
  const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> (K::LS + 2));
  if (i >= n) return;
  const uint32_t *pa = a + (size_t)i * XW, *pb = b + (size_t)i * XW;
  uint32_t* o = out + (size_t)i * XW;
  switch (op) {
    case 8: K::add(lds, pa, pb, o); break;
    case 9:
      K::copy(pa, o);
      coop_inplace_sync();
      K::add(lds, o, pb, o);
      break;
    case 10:
      K::copy(pb, o);
      coop_inplace_sync();
      K::add(lds, pa, o, o);
      break;
    case 11: K::dbl(lds, pa, o); break;
    case 12:
      K::copy(pa, o);
      coop_inplace_sync();
      K::dbl(lds, o, o);
      break;
    case 13: K::copy(pa, o); break;
    default: break;
  }
#endif
}

// ---- launch: one launcher per row of SELFCHECK_FIELDS, blocks of one wave
#define SELFCHECK_ARGS const SelfCheckField &f, int op, int variant, const uint32_t *d_a, const uint32_t *d_b, uint32_t *d_out, int n, hipStream_t st
using SelfCheckLaunch = hipError_t (*)(SELFCHECK_ARGS);

static dim3 lane_grid(const SelfCheckField& f, int n) { return dim3((unsigned)(((size_t)n * f.lanes + 63) / 64)); }
template <auto K>  // a kernel that takes (op, variant, a, b, out, n)
static hipError_t launch_lanes_v(SELFCHECK_ARGS) {
  hipLaunchKernelGGL(K, lane_grid(f, n), dim3(64), 0, st, op, variant, d_a, d_b, d_out, n);
  return hipGetLastError();
}
template <auto K>  // a kernel that takes (op, a, b, out, n)
static hipError_t launch_lanes(SELFCHECK_ARGS) {
  hipLaunchKernelGGL(K, lane_grid(f, n), dim3(64), 0, st, op, d_a, d_b, d_out, n);
  return hipGetLastError();
}
static hipError_t launch_fr29(SELFCHECK_ARGS) {
  if (variant == 0) return launch_lanes<k_field_check_fr29<Fr29Bls>>(f, op, variant, d_a, d_b, d_out, n, st);
  if (variant == 1) return launch_lanes<k_field_check_fr29<Fr29Bn>>(f, op, variant, d_a, d_b, d_out, n, st);
  return hipSuccess;  // unknown variant: out stays zero
}
template <class C>
static hipError_t launch_group(SELFCHECK_ARGS) {
  constexpr int LS = LaneShift<C>::value;
  if (op >= 0 && op <= 3) return launch_lanes<k_group_check<C>>(f, op, variant, d_a, d_b, d_out, n, st);
  if constexpr (CoopOK<C>::value) {
    if (op < 8 || op > 13) return hipSuccess;
    constexpr int GROUPS = 64 >> (LS + 2);   // per block: one wave holds 16 groups (G1) / 8 (G2)
    const size_t lds_bytes = (size_t)GROUPS * COOP_SLOTS * MsmGroup<C>::FW * 4;
    hipLaunchKernelGGL(k_group_check_coop<C>, dim3((n + GROUPS - 1) / GROUPS), dim3(64), lds_bytes, st, op, d_a, d_b, d_out, n);
    return hipGetLastError();
  }
  return hipSuccess;  // any other op: out stays zero
}
static hipError_t launch_x25519(SELFCHECK_ARGS) { return x25519_field_check(op, variant, d_a, d_b, d_out, n, st); }  // x25519.hip
static hipError_t launch_ristretto(SELFCHECK_ARGS) { return ristretto_field_check(op, d_a, d_b, d_out, n, st); }     // ristretto.hip
#undef SELFCHECK_ARGS

struct SelfCheckLauncher {
  int field;
  SelfCheckLaunch launch;
};
static constexpr SelfCheckLauncher SELFCHECK_LAUNCHERS[] = {
    {0, launch_lanes_v<k_field_check_fe9<Fe9SecpPR>>},
    {1, launch_lanes_v<k_field_check_fe9<Fe9EdPR>>},
    {2, launch_lanes<k_field_check_fe29>},
    {3, launch_lanes_v<k_field_check_fe29raw>},
    {4, launch_lanes_v<k_field_check_fe29x2p>},
    {5, launch_lanes_v<k_field_check_fused<Fe9SecpPR>>},
    {6, launch_lanes_v<k_field_check_fused<Fe9EdPR>>},
    {7, launch_lanes<k_field_check_secp_ladder>},
    {8, launch_fr29},
    {9, launch_lanes_v<k_field_check_fe9m>},
    {10, launch_group<CurveSecp>},
    {11, launch_group<CurveEd>},
    {12, launch_group<CurveG1>},
    {13, launch_group<CurveG2P>},
    {14, launch_group<CurveBn254>},
    {16, launch_x25519},
    {17, launch_ristretto},
};
// the launchers stand in the order of the rows, and the rows of the MSM groups have the group's widths and lanes
constexpr bool selfcheck_rows_match() {
  if (sizeof(SELFCHECK_LAUNCHERS) / sizeof(SELFCHECK_LAUNCHERS[0]) != SELFCHECK_NFIELDS) return false;
  for (int i = 0; i < SELFCHECK_NFIELDS; i++)
    if (SELFCHECK_LAUNCHERS[i].field != SELFCHECK_FIELDS[i].field) return false;
  return true;
}
template <class C>
constexpr bool selfcheck_group_row(int field) {
  const SelfCheckField& f = *selfcheck_field(field);
  constexpr int XW = MsmGroup<C>::ACC_WORDS;
  return f.wa == XW && f.wb == XW && f.wo == XW && f.lanes == 1 << LaneShift<C>::value;
}
static_assert(selfcheck_rows_match(), "selfcheck.hpp and the launchers name different fields");
static_assert(selfcheck_group_row<CurveSecp>(10) && selfcheck_group_row<CurveEd>(11) && selfcheck_group_row<CurveG1>(12) &&
                  selfcheck_group_row<CurveG2P>(13) && selfcheck_group_row<CurveBn254>(14),
              "selfcheck.hpp: a group's row is not its stored accumulator");

hipError_t field_check_run(int field, int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n,
                           hipStream_t st) {
  if (n <= 0) return hipSuccess;
  for (int i = 0; i < SELFCHECK_NFIELDS; i++)
    if (SELFCHECK_FIELDS[i].field == field) return SELFCHECK_LAUNCHERS[i].launch(SELFCHECK_FIELDS[i], op, variant, d_a, d_b, d_out, n, st);
  return hipErrorInvalidValue;
}

}  // namespace ncg
