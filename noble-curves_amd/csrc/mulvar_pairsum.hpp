// secp256k1 batch multiply with ONE mixed addition per window: the two table entries a window adds, +-T[e1] and +-psi(T[e2]),
// are affine points at the same Z and their sum S_w does not depend on the running point, so it is formed as an affine point
// first and the window is  R <- 16 R,  R <- R + S_w  instead of two mixed additions (mulvar.hpp mul_var_lane).
//
// The affine sum needs 1 / H_w, H_w = beta x(T[e2]) - x(T[e1]).  Montgomery's trick turns the 31 inverses of an item (window 0
// is a pair sum already, ec_sw.hpp aff_add_neg_nx) into products and one inverse per item, and the same trick over 16 items into
// one inversion per 16 items.  Three kernels:
//   1. k_mul_var_pairsum_prepare: table build and rescale (mul_var_build_table), split and recoding as in mul_var_lane, then
//      the walk w = 31 .. 1:  pre_w = acc,  acc <- acc H_w.  Stores the table, the 31 prefixes, Zg and acc.
//   2. k_fe_batch_inverse (mulvar.hpp): acc -> 1 / acc, 16 items per lane, in place.
//   3. k_mul_var_gtab<C, W, MINW, true, 1> (the ladder): window 0 as before; for w = 1 .. 31 four doublings, then
//      iw = inv pre_w = 1 / H_w,  inv <- inv H_w,  S_w = (x3, y3) by the chord through the two entries, one jac_madd_neg_nx.
//
// Scratch, behind the Jacobian results (pairsum_words_per_item; mul_var_tmp_bytes accounts for it):
//   * per lane, item-major as k_mul_var_gtab's table (the ladder gathers entries by digit): the table, 144 words;
//   * per block of 64 lanes, limb-major and lane-minor, a column of 32 elements per lane: pre_1 .. pre_31 and Zg.  While the
//     table is built the column holds the entries that wait for the rescale and the Z ratios (mul_var_build_table STAGED),
//     then the rescaled x for the walk.  Every lane reads and writes its own column in the same order, so each access is one
//     coalesced row; item-major, every such access is 64 cache lines per instruction and the prepare kernel, which has no
//     ladder to hide them behind, was bound by them (profiles/r14_pairsum_ab.txt);
//   * acc / inv item-major in the Jacobian scratch, in the Z slot of the item's own result (free until the ladder lane stores
//     it, and read only by that lane).
//
// Exceptional cases.
//   * H_w = 0 means e1 P = +-lambda e2 P with e1, e2 <= 15: no point of the prime-order group satisfies it (the lattice
//     {(a, b): a + lambda b = 0 mod n} has no vector that short), so it occurs only for P = O or a degenerate table, which
//     are flagged anyway.  The prepare lane flags it, leaves it out of the product and stores the literal zero as acc; the
//     inverse kernel passes a zero through untouched and leaves it out of its products, and the ladder lane takes inv = 0 as
//     the flag and hands the lane to mul_var_slow.  One bad item does not poison its group of 16.
//   * R = +-S_w in the one addition of a window sets the flag as in mul_var_lane.  The state between the two additions of a
//     window no longer exists, so there are fewer such states: the scalars congruent to 0 (R = -S_w in the last window) and
//     +-lambda (R = -S_w there as well; the fix-up for the even k2 then starts from R = O) - tests/ladder_pairsum.py.
#pragma once
#include "mulvar.hpp"

namespace ncg {

// Items from which mul_var_secp_inline takes this path (below it: the single kernel k_mul_var_gtab<CurveSecpI, 4, 3, true>).
// The crossover on MI355X lies between 2^18 (4096 waves, one residency of the single kernel: this path 3 % slower) and 2^19
// (1 - 3 % faster); below 2^17 the four launches cost 0.05 ms against the two (profiles/r14_pairsum_ab.txt).
constexpr int PAIRSUM_MIN_N = 1 << 19;

template <class C, int W>
struct PairSumCfg {
  using Cfg = MulVarCfg<C, W>;
  static constexpr int FW = Cfg::FW, TS = Cfg::TS, M = Cfg::M;
  static constexpr int SLOT_WORDS = TS * 2 * FW;           // the table: 144 for secp256k1, W = 4
  static constexpr int ZG_OFF = (M - 1) * FW;              // in the column, behind the prefixes
  static constexpr int PRE_WORDS = M * FW;                 // the column of a lane; pre_w, limb l at ((w - 1) FW + l) * stride
  static constexpr int ACC_STRIDE = 3 * FW, ACC_OFF = 2 * FW;   // acc / inv of item i at jac[i * ACC_STRIDE + ACC_OFF]
};
template <class C, int W>
constexpr size_t pairsum_words_per_item() { return PairSumCfg<C, W>::SLOT_WORDS + PairSumCfg<C, W>::PRE_WORDS; }

// One window's pair of entries and the signs of their y, read off the two window registers (MSB first, as mul_var_lane).
struct PairSumDigits {
  int e1, e2;
  bool n1, n2;   // y1, y2 negated: the entry is subtracted
};
template <class WIN>
NCG_DI PairSumDigits pairsum_pop(WIN& w1, WIN& w2, bool neg1, bool neg2) {
  const int d1 = w1.pop(), d2 = w2.pop();
  return {((d1 < 0 ? -d1 : d1) - 1) >> 1, ((d2 < 0 ? -d2 : d2) - 1) >> 1, (d1 < 0) != neg1, (d2 < 0) != neg2};
}

// Split and recoding of mul_var_lane for the ladder with k1 odd.
template <class C, int W>
struct PairSumScalar {
  using Cfg = MulVarCfg<C, W>;
  SignedOddWindows<Cfg::NL, W, Cfg::M> w1, w2;
  bool neg1, neg2;
  NCG_DI void init(const uint32_t (&k)[8]) {
    GlvSplit gs = C::glv_split(k);
    secp_glv_make_k1_odd(gs);
    w1.template init<5>(gs.k1);
    w2.template init<5>(gs.k2);
    neg1 = gs.k1neg;
    neg2 = gs.k2neg;
  }
};

// Phase 1.  `slot`: SLOT_WORDS words of this lane; `pre`: its prefixes, consecutive words `stride` apart; `acc_out`: FW words.
// Returns the flag (also stored: acc = 0).
template <class C, int W>
NCG_DI bool pairsum_prepare_lane(const uint32_t* __restrict__ pt_wire, const uint32_t* __restrict__ k_wire,
                                 uint32_t* __restrict__ slot, uint32_t* __restrict__ pre, const int stride,
                                 uint32_t* __restrict__ acc_out) {
  using PS = PairSumCfg<C, W>;
  using F = typename C::F;
  using F1 = decltype(F::one() * F::one());   // a reduced product
  constexpr int FW = PS::FW, M = PS::M, TS = PS::TS;
  static_assert(OddK1Half<C>::value && FusedLadder<C>::value, "the pair-sum ladder is the fused GLV ladder with k1 odd");

  const Affine<F> P = load_affine_wire<F>(pt_wire);
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = k_wire[i];
  bool degenerate = false;
  // the entries wait for the rescale in the lane's column of the prefixes, which are written after it: coalesced rows instead of
  // one cache line per lane and access
  static_assert(TS * 3 * FW <= PS::PRE_WORDS, "the staged table and its Z ratios fit the prefixes' column");
  const F Zg = mul_var_build_table<C, W, true, true>(P, slot, 1, pre, stride, degenerate);

  PairSumScalar<C, W> sc;
  sc.init(k);
  // the ladder consumes the windows 1 .. 31 in that order and peels H_w off the inverse of the whole product as it goes, so
  // pre_w is the product of the H of the windows AFTER w: this walk takes the windows LSB first.  Window 0 needs no inverse.
  const auto beta = C::beta();
  // the TS x of the table in registers (the build leaves them in the column), an entry's picked by a chain of selects: gathered
  // from the table instead, two entries a window, the kernel took 1.78 ms against 1.22 ms (profiles/r14_pairsum_ab.txt)
  F xs[TS];
#pragma unroll
  for (int e = 0; e < TS; e++) xs[e] = FieldIO<F>::load_strided(pre + (size_t)e * 2 * FW * stride, stride);
  auto entry_x = [&](int e) -> F {
    F r = xs[0];
#pragma unroll
    for (int j = 1; j < TS; j++) {
#pragma unroll
      for (int i = 0; i < FW; i++) r.v[i] = e == j ? xs[j].v[i] : r.v[i];
    }
    return r;
  };
  FieldIO<F>::store_strided(pre + (size_t)PS::ZG_OFF * stride, stride, Zg);
  F1 acc = F::one();
#pragma unroll 1
  for (int w = M - 1; w >= 1; w--) {
    const int d1 = sc.w1.pop_low(), d2 = sc.w2.pop_low();
    const int e1 = ((d1 < 0 ? -d1 : d1) - 1) >> 1, e2 = ((d2 < 0 ? -d2 : d2) - 1) >> 1;
    const F x1 = entry_x(e1);
    const F x2 = entry_x(e2);
    const F1 H = f_mul_add(x2, beta, f_neg_lin(x1));
    FieldIO<F1>::store_strided(pre + (size_t)(w - 1) * FW * stride, stride, acc);
    if (f_eqz(H)) degenerate = true;
    else acc = acc * H;
  }
  if (degenerate) acc = F1::zero();
  FieldIO<F1>::store(acc_out, acc);
  return degenerate;
}

// Phase 3.  `inv_in`: 1 / acc of phase 1 (the literal zero: flagged).  Returns whether the lane went through mul_var_slow.
template <class C, int W>
NCG_DI bool pairsum_ladder_lane(const uint32_t* __restrict__ pt_wire, const uint32_t* __restrict__ k_wire,
                                uint32_t* __restrict__ out_jac, const uint32_t* __restrict__ slot,
                                const uint32_t* __restrict__ pre, const int stride, const uint32_t* __restrict__ inv_in) {
  using PS = PairSumCfg<C, W>;
  using F = typename C::F;
  using F1 = decltype(F::one() * F::one());
  constexpr int FW = PS::FW, M = PS::M;

  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = k_wire[i];
  // P = O: its wire form is the all-zero point, which the field load keeps literal
  const bool trivial_zero = load_affine_wire<F>(pt_wire).is_inf() || mp_is_zero<8>(k);
  F1 inv = FieldIO<F1>::load(inv_in);
  bool degenerate = inv.is_zero();
  PairSumScalar<C, W> sc;
  sc.init(k);
  const auto beta = C::beta();
  auto entry_x = [&](int e) -> F { return FieldIO<F>::load(slot + e * 2 * FW); };
  auto entry_y = [&](int e) -> F { return FieldIO<F>::load(slot + e * 2 * FW + FW); };

  // R holds -(running point) while `sg` is set (mul_var_lane): window 0 leaves it clear, the doublings of a window flip it
  // four times and its one addition once, so it alternates from window to window
  bool sg = false;
  Jac<F> R;
  {
    const PairSumDigits d = pairsum_pop(sc.w1, sc.w2, sc.neg1, sc.neg2);
    R = aff_add_neg_nx(entry_x(d.e1), f_cneg_lin(entry_y(d.e1), !d.n1), entry_x(d.e2), beta, f_cneg_lin(entry_y(d.e2), !d.n2),
                       degenerate);
  }
#pragma unroll 1
  for (int w = 1; w < M; w++) {
#pragma unroll 1
    for (int d = 0; d < W; d++) R = jac_dbl_neg(R);
    const PairSumDigits d = pairsum_pop(sc.w1, sc.w2, sc.neg1, sc.neg2);
    const F x1 = entry_x(d.e1), x2 = entry_x(d.e2);
    // S_w = (-1)^sg (+-T[e1] +- psi(T[e2])): the chord through (x1, y1) and (beta x2, y2), the signs on y1 and y2
    const auto y1 = f_cneg_lin(entry_y(d.e1), d.n1 != sg);
    const auto y2 = f_cneg_lin(entry_y(d.e2), d.n2 != sg);
    const F1 H = f_mul_add(x2, beta, f_neg_lin(x1));
    const F1 iw = inv * FieldIO<F1>::load_strided(pre + (size_t)(w - 1) * FW * stride, stride);
    inv = inv * H;
    const F1 lam = (y2 - y1) * iw;
    const F1 x3 = f_sqr_add(lam, f_neg_lin(H, x1));          // lam^2 - x1 - beta x2,  beta x2 = H + x1
    const F1 y3 = f_mul_add(lam, x1 - x3, f_neg_lin(y1));
    R = jac_madd_neg_nx(R, x3, y3, degenerate);
    sg = !sg;
  }
  // k2 even: it was recoded as |k2| + 1, take psi(P) back out (P is entry 0); `sg` flips in the lanes that add
  if (sc.w2.was_even) {
    R = jac_madd_neg_nx(R, entry_x(0) * beta, f_cneg_lin(entry_y(0), !sc.neg2 != sg), degenerate);
    sg = !sg;
  }
  const F Zg = FieldIO<F>::load_strided(pre + (size_t)PS::ZG_OFF * stride, stride);
  uint8_t inf_unused;
  return mul_var_finish<C, true>(R, Zg, sg, degenerate, trivial_zero, pt_wire, k_wire, out_jac, &inf_unused, true);
}

// ---- kernels: one lane per item, 64-thread blocks
template <class C, int W>
__global__ void __launch_bounds__(64)
k_mul_var_pairsum_prepare(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ scalars, uint32_t* __restrict__ jac,
                          uint32_t* __restrict__ gtab, uint32_t* __restrict__ pre, int n) {
  using PS = PairSumCfg<C, W>;
  constexpr int WW = PS::Cfg::WW;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= n) return;
  pairsum_prepare_lane<C, W>(pts + (size_t)idx * 2 * WW, scalars + (size_t)idx * 8, gtab + (size_t)idx * PS::SLOT_WORDS,
                             pre + (size_t)blockIdx.x * PS::PRE_WORDS * 64 + threadIdx.x, 64,
                             jac + (size_t)idx * PS::ACC_STRIDE + PS::ACC_OFF);
}

// The ladder: an overload of k_mul_var_gtab (its last parameter tells the two apart), so that it stays one of that family to
// whatever looks the dominant kernel of the multiply up by name.
template <class C, int W, int MINW, bool JAC_OUT, int PAIRSUM>
__global__ void __launch_bounds__(64, MINW)
k_mul_var_gtab(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ scalars, uint32_t* __restrict__ jac,
               const uint32_t* __restrict__ gtab, const uint32_t* __restrict__ pre, int n) {
  static_assert(JAC_OUT && PAIRSUM == 1, "the pair-sum ladder writes Jacobian results");
  using PS = PairSumCfg<C, W>;
  constexpr int WW = PS::Cfg::WW;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= n) return;
  uint32_t* out = jac + (size_t)idx * PS::ACC_STRIDE;
  pairsum_ladder_lane<C, W>(pts + (size_t)idx * 2 * WW, scalars + (size_t)idx * 8, out, gtab + (size_t)idx * PS::SLOT_WORDS,
                            pre + (size_t)blockIdx.x * PS::PRE_WORDS * 64 + threadIdx.x, 64, out + PS::ACC_OFF);
}

// Launcher; jac_tmp: pad64(n) * (3 FW + pairsum_words_per_item) words.
template <class C, int W, int MINW, int K>
inline hipError_t launch_mul_var_pairsum(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n,
                                         uint32_t* jac_tmp, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  using PS = PairSumCfg<C, W>;
  using F = typename C::F;
  static_assert(LaneShift<C>::value == 0, "one lane per item");
  uint32_t* gtab = jac_tmp + pad64(n) * 3 * PS::FW;
  uint32_t* pre = gtab + pad64(n) * PS::SLOT_WORDS;
  const unsigned blocks = (unsigned)(((size_t)n + 63) / 64);
  const unsigned kblocks = (unsigned)(((size_t)(n + K - 1) / K + 63) / 64);
  constexpr size_t pre_bytes = (size_t)K * FieldIO<F>::LANE_WORDS * 64 * 4;
  hipLaunchKernelGGL((k_mul_var_pairsum_prepare<C, W>), dim3(blocks), dim3(64), 0, st, pts, scalars, jac_tmp, gtab, pre, n);
  hipLaunchKernelGGL((k_fe_batch_inverse<C, K, true>), dim3(kblocks), dim3(64), pre_bytes, st, jac_tmp + PS::ACC_OFF,
                     (int)PS::ACC_STRIDE, n);
  hipLaunchKernelGGL((k_mul_var_gtab<C, W, MINW, true, 1>), dim3(blocks), dim3(64), 0, st, pts, scalars, jac_tmp,
                     (const uint32_t*)gtab, (const uint32_t*)pre, n);
  hipLaunchKernelGGL((k_jac_batch_affine<C, K, true>), dim3(kblocks), dim3(64), pre_bytes, st, jac_tmp, out, out_inf, n);
  return hipGetLastError();
}

}  // namespace ncg
