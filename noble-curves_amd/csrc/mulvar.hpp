// Batch variable-base scalar multiplication: out[i] = k[i] * P[i], one lane per pair.
//
// Replaces, for a whole batch, the reference's Point.multiplyUnsafe(k)
// (src/abstract/weierstrass.ts:915-928 -> pushWnafPair :660-671 -> mulAddUnsafe
// src/abstract/curve.ts:820-836 -> wnafWalk :479-498) and - for the value - Point.multiply(k)
// (weierstrass.ts:900-907), whose result is the same group element, Z=1-normalised.
//
// Why not the reference's wNAF walk: on a 64-lane wavefront a data-dependent "add when the
// digit is non-zero" executes the add for the whole wave at nearly every bit.  The ladder here
// is regular instead: signed-odd fixed windows of W bits (every digit odd and non-zero), so all
// lanes do W doublings + one mixed add per scalar per window.  secp256k1 uses the GLV split
// k = k1 + lambda*k2 (two 128-bit halves sharing the doubling chain, psi(P) = (beta*x, y)) exactly
// as the reference does; bls12-381 G1/G2 get no endomorphism (the reference has none there and
// inputs may lie outside the prime-order subgroup).
//
// The per-lane table of odd multiples [1,3,..,2^W-1]*P holds *affine* points of an isomorphic
// curve (shared-Z "effective affine" trick), so every table add is a mixed add.  It lives in
// device memory (k_mul_var_gtab: item-major, one contiguous 1-3 KB block per lane - no LDS
// footprint, so wide windows and 3-4 waves/SIMD go together; the default) or in LDS (k_mul_var:
// limb-major, lane-minor, bank-conflict free for any digit pattern; used when no scratch is given).
#pragma once
#include <type_traits>

#include "curves.hpp"
#include "scalar.hpp"

namespace ncg {

// One step of the table build T' = T + D (D = 2P) in co-Z form (Meloni's ZADDU): D and T share their Z, the sum comes out with
// Z' = Z (D.x - T.x) and D is RE-EXPRESSED at that Z' for free (W1, A1 are by-products), so the next step is co-Z again:
// 4M + 2S per table entry (a mixed Jacobian addition that also returns its Z ratio, the first form of this build, costs 8M + 3S:
// Z^2 and Z^3 products that co-Z operands do not need).  `zr` = D.x - T.x is the ratio Z' / Z; the running Z itself is not tracked
// here - the rescale pass of the table build multiplies the ratios up anyway.  With dx = D.x - T.x and dy = D.y - T.y:
// X3 = dy^2 - (D.x + T.x) dx^2, Y3 = dy (D.x dx^2 - X3) - D.y dx^3.
// The formula is incomplete: it is wrong when D = +-T (dx = 0), which happens while building [1,3,..]P exactly when P has small
// order (j*P = +-2P for some odd j < 2^W) - possible for any input the reference accepts on bls12-381 G1/G2 (cofactor > 1;
// Point.fromAffine does not subgroup-check, src/abstract/weierstrass.ts:710-718).  `degenerate` records that case; the caller
// then recomputes the lane with the complete ladder mul_var_slow below.
template <class F>
NCG_DI void coz_addu(Affine<F>& D, Affine<F>& T, F& zr, bool& degenerate) {
  auto dx = D.x - T.x;
  degenerate = degenerate || f_eqz(dx);
  auto C = f_sqr(dx);
  auto W1 = D.x * C;
  auto W2 = T.x * C;
  auto dy = D.y - T.y;
  auto A1 = D.y * (W1 - W2);
  auto X3 = f_sqr(dy) - W1 - W2;
  auto Y3 = dy * (W1 - X3) - A1;
  zr = dx * F::one();  // stored: bring the bound back under the storage bound
  D = {W1, A1};
  T = {X3, Y3};
}
template <class PR, int B>
NCG_DI void coz_addu(Affine<Fe9<PR, B>>& D, Affine<Fe9<PR, B>>& T, Fe9<PR, B>& zr, bool& degenerate) {
  auto dxw = D.x - T.x;
  degenerate = degenerate || f_eqz(dxw);
  auto dx = fe9_norm(dxw);
  auto dy = fe9_norm(D.y - T.y);
  auto C = f_sqr(dx);
  auto W1 = D.x * C;
  auto W2 = T.x * C;
  auto A1 = D.y * (W1 - W2);
  auto X3 = fe9_norm(f_sqr(dy) - W1 - W2);
  auto Y3 = dy * (W1 - X3) - A1;
  zr = dx;
  D = {W1, A1};
  T = {X3, Y3};
}

// Complete (every exceptional case handled by jac_madd / jac_dbl) MSB-first double-and-add over the
// whole 256-bit scalar: the value of the reference's multiplyUnsafe for ANY curve point
// (src/abstract/weierstrass.ts:915-928 on the complete formulas :793-880).  Only lanes whose
// window table degenerated (small-order P) come here, so its cost (256 dbl + ~128 madd) is
// irrelevant; P and k are re-read from memory so nothing stays live across the main ladder.
template <class C>
NCG_DI Jac<typename C::F> mul_var_slow(const uint32_t* __restrict__ pt_wire, const uint32_t* __restrict__ k_wire) {
  using F = typename C::F;
  const Affine<F> P = load_affine_wire<F>(pt_wire);
  Jac<F> R = Jac<F>::inf();
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = k_wire[w];
    for (int bit = 31; bit >= 0; bit--) {
      R = jac_dbl(R);
      if ((word >> bit) & 1u) R = jac_madd(R, P);
    }
  }
  return R;
}

// Curve traits of the ladder (absent = false).  ODD_HALVES: the GLV halves come out odd (secp_glv_make_odd), so there is no
// was_even fix-up at the end.  K1_ODD: k1 odd and both halves below 2^128 (secp_glv_make_k1_odd): a 128-bit window register and
// one was_even fix-up, for k2.  FUSED_LADDER: Fe9 ladder with the negated fused formulas jac_dbl_neg / jac_madd_neg_nx; it needs K1_ODD.
template <class C, class = void> struct OddGlvHalves { static constexpr bool value = false; };
template <class C> struct OddGlvHalves<C, std::void_t<decltype(C::ODD_HALVES)>> { static constexpr bool value = C::GLV && C::ODD_HALVES; };
template <class C, class = void> struct OddK1Half { static constexpr bool value = false; };
template <class C> struct OddK1Half<C, std::void_t<decltype(C::K1_ODD)>> { static constexpr bool value = C::GLV && C::K1_ODD; };
template <class C, class = void> struct FusedLadder { static constexpr bool value = false; };
template <class C> struct FusedLadder<C, std::void_t<decltype(C::FUSED_LADDER)>> { static constexpr bool value = C::FUSED_LADDER; };

template <class C, int W>
struct MulVarCfg {
  using F = typename C::F;
  static constexpr int FW = FieldIO<F>::WORDS;    // stored words per field element (HBM scratch)
  static constexpr int TW = FieldIO<F>::LANE_WORDS;  // words per field element in this lane's LDS table
  static constexpr int WW = FieldWire<F>::WORDS;  // wire words per field element (HBM in/out)
  static constexpr int TS = 1 << (W - 1);                 // table entries: 1,3,..,2^W-1
  static constexpr int KBITS = OddK1Half<C>::value ? 128 : C::GLV ? 129 : 257;   // bound on |k|+1 per stream
  static constexpr int M = (KBITS + W - 1) / W;           // windows
  static constexpr int NL = (KBITS + 31) / 32;            // limbs of the window register
  static constexpr int LDS_WORDS = TS * 2 * TW * 64;      // per 64-lane block
};

// The per-lane table of odd multiples [1, 3, .., 2^W - 1] P of mul_var_lane, built and brought to one Z; returns that Z (`Zg`:
// the table holds affine points of the curve isomorphic by it).  Entry e, word w at tab[(e*2*TW + w)*stride]; with ZR_IN_TAB the TS
// Z-ratios of the build sit behind the table while it runs and are dead afterwards.  `degenerate`: see coz_addu.
// STAGED: `stg` (same layout, words `sstride` apart) is where the entries wait for the rescale, which reads them there and writes
// `tab` - a place that is cheaper to write and read back than the table.  The rescaled x of every entry is left there as well.
template <class C, int W, bool ZR_IN_TAB, bool STAGED, class TABPTR, class STGPTR>
NCG_DI typename C::F mul_var_build_table(const Affine<typename C::F>& P, TABPTR tab, const int stride, STGPTR stg, const int sstride,
                                         bool& degenerate) {
  using Cfg = MulVarCfg<C, W>;
  using F = typename C::F;
  constexpr int TW = Cfg::TW, TS = Cfg::TS;
  Jac<F> D = jac_dbl(Jac<F>{P.x, P.y, F::one()});
  auto dz2 = f_sqr(D.Z);
  auto dz3 = dz2 * D.Z;
  Affine<F> Dc{D.X, D.Y};                 // 2P and P on the isomorphic curve, both at Z = 1: co-Z from the start
  Affine<F> T{P.x * dz2, P.y * dz3};
  F zr[ZR_IN_TAB ? 1 : TS];
  auto zr_put = [&](int j, const F& v) {
    if constexpr (ZR_IN_TAB) FieldIO<F>::store_strided(stg + (TS * 2 * TW + j * TW) * sstride, sstride, v);
    else zr[j] = v;
  };
  auto zr_get = [&](int j) -> F {
    if constexpr (ZR_IN_TAB) return FieldIO<F>::load_strided(stg + (TS * 2 * TW + j * TW) * sstride, sstride);
    else return zr[j];
  };
  FieldIO<F>::store_strided(stg, sstride, T.x);
  FieldIO<F>::store_strided(stg + TW * sstride, sstride, T.y);
  // with the Z-ratios in memory nothing here indexes a register array: keep the loops rolled (the
  // unrolled build is 15 mixed additions of straight-line code in front of the ladder)
#pragma unroll(ZR_IN_TAB ? 1 : TS)
  for (int j = 1; j < TS; j++) {
    F zj;
    coz_addu(Dc, T, zj, degenerate);
    zr_put(j, zj);
    FieldIO<F>::store_strided(stg + (j * 2 * TW) * sstride, sstride, T.x);
    FieldIO<F>::store_strided(stg + (j * 2 * TW + TW) * sstride, sstride, T.y);
    if (STAGED && j == TS - 1) {   // the last entry is at the table's Z already
      FieldIO<F>::store_strided(tab + (j * 2 * TW) * stride, stride, T.x);
      FieldIO<F>::store_strided(tab + (j * 2 * TW + TW) * stride, stride, T.y);
    }
  }
  // bring every entry to the last entry's Z
  F s = F::one();
#pragma unroll(ZR_IN_TAB ? 1 : TS)
  for (int j = TS - 2; j >= 0; j--) {
    if (j == TS - 2) s = zr_get(j + 1);
    else s = s * zr_get(j + 1);
    auto s2 = f_sqr(s);
    auto s3 = s2 * s;
    F x = FieldIO<F>::load_strided(stg + (j * 2 * TW) * sstride, sstride);
    F y = FieldIO<F>::load_strided(stg + (j * 2 * TW + TW) * sstride, sstride);
    const auto xs = x * s2;
    FieldIO<F>::store_strided(tab + (j * 2 * TW) * stride, stride, xs);
    if constexpr (STAGED) FieldIO<F>::store_strided(stg + (j * 2 * TW) * sstride, sstride, xs);
    FieldIO<F>::store_strided(tab + (j * 2 * TW + TW) * stride, stride, y * s3);
  }
  return D.Z * s;   // s = the product of all the ratios = the Z the last entry was built at
}
template <class C, int W, bool ZR_IN_TAB, class TABPTR>
NCG_DI typename C::F mul_var_build_table(const Affine<typename C::F>& P, TABPTR tab, const int stride, bool& degenerate) {
  return mul_var_build_table<C, W, ZR_IN_TAB, false>(P, tab, stride, tab, stride, degenerate);
}

// The end of a ladder lane: R on the isomorphic curve of the table (Z = Zg), negated when `negated` (the fused ladder's sign);
// back to the curve, flagged lanes redone by mul_var_slow, then the Jacobian (JAC_OUT) or affine result written.  Returns whether
// the lane went through mul_var_slow.
template <class C, bool JAC_OUT>
NCG_DI bool mul_var_finish(Jac<typename C::F> R, const typename C::F& Zg, bool negated, bool degenerate, bool trivial_zero,
                           const uint32_t* __restrict__ pt_wire, const uint32_t* __restrict__ k_wire,
                           uint32_t* __restrict__ out_wire, uint8_t* __restrict__ out_inf, bool active) {
  using F = typename C::F;
  constexpr int FW = FieldIO<F>::WORDS;
  if constexpr (FusedLadder<C>::value) {
    if (negated) R.Y = f_neg(R.Y);   // the one fix-up of the negated forms (f_neg keeps a literal zero literal)
    // a lane whose result is known beforehand (P = O, where the table build sets the flag, or k = 0, whose last addition is
    // R = -Q) must not send its wave through the complete ladder
    degenerate = degenerate && !trivial_zero;
  }
  // back from the isomorphic curve, then to affine (weierstrass.ts:951-969 toAffine)
  const bool ladder_inf = R.is_inf();  // tested before the product: not every field keeps 0 * Zg literal
  R.Z = R.Z * Zg;
  if (ladder_inf) R = Jac<F>::inf();
  if (degenerate) R = mul_var_slow<C>(pt_wire, k_wire);  // small-order P, or an exceptional addition in the fused ladder: complete ladder instead
  bool inf = trivial_zero || R.is_inf();
  if constexpr (JAC_OUT) {
    if (inf) R = Jac<F>::inf();
    if (active) {
      FieldIO<F>::store(out_wire, R.X);
      FieldIO<F>::store(out_wire + FW, R.Y);
      FieldIO<F>::store(out_wire + 2 * FW, R.Z);
    }
    return degenerate;
  }
  Affine<F> A = jac_to_affine(R, f_inv(R.Z));
  if (inf) A = {F::zero(), F::zero()};
  if (active) {
    store_affine_wire<F>(out_wire, A);
    *out_inf = inf ? 1 : 0;
  }
  return degenerate;
}

// Per-lane body.  `tab` is this lane's table base, consecutive words `stride` apart
// (LDS: lds + lane, stride 64;  host unit test: a plain array, stride 1).
// JAC_OUT: write the Jacobian result (X, Y, Z in storage format, Z = 0 for infinity) to
// `out_wire` (3*FW words) and leave the inversion to k_jac_batch_affine; otherwise invert here
// and write the affine wire point.
// ZR_IN_TAB: keep the TS Z-ratios of the table build behind the table (TS more elements per lane)
// instead of in registers - for tables in device memory, where space is free and registers are not.
template <class C, int W, bool JAC_OUT = false, bool ZR_IN_TAB = false, class TABPTR>
NCG_DI void mul_var_lane(const uint32_t* __restrict__ pt_wire, const uint32_t* __restrict__ k_wire,
                         uint32_t* __restrict__ out_wire, uint8_t* __restrict__ out_inf, bool active,
                         TABPTR tab, const int stride) {
  using Cfg = MulVarCfg<C, W>;
  using F = typename C::F;
  constexpr int TW = Cfg::TW, M = Cfg::M, NL = Cfg::NL;

  Affine<F> P = load_affine_wire<F>(pt_wire);
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = k_wire[i];
  const bool trivial_zero = P.is_inf() || mp_is_zero<8>(k);

  // ---- table of odd multiples on the isomorphic curve ------------------------------------
  bool degenerate = false;
  const F Zg = mul_var_build_table<C, W, ZR_IN_TAB>(P, tab, stride, degenerate);

  // ---- scalar recoding ---------------------------------------------------------------------
  SignedOddWindows<NL, W, M> w1, w2;
  bool neg1 = false, neg2 = false;
  constexpr bool ODD = OddGlvHalves<C>::value;
  constexpr bool K1ODD = OddK1Half<C>::value;
  if constexpr (C::GLV) {
    GlvSplit gs = C::glv_split(k);
    if constexpr (ODD) secp_glv_make_odd(gs);
    if constexpr (K1ODD) secp_glv_make_k1_odd(gs);
    w1.template init<5>(gs.k1);
    w2.template init<5>(gs.k2);
    neg1 = gs.k1neg;
    neg2 = gs.k2neg;
  } else {
    w1.template init<8>(k);
  }
  const auto beta = C::beta();

  // ---- ladder -------------------------------------------------------------------------------
  // FUSED: every doubling and addition returns the negated result, so R holds -(running point) while `sg` is set; an addition
  // of +-Q then adds the point with y negated once more when sg is set.  With W doublings and two additions per window the
  // sign is static per window position; it is fixed once after the loop.
  constexpr bool FUSED = FusedLadder<C>::value;
  static_assert(!FUSED || (C::GLV && OddK1Half<C>::value), "the fused ladder is the GLV ladder with k1 odd");
  bool sg = false;
  auto dbl = [&](const Jac<F>& r) -> Jac<F> {
    if constexpr (FUSED) {
      sg = !sg;
      return jac_dbl_neg(r);
    } else {
      return jac_dbl(r);
    }
  };
  // FUSED: the additions have no exceptional cases (ec_sw.hpp jac_madd_neg_nx).  A lane that meets one - R = +-Q, which random
  // scalars never do (tests/ladder32.py) - is flagged `degenerate`, goes on with garbage and is redone by mul_var_slow below.
  auto madd = [&](const Jac<F>& r, const auto& qx, const F& qy, bool ng) -> Jac<F> {
    if constexpr (FUSED) {
      const bool s = sg;
      sg = !sg;
      return jac_madd_neg_nx(r, qx, f_cneg_lin(qy, ng != s), degenerate);
    } else {
      return jac_madd_q(r, qx, f_cneg(qy, ng));
    }
  };
  Jac<F> R = Jac<F>::inf();
  if constexpr (FUSED) {
    // window 0 is ONE addition of two table entries, +-T[d1] + psi(+-T[d2]), both at Z = 1 (ec_sw.hpp aff_add_neg_nx: 4M + 2S
    // against the 8M + 3S of a mixed addition).  It returns the negated sum, so it is given the negated operands and `sg`
    // stays clear.  Every later window then starts with its doublings.
    const int d1 = w1.pop(), d2 = w2.pop();
    const int e1 = ((d1 < 0 ? -d1 : d1) - 1) >> 1, e2 = ((d2 < 0 ? -d2 : d2) - 1) >> 1;
    const F x1 = FieldIO<F>::load_strided(tab + (e1 * 2 * TW) * stride, stride);
    const F y1 = FieldIO<F>::load_strided(tab + (e1 * 2 * TW + TW) * stride, stride);
    const F x2 = FieldIO<F>::load_strided(tab + (e2 * 2 * TW) * stride, stride);
    const F y2 = FieldIO<F>::load_strided(tab + (e2 * 2 * TW + TW) * stride, stride);
    R = aff_add_neg_nx(x1, f_cneg_lin(y1, (d1 < 0) == neg1), x2, beta, f_cneg_lin(y2, (d2 < 0) == neg2), degenerate);
  }
  for (int i = FUSED ? 1 : 0; i < M; i++) {
    if (FUSED || i > 0) {
#pragma unroll(NCG_MUL_INLINE ? 1 : W)
      for (int d = 0; d < W; d++) R = dbl(R);
    }
    // one mixed addition per stream
    if constexpr (NCG_MUL_INLINE && C::GLV && !FUSED) {
      // field multiply inlined: the two additions of the GLV pair are ONE loop body run twice (the window body - 4
      // doublings through one rolled body + this - then fits the 64 KB instruction cache; as straight-line code it
      // was 69 KB and re-fetched every window)
#pragma unroll 1
      for (int e = 0; e < 2; e++) {
        const int d = e == 0 ? w1.pop() : w2.pop();
        const bool ng = e == 0 ? neg1 : neg2;
        const int idx = ((d < 0 ? -d : d) - 1) >> 1;
        F qx = FieldIO<F>::load_strided(tab + (idx * 2 * TW) * stride, stride);
        const F qy = FieldIO<F>::load_strided(tab + (idx * 2 * TW + TW) * stride, stride);
        if (e == 1) qx = qx * beta;
        R = madd(R, qx, qy, (d < 0) != ng);
      }
    } else {
      // (FUSED with the field multiply inlined comes here too: without an inlined doubling in its additions the pair fits as
      // straight-line code - a window body of 35 KB - so R is not moved back into place between the two and the beta product is
      // not behind a branch)
      {
        int d1 = w1.pop();
        int e = ((d1 < 0 ? -d1 : d1) - 1) >> 1;
        const F qx = FieldIO<F>::load_strided(tab + (e * 2 * TW) * stride, stride);
        const F qy = FieldIO<F>::load_strided(tab + (e * 2 * TW + TW) * stride, stride);
        R = madd(R, qx, qy, (d1 < 0) != neg1);
      }
      if constexpr (C::GLV) {
        int d2 = w2.pop();
        int e = ((d2 < 0 ? -d2 : d2) - 1) >> 1;
        const auto qx = FieldIO<F>::load_strided(tab + (e * 2 * TW) * stride, stride) * beta;
        const F qy = FieldIO<F>::load_strided(tab + (e * 2 * TW + TW) * stride, stride);
        R = madd(R, qx, qy, (d2 < 0) != neg2);
      }
    }
  }
  // even scalars were bumped by one: take the extra point back out (K1ODD: k1 is odd, only k2 can have been bumped; P is
  // entry 0 of the table and psi(P) = (beta x, y).  In the fused ladder `sg` then flips in the lanes that add: it is per lane.)
  if constexpr (!ODD) {
    const F qx = FieldIO<F>::load_strided(tab, stride);
    const F qy = FieldIO<F>::load_strided(tab + TW * stride, stride);
    if constexpr (!K1ODD) {
      if (w1.was_even) R = madd(R, qx, qy, !neg1);
    }
    if constexpr (C::GLV) {
      if (w2.was_even) R = madd(R, qx * beta, qy, !neg2);
    }
  }
  mul_var_finish<C, JAC_OUT>(R, Zg, FusedLadder<C>::value && sg, degenerate, trivial_zero, pt_wire, k_wire, out_wire, out_inf, active);
}

// Batched Jacobian -> affine (the reference's normalizeZ / FpInvertBatch, src/abstract/curve.ts:
// 311-326, src/abstract/modular.ts:728-760): each lane runs Montgomery's trick over K
// consecutive points - one field inversion per K points instead of one per point.
// PRE_LDS: the K prefix products live in LDS (64-thread blocks, limb-major, lane-minor) instead of a per-lane array.
// In the translation units that inline the field multiply the array is not promoted to registers and ends up in
// scratch memory (592 bytes per lane for secp256k1, K = 16) - global-memory round trips in a dependent chain, which cost
// this kernel 0.22 ms per 2^20 on most boxes and 0.42 ms on the boxes of the pool with a slow memory path.
// batch_inverse_lane is the lane routine: z(j) is element i0 + j (read twice), emit(j, zero, zi) takes its inverse; an element
// that is the literal zero is left out of the products and reported as `zero` (zi is then not meaningful), so one such element
// does not spoil the K - 1 around it.
template <class F, int K, bool PRE_LDS, class PREPTR, class LOADZ, class EMIT>
NCG_DI void batch_inverse_lane(PREPTR pre_lds, const int cnt, LOADZ z, EMIT emit) {
  constexpr int TW = FieldIO<F>::LANE_WORDS;
  F pre[PRE_LDS ? 1 : K];   // pre[j] = product of the non-zero elements 0..j-1
  auto pre_put = [&](int j, const F& v) {
    if constexpr (PRE_LDS) FieldIO<F>::store_strided(pre_lds + (size_t)j * TW * 64, 64, v);
    else pre[j] = v;
  };
  auto pre_get = [&](int j) -> F {
    if constexpr (PRE_LDS) return FieldIO<F>::load_strided(pre_lds + (size_t)j * TW * 64, 64);
    else return pre[j];
  };
  F acc = F::one();
#pragma unroll
  for (int j = 0; j < K; j++) {
    pre_put(j, acc);
    if (j < cnt) {
      F zj = z(j);
      if (!zj.is_zero()) acc = acc * zj;
    }
  }
  F inv = f_inv(acc);
#pragma unroll
  for (int j = K - 1; j >= 0; j--) {
    if (j < cnt) {
      F zj = z(j);
      const bool zero = zj.is_zero();
      F zi = F::zero();
      if (!zero) {
        zi = inv * pre_get(j);
        inv = inv * zj;
      }
      emit(j, zero, zi);
    }
  }
}

template <class C, int K, bool PRE_LDS = false>
__global__ void __launch_bounds__(PRE_LDS ? 64 : 256) k_jac_batch_affine(const uint32_t* __restrict__ jac,
                                                                         uint32_t* __restrict__ out_wire,
                                                                         uint8_t* __restrict__ out_inf, int n) {
  using F = typename C::F;
  constexpr int FW = FieldIO<F>::WORDS, WW = FieldWire<F>::WORDS;
  extern __shared__ __attribute__((aligned(16))) uint32_t pre_lds[];
  const int t = (blockIdx.x * blockDim.x + threadIdx.x) >> LaneShift<C>::value;
  const int i0 = t * K;
  if (i0 >= n) return;
  batch_inverse_lane<F, K, PRE_LDS>(
      pre_lds + threadIdx.x, n - i0, [&](int j) -> F { return FieldIO<F>::load(jac + ((size_t)(i0 + j) * 3 + 2) * FW); },
      [&](int j, bool inf, const F& zi) {
        const uint32_t* p = jac + (size_t)(i0 + j) * 3 * FW;
        Affine<F> A{F::zero(), F::zero()};
        if (!inf) {
          auto zi2 = f_sqr(zi);
          A = {FieldIO<F>::load(p) * zi2, FieldIO<F>::load(p + FW) * zi2 * zi};
        }
        store_affine_wire<F>(out_wire + (size_t)(i0 + j) * 2 * WW, A);
        out_inf[i0 + j] = inf ? 1 : 0;
      });
}

// The same over one field element per item, in place: vals[i * stride] <- its inverse, a literal zero left as it is.
template <class C, int K, bool PRE_LDS = false>
__global__ void __launch_bounds__(PRE_LDS ? 64 : 256) k_fe_batch_inverse(uint32_t* __restrict__ vals, int stride, int n) {
  using F = typename C::F;
  extern __shared__ __attribute__((aligned(16))) uint32_t pre_lds[];
  const int i0 = (blockIdx.x * blockDim.x + threadIdx.x) * K;
  if (i0 >= n) return;
  batch_inverse_lane<F, K, PRE_LDS>(
      pre_lds + threadIdx.x, n - i0, [&](int j) -> F { return FieldIO<F>::load(vals + (size_t)(i0 + j) * stride); },
      [&](int j, bool zero, const F& zi) {
        if (!zero) FieldIO<F>::store(vals + (size_t)(i0 + j) * stride, zi);
      });
}

// Batch normalisation of the reference's projective points (X, Y, Z) with x = X/Z, y = Y/Z -
// normalizeZ / toAffine(invZ) (src/abstract/curve.ts:311-326, src/abstract/weierstrass.ts:951-969,
// src/abstract/edwards.ts:595-609; the same map on Edwards (X, Y, Z, T)).  Wire input: X || Y || Z
// canonical residues; Z = 0 is the Weierstrass identity and comes out as (0, 0) with the flag
// set.  One inversion per K points (FpInvertBatch, src/abstract/modular.ts:728-760).
template <class F, int K>
__global__ void __launch_bounds__(256) k_proj_batch_affine(const uint32_t* __restrict__ proj_wire,
                                                           uint32_t* __restrict__ out_wire,
                                                           uint8_t* __restrict__ out_inf, int n) {
  constexpr int WW = FieldWire<F>::WORDS;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i0 = t * K;
  if (i0 >= n) return;
  F pre[K];
  F acc = F::one();
#pragma unroll
  for (int j = 0; j < K; j++) {
    pre[j] = acc;
    if (i0 + j < n) {
      F z = FieldWire<F>::load(proj_wire + ((size_t)(i0 + j) * 3 + 2) * WW);
      if (!f_eqz(z)) acc = acc * z;
    }
  }
  F inv = f_inv(acc);
#pragma unroll
  for (int j = K - 1; j >= 0; j--) {
    if (i0 + j < n) {
      const uint32_t* p = proj_wire + (size_t)(i0 + j) * 3 * WW;
      F z = FieldWire<F>::load(p + 2 * WW);
      const bool inf = f_eqz(z);
      F x = F::zero(), y = F::zero();
      if (!inf) {
        F zi = inv * pre[j];
        inv = inv * z;
        x = FieldWire<F>::load(p) * zi;
        y = FieldWire<F>::load(p + WW) * zi;
      }
      FieldWire<F>::store(out_wire + (size_t)(i0 + j) * 2 * WW, x);
      FieldWire<F>::store(out_wire + (size_t)(i0 + j) * 2 * WW + WW, y);
      out_inf[i0 + j] = inf ? 1 : 0;
    }
  }
}

// Variant with the per-lane table in device memory (item-major, each entry contiguous) instead of
// LDS: no LDS footprint, so the window width is no longer tied to occupancy.
template <class C, int W, int MINW, bool JAC_OUT>
__global__ void __launch_bounds__(64, MINW)
k_mul_var_gtab(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ scalars, uint32_t* __restrict__ out,
               uint8_t* __restrict__ out_inf, uint32_t* __restrict__ gtab, int n) {
  using Cfg = MulVarCfg<C, W>;
  constexpr int WW = Cfg::WW;
  constexpr int OUTW = JAC_OUT ? 3 * Cfg::FW : 2 * WW;
  const int lane_idx = blockIdx.x * 64 + threadIdx.x;  // table slot: one per LANE (a lane pair has two)
  const int idx = lane_idx >> LaneShift<C>::value;
  const bool active = idx < n;
  const int src = active ? idx : n - 1;
  mul_var_lane<C, W, JAC_OUT, true>(pts + (size_t)src * 2 * WW, scalars + (size_t)src * 8, out + (size_t)src * OUTW,
                                    out_inf + src, active, gtab + (size_t)lane_idx * (Cfg::TS * 3 * Cfg::TW), 1);
}

template <class C, int W, int MINW, bool JAC_OUT>
__global__ void __launch_bounds__(64, MINW)
k_mul_var(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ scalars,
          uint32_t* __restrict__ out, uint8_t* __restrict__ out_inf, int n) {
  constexpr int WW = MulVarCfg<C, W>::WW;
  constexpr int OUTW = JAC_OUT ? 3 * MulVarCfg<C, W>::FW : 2 * WW;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int lane = threadIdx.x;
  const int idx = (blockIdx.x * 64 + lane) >> LaneShift<C>::value;
  const bool active = idx < n;
  const int src = active ? idx : n - 1;  // idle lanes redo the last item, stores masked
  mul_var_lane<C, W, JAC_OUT>(pts + (size_t)src * 2 * WW, scalars + (size_t)src * 8, out + (size_t)src * OUTW,
                              out_inf + src, active, lds + lane, 64);
}

// ---- launchers shared by the translation units that instantiate these kernels (host side)
// Table in device memory (k_mul_var_gtab): the table lives behind the Jacobian scratch in `jac_tmp`
// (mul_var_tmp_bytes accounts for both).
template <class C, int W>
inline size_t gtab_words_per_item() { return (size_t)MulVarCfg<C, W>::TS * 3 * MulVarCfg<C, W>::TW; }
inline size_t pad64(size_t n) { return (n + 63) / 64 * 64; }

template <class C, int W, int MINW, int K = 8>
inline hipError_t launch_mul_var_gtab(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf,
                                      int n, uint32_t* jac_tmp, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  using Cfg = MulVarCfg<C, W>;
  constexpr int LS = LaneShift<C>::value;
  uint32_t* gtab = jac_tmp + pad64(n) * 3 * Cfg::FW;
  const unsigned blocks = (unsigned)((((size_t)n << LS) + 63) / 64);
  hipLaunchKernelGGL((k_mul_var_gtab<C, W, MINW, true>), dim3(blocks), dim3(64), 0, st, pts, scalars, jac_tmp, out_inf,
                     gtab, n);
  int threads = ((n + K - 1) / K) << LS;
  constexpr size_t pre_bytes = (size_t)K * FieldIO<typename C::F>::LANE_WORDS * 64 * 4;   // 36 KB for secp256k1, K = 16
  hipLaunchKernelGGL((k_jac_batch_affine<C, K, true>), dim3((threads + 63) / 64), dim3(64), pre_bytes, st, jac_tmp, out, out_inf, n);
  return hipGetLastError();
}

}  // namespace ncg
