// HOST-ONLY unit-test shim: runs the same __host__ __device__ templates the kernels use
// (field arithmetic, group law, GLV split, window recoding, per-lane ladders) on the CPU so
// their logic can be checked against the oracle without a GPU (`pytest -m "not gpu"`).
// Built into tests/_build/libncg_hosttest.so; never linked into libncg.so, never a fallback.
#include <vector>

#include "../../include/ncg.h"  // NCG_NTT_MAX_LOG2N
#include "mulvar_pairsum.hpp"
#include "ed25519.hip"  // single-TU inclusion: lane function + host table builder
#include "decode.hip"
#include "ntt.hip"
#include "poly.hip"
#include "h2c.hip"
#include "endo.hpp"
#include "ecdsa.hip"
#include "msm_shard.hpp"
#include "msm_endo.hip"  // msm_make_plan_endo
#include "msm_schedule.hpp"
#include "fe9_check.hpp"
#include "fe9m_check.hpp"
#include "fr29_check.hpp"
#include "group_check.hpp"
#include "secp_ladder_check.hpp"
#include "selfcheck.hpp"
#include "x25519.hip"
#include "ristretto.hip"
#include "pairing.hip"
#include "ed448.hip"
#include "decaf448.hip"
#include "ed25519_sign.hip"
#include "secp256k1_sign.hip"
#include "ed448_sign.hip"
#include "oprf.hip"
#include "h2c_suites.hip"
#include "h2c448.hip"

using namespace ncg;

template <class C, int W>
static void ht_mul_var_t(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n) {
  constexpr int FW = MulVarCfg<C, W>::FW, WW = MulVarCfg<C, W>::WW;
  std::vector<uint32_t> tab(MulVarCfg<C, W>::TS * 2 * FW);
  for (int i = 0; i < n; i++)
    mul_var_lane<C, W>(pts + (size_t)i * 2 * WW, scalars + (size_t)i * 8, out + (size_t)i * 2 * WW, out_inf + i, true,
                       tab.data(), 1);
}

// The pair-sum path of the secp256k1 batch multiply (mulvar_pairsum.hpp) with its four kernels' lane routines run in the
// kernels' order: prepare, inverse over groups of K, ladder, affine step over groups of K.  flags[i]: bit 0 the prepare lane's
// flag, bit 1 the lane went through mul_var_slow.  dbg (or null): of item 0 the slot, the prefixes, acc and 1 / acc.
template <class C, int W, int K>
static void ht_mul_var_pairsum_t(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, uint8_t* flags,
                                 uint32_t* dbg, int n) {
  using PS = PairSumCfg<C, W>;
  using F = typename C::F;
  constexpr int FW = PS::FW, WW = PS::Cfg::WW;
  std::vector<uint32_t> jac((size_t)n * 3 * FW), slots((size_t)n * PS::SLOT_WORDS), pre((size_t)n * PS::PRE_WORDS);
  auto acc = [&](int i) { return jac.data() + (size_t)i * PS::ACC_STRIDE + PS::ACC_OFF; };
  for (int i = 0; i < n; i++)
    flags[i] = pairsum_prepare_lane<C, W>(pts + (size_t)i * 2 * WW, scalars + (size_t)i * 8, slots.data() + (size_t)i * PS::SLOT_WORDS,
                                          pre.data() + (size_t)i * PS::PRE_WORDS, 1, acc(i)) ? 1 : 0;
  if (dbg && n > 0) {
    memcpy(dbg, slots.data(), PS::SLOT_WORDS * 4);
    memcpy(dbg + PS::SLOT_WORDS, pre.data(), PS::PRE_WORDS * 4);
    memcpy(dbg + PS::SLOT_WORDS + PS::PRE_WORDS, acc(0), FW * 4);
  }
  for (int i0 = 0; i0 < n; i0 += K)
    batch_inverse_lane<F, K, false>((uint32_t*)nullptr, n - i0, [&](int j) -> F { return FieldIO<F>::load(acc(i0 + j)); },
                                    [&](int j, bool zero, const F& zi) { if (!zero) FieldIO<F>::store(acc(i0 + j), zi); });
  if (dbg && n > 0) memcpy(dbg + PS::SLOT_WORDS + PS::PRE_WORDS + FW, acc(0), FW * 4);
  for (int i = 0; i < n; i++)
    if (pairsum_ladder_lane<C, W>(pts + (size_t)i * 2 * WW, scalars + (size_t)i * 8, jac.data() + (size_t)i * 3 * FW,
                                  slots.data() + (size_t)i * PS::SLOT_WORDS, pre.data() + (size_t)i * PS::PRE_WORDS, 1, acc(i)))
      flags[i] |= 2;
  for (int i0 = 0; i0 < n; i0 += K)
    batch_inverse_lane<F, K, false>(
        (uint32_t*)nullptr, n - i0, [&](int j) -> F { return FieldIO<F>::load(jac.data() + ((size_t)(i0 + j) * 3 + 2) * FW); },
        [&](int j, bool inf, const F& zi) {
          const uint32_t* p = jac.data() + (size_t)(i0 + j) * 3 * FW;
          Affine<F> A{F::zero(), F::zero()};
          if (!inf) {
            auto zi2 = f_sqr(zi);
            A = {FieldIO<F>::load(p) * zi2, FieldIO<F>::load(p + FW) * zi2 * zi};
          }
          store_affine_wire<F>(out + (size_t)(i0 + j) * 2 * WW, A);
          out_inf[i0 + j] = inf ? 1 : 0;
        });
}

template <class PR>
static void ht_field_t(int op, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  Fp<PR> x = fp_to_mont<PR>(fp_load<PR>(a)), y = fp_to_mont<PR>(fp_load<PR>(b)), z;
  switch (op) {
    case 0: z = x * y; break;
    case 1: z = fp_sqr<PR>(x); break;
    case 2: z = x + y; break;
    case 3: z = x - y; break;
    case 4: z = fp_neg<PR>(x); break;
    case 5: z = fp_inv<PR>(x); break;
    default: z = Fp<PR>::zero();
  }
  fp_store<PR>(r, fp_from_mont<PR>(z));
}

// ---- sharded MSM twin (tests/test_distributed_cpu.py): the per-shard grouped window sums computed naively with the
// group-law templates, then the REAL slot format, header check, partial-sum order and finish of comm.hip / msm_finish.hpp
template <class C>
static int ht_shard_local_t(int curve, int n_local, int n_max, const uint32_t* pts_wire, const uint32_t* scalars, uint8_t* slot, int mode,
                            int part, int nparts) {
  using G = MsmGroup<C>;
  constexpr int XW = G::ACC_WORDS;
  MsmPlan pl;
  if (msm_make_plan_impl(curve, n_max, 0, &pl) != 0) return -1;
  const int ng = msm_ngroups(pl.c);
  int w0 = 0, cnt = pl.nwin;
  if (mode != SHARD_POINTS) msm_shard_window_range(pl.nwin, part, nparts, &w0, &cnt);
  // SHARD_WINDOWS_SHARED (a precomputed set: every window adds into ONE bucket set, msm.hpp): the slot is one grouped-sum array
  const size_t fin_words = (size_t)ng * (mode == SHARD_WINDOWS_SHARED ? 1 : cnt) * XW;
  memset(slot, 0, msm_shard_slot_bytes(curve));
  FinHeader h{(uint32_t)pl.c, (uint32_t)pl.nwin, (uint32_t)fin_words, (uint32_t)curve, (uint32_t)w0, (uint32_t)cnt, (uint32_t)mode, SHARD_NO_BAD};
  uint32_t* fin = (uint32_t*)(slot + sizeof h);
  std::vector<typename G::Acc> win(pl.nwin, G::identity());
  std::vector<uint32_t> st(G::AFF_WORDS);
  const uint32_t mask = (1u << pl.c) - 1u;
  const int half = 1 << (pl.c - 1);
  for (int i = 0; i < n_local; i++) {
    {  // scalar >= group order: the smallest such index travels in the header (k_msm_digits)
      uint32_t bw = 0;
      for (int j = 0; j < 8; j++) (void)__builtin_subc(scalars[(size_t)i * 8 + j], pl.order[j], bw, &bw);
      if (bw == 0 && h.bad == SHARD_NO_BAD) h.bad = (uint32_t)i;
    }
    G::wire_to_storage(pts_wire + (size_t)i * G::WIRE_AFF, st.data());
    const typename G::Aff P = G::aff_load(st.data());
    uint32_t my[11];
    uint32_t cy = 0;
    for (int j = 0; j < 8; j++) my[j] = __builtin_addc(scalars[(size_t)i * 8 + j], pl.hconst[j], cy, &cy);
    my[8] = __builtin_addc(0u, pl.hconst[8], cy, &cy);
    my[9] = pl.hconst[9] + cy;
    my[10] = 0;
    for (int w = w0; w < w0 + cnt; w++) {
      const int bp = w * pl.c, limb = bp >> 5, sft = bp & 31;
      const uint64_t two = ((uint64_t)my[limb + 1] << 32) | my[limb];
      const int d = (int)((uint32_t)(two >> sft) & mask) - half;
      if (d == 0) continue;
      const unsigned a = (unsigned)(d < 0 ? -d : d);
      typename G::Acc t = G::identity();
      for (int bit = 15; bit >= 0; bit--) {
        t = G::dbl(t);
        if ((a >> bit) & 1u) t = G::madd(t, P, d < 0);
      }
      win[w] = G::add(win[w], t);
    }
  }
  memcpy(slot, &h, sizeof h);
  if (mode == SHARD_WINDOWS_SHARED) {  // what the shifted copies 2^(c w) P make of this rank's windows: V_0 = sum_w 2^(c w) W_w
    typename G::Acc tot = G::identity();
    for (int w = w0 + cnt - 1; w >= w0; w--) {
      typename G::Acc t = win[w];
      for (int b = 0; b < pl.c * w; b++) t = G::dbl(t);
      tot = G::add(tot, t);
    }
    G::acc_store(fin, tot);  // V_j, j >= 1: all-zero words, as below
    return 0;
  }
  for (int w = 0; w < cnt; w++) G::acc_store(fin + (size_t)w * XW, win[w0 + w]);  // V_0 = W_w; V_j = identity for j >= 1
  return 0;
}
// the host half of comm.hip's job_finish_host around a naive term-by-term sum: header check, the scalar verdict of all
// ranks, window assembly (SHARD_WINDOWS) or the sum of the slots (SHARD_POINTS), host Horner
template <class C>
static int ht_shard_combine_t(int curve, int n_max, int nparts, const uint8_t* slots, uint32_t* out, uint8_t* out_inf, char* err, int errlen) {
  using G = MsmGroup<C>;
  constexpr int XW = G::ACC_WORDS;
  MsmPlan pl;
  if (msm_make_plan_impl(curve, n_max, 0, &pl) != 0) return -1;
  const size_t stride = msm_shard_slot_bytes(curve);
  std::vector<FinHeader> hs(nparts);
  for (int r = 0; r < nparts; r++) memcpy(&hs[r], slots + stride * r, sizeof(FinHeader));
  const uint32_t mode = hs[0].mode;
  char msg[400];
  if (msm_shard_check(hs.data(), nparts, curve, pl, mode, msg, sizeof msg) >= 0) {
    if (err && errlen > 0) snprintf(err, errlen, "%s", msg);
    return 1;
  }
  uint32_t bad_idx = 0;
  const int bad_rank = msm_shard_first_bad(hs.data(), nparts, &bad_idx);
  if (bad_rank >= 0) {
    if (err && errlen > 0) snprintf(err, errlen, "noble-gpu: msm_sharded: invalid scalar at index %u of shard %d (not below the group order)", bad_idx, bad_rank);
    return 2;
  }
  const int fin_nwin = mode == SHARD_WINDOWS_SHARED ? 1 : pl.nwin;   // comm.hip job_finish_host: one window, no Horner across windows
  const size_t fin_words = (size_t)msm_ngroups(pl.c) * fin_nwin * XW;
  std::vector<uint32_t> sum(fin_words);
  if (mode == SHARD_WINDOWS) {
    msm_shard_assemble_windows(slots, stride, hs.data(), nparts, curve, pl, sum.data());
  } else {
    const size_t npoints = fin_words / XW;
    for (size_t t = 0; t < npoints; t++) {
      typename G::Acc acc = G::acc_load((const uint32_t*)(slots + sizeof(FinHeader)) + t * XW);
      for (int r = 1; r < nparts; r++) acc = G::add(acc, G::acc_load((const uint32_t*)(slots + stride * r + sizeof(FinHeader)) + t * XW));
      G::acc_store(sum.data() + t * XW, acc);
    }
  }
  msm_host_finish_any<C>(sum.data(), pl.c, fin_nwin, out, out_inf);
  return 0;
}
#define HT_CURVE_DISPATCH(curve, CALL)                \
  switch (curve) {                                    \
    case CURVE_SECP256K1: return CALL(CurveSecp);     \
    case CURVE_ED25519: return CALL(CurveEd);         \
    case CURVE_BLS12_381_G1: return CALL(CurveG1);    \
    case CURVE_BLS12_381_G2: return CALL(CurveG2);    \
    case CURVE_BN254_G1: return CALL(CurveBn254);     \
    default: return -1;                               \
  }

// inversion of n operands of 9 raw limbs at the bound A (1, 2 or 7): which = 0 f_inv (division steps, fe9_inv.hpp), 1 the kept Fermat
// chain; out: 8 canonical wire words per operand and, in raw[9 n] when given, the limbs f_inv returned
template <class PR, int A>
static void ht_fe9_inv_batch_t(int which, const uint32_t* a, uint32_t* out, uint32_t* raw, int n) {
  for (int k = 0; k < n; k++) {
    Fe9<PR, A> x;
    for (int i = 0; i < 9; i++) x.v[i] = a[(size_t)k * 9 + i];
    const Fe9<PR, 1> z = which ? f_inv_fermat(x) : f_inv(x);
    fe9_to_wire(out + (size_t)k * 8, z);
    if (raw)
      for (int i = 0; i < 9; i++) raw[(size_t)k * 9 + i] = z.v[i];
  }
}

extern "C" {

// fe9_check (fe9_check.hpp, the code of ncg_field_check fields 0 / 1): field 0 secp256k1 p, 1 ed25519 p; a, b: 9 raw limbs;
// r: 8 wire words; -1 for an unknown field or variant
int ht_fe9_op(int field, int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  if (field == 0) return fe9_check<Fe9SecpPR>(op, variant, a, b, r);
  if (field == 1) return fe9_check<Fe9EdPR>(op, variant, a, b, r);
  return -1;
}

int ht_fe9_inv_batch(int field, int A, int which, const uint32_t* a, uint32_t* out, uint32_t* raw, int n) {
  if (field < 0 || field > 1 || (A != 1 && A != 2 && A != 7)) return -1;
#define CALL(PR) (A == 1 ? ht_fe9_inv_batch_t<PR, 1>(which, a, out, raw, n) : A == 2 ? ht_fe9_inv_batch_t<PR, 2>(which, a, out, raw, n) : ht_fe9_inv_batch_t<PR, 7>(which, a, out, raw, n))
  if (field == 0) CALL(Fe9SecpPR);
  else CALL(Fe9EdPR);
#undef CALL
  return 0;
}

int ht_mul_var(int curve, const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n) {
  switch (curve) {
    case CURVE_SECP256K1: ht_mul_var_t<CurveSecp, 4>(pts, scalars, out, out_inf, n); return 0;
    case CURVE_BLS12_381_G1: ht_mul_var_t<CurveG1, 3>(pts, scalars, out, out_inf, n); return 0;
    case 12: ht_mul_var_t<CurveG1E, 4>(pts, scalars, out, out_inf, n); return 0;  // subgroup points only (GLV ladder)
    case 14: ht_mul_var_t<CurveSecpI, 4>(pts, scalars, out, out_inf, n); return 0;  // the fused-formula ladder of the inlined kernel
    case CURVE_BLS12_381_G2: ht_mul_var_t<CurveG2, 3>(pts, scalars, out, out_inf, n); return 0;
    case CURVE_BN254_G1: ht_mul_var_t<CurveBn254, 4>(pts, scalars, out, out_inf, n); return 0;
  }
  return -1;
}

// the pair-sum path of mul_var_secp_inline (mulvar_pairsum.hpp) on the CPU: see ht_mul_var_pairsum_t.  ht_pairsum_min_n: the
// item count from which the device takes that path; ht_pairsum_dbg_words: the size of `dbg`
int ht_mul_var_pairsum(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, uint8_t* flags, uint32_t* dbg, int n) {
  ht_mul_var_pairsum_t<CurveSecpI, 4, 16>(pts, scalars, out, out_inf, flags, dbg, n);
  return 0;
}
int ht_pairsum_min_n() { return PAIRSUM_MIN_N; }
int ht_pairsum_dbg_words() {
  using PS = PairSumCfg<CurveSecpI, 4>;
  return PS::SLOT_WORDS + PS::PRE_WORDS + 2 * PS::FW;
}

// field: 0 secp256k1 p, 1 ed25519 p, 2 bls12-381 p; canonical LE limbs in and out
int ht_field_op(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  switch (field) {
    case 0: ht_field_t<ParamsSecpP>(op, a, b, r); return 0;
    case 1: ht_field_t<ParamsEdP>(op, a, b, r); return 0;
    case 2: ht_field_t<ParamsBlsP>(op, a, b, r); return 0;
  }
  return -1;
}

// fe9_fused_check (fe9_check.hpp, the code of ncg_field_check fields 5 / 6): field 0 secp256k1 p, 1 ed25519 p; a, b, c, d, r:
// 9 raw limbs; -1 for an unknown field or variant
int ht_fe9_fused(int field, int op, int variant, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                 uint32_t* r) {
  if (field == 0) return fe9_fused_check<Fe9SecpPR>(op, variant, a, b, c, d, r);
  if (field == 1) return fe9_fused_check<Fe9EdPR>(op, variant, a, b, c, d, r);
  return -1;
}

// the pieces of the secp256k1 fused ladder on raw limbs: secp_ladder_check (secp_ladder_check.hpp, the code of ncg_field_check
// field 7).  ht_jac_neg: its ops 0 (the negated doubling of p) and 1 (the negated mixed addition of p and (qx, qy)); p 27 limbs
// X, Y, Z at the storage bound 2, qx at bound 2, qy at bound 3 (a negated table entry)
int ht_jac_neg(int op, const uint32_t* p, const uint32_t* qx, const uint32_t* qy, uint32_t* out) {
  if (op != 0 && op != 1) return -1;
  return secp_ladder_check(op, p, qx, qy, out);
}
// secp_glv_split followed by secp_glv_make_odd; layout of ht_glv_split
int ht_glv_split_odd(const uint32_t* k, uint32_t* out) { return secp_ladder_check(2, k, nullptr, nullptr, out); }
// secp_glv_split followed by secp_glv_make_k1_odd (the split of CurveSecpI's ladder); layout of ht_glv_split
int ht_glv_split_k1_odd(const uint32_t* k, uint32_t* out) { return secp_ladder_check(3, k, nullptr, nullptr, out); }

// the exception-free additions of the fused ladder (ec_sw.hpp) on the same raw limbs; out = X, Y, Z and the `degenerate` verdict
// (28 words).  op 0: jac_madd_neg_nx(P, qx, qy);  op 1: aff_add_neg_nx((P.X, P.Y), (beta qx, qy)) - P.Z is not read
int ht_jac_neg_nx(int op, const uint32_t* p, const uint32_t* qx, const uint32_t* qy, uint32_t* out) {
  const Jac<FeSecp> P = jac_load_limbs(p);
  const Fe9<Fe9SecpPR, 2> x = fe9_load_limbs<2>(qx);
  const Fe9<Fe9SecpPR, 3> y = fe9_load_limbs<3>(qy);
  Jac<FeSecp> R;
  bool degenerate = false;
  if (op == 0) R = jac_madd_neg_nx(P, x, y, degenerate);
  else if (op == 1) R = aff_add_neg_nx(P.X, Fe9<Fe9SecpPR, 3>(P.Y), x, CurveSecpI::beta(), y, degenerate);
  else return -1;
  jac_store_limbs(out, R);
  out[27] = degenerate ? 1u : 0u;
  return 0;
}

// GLV split of a 256-bit scalar: out = k1[5] k2[5] k1neg k2neg (12 words)
int ht_glv_split(const uint32_t* k, uint32_t* out) {
  glv_store(out, glv_split_words(k));
  return 0;
}

int ht_ed25519_mul_var(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n) {
  for (int i = 0; i < n; i++) ed25519_mul_var_host(pts + (size_t)i * 16, scalars + (size_t)i * 8, out + (size_t)i * 16, out_inf + i);
  return 0;
}

// X25519 on the CPU twins of x25519.hip: rows of 32 bytes (8 LE words); flags as ncg_x25519_batch.  ht_x25519_op: the pieces of
// ncg_field_check field 16 (a 36, b 9, out 36 words), -1 for an unknown op.
int ht_x25519(const uint32_t* scalars, const uint32_t* u, int flags, uint32_t* out, uint8_t* ok, int n) {
  if (flags & ~1) return -1;
  x25519_host(scalars, u, flags & 1, out, ok, n);
  return 0;
}
int ht_x25519_base(const uint32_t* scalars, uint32_t* out, uint8_t* ok, int n) {
  x25519_base_host(scalars, out, ok, n);
  return 0;
}
int ht_ed25519_to_montgomery(const uint32_t* pk, uint32_t* out, uint8_t* ok, int n) {
  ed25519_to_montgomery_host(pk, out, ok, n);
  return 0;
}
int ht_x25519_op(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out) { return x25519_check_host(op, variant, a, b, out); }

// Ed25519 signing on the CPU twins of ed25519_sign.hip.  Rows are 4-byte aligned: seeds 32 bytes, expanded keys 96 (scalar || prefix ||
// A), scalars and compressed points 8 LE words, signatures 64 bytes.  flags as ncg_ed25519_sign_batch (ONE_KEY has no meaning for one
// row and is refused); -1 for unknown flag bits or dom_len above the maximum.
static const uint32_t* ht_ed_scan_table() {
  static const std::vector<uint32_t> tab = [] {
    std::vector<uint32_t> t(ed25519_scan_table_words());
    ed25519_build_scan_table(t.data());
    return t;
  }();
  return tab.data();
}
int ht_ed25519_expand(const uint8_t* seeds, uint32_t* out_key96, int n) {
  ed25519_expand_host(ht_ed_scan_table(), seeds, out_key96, n);
  return 0;
}
int ht_ed25519_sign_with_r(const void* key, int flags, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg, uint64_t len, const uint32_t* r,
                           uint32_t* out_sig64, uint8_t* out_ok) {
  if ((flags & ~(NCG_ED25519_SIGN_EXPANDED | NCG_ED25519_SIGN_PREHASH)) || dom_len > NCG_ED25519_DOM_MAX) return -1;
  ed25519_sign_host(ht_ed_scan_table(), key, flags & NCG_ED25519_SIGN_EXPANDED, flags & NCG_ED25519_SIGN_PREHASH, dom, dom_len, msg, len, r,
                    out_sig64, out_ok);
  return 0;
}
int ht_ed25519_sign(const void* key, int flags, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg, uint64_t len, uint32_t* out_sig64,
                    uint8_t* out_ok) {
  return ht_ed25519_sign_with_r(key, flags, dom, dom_len, msg, len, nullptr, out_sig64, out_ok);
}
// out[i] = compress(scalars[i] B) by the uniform-scan walk
int ht_ed_mul_base_scan(const uint32_t* scalars, uint32_t* out, int n) {
  ed25519_mul_base_scan_host(ht_ed_scan_table(), scalars, out, n);
  return 0;
}
// SHA-512(dom || a32 || b32 || msg); a32 / b32 may be NULL (segment left out)
int ht_sha512_segments(const uint8_t* dom, uint32_t dom_len, const uint8_t* a32, const uint8_t* b32, const uint8_t* msg, uint64_t len,
                       uint8_t* out64) {
  sha512_segments_host(dom, dom_len, a32, b32, msg, len, out64);
  return 0;
}

// secp256k1 signing on the CPU twins of secp256k1_sign.hip.  Keys, hashes, extra entropy and aux rows are 32 big-endian bytes,
// signatures 64 bytes.  ht_secp_sign_op: one row of ncg_secp256k1_sign_check, -1 for an unknown op or variant; ht_secp_sign_widths: its
// words per row.  ht_ecdsa_sign: flags as ncg_ecdsa_sign_batch (ONE_KEY has no meaning for one row and is refused: -1); extra may be
// NULL; refuse_first > 0 refuses that many leading candidates of the DRBG.  pk_mode: 0 compressed, 1 uncompressed, 2 x-only.
static const uint32_t* ht_secp_scan_table() {
  static const std::vector<uint32_t> tab = [] {
    std::vector<uint32_t> t(secp_scan_table_words());
    secp_build_scan_table(t.data());
    return t;
  }();
  return tab.data();
}
int ht_secp_sign_op(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  return secp_sign_check_host(op, variant, ht_secp_scan_table(), a, b, out);
}
void ht_secp_sign_widths(int op, int* wa, int* wb, int* wo) { secp_sign_check_row_words(op, wa, wb, wo); }
int ht_secp_public_key(const uint8_t* sk, int pk_mode, uint8_t* out, uint8_t* ok, int n) {
  if (pk_mode < 0 || pk_mode > 2) return -1;
  secp_public_key_host(ht_secp_scan_table(), sk, pk_mode, out, ok, n);
  return 0;
}
int ht_ecdsa_sign(const uint8_t* sk, const uint8_t* hash, const uint8_t* extra, int flags, int refuse_first, uint8_t* out_sig64, uint8_t* out_recid,
                  uint8_t* out_ok) {
  if (flags & ~NCG_ECDSA_LOW_S) return -1;
  ecdsa_sign_host(ht_secp_scan_table(), sk, hash, extra, (flags & NCG_ECDSA_LOW_S) != 0, refuse_first, out_sig64, out_recid, out_ok);
  return 0;
}
int ht_schnorr_sign(const uint8_t* sk, const uint8_t* aux, const uint8_t* msg, uint64_t len, uint8_t* out_sig64, uint8_t* out_ok) {
  schnorr_sign_host(ht_secp_scan_table(), sk, aux, msg, len, out_sig64, out_ok);
  return 0;
}
// SHA-256(a || b || msg) through sha256_segments; a / b may be NULL (segment left out)
int ht_sha256_segments(const uint8_t* a, uint32_t a_len, const uint8_t* b, uint32_t b_len, const uint8_t* msg, uint64_t len, uint8_t* out32) {
  const Sha256Seg seg[3] = {{a, a ? a_len : 0u}, {b, b ? b_len : 0u}, {msg, len}};
  uint32_t h[8];
  sha256_segments<3>(h, seg);
  sha256_store_be(out32, h);
  return 0;
}

// X448 and Ed448 on the CPU twins of ed448.hip: 56-byte rows as 14 LE words, encodings 57 packed bytes, signatures 114, affine
// points 28 words; flags as ncg_x448_batch / ncg_ed448_mul_batch.  u = NULL / enc = NULL: the base point.  ht_fe448_op: one row of
// ncg_fe448_check, -1 for an unknown op; ht_fe448_widths: its words per row.
int ht_x448(const uint32_t* scalars, const uint32_t* u, int flags, uint32_t* out, uint8_t* ok, int n) {
  if (flags & ~1) return -1;
  x448_host(scalars, u, flags & 1, out, ok, n);
  return 0;
}
int ht_ed448_decode(const uint8_t* enc, uint32_t* out, uint8_t* ok, int n) {
  ed448_decode_host(enc, out, ok, n);
  return 0;
}
int ht_ed448_encode(const uint32_t* affine, uint8_t* out, int n) {
  ed448_encode_host(affine, out, n);
  return 0;
}
int ht_ed448_add_pairs(const uint32_t* a, const uint32_t* b, int subtract, uint32_t* out, int n) {
  ed448_add_pairs_host(a, b, subtract, out, n);
  return 0;
}
int ht_ed448_mul(const uint8_t* enc, const uint32_t* k, int flags, uint8_t* out, uint8_t* ok, int n) {
  if (flags & ~1) return -1;
  ed448_mul_host(enc, k, flags & 1, out, ok, n);
  return 0;
}
int ht_ed448_to_montgomery(const uint8_t* pk, uint32_t* out, uint8_t* ok, int n) {
  ed448_to_montgomery_host(pk, out, ok, n);
  return 0;
}
int ht_ed448_verify(const uint8_t* sig, const uint8_t* pk, const uint32_t* k, uint8_t* ok, int n) {
  ed448_verify_host(sig, pk, k, ok, n);
  return 0;
}
int ht_fe448_op(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out) { return fe448_check_host(op, variant, a, b, out); }
void ht_fe448_widths(int op, int* wa, int* wb, int* wo) { fe448_check_row_words(op, wa, wb, wo); }

// SHAKE256 and Ed448 signing on the CPU twins of ed448_sign.hip.  Seeds 57 bytes, expanded keys 172 (4-byte aligned: scalar || prefix
// || A || 2 zero bytes), scalars 14 LE words, signatures 114 bytes.  flags as ncg_ed448_sign_batch (ONE_KEY has no meaning for one row
// and is refused); -1 for unknown flag bits or dom_len above the maximum.  ht_ed448_sign_op: one row of ops 0-2 of
// ncg_ed448_sign_check, -1 for any other op; ht_ed448_sign_widths: the words per row of ops 0-3.
// SHAKE256(dom || a || b || msg, out_len); a / b may be NULL (segment left out)
int ht_shake256(const uint8_t* dom, uint32_t dom_len, const uint8_t* a, uint32_t a_len, const uint8_t* b, uint32_t b_len, const uint8_t* msg,
                uint64_t len, uint8_t* out, uint32_t out_len) {
  shake256_segments_host(dom, dom_len, a, a_len, b, b_len, msg, len, out, out_len);
  return 0;
}
int ht_ed448_sign_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) { return ed448_sign_check_host(op, a, b, out); }
void ht_ed448_sign_widths(int op, int* wa, int* wb, int* wo) { ed448_sign_check_row_words(op, wa, wb, wo); }
int ht_ed448_mod_n(const uint32_t* x29, uint32_t* out14, int n) {
  for (int i = 0; i < n; i++)
    if (ed448_sign_check_host(1, x29 + (size_t)i * 29, nullptr, out14 + (size_t)i * 14)) return -1;
  return 0;
}
int ht_ed448_muladd(const uint32_t* r, const uint32_t* k, const uint32_t* s, uint32_t* out14, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t a[28];
    for (int j = 0; j < 14; j++) {
      a[j] = r[(size_t)i * 14 + j];
      a[14 + j] = k[(size_t)i * 14 + j];
    }
    if (ed448_sign_check_host(2, a, s + (size_t)i * 14, out14 + (size_t)i * 14)) return -1;
  }
  return 0;
}
int ht_ed448_expand(const uint8_t* seeds, uint32_t* out_key172, int n) {
  ed448_expand_host(seeds, out_key172, n);
  return 0;
}
int ht_ed448_sign_with_r(const void* key, int flags, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg, uint64_t len, const uint32_t* r,
                         uint8_t* out_sig114, uint8_t* out_ok) {
  if ((flags & ~(NCG_ED448_SIGN_EXPANDED | NCG_ED448_PREHASH)) || dom_len > NCG_ED448_DOM_MAX) return -1;
  ed448_sign_host(key, flags & NCG_ED448_SIGN_EXPANDED, flags & NCG_ED448_PREHASH, dom, dom_len, msg, len, r, out_sig114, out_ok);
  return 0;
}
int ht_ed448_sign(const void* key, int flags, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg, uint64_t len, uint8_t* out_sig114,
                  uint8_t* out_ok) {
  return ht_ed448_sign_with_r(key, flags, dom, dom_len, msg, len, nullptr, out_sig114, out_ok);
}

// decaf448 on the CPU twins of decaf448.hip: encodings and scalars 14 LE words per row, Edwards representatives and uniform bytes
// 28; flags as ncg_decaf448_mul_batch, enc = NULL: the decaf base.  ht_decaf448_encode_proj: X Y Z as wire words (42 per row).
// ht_decaf448_op: one row of ncg_decaf448_check, -1 for an unknown op; ht_decaf448_widths: its words per row.
// ht_decaf448_consts: 1 - d, 1 - 2 d, sqrt(-d), 1 / sqrt(-d) and the base point x, y as the lane code holds them, 14 words each.
int ht_decaf448_decode(const uint32_t* enc, uint32_t* out, uint8_t* ok, int n) {
  decaf448_decode_host(enc, out, ok, n);
  return 0;
}
int ht_decaf448_encode(const uint32_t* affine, uint32_t* out, int n) {
  decaf448_encode_host(affine, out, n);
  return 0;
}
int ht_decaf448_encode_proj(const uint32_t* xyz, uint32_t* out, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t c[3][14], w[14];
    for (int j = 0; j < 3; j++)
      for (int l = 0; l < 14; l++) c[j][l] = xyz[(size_t)i * 42 + j * 14 + l];
    decaf_encode_proj(Ed448Pt{fe448_from_words(c[0]), fe448_from_words(c[1]), fe448_from_words(c[2])}, w);
    for (int l = 0; l < 14; l++) out[(size_t)i * 14 + l] = w[l];
  }
  return 0;
}
int ht_decaf448_equals(const uint32_t* a, const uint32_t* b, uint8_t* eq, int n) {
  decaf448_equals_host(a, b, eq, n);
  return 0;
}
int ht_decaf448_from_uniform(const uint32_t* uniform, uint32_t* out, int n) {
  decaf448_from_uniform_host(uniform, out, n);
  return 0;
}
int ht_decaf448_mul(const uint32_t* enc, const uint32_t* k, int flags, uint32_t* out, uint8_t* ok, int n) {
  if (flags & ~1) return -1;
  decaf448_mul_host(enc, k, flags & 1, out, ok, n);
  return 0;
}
int ht_decaf448_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) { return decaf448_check_host(op, a, b, out); }
void ht_decaf448_widths(int op, int* wa, int* wb, int* wo) { decaf448_check_row_words(op, wa, wb, wo); }
void ht_decaf448_consts(uint32_t* out) {
  const F448 c[6] = {DecafConsts::one_minus_d(), DecafConsts::one_minus_two_d(), DecafConsts::sqrt_minus_d(), DecafConsts::invsqrt_minus_d(),
                     decaf_base().X, decaf_base().Y};
  for (int j = 0; j < 6; j++) {
    uint32_t w[14];
    fe448_to_words(w, c[j]);
    for (int l = 0; l < 14; l++) out[j * 14 + l] = w[l];
  }
}

// ristretto255 on the CPU twins of ristretto.hip: encodings and scalars 8 LE words per row, Edwards representatives 16, uniform
// bytes 16; flags as ncg_ristretto_mul_batch.  ht_ristretto_encode_proj: X Y Z as wire words (24 per row).  ht_ristretto_op: the
// pieces of ncg_field_check field 17 (a 36, b 9, out 36 words), -1 for an unknown op.  ht_ristretto_consts: the four constants
// of src/ed25519.ts:410-424 as the lane code holds them, 8 wire words each (sqrt(ad - 1), 1 / sqrt(a - d), 1 - d^2, (d - 1)^2).
int ht_ristretto_decode(const uint32_t* enc, uint32_t* out_affine, uint8_t* ok, int n) {
  ristretto_decode_host(enc, out_affine, ok, 0, n);
  return 0;
}
int ht_ristretto_encode(const uint32_t* affine, uint32_t* out, int n) {
  ristretto_encode_host(affine, out, n);
  return 0;
}
int ht_ristretto_encode_proj(const uint32_t* proj_wire, uint32_t* out, int n) {
  ristretto_encode_proj_host(proj_wire, out, n);
  return 0;
}
int ht_ristretto_equals(const uint32_t* a, const uint32_t* b, uint8_t* eq, int n) {
  ristretto_equals_host(a, b, eq, n);
  return 0;
}
int ht_ristretto_from_uniform(const uint32_t* bytes64, uint32_t* out, uint32_t* out_affine, int n) {
  ristretto_from_uniform_host(bytes64, out, out_affine, n);
  return 0;
}
int ht_ristretto_mul(const uint32_t* enc, const uint32_t* scalars, int flags, uint32_t* out, uint8_t* ok, int n) {
  if (flags & ~1) return -1;
  ristretto_mul_host(enc, scalars, flags & 1, out, ok, n);
  return 0;
}
int ht_ristretto_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) { return ristretto_check_host(op, a, b, out); }
int ht_ristretto_consts(uint32_t* out32) {
  fe9_to_wire(out32, RistrettoConsts::sqrt_ad_minus_one());
  fe9_to_wire(out32 + 8, RistrettoConsts::invsqrt_a_minus_d());
  fe9_to_wire(out32 + 16, RistrettoConsts::one_minus_d_sq());
  fe9_to_wire(out32 + 24, RistrettoConsts::d_minus_one_sq());
  return 0;
}

// RFC 9380 for secp256k1 (suite 0) and edwards25519 (suite 1) on the CPU twins of h2c_suites.hip, one row per call: dst as the caller
// has it (1..255 bytes), count 1 or 2, u as count elements of 12 LE words, points as affine wire (16 words) and a ZERO flag; -1 for an
// argument outside these.  ht_h2c_check: the pieces of ncg_h2c_check (24 words in and out), -1 for an unknown op.
int ht_h2c_xmd_sha256(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out) {
  if (dst_len < 1 || dst_len > 255 || out_len < 1 || out_len > 256) return -1;
  h2c_xmd_sha256_host(msg, len, dst, dst_len, out_len, out);
  return 0;
}
int ht_h2c_hash_to_field(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out_u) {
  if (dst_len < 1 || dst_len > 255 || (count != 1 && count != 2)) return -1;
  return h2c_hash_to_field_host(suite, msg, len, dst, dst_len, count, out_u);
}
int ht_h2c_hash_to_scalar(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out8) {
  if (dst_len < 1 || dst_len > 255) return -1;
  return h2c_hash_to_scalar_host(suite, msg, len, dst, dst_len, out8);
}
int ht_h2c_map(int suite, const uint32_t* u, int count, uint32_t* out, uint8_t* inf) {
  if (count != 1 && count != 2) return -1;
  return h2c_map_host(suite, u, 12, count, out, inf);
}
int ht_h2c_hash(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out, uint8_t* inf) {
  if (dst_len < 1 || dst_len > 255 || (count != 1 && count != 2)) return -1;
  return h2c_hash_host(suite, msg, len, dst, dst_len, count, out, inf);
}
int ht_h2c_check(int op, const uint32_t* a, uint32_t* out) { return h2c_check_host(op, a, out); }

// RFC 9380 for edwards448 and the hash side of decaf448 on the CPU twins of h2c448.hip, one row per call: dst as the caller has it
// (1..255 bytes), count 1 or 2, elements, scalars and encodings 14 LE words, points x || y 28 words; -1 for an argument outside these.
// ht_h2c448_check: the pieces of ncg_h2c448_check (42 words in and out), -1 for an unknown op.
int ht_h2c448_xof(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out) {
  if (dst_len < 1 || dst_len > 255 || out_len < 1 || out_len > 65535) return -1;
  h2c448_xof_host(msg, len, dst, dst_len, out_len, out);
  return 0;
}
int ht_h2c448_hash_to_field(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out_u) {
  if (dst_len < 1 || dst_len > 255 || (count != 1 && count != 2)) return -1;
  h2c448_hash_to_field_host(msg, len, dst, dst_len, count, out_u);
  return 0;
}
int ht_h2c448_hash_to_scalar(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14) {
  if (dst_len < 1 || dst_len > 255) return -1;
  h2c448_hash_to_scalar_host(msg, len, dst, dst_len, out14);
  return 0;
}
int ht_h2c448_map(const uint32_t* u, int count, uint32_t* out28) {
  if (count != 1 && count != 2) return -1;
  h2c448_map_host(u, count, out28);
  return 0;
}
int ht_h2c448_hash(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out28) {
  if (dst_len < 1 || dst_len > 255 || (count != 1 && count != 2)) return -1;
  h2c448_hash_host(msg, len, dst, dst_len, count, out28);
  return 0;
}
int ht_h2c448_decaf_hash_to_group(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14) {
  if (dst_len < 1 || dst_len > 255) return -1;
  decaf448_hash_to_group_host(msg, len, dst, dst_len, out14);
  return 0;
}
int ht_h2c448_decaf_hash_to_scalar(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14) {
  if (dst_len < 1 || dst_len > 255) return -1;
  decaf448_hash_to_scalar_host(msg, len, dst, dst_len, out14);
  return 0;
}
int ht_h2c448_check(int op, const uint32_t* a, uint32_t* out) { return h2c448_check_host(op, a, out); }

// The ristretto255 OPRF on the CPU twins of oprf.hip, one row per call unless n is given: elements and scalars 8 LE words, outputs 64
// bytes, dst as the caller has it (1..255 bytes, -1 otherwise), flags as ncg_oprf_mul_batch without ONE_SCALAR.  The row functions
// return the row status.  ht_oprf_check: the pieces of ncg_oprf_check, -1 for an unknown op.  ht_oprf_proof: c || s of generateProof
// from M = the composite of C (the caller's MSM), with Z, t2 and t3 through the secret multiplies; ht_oprf_challenge: the challenge
// of the five encodings B M Z t2 t3.
int ht_oprf_xmd(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out) {
  if (dst_len < 1 || dst_len > 255 || out_len < 1 || out_len > 256) return -1;
  oprf_xmd_host(msg, len, dst, dst_len, out_len, out);
  return 0;
}
int ht_oprf_hash_to_group(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out, uint32_t* out_affine) {
  if (dst_len < 1 || dst_len > 255) return -1;
  oprf_hash_to_group_host(msg, len, dst, dst_len, out, out_affine);
  return 0;
}
int ht_oprf_hash_to_scalar(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out) {
  if (dst_len < 1 || dst_len > 255) return -1;
  oprf_hash_to_scalar_host(msg, len, dst, dst_len, out);
  return 0;
}
int ht_oprf_blind(int mode, const uint8_t* input, uint64_t len, const uint32_t* blind, uint32_t* out) { return oprf_blind_host(mode, input, len, blind, out); }
int ht_oprf_mul(const uint32_t* element, const uint32_t* scalar, int flags, uint32_t* out) {
  if (flags & ~NCG_OPRF_INVERT) return -1;
  return oprf_mul_host(element, scalar, (flags & NCG_OPRF_INVERT) != 0, out);
}
int ht_oprf_finalize(int mode, const uint8_t* input, uint64_t len, const uint8_t* info, uint32_t info_len, const uint32_t* blind,
                     const uint32_t* evaluated, uint8_t* out64) {
  return oprf_finalize_host(mode, input, len, info, info_len, blind, evaluated, out64);
}
int ht_oprf_evaluate(int mode, const uint8_t* input, uint64_t len, const uint8_t* info, uint32_t info_len, const uint32_t* scalar, int flags,
                     uint8_t* out64) {
  if (flags & ~NCG_OPRF_INVERT) return -1;
  return oprf_evaluate_host(mode, input, len, info, info_len, scalar, (flags & NCG_OPRF_INVERT) != 0, out64);
}
int ht_oprf_composite(int mode, const uint8_t* B32, const uint32_t* C, const uint32_t* D, uint32_t* out, uint8_t* status, int n) {
  oprf_composite_host(mode, B32, C, D, out, status, n);
  return 0;
}
int ht_oprf_challenge(int mode, const uint8_t* pts160, uint32_t* c) {
  oprf_challenge_host(mode, pts160, c);
  return 0;
}
int ht_oprf_proof(int mode, const uint32_t* k, const uint8_t* B32, const uint32_t* M, const uint32_t* r, uint32_t* out_proof16) {
  uint32_t kr[16], zt[24], pts[40];
  if (!oprf_scalar_ok_host(k, 0) || !oprf_scalar_ok_host(r, 0)) return -1;
  for (int i = 0; i < 8; i++) kr[i] = k[i], kr[8 + i] = r[i];
  oprf_proof_points_host(ht_ed_scan_table(), M, kr, zt);
  memcpy(pts, B32, 32);
  memcpy(pts + 8, M, 32);
  memcpy(pts + 16, zt, 32);
  memcpy(pts + 24, zt + 16, 32);
  memcpy(pts + 32, zt + 8, 32);
  oprf_challenge_host(mode, (const uint8_t*)pts, out_proof16);
  oprf_proof_s_host(out_proof16, k, r, out_proof16 + 8);
  return 0;
}
int ht_oprf_check(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out) { return oprf_check_host(op, variant, a, b, out); }

// Fp2 square root lane: in = c0 c1 wire (24 words); out = root wire; returns 1 if a root exists
int ht_fp2_sqrt(const uint32_t* in, uint32_t* out) {
  Fe29x2<2> a{fe29_from_wire(in), fe29_from_wire(in + 12)}, r;
  bool ok = fe29x2_sqrt(a, r);
  fe29_to_wire(out, r.c0);
  fe29_to_wire(out + 12, r.c1);
  return ok ? 1 : 0;
}

int ht_decode_points(int curve, const uint8_t* in, int flags, uint32_t* out, uint8_t* ok, uint8_t* inf, int n) {
  decode_points_host(curve, in, flags, out, ok, inf, n);
  return 0;
}

int ht_encode_points(int curve, const uint32_t* in, uint8_t* out, uint8_t* ok, int n) {
  encode_points_host(curve, in, out, ok, n);
  return 0;
}

int ht_map_to_curve(int curve, const uint32_t* u, int count, uint32_t* out, uint8_t* inf, int n) {
  map_to_curve_host(curve, u, count, out, inf, n);
  return 0;
}

// NTT over Fr on the CPU through the device field code (butterflies + table walk of ntt.hip)
int ht_ntt(int n, const uint32_t* omega, const uint32_t* in, uint32_t* out, int flags) {
  return ntt_host(NCG_FIELD_BLS12_381_FR, n, omega, in, out, flags);  // number of column / limb overflows seen by the host checks
}
// the same with smaller passes (first pass of at most t0max stages, the others of at most tmax)
int ht_ntt_small_passes(int n, const uint32_t* omega, const uint32_t* in, uint32_t* out, int flags, int t0max, int tmax) {
  if (t0max < 1 || tmax < 1 || 1 + (n - (n < t0max ? n : t0max) + tmax - 1) / tmax > 8) return -1;
  return ntt_host(NCG_FIELD_BLS12_381_FR, n, omega, in, out, flags, t0max, tmax);
}
// the two above for either field of ncg_ntt (NCG_FIELD_BLS12_381_FR, NCG_FIELD_BN254_FR); t0max = tmax = 0: the device's pass limits
int ht_ntt_field(int field, int n, const uint32_t* omega, const uint32_t* in, uint32_t* out, int flags, int t0max, int tmax) {
  if (field != NCG_FIELD_BLS12_381_FR && field != NCG_FIELD_BN254_FR) return -1;
  if (t0max == 0 && tmax == 0) return ntt_host(field, n, omega, in, out, flags);
  if (t0max < 1 || tmax < 1 || 1 + (n - (n < t0max ? n : t0max) + tmax - 1) / tmax > 8) return -1;
  return ntt_host(field, n, omega, in, out, flags, t0max, tmax);
}
// fr29.hpp on RAW limbs (9 words each): fr29_check (fr29_check.hpp, the code of ncg_field_check field 8), `variant` numbered
// as there: 0 bls12-381 Fr, 1 bn254 Fr.  op 0: mont(a, b) -> 9 limbs; 1: a + b; 2: a + 3r - b; 3: weak(a); 4: reduce256(a);
// 5: cond_sub(a); 6: from_words(a[0..7]); 7: to_words(a) -> 8 words; 8: one fold.  b may be null.
// Returns the overflow count of the call, or -1 for an unknown op / variant.
int ht_fr29_field_op(int variant, int op, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  fr29_overflows() = 0;
  const int rc = variant == 0 ? fr29_check<Fr29Bls>(op, a, b, r) : variant == 1 ? fr29_check<Fr29Bn>(op, a, b, r) : -1;
  return rc ? -1 : fr29_overflows();
}
// bls12-381 Fr, ops 0..7
int ht_fr29_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  if (op < 0 || op > 7) return -1;
  return ht_fr29_field_op(0, op, a, b, r);
}
// the row of ncg_field_check's field table (selfcheck.hpp): out = words per row of a, b and out; -1 for a field that is refused
int ht_field_check_shape(int field, int out[3]) {
  const SelfCheckField* f = selfcheck_field(field);
  if (!f) return -1;
  out[0] = f->wa;
  out[1] = f->wb;
  out[2] = f->wo;
  return 0;
}
// fe9m.hpp (bn254 base field, Montgomery radix 2^29) on RAW limbs: fe9m_check (fe9m_check.hpp), the same code as
// ncg_field_check field 9.  Returns the overflow count of the call, or -1 for an unknown op / variant.
int ht_fe9m_op(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  fe9m_overflows() = 0;
  if (fe9m_check(op, variant, a, b, r) != 0) return -1;
  return fe9m_overflows();
}
// the group law of the MSM buckets on STORED words (group_check.hpp, the code of ncg_field_check fields 10-14): field 10 secp256k1,
// 11 ed25519, 12 bls12-381 G1, 13 G2, 14 bn254 G1; ops 0-3; a, b, out: ACC_WORDS raw words.  Field 13 runs the UNPAIRED Fp2 form
// (CurveG2: the lane-paired products exist on the device only); the stored layout is the same, c0 then c1.
int ht_group_op(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (op < 0 || op > 3) return -1;
  switch (field) {
    case 10: group_check_op<CurveSecp>(op, a, b, out); return 0;
    case 11: group_check_op<CurveEd>(op, a, b, out); return 0;
    case 12: group_check_op<CurveG1>(op, a, b, out); return 0;
    case 13: group_check_op<CurveG2>(op, a, b, out); return 0;
    case 14: group_check_op<CurveBn254>(op, a, b, out); return 0;
  }
  return -1;
}
// f_eqz of raw limbs at the bound A (4, 66 or 128: group_check.hpp): 14 limbs as Fe29<A>, or - paired - 28 limbs c0, c1.  No host
// case emulates pair_swap (on the host it is the identity), so the paired twin takes the two halves through the unpaired
// Fe29x2<A>, whose verdict is the and of the halves as well.  Returns 0 / 1, or -1 for an unknown bound.
int ht_fe29_eqz(int paired, int A, const uint32_t* a) {
  const int z0 = fe29_eqz_check<Fe29>(A, a);
  if (!paired || z0 < 0) return z0;
  auto half = [&](auto x, int h) {
    for (int i = 0; i < 14; i++) x.v[i] = a[14 * h + i];
    return x;
  };
  switch (A) {
    case 4: return f_eqz(Fe29x2<4>(half(Fe29<4>(), 0), half(Fe29<4>(), 1))) ? 1 : 0;
    case 66: return f_eqz(Fe29x2<66>(half(Fe29<66>(), 0), half(Fe29<66>(), 1))) ? 1 : 0;
    case 128: return f_eqz(Fe29x2<128>(half(Fe29<128>(), 0), half(Fe29<128>(), 1))) ? 1 : 0;
  }
  return -1;
}
// the pass schedule of ntt_run (the shipped ntt_schedule with the device's pass limits and table): 11 ints per pass,
// T logC colhi dit inverse brp_store scale canon s_lo in out (buffers 0 src, 1 dst, 2 ws); returns the number of passes
int ht_ntt_schedule(int n, int flags, int* out) {
  if (n < 0 || n > NCG_NTT_MAX_LOG2N || flags < 0 || flags > 7) return -1;
  const NttSchedule sc = ntt_schedule(n, n, flags);
  for (int k = 0; k < sc.np; k++) {
    const NttPass& ps = sc.ps[k];
    const int row[11] = {ps.T, ps.logC, ps.colhi, ps.dit, ps.inverse, ps.brp_store, ps.scale, ps.canon, ps.s_lo, sc.in[k], sc.out[k]};
    for (int i = 0; i < 11; i++) out[11 * k + i] = row[i];
  }
  return sc.np;
}
// poly.hip on the CPU: the per-element and per-run functions of the kernels, T threads executed one after the other (T = 0: the
// thread count the device launches).  Each returns the overflow count of fr29.hpp's host checks (the table entries are the only
// fr29 values poly.hip touches), or -1 for an unknown request.
int ht_poly_pointwise(int field, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  return poly_host(field, 0, op, n, a, b, 1, nullptr, 0, out);
}
int ht_poly_scale(int field, size_t n, const uint32_t* a, const uint32_t* s, int powers, size_t T, uint32_t* out) {
  return poly_host(field, 1, powers, n, a, nullptr, 1, s, T, out);
}
int ht_poly_eval(int field, size_t n, const uint32_t* a, const uint32_t* basis, size_t T, uint32_t* out) {
  return poly_host(field, 2, 0, n, a, basis, 1, nullptr, T, out);
}
int ht_poly_eval_monomial(int field, size_t n, const uint32_t* a, int m, const uint32_t* xs, size_t T, uint32_t* out) {
  if (m < 1 || m > NCG_POLY_MAX_POINTS) return -1;
  return poly_host(field, 3, 0, n, a, nullptr, m, xs, T, out);
}
// s^start: the start power of the run that begins at index `start`
int ht_poly_pow(int field, const uint32_t* s, uint64_t start, uint32_t* out) {
  return poly_host(field, 4, 0, (size_t)start, nullptr, nullptr, 1, s, 0, out);
}
int ht_poly_lagrange(int field, int log2n, const uint32_t* omega, const uint32_t* x, int brp, size_t T, uint32_t* out, uint32_t* root_out) {
  if (log2n < 0 || log2n > 20) return -1;
  return poly_host_lagrange(field, log2n, omega, x, brp, T, out, root_out);
}
int ht_poly_lag_run() { return POLY_LAG_RUN; }
int ht_ntt_max_log2n() { return NCG_NTT_MAX_LOG2N; }
// the pass planner of ntt_run: writes s_lo/T pairs, returns the number of passes
int ht_ntt_plan(int n, int* out) {
  int s_lo[8], T[8];
  int np = ntt_plan(n, s_lo, T);
  for (int i = 0; i < np; i++) {
    out[2 * i] = s_lo[i];
    out[2 * i + 1] = T[i];
  }
  return np;
}

// challenge scalar k = SHA-512(R || A || M) mod L through the device code (sha512.hpp); out: 8 words
int ht_ed25519_challenge(const uint8_t* sig, const uint8_t* pk, const uint8_t* msg, uint64_t len, uint32_t* out) {
  ed25519_challenge_host(sig, pk, msg, len, out);
  return 0;
}

// bls12-381 scalar split of the endomorphism MSM (endo.hpp): E = 2 (G1) or 4 (G2) sub-scalars, 6 words each
// (192-bit two's complement)
int ht_bls_endo_split(int E, const uint32_t* k8, uint32_t* out) {
  uint32_t k[8];
  for (int i = 0; i < 8; i++) k[i] = k8[i];
  if (E == 2) {
    uint32_t o[2][6];
    bls_endo_split2(o, k);
    for (int e = 0; e < 2; e++)
      for (int i = 0; i < 6; i++) out[e * 6 + i] = o[e][i];
    return 0;
  }
  if (E == 4) {
    uint32_t o[4][6];
    bls_endo_split4(o, k);
    for (int e = 0; e < 4; e++)
      for (int i = 0; i < 6; i++) out[e * 6 + i] = o[e][i];
    return 0;
  }
  return -1;
}

// ECDSA scalar side of one signature through the lane code (ecdsa.hip): u1 = h / s, u2 = r / s mod n, 8 LE words each
int ht_ecdsa_prepare(const uint8_t* sig64, const uint8_t* hash32, int low_s, uint32_t* u1, uint32_t* u2) {
  uint8_t ok = 0;
  ecdsa_prepare_host(sig64, hash32, low_s != 0, u1, u2, &ok);
  return ok;
}

// ed25519 verify of one item on the CPU through the kernel's lane function
int ht_ed25519_verify(const uint32_t* sig, const uint32_t* pk, const uint32_t* k, int zip215) {
  static uint32_t btab[ED25519_BTAB_WORDS];
  static bool built = false;
  if (!built) {
    ed25519_build_base_table(btab);
    built = true;
  }
  return ed25519_verify_host(sig, pk, k, btab, zip215 != 0) ? 1 : 0;
}

// the scalar side of the halved ed25519 verification (ed_halve.hpp): out = u[4] | v[4] | uneg | w[8], w = u s mod L
int ht_ed_halve(const uint32_t* k, const uint32_t* s, uint32_t* out) {
  uint32_t kk[8], ss[8], w[8];
  for (int i = 0; i < 8; i++) {
    kk[i] = k[i];
    ss[i] = s[i];
  }
  const EdHalf h = ed_halve_scalar(kk);
  ed_mul_mod_l(w, h.u, ss);
  for (int i = 0; i < 4; i++) {
    out[i] = h.u[i];
    out[4 + i] = h.v[i];
  }
  out[8] = h.uneg ? 1u : 0u;
  for (int i = 0; i < 8; i++) out[9 + i] = w[i];
  return 0;
}

size_t ht_msm_shard_slot_bytes(int curve) { return msm_shard_slot_bytes(curve); }
int ht_msm_shard_windows_local(int curve, int n, int part, int nparts, const uint32_t* pts_wire, const uint32_t* scalars, uint8_t* slot, int shared) {
#define CALL(C) ht_shard_local_t<C>(curve, n, n, pts_wire, scalars, slot, shared ? SHARD_WINDOWS_SHARED : SHARD_WINDOWS, part, nparts)
  HT_CURVE_DISPATCH(curve, CALL)
#undef CALL
}
int ht_msm_shard_local(int curve, int n_local, int n_max, const uint32_t* pts_wire, const uint32_t* scalars, uint8_t* slot) {
#define CALL(C) ht_shard_local_t<C>(curve, n_local, n_max, pts_wire, scalars, slot, SHARD_POINTS, 0, 1)
  HT_CURVE_DISPATCH(curve, CALL)
#undef CALL
}
// the lane segment msm_seg picks for a whole generic plan of n points (msm_plan.hpp): out = {c, nwin, nb, seg, nseg, lanes per window << ls, accum_waves}
int ht_msm_seg(int curve, int n, int c_override, int* out) {
  MsmPlan pl;
  if (msm_make_plan_impl(curve, n, c_override, &pl) != 0) return -1;
  const MsmSeg sg = msm_seg(pl);
  out[0] = pl.c; out[1] = pl.nwin; out[2] = pl.nb; out[3] = sg.seg; out[4] = sg.nseg; out[5] = sg.nseg << pl.ls; out[6] = pl.accum_waves;
  return 0;
}
// the launch schedule of the device phase (msm_schedule.hpp) as integers.  The plan is built as the entry points build it:
// opt = {endo (msm_make_plan_endo), shared (precomputed set), part_flags, n_layout (> 0: a part of a host-pointer MSM whose
// layout plan has n_layout points), w0, window count (0 = all; the window-sharded ranks' msm_plan_take_windows), seg override,
// run_serial override, pts_stored}.  out: the fields named in tests/hosttest.py MSM_SCHEDULE_FIELDS, then (tasks, coop, grid) of
// the 16 fold-level slots.
int ht_msm_schedule(int curve, int n, int c_override, const int* opt, long long* out) {
  MsmPlan pl;
  if ((opt[0] ? msm_make_plan_endo(curve, n, c_override, &pl) : msm_make_plan_impl(curve, n, c_override, &pl)) != 0) return -1;
  if (opt[1]) {  // api.hip ncg_resident_plan
    pl.shared = 1;
    pl.top_tb = 0;
    pl.top_submask = 0;
  }
  pl.pts_stored = opt[8] || opt[1];
  pl.part_flags = opt[2];
  if (opt[3] > 0) {  // api.hip ncg_msm: the layout plan has the same window width
    MsmPlan layout;
    if (msm_make_plan_impl(curve, opt[3], pl.c, &layout) != 0) return -1;
    pl.n_layout = layout.n;
    pl.Q_layout = layout.Q;
  }
  if (opt[5] > 0) msm_plan_take_windows(pl, opt[4], opt[5], opt[5] <= 2 ? 128 : 512);  // comm.hip shard_local
  pl.seg_override = opt[6];
  pl.run_serial_override = opt[7];
  const MsmShape sh = msm_shape(curve);
  const MsmSchedule S = msm_schedule(pl, sh);
  const MsmLayout& L = S.layout;
  // msm_seg prices the placement of the grid it proposes with the rule the launch pins it by
  const long seg_wgs = (long)S.av.nwin * ((((long)S.sg.nseg << sh.ls) + 255) / 256);
  const long long v[] = {
      (long long)L.pts_mont, (long long)L.digits, (long long)L.counts, (long long)L.bucket_start, (long long)L.sorted, (long long)L.sort_tmp,
      (long long)L.shared_start, (long long)L.buckets, (long long)L.part_pts, (long long)L.part_meta, (long long)L.long_runs, (long long)L.bad,
      (long long)L.red0, (long long)L.red1, (long long)L.tail0, (long long)L.tail1, (long long)L.fin, (long long)L.total,
      pl.c, pl.nwin, pl.nb, pl.Q, S.av.n, S.av.nwin, pl.top_tb, sh.ls, sh.coop,
      S.part_first, S.part_last, S.pts_in_place, S.pts_grid, S.digits_grid,
      S.sort, S.s2.lgr, S.sort_grid.x, S.sort_grid.y, (long long)S.small_lds, (long long)S.hist_lds, (long long)S.scan_lds, S.split_totals,
      S.totals_grid.x, S.totals_grid.y, S.shared_grid, S.scatter_n, S.scatter_per,
      S.sg.seg, S.sg.nseg, S.acc_grid.x, S.acc_grid.y, (long long)S.acc_reserve, S.acc_sparse, msm_acc_pinned(seg_wgs), S.run_serial, S.merge,
      S.merge_grid.x, S.merge_grid.y, (long long)S.merge_lds, (long long)S.long_lds,
      S.nfold, (long long)S.fold_coop_lds, S.narr, S.n_in, S.tail_units, (long long)S.tail_lds, S.ngroups, S.top_w,
      MSM_LONG_BLOCKS, MSM_TAIL_THREADS, (long long)SORT2_STAGE * 4};
  const int nv = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < nv; i++) out[i] = v[i];
  for (int l = 0; l < 16; l++) {
    const bool on = l < S.nfold;
    out[nv + 3 * l] = on ? S.fold[l].tasks : 0;
    out[nv + 3 * l + 1] = on ? S.fold[l].coop : 0;
    out[nv + 3 * l + 2] = on ? S.fold[l].grid : 0;
  }
  return nv;
}
int ht_msm_shard_combine(int curve, int n_max, int nparts, const uint8_t* slots, uint32_t* out, uint8_t* out_inf, char* err, int errlen) {
#define CALL(C) ht_shard_combine_t<C>(curve, n_max, nparts, slots, out, out_inf, err, errlen)
  HT_CURVE_DISPATCH(curve, CALL)
#undef CALL
}
// host finish of the MSM alone: variant 0 = the device templates compiled for the host, 1 = the default
// (bls12-381: 64-bit-limb Jacobian form of bls_host64.hpp; its field product on MULX / ADX where the CPU has them),
// 2 = the default with the portable field product forced, 3 = the default with the helper threads of the finish woken inside the
// call (bls_host64.hpp FinishPool: windows built by the helpers, the chain by the caller), 4 = the helper threads off
static int ht_msm_finish_default(int curve, int c, int nwin, const uint32_t* fin, uint32_t* out, uint8_t* out_inf) {
#define CALL(C) (msm_host_finish_any<C>(fin, c, nwin, out, out_inf), 0)
  HT_CURVE_DISPATCH(curve, CALL)
#undef CALL
}
int ht_msm_finish(int curve, int c, int nwin, const uint32_t* fin, uint32_t* out, uint8_t* out_inf, int variant) {
  if (variant == 0) {
#define CALL(C) (msm_host_finish<C>(fin, c, nwin, out, out_inf), 0)
    HT_CURVE_DISPATCH(curve, CALL)
#undef CALL
  }
  h64::adx_override() = variant == 2 ? 0 : -1;
  h64::finish_threads_override() = variant == 3 ? 2 : variant == 4 ? 0 : 1;
  const int rc = ht_msm_finish_default(curve, c, nwin, fin, out, out_inf);
  h64::adx_override() = -1;
  h64::finish_threads_override() = 1;
  return rc;
}
int ht_h64_have_adx(void) { return h64::have_adx() ? 1 : 0; }
// bls_host64.hpp on raw operands: op 0 / 2: Montgomery product of two canonical residues given as 6 x 64-bit words (result
// 6 words; 0 = as dispatched, 2 = the portable form); op 1: from_fe29 of 14 stored limbs (result 6 words, Montgomery form R = 2^384)
int ht_h64_op(int op, const uint64_t* a, const uint64_t* b, const uint32_t* limbs, uint64_t* r) {
  h64::Fp x, y, z;
  if (op == 0) {
    for (int i = 0; i < 6; i++) {
      x.v[i] = a[i];
      y.v[i] = b[i];
    }
    z = h64::mul(x, y);
  } else if (op == 2) {  // the portable product, whatever the CPU
    for (int i = 0; i < 6; i++) {
      x.v[i] = a[i];
      y.v[i] = b[i];
    }
    z = h64::mul_c(x, y);
  } else if (op == 1) {
    z = h64::from_fe29(limbs);
  } else {
    return -1;
  }
  for (int i = 0; i < 6; i++) r[i] = z.v[i];
  return 0;
}
int ht_msm_plan(int curve, int n, int* out) {  // c, nwin, ngroups, acc words
  MsmPlan pl;
  if (msm_make_plan_impl(curve, n, 0, &pl) != 0) return -1;
  out[0] = pl.c;
  out[1] = pl.nwin;
  out[2] = msm_ngroups(pl.c);
  out[3] = (int)msm_shape(curve).acc_words;
  return 0;
}

// the short-top-window part of a plan (MsmPlan::top_tb): c (forced when c_override > 0), nwin, top_tb, top_submask, the
// largest field the top window can hold (msm_plan_top_vmax) and H' (10 words) - tests/test_host_logic.py replays the digit
// kernel's mapping on them with Python integers
int ht_msm_plan_top(int curve, int n, int c_override, uint32_t* out16) {
  MsmPlan pl;
  if (msm_make_plan_impl(curve, n, c_override, &pl) != 0) return -1;
  out16[0] = (uint32_t)pl.c;
  out16[1] = (uint32_t)pl.nwin;
  out16[2] = (uint32_t)pl.top_tb;
  out16[3] = pl.top_submask;
  out16[4] = msm_plan_top_vmax(pl);
  out16[5] = (uint32_t)pl.nb;
  for (int i = 0; i < 10; i++) out16[6 + i] = pl.hconst[i];
  return 0;
}

// bls12-381 pairing twins (tests/pairing_helpers.py): the templates of fp12.hpp / pairing.hpp on the unpaired Fp2.
// ht_fp12_op: the ops of ncg_fp12_batch on wire rows; raw != 0 reads `a` as 168 stored words (Montgomery limbs below 256 p).
// ht_pairing: ncg_pairing_batch (flags as there); returns -1 or the first refused pair with its code in *bad_code.
int ht_fp12_op(int op, const uint32_t* a, const uint32_t* b, void* out, int n, int raw) {
  if (op < 0 || op > 10) return -1;
  fp12_op_host(op, a, b, out, n, raw != 0);
  return 0;
}
long long ht_pairing(const uint32_t* g1, const uint32_t* g2, int n, const uint32_t* off, int n_groups, int flags, uint32_t* out_gt,
                     uint8_t* out_is_one, uint32_t* bad_code) {
  return (long long)pairing_host(g1, g2, n, off, n_groups, flags & NCG_PAIRING_CHECK_SUBGROUP, out_gt, out_is_one, bad_code);
}
// Frobenius coefficients as the lane code holds them: 3 tables x 4 powers x (c0, c1) as 12 canonical wire words each
int ht_tower_consts(uint32_t* out) {
  const uint32_t (*tabs[3])[2][14] = {BlsTower::FROB6_C1, BlsTower::FROB6_C2, BlsTower::FROB12};
  for (int t = 0; t < 3; t++)
    for (int k = 0; k < 4; k++)
      for (int c = 0; c < 2; c++) fe29_to_wire(out + ((t * 4 + k) * 2 + c) * 12, fe29_const(tabs[t][k][c]));
  return 0;
}

}  // extern "C"
