// Internal C++ interface between the C ABI (api.hip) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ncg {

// jac_tmp: device scratch of mul_var_tmp_bytes(curve, n) bytes, or nullptr (per-lane inversion)
hipError_t mul_var_batch(int curve, const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf,
                         int n, uint32_t* jac_tmp, hipStream_t st);
size_t mul_var_tmp_bytes(int curve, int n);
// the secp256k1 ladder with the field multiply inlined (mulvar_inl.hip), for mul_var_batch with scratch
hipError_t mul_var_secp_inline(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n,
                               uint32_t* jac_tmp, hipStream_t st);
// projective (X, Y, Z) wire points -> affine wire points, x = X/Z, y = Y/Z (normalizeZ)
hipError_t normalize_batch(int curve, const uint32_t* proj_wire, uint32_t* out_wire, uint8_t* out_inf, int n,
                           hipStream_t st);

// pairwise A[i] + B[i] (subtract: A[i] - B[i]) on affine wire points; jac_tmp as for mul_var_batch
hipError_t pair_add_batch(int curve, const uint32_t* a, const uint32_t* b, int subtract, uint32_t* out, uint8_t* out_inf,
                          int n, uint32_t* jac_tmp, hipStream_t st);
hipError_t ed25519_proj_to_affine(const uint32_t* proj, uint32_t* out, uint8_t* out_inf, int n, hipStream_t st);

// fixed-base batch multiply (mulbase.hip)
size_t mul_base_table_bytes(int curve);
hipError_t mul_base_build_table(int curve, const uint32_t* base_wire_host, uint32_t* d_table, hipStream_t st);
hipError_t mul_base_batch(int curve, const uint32_t* table, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf,
                          int n, uint32_t* jac_tmp, hipStream_t st);

// batch point decoding (decode.hip): bytes per encoded point, 0 if the curve has no decoder
int decode_in_bytes(int curve);
hipError_t decode_points_batch(int curve, const uint8_t* in, int flags, uint32_t* out, uint8_t* ok, uint8_t* inf, int n,
                               hipStream_t st);
// compressed encodings of affine wire points (Point.toBytes); ok = 0 where the reference throws
hipError_t encode_points_batch(int curve, const uint32_t* in, uint8_t* out, uint8_t* ok, int n, hipStream_t st);
void encode_points_host(int curve, const uint32_t* in, uint8_t* out, uint8_t* ok, int n);
void decode_points_host(int curve, const uint8_t* in, int flags, uint32_t* out, uint8_t* ok, uint8_t* inf, int n);

// batch map-to-curve + cofactor clearing for bls12-381 G1 / G2 (h2c.hip); count = 1 or 2 field
// elements per output point
hipError_t map_to_curve_batch(int curve, const uint32_t* u, int count, uint32_t* out, uint8_t* inf, int n,
                              uint32_t* jac_tmp, hipStream_t st);
void map_to_curve_host(int curve, const uint32_t* u, int count, uint32_t* out, uint8_t* inf, int n);

// radix-2 NTT over bls12-381 Fr or bn254 Fr (ntt.hip); field = NCG_FIELD_BLS12_381_FR | NCG_FIELD_BN254_FR
size_t ntt_table_bytes(int n);
int ntt_tw_words();
void ntt_tw_from_canonical(const uint32_t (&w)[8], uint32_t* out);
size_t ntt_small_bytes(int n);
void ntt_field_consts(int field, const uint32_t** p, const uint32_t** k261);  // r and 2^261 mod r, 8 LE words each
hipError_t ntt_build_table(int field, int n, const uint32_t* d_omega, uint32_t* d_small, uint32_t* d_tab, hipStream_t st);
hipError_t ntt_run(int field, int n, size_t batch, const uint32_t* src, uint32_t* dst, uint32_t* ws, const uint32_t* tab,
                   int tab_log, int flags, hipStream_t st);
int ntt_host(int field, int n, const uint32_t* omega_wire, const uint32_t* src, uint32_t* dst, int flags, int t0max = 10, int tmax = 8);

// polynomial arithmetic over the same two fields on resident vectors (poly.hip; reference poly(), fft.ts:583-926).  Small operands
// (s, xs, x) are HOST pointers to canonical residues; ws: poly_ws_bytes(log2n of a product, or -1) bytes of device memory, whose head holds
// the partial sums and the root-index word; tab: the cached twiddle table of (field, log2n)
size_t poly_ws_bytes(int log2n_mul);
hipError_t poly_pointwise(int field, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, hipStream_t st);
hipError_t poly_scale(int field, size_t n, const uint32_t* a, const uint32_t* s_host, int powers, uint32_t* out, hipStream_t st);
hipError_t poly_eval(int field, size_t n, const uint32_t* a, const uint32_t* basis, void* ws, uint32_t* out, hipStream_t st);
hipError_t poly_eval_monomial(int field, size_t n, const uint32_t* a, int m, const uint32_t* xs_host, void* ws, uint32_t* out, hipStream_t st);
hipError_t poly_lagrange_basis(int field, int log2n, const uint32_t* tab, const uint32_t* x_host, int brp, void* ws, uint32_t* out,
                               hipStream_t st);
hipError_t poly_mul(int field, int log2n, const uint32_t* tab, size_t na, const uint32_t* a, size_t nb, const uint32_t* b, void* ws,
                    uint32_t* out, hipStream_t st);
// host twin: kind 0 pointwise (op), 1 scale (op = powers), 2 dot-sum, 3 monomial evaluation at m points, 4 small^n; T threads (0: the device's)
int poly_host(int field, int kind, int op, size_t n, const uint32_t* a, const uint32_t* b, int m, const uint32_t* small, size_t T, uint32_t* out);
int poly_host_lagrange(int field, int log2n, const uint32_t* omega_wire, const uint32_t* x_wire, int brp, size_t T, uint32_t* out,
                       uint32_t* root_out);

struct MsmPlan;
// Optional second stream of a context: the wire -> storage conversion of the points has no consumer before
// the accumulate kernel, so it runs beside the digit / sort kernels (LDS- and memory-bound) instead of in
// front of them.  fork / join are timing-disabled events.
struct MsmSide {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  // set by the host-pointer entry point: the stored points are being produced elsewhere (chunked upload + conversion on
  // other streams); the accumulate kernel waits for this event, the digit / sort kernels do not
  hipEvent_t pts_ready = nullptr;
};

int msm_make_plan(int curve, int n, int c_override, MsmPlan* pl);
size_t msm_workspace_bytes(int curve, const MsmPlan& pl);
// d_pts / d_scalars: device; out_*: host.  Synchronises `st` (host-side Horner finish).
// *bad_index (optional): smallest index of a scalar >= the group order, 0xFFFFFFFF if none (the result is
// then meaningless: the caller fails the call like the reference's validateMSMScalars, curve.ts:398-404)
hipError_t msm_run(int curve, const MsmPlan& pl, const uint32_t* d_pts, const uint32_t* d_scalars, void* ws,
                   uint32_t* out_affine_host, uint8_t* out_inf_host, hipStream_t st, uint32_t* bad_index = nullptr,
                   const MsmSide* side = nullptr);
// wire points -> the accumulate kernel's storage format (what a plan with pts_stored = 1 takes as d_pts)
size_t msm_stored_words_per_point(int curve);
hipError_t msm_points_to_stored(int curve, const uint32_t* d_pts_wire, int n, uint32_t* d_out, hipStream_t st);

// The same in two phases, for the multi-GPU path: msm_device_phase leaves the grouped window sums
// (msm_fin_words(curve, pl) words = npoints accumulators of msm_acc_words(curve) words) in the workspace
// and returns their device address; msm_sum_partials adds nparts such arrays element by element;
// msm_finish brings one array to the host and finishes (synchronises `st`).
hipError_t msm_device_phase(int curve, const MsmPlan& pl, const uint32_t* d_pts, const uint32_t* d_scalars, void* ws,
                            const uint32_t** d_fin, hipStream_t st, const uint32_t** d_bad = nullptr,
                            const MsmSide* side = nullptr);
hipError_t msm_finish(int curve, const MsmPlan& pl, const uint32_t* d_fin, uint32_t* out_affine_host,
                      uint8_t* out_inf_host, hipStream_t st, const uint32_t* d_bad = nullptr, uint32_t* bad_host = nullptr);
hipError_t msm_sum_partials(int curve, uint32_t* d_gathered, int nparts, size_t npoints, uint32_t* d_out,
                            hipStream_t st);  // d_gathered is scratch: reduced in place
// asynchronous form: device phase + D2H of the grouped sums and the scalar-range flag into `land` (pinned host memory,
// msm_fin_words + 1 words), nothing synchronised; msm_finish_host is the host half of msm_finish on a host array of
// [ngroups(c)][nwin] grouped sums (also what the window-sharded multi-GPU mode assembles from the ranks' slots)
hipError_t msm_enqueue(int curve, const MsmPlan& pl, const uint32_t* d_pts, const uint32_t* d_scalars, void* ws, uint32_t* land,
                       hipStream_t st, const MsmSide* side = nullptr);
void msm_finish_host(int curve, int c, int nwin, const uint32_t* fin_host, uint32_t* out_affine_host, uint8_t* out_inf_host);
// the host finish of this curve is about to run (tens of microseconds from now): wakes its helper threads, if it has any
// (bls12-381: bls_host64.hpp FinishPool); a no-op otherwise
void msm_finish_prewake(int curve);
size_t msm_fin_words(int curve, const MsmPlan& pl);
size_t msm_acc_words(int curve);

// Window-shifted copies of a stored affine set for the shared-bucket MSM (msm_precomp.hip): d_levels holds nlev
// levels of m points (level 0 = the set itself, filled by the caller); level w = 2^(c w) * level 0.  Weierstrass
// curves only.  A plan with shared = 1 (and c, nwin = nlev) then takes d_levels as its point array.
size_t msm_shift_tmp_bytes(int curve, int m);
hipError_t msm_shift_levels(int curve, uint32_t* d_levels, int m, int nlev, int c, void* d_tmp, hipStream_t st);

// G1 batch multiply on verified subgroup points (mulvar_endo.hip): GLV ladder with the phi endomorphism
hipError_t mul_var_batch_g1_subgroup(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n,
                                     uint32_t* jac_tmp, hipStream_t st);
// G2 likewise: four 64-bit streams along psi; jac_tmp holds mul_var_g2_subgroup_tmp_bytes(n) bytes
hipError_t mul_var_batch_g2_subgroup(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n,
                                     uint32_t* jac_tmp, hipStream_t st);
size_t mul_var_g2_subgroup_tmp_bytes(int n);

// secp256k1 ECDSA batch verify, scalar side (ecdsa.hip): sig = r || s (big-endian), hash = 32 bytes.
hipError_t ecdsa_prepare(const uint8_t* d_sig, const uint8_t* d_hash, int n, bool low_s, uint32_t* d_u1, uint32_t* d_u2,
                         uint8_t* d_sig_ok, hipStream_t st);
hipError_t ecdsa_finish(const uint8_t* d_sig, const uint32_t* d_R, const uint8_t* d_R_inf, const uint8_t* d_sig_ok,
                        const uint8_t* d_pub_ok, const uint8_t* d_pub_inf, int n, uint8_t* d_out_ok, hipStream_t st);
hipError_t sha256_msgs(const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sig64, const uint8_t* d_pkx, int mode, int n,
                       uint8_t* d_out32, hipStream_t st);
hipError_t ecdsa_recover_prepare(const uint8_t* d_sig65, const uint8_t* d_hash, int n, uint32_t* d_u1, uint32_t* d_u2,
                                 uint8_t* d_pub33, uint8_t* d_pre_ok, hipStream_t st);
hipError_t ecdsa_recover_finish(uint32_t* d_Q, const uint8_t* d_Q_inf, const uint8_t* d_pre_ok, const uint8_t* d_pub_ok, int n,
                                uint8_t* d_out_ok, hipStream_t st);
hipError_t secp_load_uncompressed(const uint8_t* d_pub65, uint32_t* d_out, uint8_t* d_ok, uint8_t* d_inf, int n, hipStream_t st);
hipError_t schnorr_prepare(const uint8_t* d_sig, const uint8_t* d_e, const uint8_t* d_pkx, int n, uint32_t* d_u1, uint32_t* d_u2,
                           uint8_t* d_pub33, uint8_t* d_pre_ok, hipStream_t st);
hipError_t schnorr_finish(const uint8_t* d_sig, const uint32_t* d_R, const uint8_t* d_R_inf, const uint8_t* d_pre_ok,
                          const uint8_t* d_pub_ok, const uint8_t* d_pub_inf, int n, uint8_t* d_out_ok, hipStream_t st);
void ecdsa_prepare_host(const uint8_t* sig, const uint8_t* hash, bool low_s, uint32_t* u1, uint32_t* u2, uint8_t* ok);

// Endomorphism mode for bls12-381 point sets verified to lie in the prime-order subgroup (msm_endo.hip,
// endo.hpp).  msm_endo_factor: sub-scalars per scalar (2 on G1, 4 on G2, 0 = not offered).  msm_endo_expand
// writes the factor * n images of n wire points in the accumulate kernel's input format; a plan from
// msm_make_plan_endo makes msm_device_phase / msm_run take that array as `d_pts`.  msm_endo_verify compares
// [z^2]P (G1) / [z]P (G2) from the generic batch multiply with image 1: *d_bad = smallest failing index.
int msm_endo_factor(int curve);
int msm_make_plan_endo(int curve, int n_src, int c_override, MsmPlan* pl);
size_t msm_endo_words_per_point(int curve);
hipError_t msm_endo_expand(int curve, const uint32_t* d_pts_wire, int n, uint32_t* d_out, hipStream_t st);
hipError_t msm_endo_digits(const MsmPlan& pl, const uint32_t* d_scalars, int16_t* digits, uint32_t* bad, hipStream_t st);
hipError_t msm_endo_verify(int curve, const uint32_t* d_mult, const uint8_t* d_mult_inf, const uint32_t* d_images, int n,
                           uint32_t* d_bad, hipStream_t st);
void msm_endo_verify_scalar(int curve, uint32_t (&k)[8]);

// ed25519 batch verify (ed25519.hip).  btab: device copy of the table built by ed25519_build_base_table.
constexpr int ED25519_BTAB_WORDS = 256 * 27;  // [1,3,..,255] B then [1,3,..,255] 2^128 B, affine Niels, 3 x 9 stored words each
void ed25519_build_base_table(uint32_t* out_words);
size_t ed25519_verify_tmp_words(int n);
size_t ed25519_tmp_words(int n);
hipError_t ed25519_verify_batch(const uint32_t* sigs, const uint32_t* pks, const uint32_t* ks, const uint32_t* btab,
                                int zip215, uint8_t* out_ok, int n, uint32_t* gtab, hipStream_t st);
// challenge scalars k[i] = SHA-512(R_i || A_i || M_i) mod L (edwards.ts:984, :900-906) for a batch; ks: n x 8 words
hipError_t ed25519_challenge_batch(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* msg_off,
                                   uint32_t* ks, int n, hipStream_t st);
void ed25519_challenge_host(const uint8_t* sig, const uint8_t* pk, const uint8_t* msg, uint64_t len, uint32_t* k_out);
hipError_t ed25519_mul_var_batch(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n,
                                 uint32_t* proj_tmp, hipStream_t st);
// fixed-base multiply: table of ed25519_fixed_table_words() words built by ed25519_build_fixed_table (host)
size_t ed25519_fixed_table_words();
void ed25519_build_fixed_table(uint32_t* out_words);
hipError_t ed25519_mul_base_batch(const uint32_t* table, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n,
                                  uint32_t* proj_tmp, hipStream_t st);
hipError_t ed25519_mul_base_proj(const uint32_t* table, const uint32_t* scalars, uint32_t* proj_out, int n, hipStream_t st);
void ed25519_mul_var_host(const uint32_t* pt, const uint32_t* k, uint32_t* out, uint8_t* out_inf);
bool ed25519_verify_host(const uint32_t* sig, const uint32_t* pk, const uint32_t* k, const uint32_t* btab, bool zip215);

// Ed25519 signing (ed25519_sign.hip).  table: device copy of ed25519_build_scan_table's output (ed25519_scan_table_words() words),
// [w][j] = (2 j + 1) 2^(W w) B from ed25519_build_window_table (ed25519.hip; entries of 27 stored words).  Expanded key rows are
// 24 LE words: scalar || prefix || A.  ed25519_expand_batch: see ed25519_sign.hip.  ed25519_sign_batch: keys are seeds (32 bytes) or
// expanded rows, one per message or one in all; dom_host is a HOST pointer; msgs / msg_off as for ed25519_challenge_batch; sigs: 16
// words per row; ws: ed25519_sign_ws_words(n, rows to expand, prehash) words of device memory that hold secrets afterwards.
constexpr int ED25519_DOM_MAX = 289;      // 32 + 2 + 255
constexpr int ED_SIGN_DOM_WORDS = 80;     // dom at the head of the workspace
void ed25519_build_window_table(uint32_t* out_words, int w_bits, int windows);
size_t ed25519_scan_table_words();
void ed25519_build_scan_table(uint32_t* out_words);
hipError_t ed25519_mul_base_scan_batch(const uint32_t* table, const uint32_t* scalars, int in_stride, uint32_t* out, int out_stride, int n,
                                       hipStream_t st);
hipError_t ed25519_expand_batch(const uint32_t* table, const uint8_t* seeds, uint32_t* keys, uint32_t* out_a, int out_stride, int n,
                                hipStream_t st);
size_t ed25519_sign_ws_words(int n, int nkeys_to_expand, int prehash);
hipError_t ed25519_sign_batch(const uint32_t* table, const void* keys, int expanded, int one_key, int prehash, const uint8_t* dom_host,
                              uint32_t dom_len, const uint8_t* msgs, const uint64_t* msg_off, uint32_t* sigs, uint8_t* ok, int n, uint32_t* ws,
                              hipStream_t st);
void ed25519_mul_base_scan_host(const uint32_t* table, const uint32_t* scalars, uint32_t* out, int n);
void ed25519_expand_host(const uint32_t* table, const uint8_t* seeds, uint32_t* keys, int n);
void ed25519_sign_host(const uint32_t* table, const void* key, int expanded, int prehash, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg,
                       uint64_t len, const uint32_t* r_in, uint32_t* sig, uint8_t* ok);
void sha512_segments_host(const uint8_t* dom, uint32_t dom_len, const uint8_t* a32, const uint8_t* b32, const uint8_t* msg, uint64_t len,
                          uint8_t* out64);

// secp256k1 signing (secp256k1_sign.hip).  table: device copy of secp_build_scan_table's output (secp_scan_table_words() words):
// [w][j] = (2 j + 1) 2^(4 w) G as affine points of 18 stored words, then the BIP-340 tag hashes.
// Keys, hashes, extra entropy and aux rows are 32 big-endian bytes; signatures 64 bytes r || s (ECDSA) or x(R) || s (BIP-340).
// one_key: `sk` is one row used for every message.  ws: secp_sign_ws_words(n, keys whose point is needed) words of device memory that
// hold secrets afterwards.  pk_mode: 0 compressed (33 bytes), 1 uncompressed (65), 2 x-only (32).
size_t secp_scan_table_words();
void secp_build_scan_table(uint32_t* out_words);
size_t secp_sign_ws_words(int n, int nkeys);
hipError_t secp_public_key_batch(const uint32_t* table, const uint8_t* sk, int pk_mode, uint8_t* out, uint8_t* ok, int n, hipStream_t st);
hipError_t ecdsa_sign_batch(const uint32_t* table, const uint8_t* sk, int one_key, const uint8_t* hash, const uint8_t* extra, int low_s, uint8_t* sig,
                            uint8_t* recid, uint8_t* ok, int n, uint32_t* ws, hipStream_t st);
hipError_t schnorr_sign_batch(const uint32_t* table, const uint8_t* sk, int one_key, const uint8_t* aux, const uint8_t* msgs, const uint64_t* off,
                              uint8_t* sig, uint8_t* ok, int n, uint32_t* ws, hipStream_t st);
// the pieces of secp256k1_sign.hpp on raw words (ncg_secp256k1_sign_check); words per row of each op: secp_sign_check_row_words
// (0 = unknown op); ws: n rows of secp_sign_ws_words(1, 0) words
void secp_sign_check_row_words(int op, int* wa, int* wb, int* wo);
hipError_t secp_sign_check(int op, int variant, const uint32_t* table, uint32_t* ws, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n,
                           hipStream_t st);
int secp_sign_check_host(int op, int variant, const uint32_t* table, const uint32_t* a, const uint32_t* b, uint32_t* out);
void secp_public_key_host(const uint32_t* table, const uint8_t* sk, int pk_mode, uint8_t* out, uint8_t* ok, int n);
void ecdsa_sign_host(const uint32_t* table, const uint8_t* sk, const uint8_t* hash, const uint8_t* extra, int low_s, int refuse_first, uint8_t* sig,
                     uint8_t* recid, uint8_t* ok);
void schnorr_sign_host(const uint32_t* table, const uint8_t* sk, const uint8_t* aux, const uint8_t* msg, uint64_t len, uint8_t* sig, uint8_t* ok);

// X25519 and ed25519.utils.toMontgomery (x25519.hip): rows of 8 LE words (32 bytes) in and out, out_ok = 0 and a zero row where
// the reference throws.  one_scalar: `scalars` is one row used for every item.  x25519_base_batch walks the fixed-base Edwards
// table of ed25519_build_fixed_table; tmp: x25519_base_tmp_words(n) words of device memory.
hipError_t x25519_batch(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st);
size_t x25519_base_tmp_words(int n);
hipError_t x25519_base_batch(const uint32_t* table, const uint32_t* scalars, uint32_t* out, uint8_t* out_ok, int n, uint32_t* tmp,
                             hipStream_t st);
hipError_t ed25519_to_montgomery_batch(const uint32_t* pk, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st);
// the ladder pieces on raw words (ncg_field_check field 16): a 36, b 9, out 36 words per row
hipError_t x25519_field_check(int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st);
void x25519_host(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n);
void x25519_base_host(const uint32_t* scalars, uint32_t* out, uint8_t* out_ok, int n);
void ed25519_to_montgomery_host(const uint32_t* pk, uint32_t* out, uint8_t* out_ok, int n);
int x25519_check_host(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out);

// X448 and Ed448 (ed448.hip).  56-byte rows are 14 LE words; encodings (57 bytes), signatures (114) are packed bytes; affine points
// are x || y, 28 words.  out_ok = 0 and a zero row where the reference throws.  u = NULL (x448_batch) / enc = NULL (ed448_mul_batch):
// the base point.  one_scalar: one row of `scalars` / `k` for every item.
hipError_t x448_batch(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st);
hipError_t ed448_decode_batch(const uint8_t* enc, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st);
hipError_t ed448_encode_batch(const uint32_t* affine, uint8_t* out, int n, hipStream_t st);
hipError_t ed448_add_pairs_batch(const uint32_t* a, const uint32_t* b, int subtract, uint32_t* out, int n, hipStream_t st);
hipError_t ed448_mul_batch(const uint8_t* enc, const uint32_t* k, int one_scalar, uint8_t* out, uint8_t* out_ok, int n, hipStream_t st);
hipError_t ed448_to_montgomery_batch(const uint8_t* pk, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st);
hipError_t ed448_verify_batch(const uint8_t* sig, const uint8_t* pk, const uint32_t* k, uint8_t* out_ok, int n, hipStream_t st);
// the pieces of fe448.hpp / ed448.hpp on raw limbs (ncg_fe448_check); words per row of each op: fe448_check_row_words (0 = unknown op)
void fe448_check_row_words(int op, int* wa, int* wb, int* wo);
hipError_t fe448_check(int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st);
void x448_host(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n);
void ed448_decode_host(const uint8_t* enc, uint32_t* out, uint8_t* out_ok, int n);
void ed448_encode_host(const uint32_t* affine, uint8_t* out, int n);
void ed448_add_pairs_host(const uint32_t* a, const uint32_t* b, int subtract, uint32_t* out, int n);
void ed448_mul_host(const uint8_t* enc, const uint32_t* k, int one_scalar, uint8_t* out, uint8_t* out_ok, int n);
void ed448_to_montgomery_host(const uint8_t* pk, uint32_t* out, uint8_t* out_ok, int n);
void ed448_verify_host(const uint8_t* sig, const uint8_t* pk, const uint32_t* k, uint8_t* out_ok, int n);
int fe448_check_host(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out);

// SHAKE256, Ed448 signing and the challenge of Ed448 verification (ed448_sign.hip).  Seeds are 57 packed bytes; an expanded key is 43
// LE words: scalar (14) || prefix (57 bytes) || A (57 bytes) || 2 zero bytes; signatures are 114 packed bytes, r and k 14 words.
// dom_host is a HOST pointer (at most 265 bytes).  ed448_sign_batch: keys are seeds or expanded rows (`expanded`), one per message or
// ONE for all (`one_key`); ws: ed448_sign_ws_words(n, rows to expand, prehash) words of device memory that hold secrets afterwards.
// ed448_challenge_batch: ws of ed448_challenge_ws_words(n, prehash) words.  ed448_expand_batch: see ed448_sign.hip.
hipError_t shake256_batch(const uint8_t* msgs, const uint64_t* msg_off, uint32_t out_len, uint8_t* out, int n, hipStream_t st);
hipError_t ed448_expand_batch(const uint8_t* seeds, uint32_t* keys, uint8_t* out_a, int out_stride, int n, hipStream_t st);
size_t ed448_sign_ws_words(int n, int nkeys_to_expand, int prehash);
hipError_t ed448_sign_batch(const void* keys, int expanded, int one_key, int prehash, const uint8_t* dom_host, uint32_t dom_len,
                            const uint8_t* msgs, const uint64_t* msg_off, uint8_t* sigs, uint8_t* ok, int n, uint32_t* ws, hipStream_t st);
size_t ed448_challenge_ws_words(int n, int prehash);
hipError_t ed448_challenge_batch(const uint8_t* sigs, const uint8_t* pks, int prehash, const uint8_t* dom_host, uint32_t dom_len,
                                 const uint8_t* msgs, const uint64_t* msg_off, uint32_t* out_k, int n, uint32_t* ws, hipStream_t st);
// the pieces of keccak.hpp / ed448_sign.hpp on raw words (ncg_ed448_sign_check); words per row of each op: ed448_sign_check_row_words
// (0 = unknown op); ws: ed448_sign_check_ws_words() words
void ed448_sign_check_row_words(int op, int* wa, int* wb, int* wo);
size_t ed448_sign_check_ws_words();
hipError_t ed448_sign_check(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, uint32_t* ws, hipStream_t st);
int ed448_sign_check_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out);
void ed448_expand_host(const uint8_t* seeds, uint32_t* keys, int n);
void ed448_sign_host(const void* key, int expanded, int prehash, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg, uint64_t len,
                     const uint32_t* r_in, uint8_t* sig, uint8_t* ok);
void shake256_segments_host(const uint8_t* dom, uint32_t dom_len, const uint8_t* a, uint32_t a_len, const uint8_t* b, uint32_t b_len,
                            const uint8_t* msg, uint64_t len, uint8_t* out, uint32_t out_len);

// decaf448 (decaf448.hip): every row is made of 56-byte values read as 14 LE words: encodings and scalars 14 words, Edwards
// representatives (Ed448 affine points x || y) and uniform input 28.  A refused encoding gives out_ok = 0 and a zero row.
// enc = NULL (decaf448_mul_batch): the decaf base point, out_ok is not written.  one_scalar: one row of `k` for every item.
hipError_t decaf448_decode_batch(const uint32_t* enc, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st);
hipError_t decaf448_encode_batch(const uint32_t* affine, uint32_t* out, int n, hipStream_t st);
hipError_t decaf448_equals_batch(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n, hipStream_t st);
hipError_t decaf448_from_uniform_batch(const uint32_t* uniform, uint32_t* out, int n, hipStream_t st);
hipError_t decaf448_mul_batch(const uint32_t* enc, const uint32_t* k, int one_scalar, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st);
// the pieces of decaf448.hpp on raw limbs (ncg_decaf448_check); words per row of each op: decaf448_check_row_words (0 = unknown op)
void decaf448_check_row_words(int op, int* wa, int* wb, int* wo);
hipError_t decaf448_check(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st);
void decaf448_decode_host(const uint32_t* enc, uint32_t* out, uint8_t* out_ok, int n);
void decaf448_encode_host(const uint32_t* affine, uint32_t* out, int n);
void decaf448_equals_host(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n);
void decaf448_from_uniform_host(const uint32_t* uniform, uint32_t* out, int n);
void decaf448_mul_host(const uint32_t* enc, const uint32_t* k, int one_scalar, uint32_t* out, uint8_t* out_ok, int n);
int decaf448_check_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out);

// ristretto255 (ristretto.hip): encodings and scalars are rows of 8 LE words, Edwards representatives ed25519 wire points (16
// words), uniform input 16 words.  A rejected encoding gives out_ok = 0 and a zero row - or the identity (0, 1) with
// identity_on_reject, for a caller that multiplies what comes out.  ristretto_encode_proj_batch takes the (X, Y, Z) rows of
// ed25519_mul_base_proj (ristretto_proj_words(n) words).  out_affine of ristretto_from_uniform_batch may be null.
hipError_t ristretto_decode_batch(const uint32_t* enc, uint32_t* out_affine, uint8_t* out_ok, int identity_on_reject, int n, hipStream_t st);
hipError_t ristretto_encode_batch(const uint32_t* affine, uint32_t* out, int n, hipStream_t st);
hipError_t ristretto_encode_proj_batch(const uint32_t* proj, uint32_t* out, int n, hipStream_t st);
hipError_t ristretto_equals_batch(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n, hipStream_t st);
hipError_t ristretto_from_uniform_batch(const uint32_t* bytes64, uint32_t* out, uint32_t* out_affine, int n, hipStream_t st);
hipError_t ristretto_broadcast_scalar(const uint32_t* scalar, uint32_t* out, int n, hipStream_t st);
size_t ristretto_proj_words(int n);
// the pieces on raw words (ncg_field_check field 17): a 36, b 9, out 36 words per row
hipError_t ristretto_field_check(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st);
void ristretto_decode_host(const uint32_t* enc, uint32_t* out_affine, uint8_t* out_ok, int identity_on_reject, int n);
void ristretto_encode_host(const uint32_t* affine, uint32_t* out, int n);
void ristretto_encode_proj_host(const uint32_t* proj_wire, uint32_t* out, int n);  // X Y Z as wire words, 24 per row
void ristretto_equals_host(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n);
void ristretto_from_uniform_host(const uint32_t* bytes64, uint32_t* out, uint32_t* out_affine, int n);
void ristretto_mul_host(const uint32_t* enc, const uint32_t* scalars, int one_scalar, uint32_t* out, uint8_t* out_ok, int n);
int ristretto_check_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out);

// ristretto255-SHA512 OPRF (oprf.hip).  Elements and scalars are rows of 8 LE words, outputs 64 packed bytes, messages a blob with
// n + 1 offsets; status: one byte per row (0 ok, 1 undecodable, 2 identity, 3 scalar zero or not below L).  dst_host, info_host and
// B_host are HOST pointers; ws: oprf_ws_bytes(info_len) bytes of device memory laid out as below, which hold a secret (the one
// scalar inverted) after a call with ONE_SCALAR | INVERT.  flags: bit 0 one scalar for every row, bit 1 multiply by its inverse.
constexpr size_t OPRF_PUT_CHUNK = 1024;
constexpr size_t OPRF_WS_DST = 0, OPRF_WS_SDST = 256, OPRF_WS_B = 320, OPRF_WS_SCALAR = 352, OPRF_WS_SEED = 384, OPRF_WS_INFO = 512;
size_t oprf_ws_bytes(size_t info_len);
size_t oprf_dst(const char* prefix, int mode, int with_len, uint8_t* out);  // prefix || "OPRFV1-" || mode || "-ristretto255-SHA512" [|| its length]
hipError_t oprf_put(uint8_t* d_out, const uint8_t* host, size_t len, hipStream_t st);
hipError_t oprf_xmd_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t out_len, uint8_t* out,
                          int n, uint8_t* ws, hipStream_t st);
hipError_t oprf_hash_to_group_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out,
                                    uint32_t* out_affine, int n, uint8_t* ws, hipStream_t st);
hipError_t oprf_hash_to_scalar_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                     uint8_t* ws, hipStream_t st);
hipError_t oprf_blind_batch(int mode, const uint8_t* inputs, const uint64_t* off, const uint32_t* blinds, uint32_t* out, uint8_t* status, int n,
                            uint8_t* ws, hipStream_t st);
hipError_t oprf_mul_batch(const uint32_t* elements, const uint32_t* scalars, int flags, uint32_t* out, uint8_t* status, int n, uint8_t* ws,
                          hipStream_t st);
hipError_t oprf_finalize_batch(int mode, const uint8_t* inputs, const uint64_t* off, const uint8_t* info_host, uint32_t info_len,
                               const uint32_t* blinds, const uint32_t* evaluated, uint8_t* out64, uint8_t* status, int n, uint8_t* ws,
                               hipStream_t st);
hipError_t oprf_evaluate_batch(int mode, const uint8_t* inputs, const uint64_t* off, const uint8_t* info_host, uint32_t info_len,
                               const uint32_t* scalars, int flags, uint8_t* out64, uint8_t* status, int n, uint8_t* ws, hipStream_t st);
hipError_t oprf_composite_batch(int mode, const uint8_t* B_host, const uint32_t* C, const uint32_t* D, uint32_t* out, uint8_t* status, int n,
                                uint8_t* ws, hipStream_t st);
// the proof: Z = k M, t3 = r M and t2 = r B (table: the signing scan table) from M (8 words) and kr = k || r (16 words) into out (24
// words); then, on the host, the challenge of the five encodings B M Z t2 t3 and s = r - c k
hipError_t oprf_proof_points(const uint32_t* table, const uint32_t* M, const uint32_t* kr, uint32_t* out, hipStream_t st);
void oprf_proof_points_host(const uint32_t* table, const uint32_t* M, const uint32_t* kr, uint32_t* out);
int oprf_scalar_ok_host(const uint32_t* k, int allow_zero);
void oprf_challenge_host(int mode, const uint8_t* pts160, uint32_t* c);
void oprf_proof_s_host(const uint32_t* c, const uint32_t* k, const uint32_t* r, uint32_t* s);
// the pieces of oprf.hpp on raw words (ncg_oprf_check); words per row of each op: oprf_check_words (0 = unknown op)
void oprf_check_words(int op, int* wa, int* wb, int* wo);
hipError_t oprf_check(int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st);
int oprf_check_host(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out);
// one row each on the CPU; dst as the caller gave it (the twin appends the length byte)
void oprf_xmd_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out);
void oprf_hash_to_group_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out, uint32_t* out_affine);
void oprf_hash_to_scalar_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out);
uint8_t oprf_blind_host(int mode, const uint8_t* input, uint64_t len, const uint32_t* blind, uint32_t* out);
uint8_t oprf_mul_host(const uint32_t* element, const uint32_t* scalar, int invert, uint32_t* out);
uint8_t oprf_finalize_host(int mode, const uint8_t* input, uint64_t len, const uint8_t* info, uint32_t info_len, const uint32_t* blind,
                           const uint32_t* evaluated, uint8_t* out64);
uint8_t oprf_evaluate_host(int mode, const uint8_t* input, uint64_t len, const uint8_t* info, uint32_t info_len, const uint32_t* scalar,
                           int invert, uint8_t* out64);
void oprf_composite_host(int mode, const uint8_t* B32, const uint32_t* C, const uint32_t* D, uint32_t* out, uint8_t* status, int n);

// RFC 9380 hash-to-curve for secp256k1 and edwards25519 (h2c_suites.hip).  suite: 0 secp256k1_XMD:SHA-256_SSWU, 1
// edwards25519_XMD:SHA-512_ELL2; count: 1 (encodeToCurve, mapToCurve) or 2 (hashToCurve) field elements per row.  Messages are a blob
// with n + 1 offsets; dst_host is a HOST pointer (1..255 bytes); u: n * count elements of in_words words (12: 48 bytes, any value;
// 8: reduced); out: affine wire points of the curve (16 words) and their ZERO flags.  ws: h2c_suites_ws_bytes(suite, n, count) bytes
// of device memory (256 for h2c_xmd_sha256_batch).
size_t h2c_suites_ws_bytes(int suite, size_t n, int count);
hipError_t h2c_suites_map(int suite, const uint32_t* u, int in_words, int count, uint32_t* out, uint8_t* inf, int n, uint8_t* ws,
                          hipStream_t st);
hipError_t h2c_suites_hash_to_field(int suite, const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count,
                                    uint32_t* out_u, int n, uint8_t* ws, hipStream_t st);
hipError_t h2c_suites_hash(int suite, const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count,
                           uint32_t* out, uint8_t* inf, int n, uint8_t* ws, hipStream_t st);
hipError_t h2c_suites_hash_to_scalar(int suite, const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len,
                                     uint32_t* out, int n, uint8_t* ws, hipStream_t st);
hipError_t h2c_xmd_sha256_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t out_len,
                                uint8_t* out, int n, uint8_t* ws, hipStream_t st);
// the pieces of h2c_suites.hpp on raw words (ncg_h2c_check): 24 words per row of a and out; an unknown op writes nothing
hipError_t h2c_check(int op, const uint32_t* d_a, uint32_t* d_out, int n, hipStream_t st);
// one row each on the CPU; dst as the caller gave it (the twin appends the length byte); -1 for an unknown suite or op
void h2c_xmd_sha256_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out);
int h2c_hash_to_field_host(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out_u);
int h2c_hash_to_scalar_host(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out8);
int h2c_map_host(int suite, const uint32_t* u, int in_words, int count, uint32_t* out, uint8_t* inf);
int h2c_hash_host(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out, uint8_t* inf);
int h2c_check_host(int op, const uint32_t* a, uint32_t* out);

// RFC 9380 for edwards448 (edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_) and the hash side of decaf448 (h2c448.hip).  Messages are a blob with
// n + 1 offsets; dst_host is a HOST pointer (1..255 bytes); elements, scalars and encodings are 14 LE words, affine points x || y 28.
// ws: h2c448_ws_bytes(n) bytes of device memory (512 for h2c448_xof_batch); h2c448_map needs none.
size_t h2c448_ws_bytes(size_t n);
hipError_t h2c448_xof_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t out_len, uint8_t* out,
                            int n, uint8_t* ws, hipStream_t st);
hipError_t h2c448_hash_to_field(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count, uint32_t* out_u,
                                int n, uint8_t* ws, hipStream_t st);
hipError_t h2c448_map(const uint32_t* u, int count, uint32_t* out, int n, hipStream_t st);
hipError_t h2c448_hash(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count, uint32_t* out, int n,
                       uint8_t* ws, hipStream_t st);
hipError_t h2c448_hash_to_scalar(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                 uint8_t* ws, hipStream_t st);
hipError_t decaf448_hash_to_group(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                  uint8_t* ws, hipStream_t st);
hipError_t decaf448_hash_to_scalar(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                   uint8_t* ws, hipStream_t st);
// the pieces of h2c448.hpp on raw words (ncg_h2c448_check): 42 words per row of a and out; an unknown op writes nothing
hipError_t h2c448_check(int op, const uint32_t* d_a, uint32_t* d_out, int n, hipStream_t st);
// one row each on the CPU; dst as the caller gave it
void h2c448_xof_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out);
void h2c448_hash_to_field_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out_u);
void h2c448_hash_to_scalar_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14);
void h2c448_map_host(const uint32_t* u, int count, uint32_t* out28);
void h2c448_hash_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out28);
void decaf448_hash_to_group_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14);
void decaf448_hash_to_scalar_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14);
int h2c448_check_host(int op, const uint32_t* a, uint32_t* out);

// bls12-381 pairings (pairing.hip).  ws: PAIRING_WS_WORDS words per pair; off: n_groups + 1 ascending pair offsets (device);
// first_bad: one 64-bit word, all ones or (index << 8 | PairingBad code) of the first refused pair after pairing_miller;
// pairing_finish multiplies each group's Miller values (largest_group decides the number of passes), exponentiates and stores
// 144 canonical wire words per group (out_gt may be null) and the is_one bytes.  fp12_batch: the Fp12 ops of ncg_fp12_batch.
constexpr size_t PAIRING_WS_WORDS = 168;
hipError_t pairing_miller(const uint32_t* g1, const uint32_t* g2, int subgroup, uint32_t* ws, unsigned long long* first_bad, int n, hipStream_t st);
hipError_t pairing_finish(uint32_t* ws, const uint32_t* off, int n_groups, int n, uint32_t largest_group, uint32_t* out_gt,
                          uint8_t* out_is_one, hipStream_t st);
hipError_t fp12_batch(int op, const uint32_t* a, const uint32_t* b, void* out, int n, hipStream_t st);
void fp12_op_host(int op, const uint32_t* a, const uint32_t* b, void* out, int n, bool raw = false);  // raw: a as 168 stored words
int64_t pairing_host(const uint32_t* g1, const uint32_t* g2, int n, const uint32_t* off, int n_groups, int subgroup, uint32_t* out_gt,
                     uint8_t* out_is_one, uint32_t* bad_code);
// BLS verification rows (pairing.hip): two pairs per row from decoded keys / signatures and mapped messages; bad[i] = 1 and generator
// pairs where a key or signature did not decode or any of the three points is ZERO; out_ok = is_one && !bad
hipError_t bls_build_pairs(int scheme, const uint32_t* pk, const uint8_t* pk_ok, const uint8_t* pk_inf, const uint32_t* sig,
                           const uint8_t* sig_ok, const uint8_t* sig_inf, const uint32_t* hm, const uint8_t* hm_inf, uint32_t* g1,
                           uint32_t* g2, uint8_t* bad, int n, hipStream_t st);
hipError_t bls_verdict(const uint8_t* is_one, const uint8_t* bad, uint8_t* out_ok, int n, hipStream_t st);

// field-level self-check (selfcheck.hip; the fields and their row widths: selfcheck.hpp): out[i] = op(a[i], b[i]) on the device
// field code
hipError_t field_check_run(int field, int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n,
                           hipStream_t st);
// instruction-rate and field-multiply micro-benchmarks (ubench.hip)
hipError_t ubench_run(int kind, int blocks, int threads, int iters, uint32_t* d_out, const uint32_t* d_in,
                      hipStream_t st, float* ms);

}  // namespace ncg
