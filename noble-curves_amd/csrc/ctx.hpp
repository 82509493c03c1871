// Internal: the context behind the opaque ncg_ctx of include/ncg.h, shared by the translation units
// that implement the C ABI (api.hip, comm.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ncg.h"
#include "host_api.hpp"
#include "msm.hpp"

// One MSM in flight of the asynchronous entry points (ncg_msm_async_submit / _collect): its own stream, workspace,
// gather buffer and pinned landing area, so that the dependent tail of one MSM (narrow fold levels, per-window tail,
// D2H, host Horner) overlaps the sort / accumulate kernels of the next.
constexpr int NCG_MSM_LANES = 4;
struct ncg_msm_lane {
  hipStream_t stream = nullptr;
  ncg::MsmSide side;
  hipEvent_t done = nullptr, input_ready = nullptr;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  uint32_t* land = nullptr;  // pinned host memory
  size_t land_words = 0;
  void* comm_buf = nullptr;  // window-sharded mode: the slots of all ranks (device)
  size_t comm_buf_bytes = 0;
  bool busy = false, state_identity = false, part_only = false;
  int curve = 0, mode = 0, nparts = 1, c = 0, nwin = 0;  // what collect needs to know about the enqueued job
  size_t stride = 0;
};

struct ncg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string last_error;
  // reusable device scratch for the host-pointer entry points
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  void* mul_ws = nullptr;  // batch-multiply Jacobian scratch (device)
  size_t mul_ws_bytes = 0;
  void* msm_ws = nullptr;  // MSM workspace (device)
  size_t msm_ws_bytes = 0;
  int msm_seg_override = 0, msm_run_serial_override = -1;  // ncg_msm_set_tuning
  ncg::MsmTrace msm_trace;                                  // what the last MSM launch used (ncg_msm_last_plan)
  ncg_msm_lane lanes[NCG_MSM_LANES];                        // asynchronous MSMs in flight
  ncg::MsmSide msm_side;   // second stream + fork / join events of the MSM (msm.hip)
  uint32_t* ed_btab = nullptr;  // ed25519 base-point table (device)
  void* ed_ks = nullptr;        // ed25519 challenge scalars of the message-taking verify (device)
  size_t ed_ks_bytes = 0;
  // ed25519 signing (ed25519_sign.hip): the 4-bit window table of B, and the workspace of one call (dom, nonces, prehashes, expanded
  // keys) - it holds secrets during a call and is cleared on the call's stream before the call returns
  uint32_t* ed_scan_tab = nullptr;
  void* ed_sign_ws = nullptr;
  size_t ed_sign_ws_bytes = 0;
  // secp256k1 signing (secp256k1_sign.hip): the 4-bit window table of G with the hash constants behind it, and the workspace of one
  // call (keys, nonces, DRBG state, staged hashes) - it holds secrets during a call and is cleared on the call's stream before the
  // call returns
  uint32_t* secp_scan_tab = nullptr;
  void* secp_sign_ws = nullptr;
  size_t secp_sign_ws_bytes = 0;
  // Ed448 signing and the message-taking verify (ed448_sign.hip): the workspace of one call (dom, nonces or challenges, prehashes,
  // expanded keys) - it holds secrets during a signing call and is cleared on the call's stream before the call returns
  void* ed448_ws = nullptr;
  size_t ed448_ws_bytes = 0;
  void* ecdsa_ws = nullptr;     // ECDSA batch verify: decoded keys, u1 / u2, partial points (device)
  size_t ecdsa_ws_bytes = 0;
  uint32_t* base_tab[4] = {nullptr, nullptr, nullptr, nullptr};  // fixed-base tables per curve (device)
  uint32_t* ub_in = nullptr;
  uint32_t* ub_out = nullptr;
  size_t ub_out_bytes = 0;
  // NTT: one twiddle table per (field, transform size) (device), keyed by the root it was built from;
  // field slot 0 = bls12-381 Fr, 1 = bn254 Fr
  uint32_t* ntt_tab[2][NCG_NTT_MAX_LOG2N + 1] = {};
  uint32_t ntt_omega[2][NCG_NTT_MAX_LOG2N + 1][8] = {};
  void* ntt_ws = nullptr;
  size_t ntt_ws_bytes = 0;
  // polynomial operations (poly.hip): partial sums, the root-index word and the 2 N transform buffer of a product; like ntt_ws it
  // serves one call at a time
  void* poly_ws = nullptr;
  size_t poly_ws_bytes = 0;
  // ristretto255 (ristretto.hip): what lies between a decode and an encode - the decoded points, their flags, the products,
  // the (X, Y, Z) rows of the fixed-base walk, a broadcast scalar; one call at a time
  void* rist_ws = nullptr;
  size_t rist_ws_bytes = 0;
  // OPRF (oprf.hip): the strings of a call (DST', "Seed-" || ctx, info), the seed of the composites, the one scalar inverted, and the
  // rows of the proof calls - it holds secrets during a call and is cleared on the call's stream before the call returns
  void* oprf_ws = nullptr;
  size_t oprf_ws_bytes = 0;
  // RFC 9380 suites for secp256k1 and edwards25519 (h2c_suites.hip): DST', the uniform bytes, the reduced elements and the mapped points
  // of one call: one call at a time per context, on whatever stream.  The edwards448 / decaf448 suites (h2c448.hip) keep their staged
  // DST, uniform bytes and reduced elements here as well, under the same rule
  void* h2c_ws = nullptr;
  size_t h2c_ws_bytes = 0;
  // pairings (pairing.hip): the verdict word, the group offsets and one Miller value per pair; one call at a time
  void* pair_ws = nullptr;
  size_t pair_ws_bytes = 0;
  // BLS verification (ncg_bls_verify_batch): decoded keys and signatures, mapped messages, their flags and the two pairs per row
  void* bls_ws = nullptr;
  size_t bls_ws_bytes = 0;
  // multi-GPU (comm.hip): RCCL communicator of this rank and the gather buffer of the sharded MSM
  void* comm = nullptr;  // ncclComm_t
  int comm_rank = 0, comm_size = 1;
  void* comm_buf = nullptr;
  size_t comm_buf_bytes = 0;
  // host-pointer entry points (ncg_msm, ncg_mul_var_batch): copy streams and per-chunk events, so that the chunks of a
  // large host buffer cross PCIe while the kernels of earlier chunks (or the digit / sort kernels of the MSM) run
  static constexpr int COPY_CHUNKS = 8;
  hipStream_t copy_in = nullptr, copy_out = nullptr;
  hipEvent_t ev_in[COPY_CHUNKS] = {}, ev_k[COPY_CHUNKS] = {}, ev_sc[COPY_CHUNKS] = {}, ev_ready = nullptr;
  hipStream_t comm_stream = nullptr;  // the one stream every collective of the asynchronous lanes is enqueued on
  hipEvent_t comm_fork = nullptr, comm_join = nullptr;
  uint32_t* sync_land = nullptr;  // pinned landing area of the synchronous sharded entry points
  size_t sync_land_words = 0;
};


// ---- resident point sets (api.hip): upload once, multiply many (interleavedMSMUnsafe's usage pattern,
// src/abstract/curve.ts:907-959; SURVEY 8a gotcha 8: marshalling dominates an end-to-end call)
struct ncg_points {
  ncg_ctx* ctx;
  int curve;
  size_t n;
  void* d_pts;
  void* d_endo = nullptr;  // endomorphism images (msm_endo_expand) once the set is known to lie in the subgroup
  void* d_stored = nullptr;  // the points in the accumulate kernel's storage format (built at the first generic MSM)
  // window-shifted copies for the shared-bucket MSM (ncg_points_precompute, msm_precomp.hip): shift_nwin levels of
  // shift_m stored points; shift_mode 1 = levels of the points themselves, 2 = of the endomorphism images
  void* d_shift = nullptr;
  int shift_c = 0, shift_nwin = 0, shift_mode = 0;
  size_t shift_m = 0;
};

// which window plan and which device point array an MSM on a resident set uses (api.hip)
int ncg_resident_plan(ncg_ctx* ctx, const ncg_points* pts, ncg::MsmPlan* pl, const uint32_t** d_pts, hipStream_t st);
// whole plan for n points restricted to windows [w0, w0 + cnt), workspace grown as needed (ws / ws_bytes NULL: the context's own)
int ncg_msm_plan_ws_windows(ncg_ctx* ctx, int curve, size_t n, int w0, int cnt, ncg::MsmPlan* pl, void** ws, size_t* ws_bytes);
// tuning overrides + trace slot of the context into a plan, workspace (any of the context's) grown as needed
int ncg_msm_ensure_buf(ncg_ctx* ctx, int curve, ncg::MsmPlan& pl, void** ws, size_t* ws_bytes);

// records the message (per context and globally) and returns `code`
int ncg_set_err(ncg_ctx* ctx, int code, const char* fmt, ...);
#define set_err ncg_set_err

int ncg_msm_plan_ws(ncg_ctx* ctx, int curve, size_t n, int c_override, ncg::MsmPlan* pl);

// Grows a device buffer of the context to hold `need` bytes, allocating `alloc` >= need (its headroom); what it held is
// lost.  Each buffer keeps the policy it has always had: what is waited for before the old buffer is freed (`st`, or the
// whole device for a buffer that any stream may still be reading - only when there is an old buffer), and whether the
// fresh memory is cleared on `st`.  A failed allocation leaves the buffer empty and returns NCG_ERR_NOMEM.
enum class GrowWait { none, stream, device };
int ncg_grow_buf(ncg_ctx* ctx, void** p, size_t* have, size_t need, size_t alloc, GrowWait wait = GrowWait::none,
                 hipStream_t st = nullptr, bool zero = false);

// device buffers are read with 16-byte accesses (ncg.h "Conventions"): refuse a misaligned pointer instead of faulting
inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15u) != 0; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

#define NCG_HIP(ctx, expr)                                                                   \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return set_err(ctx, NCG_ERR_HIP, "noble-gpu: HIP error %d (%s) at %s:%d", (int)_e,    \
                     hipGetErrorString(_e), __FILE__, __LINE__);                             \
  } while (0)

