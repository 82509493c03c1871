// C ABI (include/ncg.h): context, workspace and dispatch.  No torch types cross here.
#include <hip/hip_runtime.h>
#include "knobs.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ncg.h"
#include "host_api.hpp"
#include "consts_gen.hpp"
#include "msm.hpp"
#include "selfcheck.hpp"

namespace {
std::mutex g_err_mu;
std::string g_last_error;
}  // namespace

#include "ctx.hpp"

int ncg_set_err(ncg_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  {
    std::lock_guard<std::mutex> g(g_err_mu);
    g_last_error = buf;
  }
  if (ctx) ctx->last_error = buf;
  return code;
}

// Host <-> device copies of the host-pointer entry points.  Pageable user buffers move at a few
// GB/s through the runtime's staging path; registering (pinning) a large buffer for the duration of
// the call lets the DMA engines read/write it directly at PCIe speed.  Everything registered here is
// released when the object goes out of scope, after the stream has been drained.
struct PinSet {
  ncg_ctx* ctx;
  struct Range { uintptr_t lo, hi; };
  Range regs[24];
  int n = 0;
  explicit PinSet(ncg_ctx* c) : ctx(c) {}
  // Page-locks [p, p + bytes) for the duration of the call.  A copy must lie inside ONE registration, and two registrations
  // must not share a page: callers that pin an array piecewise cut it at page boundaries (PagedParts below).
  // Buffers the caller registered itself (ncg_host_register) fail here and are left alone.
  // (The EXACT range is registered, not its pages: the runtime treats a pointer as pinned by the registered range, and a range
  // widened to its pages would claim the head of whatever the caller allocated next to the buffer - a copy into that neighbour
  // would then start inside a registration and run out of it: hipErrorInvalidValue.)
  void pin(const void* p, size_t bytes) {
    if (bytes < ((size_t)1 << 20) || n >= 24) return;
    {  // already pinned (ncg_host_register, hipHostMalloc): a second registration of a PIECE of it would succeed and cost the
       // page locking again - ask first
      // (both ends: a buffer registered only as a PREFIX of this piece is not "already pinned" - it is left to the plain copy,
      // which reports the partial registration instead of a DMA running past it)
      hipPointerAttribute_t at;
      if (hipPointerGetAttributes(&at, p) == hipSuccess) {
        if (at.type == hipMemoryTypeHost) return;
      } else {
        (void)hipGetLastError();  // plain pageable memory is "invalid value" to this query on some runtimes
      }
      if (hipPointerGetAttributes(&at, (const char*)p + bytes - 1) == hipSuccess) {
        if (at.type == hipMemoryTypeHost) return;   // the tail belongs to someone's registration: registering the range would overlap it
      } else {
        (void)hipGetLastError();
      }
    }
    if (hipHostRegister((void*)p, bytes, hipHostRegisterDefault) == hipSuccess) regs[n++] = Range{(uintptr_t)p, (uintptr_t)p + bytes};
    else (void)hipGetLastError();  // not registrable: plain copy
  }
  hipError_t h2d(void* dst, const void* src, size_t bytes) {
    pin(src, bytes);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream);
  }
  hipError_t d2h(void* dst, const void* src, size_t bytes) {
    pin(dst, bytes);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
  }
  ~PinSet() {
    if (n) {  // nothing may still be reading or writing the buffers when they are unpinned - on ANY path out of the caller
      (void)hipStreamSynchronize(ctx->stream);
      if (ctx->copy_in) (void)hipStreamSynchronize(ctx->copy_in);
      if (ctx->copy_out) (void)hipStreamSynchronize(ctx->copy_out);
    }
    for (int i = 0; i < n; i++) (void)hipHostUnregister((void*)regs[i].lo);
  }
};

// One host array crossing the bus piecewise: consecutive byte ranges whose INNER boundaries are page boundaries of the host
// address space, so that each piece can be page-locked on its own just before its copy is enqueued (the host locks piece p + 1
// while piece p is on the bus; locking 128 MB up front costs ~3 ms before the first byte moves) and no two registrations share a
// page.  Uploads round a piece's end UP (a few bytes of the next piece travel early); downloads round it DOWN (the last partial
// page of a piece is fetched with the next one, when all of it has been computed).
struct PagedParts {
  const char* base;
  size_t total, done = 0;
  PagedParts(const void* b, size_t t) : base((const char*)b), total(t) {}
  // piece that makes bytes [0, need_end) available (upload) / that may fetch everything below need_end (download)
  bool next(size_t need_end, bool last, bool round_up, size_t* lo, size_t* hi) {
    const uintptr_t a = (uintptr_t)base + need_end;
    size_t e = last ? total : (size_t)(((round_up ? a + 4095 : a) & ~(uintptr_t)4095) - (uintptr_t)base);
    if (!last && (a & ~(uintptr_t)4095) < (uintptr_t)base) e = 0;   // (download, first page before the array)
    e = std::min(e, total);
    if (e <= done) return false;
    *lo = done;
    *hi = e;
    done = e;
    return true;
  }
};

int ncg_grow_buf(ncg_ctx* ctx, void** p, size_t* have, size_t need, size_t alloc, GrowWait wait, hipStream_t st, bool zero) {
  if (*have >= need) return NCG_OK;
  if (wait == GrowWait::stream) NCG_HIP(ctx, hipStreamSynchronize(st));
  if (wait == GrowWait::device && *p) NCG_HIP(ctx, hipDeviceSynchronize());
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  hipError_t e = hipMalloc(p, alloc);
  if (e != hipSuccess) return set_err(ctx, NCG_ERR_NOMEM, "noble-gpu: hipMalloc(%zu) failed: %s", alloc, hipGetErrorString(e));
  *have = alloc;
  if (zero) NCG_HIP(ctx, hipMemsetAsync(*p, 0, alloc, st));
  return NCG_OK;
}

static int ensure_scratch(ncg_ctx* ctx, size_t bytes) {
  return ncg_grow_buf(ctx, &ctx->scratch, &ctx->scratch_bytes, bytes, bytes + (bytes >> 2) + 4096);
}

// One host-pointer call staged through ctx->scratch.  The caller declares its slots - in(): uploaded; out(): copied back
// unless its host pointer is NULL, optionally zero-filled first; inout(): both, in place; dev_only(): device memory only -
// then stage() grows the scratch once, lays the slots out at 256-byte boundaries and enqueues the uploads on ctx->stream,
// and finish() takes the status of the _dev call, copies the outputs back and synchronises.  Once stage() has enqueued
// anything, every exit waits for ctx->stream (the destructor), so the host memory handed to in() - temporaries included -
// must be declared BEFORE the HostCall.
// The slots live in ctx->scratch: a _dev form called from a host wrapper must never use ctx->scratch itself.
// (The chunked pipelines of ncg_mul_var_batch / ncg_msm lay out the scratch on their own.)
struct HostCall {
  struct Slot {
    const void* in;
    void* out;
    size_t bytes, off;
    bool zero;
  };
  ncg_ctx* ctx;
  PinSet pins;
  std::vector<Slot> slots;
  bool enqueued = false;
  explicit HostCall(ncg_ctx* c) : ctx(c), pins(c) {}
  ~HostCall() {
    if (enqueued) (void)hipStreamSynchronize(ctx->stream);
  }
  int in(const void* host, size_t bytes) { return add(host, nullptr, bytes, false); }
  int out(void* host, size_t bytes, bool zero = false) { return add(nullptr, host, bytes, zero); }
  int inout(const void* in_host, void* out_host, size_t bytes) { return add(in_host, out_host, bytes, false); }
  int dev_only(size_t bytes) { return add(nullptr, nullptr, bytes, false); }
  template <class T = void>
  T* dev(int i) const { return (T*)((char*)ctx->scratch + slots[i].off); }
  int stage() {
    size_t total = 0;
    for (Slot& s : slots) {
      s.off = total;
      total += align256(s.bytes);
    }
    if (int rc = ensure_scratch(ctx, total)) return rc;
    enqueued = true;
    for (const Slot& s : slots) {
      if (s.in && s.bytes) NCG_HIP(ctx, pins.h2d((char*)ctx->scratch + s.off, s.in, s.bytes));
      if (s.zero) NCG_HIP(ctx, hipMemsetAsync((char*)ctx->scratch + s.off, 0, s.bytes, ctx->stream));
    }
    return NCG_OK;
  }
  int finish(int rc) {
    if (rc) return rc;
    for (const Slot& s : slots)
      if (s.out && s.bytes) NCG_HIP(ctx, pins.d2h(s.out, (char*)ctx->scratch + s.off, s.bytes));
    NCG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    enqueued = false;
    return NCG_OK;
  }

 private:
  int add(const void* in, void* out, size_t bytes, bool zero) {
    slots.push_back(Slot{in, out, bytes, 0, zero});
    return (int)slots.size() - 1;
  }
};

// ---- What each operation accepts - its curves or field and its own argument rules - written once and checked by its host
// and _dev forms alike through NCG_BEGIN.  `rc` is NCG_OK or the status already recorded; `op` names the operation in the
// messages of the prologue.
struct Rule {
  const char* op;
  int rc;
};
static Rule curve_rule(ncg_ctx* ctx, const char* op, int curve, bool ok) {
  return {op, ok ? NCG_OK : set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: %s: unsupported curve %d", op, curve)};
}
static Rule mul_var_rule(ncg_ctx* ctx, int curve) { return curve_rule(ctx, "mul_var_batch", curve, ncg_point_bytes(curve) != 0); }
static Rule add_pairs_rule(ncg_ctx* ctx, int curve) { return curve_rule(ctx, "add_pairs_batch", curve, ncg_point_bytes(curve) != 0); }
static Rule mul_base_rule(ncg_ctx* ctx, int curve) {  // no fixed-base table for bn254 G1
  return curve_rule(ctx, "mul_base_batch", curve, ncg_point_bytes(curve) != 0 && curve != NCG_BN254_G1);
}
static Rule normalize_rule(ncg_ctx* ctx, int curve) { return curve_rule(ctx, "normalize_batch", curve, ncg_point_bytes(curve) != 0); }
static Rule msm_rule(ncg_ctx* ctx, int curve) { return curve_rule(ctx, "msm", curve, ncg_point_bytes(curve) != 0); }
// the curves with a wire encoding (decode, encode and everything that takes encoded points)
static Rule encoded_rule(ncg_ctx* ctx, const char* op, int curve) { return curve_rule(ctx, op, curve, ncg::decode_in_bytes(curve) != 0); }
static Rule map_rule(ncg_ctx* ctx, int curve, int count) {
  Rule r = curve_rule(ctx, "map_to_curve_batch", curve, curve == NCG_BLS12_381_G1 || curve == NCG_BLS12_381_G2);
  if (r.rc == NCG_OK && count != 1 && count != 2)
    r.rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: map_to_curve_batch: count must be 1 or 2");
  return r;
}
static Rule secp_rule(ncg_ctx* ctx, const char* op, int curve) {
  return {op, curve == NCG_SECP256K1 ? NCG_OK : set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: %s: secp256k1 only", op)};
}
static Rule ntt_rule(ncg_ctx* ctx, int field, int log2n, size_t batch) {
  int rc = NCG_OK;
  if (field != NCG_FIELD_BLS12_381_FR && field != NCG_FIELD_BN254_FR) rc = set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: ntt: unsupported field %d", field);
  else if (log2n < 0 || log2n > NCG_NTT_MAX_LOG2N)
    rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ntt: log2n %d out of range 0..%d", log2n, NCG_NTT_MAX_LOG2N);
  else if (batch > 65535) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ntt: batch %zu too large (max 65535)", batch);
  return {"ntt", rc};
}
// the polynomial operations share one rule; `kind` names the entry point, the arguments an entry point does not have are passed as
// values that pass (op 0, log2n 0, m 1, na = nb = 0)
enum { POLY_POINTWISE, POLY_SCALE, POLY_EVAL, POLY_EVAL_MONOMIAL, POLY_LAGRANGE, POLY_MUL };
static Rule poly_rule(ncg_ctx* ctx, int kind, int field, int op, int log2n, int m, size_t na, size_t nb) {
  static const char* const names[] = {"poly_pointwise", "poly_scale", "poly_eval", "poly_eval_monomial", "poly_lagrange_basis", "poly_mul"};
  int rc = NCG_OK;
  if (field != NCG_FIELD_BLS12_381_FR && field != NCG_FIELD_BN254_FR) rc = set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: poly: unsupported field %d", field);
  else if (kind == POLY_POINTWISE && (op < NCG_POLY_ADD || op > NCG_POLY_DOT)) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly: unknown op %d", op);
  else if (kind == POLY_SCALE && op != 0 && op != 1) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly: powers must be 0 or 1, got %d", op);
  else if (log2n < 0 || log2n > NCG_NTT_MAX_LOG2N)
    rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly: log2n %d out of range 0..%d", log2n, NCG_NTT_MAX_LOG2N);
  else if (m < 1 || m > NCG_POLY_MAX_POINTS) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly: m %d out of range 1..%d", m, NCG_POLY_MAX_POINTS);
  else if (na > ((size_t)1 << log2n) || nb > ((size_t)1 << log2n))
    rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly: %zu and %zu coefficients do not fit the length 2^%d", na, nb, log2n);
  return {names[kind], rc};
}
static Rule no_rule(const char* op) { return {op, NCG_OK}; }  // nothing to check beyond the prologue
static Rule handle_rule(ncg_ctx* ctx, const char* op, const ncg_points* pts) {
  return {op, pts && pts->ctx == ctx ? NCG_OK
                                     : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: handle does not belong to this context", op)};
}

// the batch limit and the buffers the calling form requires, then the device
static int batch_args(ncg_ctx* ctx, const char* op, size_t n, std::initializer_list<const void*> bufs) {
  if (n > 0x7fffffffu) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: batch too large", op);
  for (const void* p : bufs)
    if (!p) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: NULL buffer", op);
  NCG_HIP(ctx, hipSetDevice(ctx->device));
  return NCG_OK;
}
// The prologue of every batch entry point, in this order: the context, the operation's rule, the empty batch (`if_empty`,
// before any buffer is looked at), the batch limit, the buffers this form requires (`...`), hipSetDevice.
#define NCG_BEGIN_OR(ctx, rule, n, if_empty, ...)                                     \
  do {                                                                                \
    if (!(ctx)) return set_err(nullptr, NCG_ERR_INVALID_ARG, "noble-gpu: ctx is NULL"); \
    const Rule r_ = (rule);                                                           \
    if (r_.rc) return r_.rc;                                                          \
    if ((n) == 0) return (if_empty);                                                  \
    if (const int rc_ = batch_args(ctx, r_.op, n, {__VA_ARGS__})) return rc_;         \
  } while (0)
#define NCG_BEGIN(ctx, rule, n, ...) NCG_BEGIN_OR(ctx, rule, n, NCG_OK, __VA_ARGS__)

static hipStream_t stream_of(ncg_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }

// An empty MSM is the identity (reference curve.ts:878): written, not refused, so the output is required even then.
static int msm_identity(ncg_ctx* ctx, int curve, void* out_affine, uint8_t* out_is_inf) {
  if (!out_affine) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: NULL output");
  memset(out_affine, 0, ncg_point_bytes(curve));
  if (curve == NCG_ED25519) ((uint8_t*)out_affine)[32] = 1;  // Edwards identity is (0, 1)
  if (out_is_inf) *out_is_inf = 1;
  return NCG_OK;
}

// window plan for an n-point MSM (c_override > 0 fixes the window width) and a workspace big enough for it
static int msm_ensure_ws(ncg_ctx* ctx, int curve, ncg::MsmPlan& pl);
int ncg_msm_plan_ws(ncg_ctx* ctx, int curve, size_t n, int c_override, ncg::MsmPlan* pl) {
  if (ncg::msm_make_plan(curve, (int)n, c_override, pl) != 0)
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: cannot plan windows");
  return msm_ensure_ws(ctx, curve, *pl);
}
// the context's tuning overrides and trace slot go into the plan (every MSM entry point passes through here or
// through ncg_msm_ensure_buf), then the workspace grows if the plan needs more
static void msm_apply_ctx(ncg_ctx* ctx, ncg::MsmPlan& pl) {
  pl.seg_override = ctx->msm_seg_override;
  pl.run_serial_override = ctx->msm_run_serial_override;
  pl.trace = &ctx->msm_trace;
}
int ncg_msm_ensure_buf(ncg_ctx* ctx, int curve, ncg::MsmPlan& pl, void** ws, size_t* ws_bytes) {
  msm_apply_ctx(ctx, pl);
  const size_t need = ncg::msm_workspace_bytes(curve, pl);
  // ncg_msm_last_plan reads the long-run counter of the last MSM out of ITS workspace: forget the pointer when that
  // workspace is the one being replaced (the trace then reports 0 runs instead of reading freed memory)
  const char* lr = (const char*)ctx->msm_trace.d_long_runs;
  if (*ws_bytes < need && *ws && lr && lr >= (const char*)*ws && lr < (const char*)*ws + *ws_bytes) ctx->msm_trace.d_long_runs = nullptr;
  return ncg_grow_buf(ctx, ws, ws_bytes, need, need);
}
static int msm_ensure_ws(ncg_ctx* ctx, int curve, ncg::MsmPlan& pl) { return ncg_msm_ensure_buf(ctx, curve, pl, &ctx->msm_ws, &ctx->msm_ws_bytes); }
int ncg_msm_plan_ws_windows(ncg_ctx* ctx, int curve, size_t n, int w0, int cnt, ncg::MsmPlan* pl, void** ws, size_t* ws_bytes) {
  if (ncg::msm_make_plan(curve, (int)n, 0, pl) != 0)
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: cannot plan windows");
  if (w0 < 0 || cnt < 0 || w0 + cnt > pl->nwin) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: window range outside the plan");
  ncg::msm_plan_take_windows(*pl, w0, cnt);
  return ncg_msm_ensure_buf(ctx, curve, *pl, ws ? ws : &ctx->msm_ws, ws_bytes ? ws_bytes : &ctx->msm_ws_bytes);
}

// only the C ABI of include/ncg.h is exported (the objects are built with -fvisibility=hidden)
#pragma GCC visibility push(default)
extern "C" {

const char* ncg_version(void) { return "noble-curves-amd 0.1 (gfx950)"; }

int ncg_point_bytes(int curve) {
  switch (curve) {
    case NCG_SECP256K1: return 64;
    case NCG_ED25519: return 64;
    case NCG_BLS12_381_G1: return 96;
    case NCG_BLS12_381_G2: return 192;
    case NCG_BN254_G1: return 64;
    default: return 0;
  }
}
int ncg_field_bytes(int curve) { return ncg_point_bytes(curve) / 2; }

int ncg_init(int device_id, ncg_ctx** out_ctx) {
  if (!out_ctx) return set_err(nullptr, NCG_ERR_INVALID_ARG, "noble-gpu: out_ctx is NULL");
  *out_ctx = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return set_err(nullptr, NCG_ERR_NO_DEVICE, "noble-gpu: no HIP device visible (%s)", hipGetErrorString(e));
  if (device_id < 0 || device_id >= count)
    return set_err(nullptr, NCG_ERR_INVALID_ARG, "noble-gpu: device %d out of range (have %d)", device_id, count);
  ncg_ctx* ctx = new ncg_ctx();
  ctx->device = device_id;
  e = hipSetDevice(device_id);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->msm_side.stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->msm_side.fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->msm_side.join, hipEventDisableTiming);
  if (e != hipSuccess) {
    int rc = set_err(nullptr, NCG_ERR_HIP, "noble-gpu: cannot create stream on device %d: %s", device_id, hipGetErrorString(e));
    ncg_destroy(ctx);  // releases whichever streams / events were created before the failure
    return rc;
  }
  *out_ctx = ctx;
  return NCG_OK;
}

void ncg_destroy(ncg_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->msm_ws) (void)hipFree(ctx->msm_ws);
  if (ctx->mul_ws) (void)hipFree(ctx->mul_ws);
  if (ctx->ed_btab) (void)hipFree(ctx->ed_btab);
  if (ctx->ed_ks) (void)hipFree(ctx->ed_ks);
  if (ctx->ed_scan_tab) (void)hipFree(ctx->ed_scan_tab);
  if (ctx->ed_sign_ws) (void)hipFree(ctx->ed_sign_ws);
  if (ctx->secp_scan_tab) (void)hipFree(ctx->secp_scan_tab);
  if (ctx->secp_sign_ws) (void)hipFree(ctx->secp_sign_ws);
  if (ctx->ed448_ws) (void)hipFree(ctx->ed448_ws);
  if (ctx->ecdsa_ws) (void)hipFree(ctx->ecdsa_ws);
  for (int i = 0; i < 4; i++)
    if (ctx->base_tab[i]) (void)hipFree(ctx->base_tab[i]);
  if (ctx->ub_in) (void)hipFree(ctx->ub_in);
  if (ctx->ub_out) (void)hipFree(ctx->ub_out);
  for (int f = 0; f < 2; f++)
    for (int i = 0; i <= NCG_NTT_MAX_LOG2N; i++)
      if (ctx->ntt_tab[f][i]) (void)hipFree(ctx->ntt_tab[f][i]);
  if (ctx->ntt_ws) (void)hipFree(ctx->ntt_ws);
  if (ctx->poly_ws) (void)hipFree(ctx->poly_ws);
  if (ctx->rist_ws) (void)hipFree(ctx->rist_ws);
  if (ctx->oprf_ws) (void)hipFree(ctx->oprf_ws);
  if (ctx->h2c_ws) (void)hipFree(ctx->h2c_ws);
  if (ctx->pair_ws) (void)hipFree(ctx->pair_ws);
  if (ctx->bls_ws) (void)hipFree(ctx->bls_ws);
  (void)ncg_comm_destroy(ctx);
  if (ctx->comm_buf) (void)hipFree(ctx->comm_buf);
  if (ctx->sync_land) (void)hipHostFree(ctx->sync_land);
  if (ctx->comm_fork) (void)hipEventDestroy(ctx->comm_fork);
  if (ctx->comm_join) (void)hipEventDestroy(ctx->comm_join);
  if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
  for (int i = 0; i < ncg_ctx::COPY_CHUNKS; i++) {
    if (ctx->ev_in[i]) (void)hipEventDestroy(ctx->ev_in[i]);
    if (ctx->ev_k[i]) (void)hipEventDestroy(ctx->ev_k[i]);
    if (ctx->ev_sc[i]) (void)hipEventDestroy(ctx->ev_sc[i]);
  }
  if (ctx->ev_ready) (void)hipEventDestroy(ctx->ev_ready);
  if (ctx->copy_in) (void)hipStreamDestroy(ctx->copy_in);
  if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
  for (ncg_msm_lane& ln : ctx->lanes) {
    if (ln.stream) (void)hipStreamSynchronize(ln.stream);
    if (ln.ws) (void)hipFree(ln.ws);
    if (ln.comm_buf) (void)hipFree(ln.comm_buf);
    if (ln.land) (void)hipHostFree(ln.land);
    if (ln.done) (void)hipEventDestroy(ln.done);
    if (ln.input_ready) (void)hipEventDestroy(ln.input_ready);
    if (ln.side.fork) (void)hipEventDestroy(ln.side.fork);
    if (ln.side.join) (void)hipEventDestroy(ln.side.join);
    if (ln.side.stream) (void)hipStreamDestroy(ln.side.stream);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
  }
  if (ctx->msm_side.fork) (void)hipEventDestroy(ctx->msm_side.fork);
  if (ctx->msm_side.join) (void)hipEventDestroy(ctx->msm_side.join);
  if (ctx->msm_side.stream) (void)hipStreamDestroy(ctx->msm_side.stream);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* ncg_last_error(ncg_ctx* ctx) {
  if (ctx) return ctx->last_error.c_str();
  std::lock_guard<std::mutex> g(g_err_mu);
  static thread_local std::string copy;
  copy = g_last_error;
  return copy.c_str();
}

int ncg_sync(ncg_ctx* ctx) {
  if (!ctx) return set_err(nullptr, NCG_ERR_INVALID_ARG, "noble-gpu: ctx is NULL");
  NCG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return NCG_OK;
}

// (the fresh allocation is cleared here, so the first kernel that uses it is not the one paying for the page mappings of a
// GB-sized buffer)
static int ensure_mul_ws(ncg_ctx* ctx, int curve, size_t n, hipStream_t st) {
  const size_t need = ncg::mul_var_tmp_bytes(curve, (int)n);
  return ncg_grow_buf(ctx, &ctx->mul_ws, &ctx->mul_ws_bytes, need, need, GrowWait::stream, st, true);
}

int ncg_mul_var_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* points_affine_dev, const void* scalars_dev,
                          void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, mul_var_rule(ctx, curve), n, points_affine_dev, scalars_dev, out_affine_dev, out_is_inf_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_mul_ws(ctx, curve, n, st)) return rc;
  NCG_HIP(ctx, ncg::mul_var_batch(curve, (const uint32_t*)points_affine_dev, (const uint32_t*)scalars_dev,
                                  (uint32_t*)out_affine_dev, out_is_inf_dev, (int)n, (uint32_t*)ctx->mul_ws, st));
  return NCG_OK;
}

// Long-lived host buffers (the Node addon's Buffers, a prover's witness arrays) can be pinned ONCE: the host-pointer entry
// points then DMA straight from / to them.  Without it every call registers the large buffers it is handed and releases
// them again (PinSet): correct, but the page locking is paid per call.
int ncg_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return set_err(nullptr, NCG_ERR_INVALID_ARG, "noble-gpu: host_register: NULL buffer");
  hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(nullptr, NCG_ERR_HIP, "noble-gpu: host_register: %s", hipGetErrorString(e));
  }
  return NCG_OK;
}
int ncg_host_unregister(void* p) {
  if (!p) return NCG_OK;
  hipError_t e = hipHostUnregister(p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(nullptr, NCG_ERR_HIP, "noble-gpu: host_unregister: %s", hipGetErrorString(e));
  }
  return NCG_OK;
}

// copy streams + chunk events of the host-pointer entry points (made on first use)
static int ensure_copy_streams(ncg_ctx* ctx) {
  if (ctx->copy_in) return NCG_OK;
  hipError_t e = hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking);
  for (int i = 0; i < ncg_ctx::COPY_CHUNKS && e == hipSuccess; i++) {
    e = hipEventCreateWithFlags(&ctx->ev_in[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_k[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_sc[i], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_ready, hipEventDisableTiming);
  if (e != hipSuccess) return set_err(ctx, NCG_ERR_HIP, "noble-gpu: cannot create copy streams: %s", hipGetErrorString(e));
  return NCG_OK;
}
// Waits for every stream a host-pointer call may have used; returns the FIRST failure (an asynchronous copy or kernel error
// surfaces here, not at enqueue time), after having waited on all of them.
static hipError_t drain_copy_streams(ncg_ctx* ctx) {
  hipError_t first = hipSuccess, e;
  if (ctx->copy_in && (e = hipStreamSynchronize(ctx->copy_in)) != hipSuccess && first == hipSuccess) first = e;
  if (ctx->copy_out && (e = hipStreamSynchronize(ctx->copy_out)) != hipSuccess && first == hipSuccess) first = e;
  if (ctx->msm_side.stream && (e = hipStreamSynchronize(ctx->msm_side.stream)) != hipSuccess && first == hipSuccess) first = e;
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess && first == hipSuccess) first = e;
  return first;
}

int ncg_mul_var_batch(ncg_ctx* ctx, int curve, size_t n, const void* points_affine, const void* scalars,
                      void* out_affine, uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, mul_var_rule(ctx, curve), n, points_affine, scalars, out_affine);
  const int pb = ncg_point_bytes(curve);
  PinSet pins(ctx);
  size_t pts_b = n * pb, sc_b = n * 32, inf_b = align256(n);
  int rc = ensure_scratch(ctx, 2 * pts_b + sc_b + inf_b + 1024);
  if (rc) return rc;
  char* base = (char*)ctx->scratch;
  char* d_pts = base;
  char* d_out = d_pts + pts_b;
  char* d_sc = d_out + pts_b;
  char* d_inf = d_sc + sc_b;
  if (n >= ((size_t)1 << 17)) {
    // Large batches in chunks: chunk i + 1 crosses PCIe while the kernels of chunk i run and the results of chunk i - 1
    // go back (three streams, one event per chunk and direction).  The kernels are the batch's whole cost but for the
    // first upload and the last download: 2^20 secp256k1 pairs 13.4 -> ~9.6 ms end to end.
    rc = ensure_copy_streams(ctx);
    if (rc) return rc;
    // (page locking per chunk, just ahead of its copies - see ncg_msm)
    // Chunk sizes 1 : 3 : 3 : 1 (in eighths of the batch) for large batches: a launch of the ladder pays ~0.3 ms of ramp whatever
    // its size (tools/secp_rounds.py: 9.8 ns per item for one round of 196 608 items, 8.6 for two, 8.3 for the whole batch), so the
    // middle chunks are big, and only the first upload and the last download are exposed, so the outer ones are small.
    // (eight equal chunks: 10.7 ms for 2^20 secp256k1 pairs from pinned memory.)
    static const int k_eighths_big[4] = {1, 3, 3, 1}, k_eighths_even[4] = {2, 2, 2, 2};
    const int* eighths = n >= ((size_t)1 << 19) ? k_eighths_big : k_eighths_even;
    const int chunks = 4;
    const size_t unit = (((n + 7) / 8) + 255) & ~(size_t)255;
    hipError_t e = hipSuccess;
    size_t lo = 0;
    PagedParts in_pts(points_affine, pts_b), in_sc(scalars, sc_b), out_pts(out_affine, pts_b), out_inf(out_is_inf, n);
    for (int c = 0; c < chunks && e == hipSuccess && rc == NCG_OK; c++) {
      const size_t cnt = std::min(n - lo, unit * (size_t)eighths[c]);
      if (cnt == 0) break;
      const bool last = lo + cnt >= n;
      size_t a, b;
      if (in_pts.next((lo + cnt) * pb, last, true, &a, &b)) {
        pins.pin((const char*)points_affine + a, b - a);
        e = hipMemcpyAsync(d_pts + a, (const char*)points_affine + a, b - a, hipMemcpyHostToDevice, ctx->copy_in);
      }
      if (e == hipSuccess && in_sc.next((lo + cnt) * 32, last, true, &a, &b)) {
        pins.pin((const char*)scalars + a, b - a);
        e = hipMemcpyAsync(d_sc + a, (const char*)scalars + a, b - a, hipMemcpyHostToDevice, ctx->copy_in);
      }
      if (e == hipSuccess) e = hipEventRecord(ctx->ev_in[c], ctx->copy_in);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_in[c], 0);
      if (e != hipSuccess) break;
      rc = ncg_mul_var_batch_dev(ctx, curve, cnt, d_pts + lo * pb, d_sc + lo * 32, d_out + lo * pb, (uint8_t*)d_inf + lo, ctx->stream);
      if (rc) break;
      e = hipEventRecord(ctx->ev_k[c], ctx->stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_out, ctx->ev_k[c], 0);
      if (e == hipSuccess && out_pts.next((lo + cnt) * pb, last, false, &a, &b)) {
        pins.pin((char*)out_affine + a, b - a);   // (locked while the chunk's kernels run)
        e = hipMemcpyAsync((char*)out_affine + a, d_out + a, b - a, hipMemcpyDeviceToHost, ctx->copy_out);
      }
      if (e == hipSuccess && out_is_inf && out_inf.next(lo + cnt, last, false, &a, &b)) {
        pins.pin(out_is_inf + a, b - a);
        e = hipMemcpyAsync(out_is_inf + a, d_inf + a, b - a, hipMemcpyDeviceToHost, ctx->copy_out);
      }
      lo += cnt;
    }
    const hipError_t ed = drain_copy_streams(ctx);
    if (rc) return rc;
    if (e == hipSuccess) e = ed;
    if (e != hipSuccess) return set_err(ctx, NCG_ERR_HIP, "noble-gpu: mul_var_batch: %s", hipGetErrorString(e));
    return NCG_OK;
  }
  NCG_HIP(ctx, pins.h2d(d_pts, points_affine, pts_b));
  NCG_HIP(ctx, pins.h2d(d_sc, scalars, sc_b));
  rc = ncg_mul_var_batch_dev(ctx, curve, n, d_pts, d_sc, d_out, (uint8_t*)d_inf, ctx->stream);
  if (rc) return rc;
  NCG_HIP(ctx, pins.d2h(out_affine, d_out, pts_b));
  if (out_is_inf) NCG_HIP(ctx, pins.d2h(out_is_inf, d_inf, n));
  NCG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return NCG_OK;
}

int ncg_add_pairs_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* a_dev, const void* b_dev, int subtract,
                            void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, add_pairs_rule(ctx, curve), n, a_dev, b_dev, out_affine_dev, out_is_inf_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_mul_ws(ctx, curve, n, st)) return rc;
  NCG_HIP(ctx, ncg::pair_add_batch(curve, (const uint32_t*)a_dev, (const uint32_t*)b_dev, subtract, (uint32_t*)out_affine_dev,
                                   out_is_inf_dev, (int)n, (uint32_t*)ctx->mul_ws, st));
  return NCG_OK;
}

int ncg_add_pairs_batch(ncg_ctx* ctx, int curve, size_t n, const void* a, const void* b, int subtract, void* out_affine,
                        uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, add_pairs_rule(ctx, curve), n, a, b, out_affine);
  const size_t pts_b = n * (size_t)ncg_point_bytes(curve);
  HostCall hc(ctx);
  const int da = hc.in(a, pts_b), db = hc.in(b, pts_b);
  const int o = hc.out(out_affine, pts_b), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_add_pairs_batch_dev(ctx, curve, n, hc.dev(da), hc.dev(db), subtract, hc.dev(o), hc.dev<uint8_t>(f), ctx->stream));
}

// the ed25519 fixed-base table: computed on the host (33 x 128 affine Niels points), cached per context
static int ensure_ed_base_table(ncg_ctx* ctx) {
  if (ctx->base_tab[NCG_ED25519]) return NCG_OK;
  std::vector<uint32_t> host(ncg::ed25519_fixed_table_words());
  ncg::ed25519_build_fixed_table(host.data());
  uint32_t* tab = nullptr;
  NCG_HIP(ctx, hipMalloc((void**)&tab, host.size() * 4));
  hipError_t e = hipMemcpy(tab, host.data(), host.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(tab);
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: uploading the ed25519 fixed-base table failed: %s", hipGetErrorString(e));
  }
  ctx->base_tab[NCG_ED25519] = tab;
  return NCG_OK;
}

int ncg_mul_base_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* scalars_dev, void* out_affine_dev,
                           uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, mul_base_rule(ctx, curve), n, scalars_dev, out_affine_dev, out_is_inf_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_mul_ws(ctx, curve, n > 8192 ? n : 8192, st)) return rc;
  if (curve == NCG_ED25519) {
    if (int rc = ensure_ed_base_table(ctx)) return rc;
    NCG_HIP(ctx, ncg::ed25519_mul_base_batch(ctx->base_tab[curve], (const uint32_t*)scalars_dev, (uint32_t*)out_affine_dev,
                                             out_is_inf_dev, (int)n, (uint32_t*)ctx->mul_ws, st));
    return NCG_OK;
  }
  if (!ctx->base_tab[curve]) {  // built once per context with the variable-base kernel
    const uint32_t* base = curve == NCG_SECP256K1 ? ncg::BasePoints::SECP
                           : curve == NCG_BLS12_381_G1 ? ncg::BasePoints::G1 : ncg::BasePoints::G2;
    uint32_t* tab = nullptr;
    NCG_HIP(ctx, hipMalloc((void**)&tab, ncg::mul_base_table_bytes(curve)));
    hipError_t e = ncg::mul_base_build_table(curve, base, tab, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // cache the table only once the build is known to have completed
    if (e != hipSuccess) {
      (void)hipFree(tab);
      return set_err(ctx, NCG_ERR_HIP, "noble-gpu: building the fixed-base table failed: %s", hipGetErrorString(e));
    }
    ctx->base_tab[curve] = tab;
  }
  NCG_HIP(ctx, ncg::mul_base_batch(curve, ctx->base_tab[curve], (const uint32_t*)scalars_dev, (uint32_t*)out_affine_dev,
                                   out_is_inf_dev, (int)n, (uint32_t*)ctx->mul_ws, st));
  return NCG_OK;
}

int ncg_mul_base_batch(ncg_ctx* ctx, int curve, size_t n, const void* scalars, void* out_affine, uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, mul_base_rule(ctx, curve), n, scalars, out_affine);
  HostCall hc(ctx);
  const int sc = hc.in(scalars, n * 32);
  const int o = hc.out(out_affine, n * (size_t)ncg_point_bytes(curve)), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_mul_base_batch_dev(ctx, curve, n, hc.dev(sc), hc.dev(o), hc.dev<uint8_t>(f), ctx->stream));
}

// window plan the MSM entry points use for n points: out = {c, nwin, buckets per window, grouped sums per window}
int ncg_msm_plan_info(int curve, size_t n, int* out4) {
  if (!out4 || ncg_point_bytes(curve) == 0 || n == 0 || n > 0x7fffffffu) return NCG_ERR_INVALID_ARG;
  ncg::MsmPlan pl;
  if (ncg::msm_make_plan(curve, (int)n, 0, &pl) != 0) return NCG_ERR_INVALID_ARG;
  out4[0] = pl.c;
  out4[1] = pl.nwin;
  out4[2] = pl.nb;
  out4[3] = (int)(ncg::msm_fin_words(curve, pl) / ncg::msm_acc_words(curve) / (size_t)pl.nwin);
  return NCG_OK;
}

// Tuning overrides of the MSM on this context (diagnostics / tests: the lane segment decides how the accumulate kernel
// cuts buckets, run_serial which cut buckets go to the long-run work list).  seg <= 0 and run_serial < 0 restore the defaults.
int ncg_msm_set_tuning(ncg_ctx* ctx, int seg, int run_serial) {
  if (!ctx) return set_err(nullptr, NCG_ERR_INVALID_ARG, "noble-gpu: ctx is NULL");
  if (seg > (1 << 24) || run_serial > (1 << 24)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm_set_tuning: value out of range");
  ctx->msm_seg_override = seg > 0 ? seg : 0;
  ctx->msm_run_serial_override = run_serial >= 0 ? run_serial : -1;
  return NCG_OK;
}
// What the last MSM launch on this context ran with: out8 = {c, local windows, buckets per window, first window, windows of
// the whole plan, entries per accumulate lane (seg), run_serial, runs that went to the long-run work list}.  Synchronises.
int ncg_msm_last_plan(ncg_ctx* ctx, int* out8) {
  if (!ctx || !out8) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm_last_plan: NULL argument");
  const ncg::MsmTrace& tr = ctx->msm_trace;
  if (tr.c == 0) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm_last_plan: no MSM has run on this context");
  NCG_HIP(ctx, hipSetDevice(ctx->device));
  NCG_HIP(ctx, hipDeviceSynchronize());
  uint32_t runs = 0;
  if (tr.d_long_runs) NCG_HIP(ctx, hipMemcpy(&runs, tr.d_long_runs, 4, hipMemcpyDeviceToHost));
  out8[0] = tr.c; out8[1] = tr.nwin; out8[2] = tr.nb; out8[3] = tr.w0; out8[4] = tr.nwin_total;
  out8[5] = tr.seg; out8[6] = tr.run_serial; out8[7] = (int)runs;
  return NCG_OK;
}

int ncg_msm_dev(ncg_ctx* ctx, int curve, size_t n, const void* points_affine_dev, const void* scalars_dev,
                void* out_affine, uint8_t* out_is_inf, void* stream) {
  NCG_BEGIN_OR(ctx, msm_rule(ctx, curve), n, msm_identity(ctx, curve, out_affine, out_is_inf), points_affine_dev, scalars_dev,
               out_affine);
  if (misaligned16(points_affine_dev) || misaligned16(scalars_dev))
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: device buffers must be 16-byte aligned");
  ncg::MsmPlan pl;
  if (int rc = ncg_msm_plan_ws(ctx, curve, n, 0, &pl)) return rc;
  uint32_t bad = 0xFFFFFFFFu;
  uint8_t inf_local = 0;
  NCG_HIP(ctx, ncg::msm_run(curve, pl, (const uint32_t*)points_affine_dev, (const uint32_t*)scalars_dev, ctx->msm_ws,
                            (uint32_t*)out_affine, &inf_local, stream_of(ctx, stream), &bad, &ctx->msm_side));
  if (bad != 0xFFFFFFFFu)  // validateMSMScalars (curve.ts:398-404): scalars must be below the group order
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: invalid scalar at index %u (not below the group order)", bad);
  if (out_is_inf) *out_is_inf = inf_local;
  return NCG_OK;
}

int ncg_msm(ncg_ctx* ctx, int curve, size_t n, const void* points_affine, const void* scalars, void* out_affine,
            uint8_t* out_is_inf) {
  NCG_BEGIN_OR(ctx, msm_rule(ctx, curve), n, msm_identity(ctx, curve, out_affine, out_is_inf), points_affine, scalars, out_affine);
  const int pb = ncg_point_bytes(curve);
  PinSet pins(ctx);
  size_t pts_b = n * pb, sc_b = n * 32;
  const size_t pts_al = align256(pts_b), sc_al = align256(sc_b);
  const size_t stored_b = n * ncg::msm_stored_words_per_point(curve) * 4;
  int rc = ensure_scratch(ctx, pts_al + sc_al + stored_b + 2048);
  if (rc) return rc;
  char* d_pts = (char*)ctx->scratch;
  char* d_sc = d_pts + pts_al;
  if (n >= ((size_t)1 << 16)) {
    // Points AND scalars cross in PARTS, each part's scalars (a quarter of its bytes) ahead of its points: a part's digits and
    // counting sort need only its own scalars, its points are converted to the accumulate kernel's storage format on the side
    // stream as they land, and it is accumulated into the shared buckets (MsmPlan::part_flags) while the next part is still on
    // the bus - only the last part's accumulate, the fold and the tail run after the last byte.  2^20 G1 points from pinned host
    // memory: 9.3 ms (round 2, one copy then one MSM) -> 6.2 ms (sort under the transfer) -> 5.4 ms (parts; all scalars first)
    // -> see profiles/r04_host_path.json (the first part is ready after 32 MB instead of 56).
    rc = ensure_copy_streams(ctx);
    if (rc) return rc;
    char* d_stored = d_sc + sc_al;
    // measured on one box: G1 2^20 6.0 / 5.0 / 4.5 / 4.9 ms with 1 / 2 / 4 / 8 parts, G2 2^18 5.7 / 4.3 / 4.4 / 6.2
    const int parts = n >= ((size_t)1 << 19) ? 4 : n >= ((size_t)1 << 17) ? 2 : 1;
    const size_t per = (((n + parts - 1) / parts) + 255) & ~(size_t)255;
    ncg::MsmPlan whole, layout;
    if (ncg::msm_make_plan(curve, (int)n, 0, &whole) != 0 || ncg::msm_make_plan(curve, (int)std::min(n, per), whole.c, &layout) != 0)
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: cannot plan windows");
    layout.pts_stored = 1;
    layout.n_layout = layout.n;
    layout.Q_layout = layout.Q;
    rc = msm_ensure_ws(ctx, curve, layout);
    if (rc) return rc;
    // page locking per PART, right before the part's copies are enqueued: the copies are asynchronous, so the host locks the
    // pages of part p + 1 while part p is on the bus (locking all 128 MB of a 2^20-point G1 MSM up front costs ~3 ms before the
    // first byte moves).  Buffers the caller pinned with ncg_host_register are left alone (the registration attempt fails fast).
    const size_t sw = ncg::msm_stored_words_per_point(curve) * 4;
    hipError_t e = hipSuccess;
    PagedParts in_pts(points_affine, pts_b), in_sc(scalars, sc_b);
    const uint32_t *d_fin = nullptr, *d_bad = nullptr;
    ncg::MsmPlan last = layout;
    for (int p = 0; p < parts && e == hipSuccess; p++) {
      const size_t lo = std::min(n, per * (size_t)p), cnt = std::min(n, lo + per) - lo;
      const bool is_last = p == parts - 1 || lo + cnt >= n;
      if (cnt) {
        size_t a, b;
        if (in_sc.next((lo + cnt) * 32, is_last, true, &a, &b)) {
          pins.pin((const char*)scalars + a, b - a);
          e = hipMemcpyAsync(d_sc + a, (const char*)scalars + a, b - a, hipMemcpyHostToDevice, ctx->copy_in);
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev_sc[p], ctx->copy_in);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_sc[p], 0);   // this part's digits wait for its scalars only
        if (e == hipSuccess && in_pts.next((lo + cnt) * pb, is_last, true, &a, &b)) {
          pins.pin((const char*)points_affine + a, b - a);
          e = hipMemcpyAsync(d_pts + a, (const char*)points_affine + a, b - a, hipMemcpyHostToDevice, ctx->copy_in);
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev_in[p], ctx->copy_in);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->msm_side.stream, ctx->ev_in[p], 0);
        if (e == hipSuccess)
          e = ncg::msm_points_to_stored(curve, (const uint32_t*)(d_pts + lo * pb), (int)cnt, (uint32_t*)(d_stored + lo * sw), ctx->msm_side.stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev_k[p], ctx->msm_side.stream);
        if (e != hipSuccess) break;
      }
      ncg::MsmPlan pl;
      if (ncg::msm_make_plan(curve, (int)std::max<size_t>(cnt, 1), whole.c, &pl) != 0) {
        (void)drain_copy_streams(ctx);   // copies of this and earlier parts are in flight
        return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: cannot plan windows");
      }
      msm_apply_ctx(ctx, pl);
      pl.pts_stored = 1;
      pl.n_layout = layout.n;
      pl.Q_layout = layout.Q;
      pl.index_base = (uint32_t)lo;
      pl.part_flags = (p == 0 ? 1 : 0) | (is_last ? 2 : 0);
      ncg::MsmSide side;            // no fork / join of its own: the conversion is already in flight on the side stream
      side.pts_ready = cnt ? ctx->ev_k[p] : nullptr;
      e = ncg::msm_device_phase(curve, pl, (const uint32_t*)(d_stored + lo * sw), (const uint32_t*)(d_sc + lo * 32), ctx->msm_ws, &d_fin,
                                ctx->stream, &d_bad, &side);
      last = pl;
      if (is_last) break;
    }
    uint32_t bad = 0xFFFFFFFFu;
    uint8_t inf_local = 0;
    if (e == hipSuccess) e = ncg::msm_finish(curve, last, d_fin, (uint32_t*)out_affine, &inf_local, ctx->stream, d_bad, &bad);
    const hipError_t ed = drain_copy_streams(ctx);
    if (e == hipSuccess) e = ed;
    if (e != hipSuccess) return set_err(ctx, NCG_ERR_HIP, "noble-gpu: msm: %s", hipGetErrorString(e));
    if (bad != 0xFFFFFFFFu)
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: invalid scalar at index %u (not below the group order)", bad);
    if (out_is_inf) *out_is_inf = inf_local;
    return NCG_OK;
  }
  NCG_HIP(ctx, pins.h2d(d_pts, points_affine, pts_b));
  NCG_HIP(ctx, pins.h2d(d_sc, scalars, sc_b));
  return ncg_msm_dev(ctx, curve, n, d_pts, d_sc, out_affine, out_is_inf, ctx->stream);
}

// ---- resident point sets: upload once, multiply many (interleavedMSMUnsafe's usage pattern,
// src/abstract/curve.ts:907-959; SURVEY 8a gotcha 8: marshalling dominates an end-to-end call)

// The point of a resident set (curve.ts:907-918: precompute once, call with scalars): the wire -> storage
// conversion of the points is paid at the first MSM, every later call starts at the digits.
static int points_build_stored(ncg_ctx* ctx, ncg_points* h, hipStream_t st) {
  if (h->d_stored || h->n == 0) return NCG_OK;
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, h->n * ncg::msm_stored_words_per_point(h->curve) * 4);
  if (e != hipSuccess) {  // not fatal: the generic path converts per call
    (void)hipGetLastError();
    return NCG_OK;
  }
  e = ncg::msm_points_to_stored(h->curve, (const uint32_t*)h->d_pts, (int)h->n, (uint32_t*)d, st);
  // the cache is published only once the conversion has FINISHED: another lane's stream (ncg_msm_async_submit) or a later call on
  // ctx->stream reads d_stored with no ordering against `st` otherwise (one synchronisation per set, as points_build_endo does)
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: points_to_stored: %s", hipGetErrorString(e));
  }
  h->d_stored = d;
  return NCG_OK;
}

// Build the endomorphism images of a set whose points are KNOWN to lie in the prime-order subgroup.
static int points_build_endo(ncg_ctx* ctx, ncg_points* h) {
  const int E = ncg::msm_endo_factor(h->curve);
  if (E == 0 || h->n == 0 || h->d_endo) return NCG_OK;
  if (h->n * (size_t)E > 0x7fffffffu) return NCG_OK;  // too large for the expanded index space: generic path
  const size_t bytes = h->n * (size_t)E * ncg::msm_endo_words_per_point(h->curve) * 4;
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, bytes);
  if (e != hipSuccess) return set_err(ctx, NCG_ERR_NOMEM, "noble-gpu: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  e = ncg::msm_endo_expand(h->curve, (const uint32_t*)h->d_pts, (int)h->n, (uint32_t*)d, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: endomorphism images: %s", hipGetErrorString(e));
  }
  h->d_endo = d;
  return NCG_OK;
}

int ncg_points_upload(ncg_ctx* ctx, int curve, size_t n, const void* points_affine, ncg_points** out) {
  if (!ctx || !out) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: points_upload: NULL argument");
  *out = nullptr;
  const int pb = ncg_point_bytes(curve);
  if (pb == 0) return set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: points_upload: unsupported curve %d", curve);
  if (n > 0x7fffffffu) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: batch too large");
  if (n && !points_affine) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: points_upload: NULL buffer");
  NCG_HIP(ctx, hipSetDevice(ctx->device));
  ncg_points* h = new ncg_points{ctx, curve, n, nullptr};
  if (n) {
    hipError_t e = hipMalloc(&h->d_pts, n * (size_t)pb);
    if (e != hipSuccess) {
      delete h;
      return set_err(ctx, NCG_ERR_NOMEM, "noble-gpu: hipMalloc(%zu) failed: %s", n * (size_t)pb, hipGetErrorString(e));
    }
    PinSet pins(ctx);
    e = pins.h2d(h->d_pts, points_affine, n * (size_t)pb);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      (void)hipFree(h->d_pts);
      delete h;
      return set_err(ctx, NCG_ERR_HIP, "noble-gpu: points_upload: copy failed: %s", hipGetErrorString(e));
    }
  }
  *out = h;
  return NCG_OK;
}

int ncg_points_from_encoded(ncg_ctx* ctx, int curve, size_t n, const void* encoded, int flags, ncg_points** out,
                            int64_t* out_bad_index) {
  if (!ctx || !out) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: points_from_encoded: NULL argument");
  *out = nullptr;
  if (out_bad_index) *out_bad_index = -1;
  if (const int rc = encoded_rule(ctx, "points_from_encoded", curve).rc) return rc;
  if (const int rc = n ? batch_args(ctx, "points_from_encoded", n, {encoded}) : NCG_OK) return rc;
  ncg_points* h = new ncg_points{ctx, curve, n, nullptr};
  if (n) {
    const size_t pts_b = n * (size_t)ncg_point_bytes(curve);
    hipError_t e = hipMalloc(&h->d_pts, pts_b);
    if (e != hipSuccess) {
      delete h;
      return set_err(ctx, NCG_ERR_NOMEM, "noble-gpu: hipMalloc(%zu) failed: %s", pts_b, hipGetErrorString(e));
    }
    std::vector<uint8_t> ok(n);
    int rc;
    {
      HostCall hc(ctx);
      const int in = hc.in(encoded, n * (size_t)ncg::decode_in_bytes(curve));
      const int dok = hc.out(ok.data(), n), inf = hc.dev_only(n);
      rc = hc.stage();
      if (rc == NCG_OK)
        rc = hc.finish(ncg_decode_points_batch_dev(ctx, curve, n, hc.dev(in), flags, h->d_pts, hc.dev<uint8_t>(dok),
                                                   hc.dev<uint8_t>(inf), ctx->stream));
    }
    if (rc == NCG_OK)
      for (size_t i = 0; i < n; i++)
        if (!ok[i]) {  // the reference throws while decoding (Point.fromBytes / assertValidity)
          if (out_bad_index) *out_bad_index = (int64_t)i;
          rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: points_from_encoded: invalid point encoding at index %zu", i);
          break;
        }
    // the bls12-381 decoders include the subgroup test (bls12-381.ts:567-577, :599-601), so a decoded set
    // qualifies for the endomorphism MSM; infinity encodings decode to ZERO and stay ZERO in every image
    if (rc == NCG_OK) (void)points_build_endo(ctx, h);  // best effort: without the images the set uses the generic MSM
    if (rc != NCG_OK) {
      (void)hipFree(h->d_pts);
      delete h;
      return rc;
    }
  }
  *out = h;
  return NCG_OK;
}

int ncg_points_verify_subgroup(ncg_ctx* ctx, ncg_points* h, int64_t* out_bad_index) {
  if (out_bad_index) *out_bad_index = -1;
  if (!ctx || !h || h->ctx != ctx) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: points_verify_subgroup: handle does not belong to this context");
  const int E = ncg::msm_endo_factor(h->curve);
  if (E == 0) return set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: points_verify_subgroup: bls12-381 G1 / G2 only");
  if (h->n == 0 || h->d_endo) return NCG_OK;
  NCG_HIP(ctx, hipSetDevice(ctx->device));
  int rc = points_build_endo(ctx, h);
  if (rc != NCG_OK || !h->d_endo) return rc;
  // [z^2] P (G1) / [z] P (G2) by the generic (complete) batch multiply, compared with the first image
  const size_t n = h->n, pb = (size_t)ncg_point_bytes(h->curve);
  char* tmp = nullptr;
  const size_t sc_b = align256(n * 32), out_b = align256(n * pb), inf_b = align256(n);
  hipError_t e = hipMalloc((void**)&tmp, sc_b + out_b + inf_b + 256);
  auto drop = [&]() {
    if (tmp) (void)hipFree(tmp);
    (void)hipFree(h->d_endo);
    h->d_endo = nullptr;
  };
  if (e != hipSuccess) {
    tmp = nullptr;
    drop();
    return set_err(ctx, NCG_ERR_NOMEM, "noble-gpu: hipMalloc failed: %s", hipGetErrorString(e));
  }
  uint32_t kz[8];
  ncg::msm_endo_verify_scalar(h->curve, kz);
  std::vector<uint32_t> sc(n * 8);
  for (size_t i = 0; i < n; i++) memcpy(&sc[i * 8], kz, 32);
  uint32_t bad = 0xFFFFFFFFu;
  uint32_t* d_bad = (uint32_t*)(tmp + sc_b + out_b + inf_b);
  e = hipMemcpyAsync(tmp, sc.data(), n * 32, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_bad, &bad, 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `sc` and `bad` are pageable
  if (e == hipSuccess) {
    rc = ncg_mul_var_batch_dev(ctx, h->curve, n, h->d_pts, tmp, tmp + sc_b, (uint8_t*)(tmp + sc_b + out_b), ctx->stream);
    if (rc != NCG_OK) {
      drop();
      return rc;
    }
    e = ncg::msm_endo_verify(h->curve, (const uint32_t*)(tmp + sc_b), (const uint8_t*)(tmp + sc_b + out_b),
                             (const uint32_t*)h->d_endo, (int)n, d_bad, ctx->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    drop();
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: points_verify_subgroup: %s", hipGetErrorString(e));
  }
  (void)hipFree(tmp);
  tmp = nullptr;
  if (bad != 0xFFFFFFFFu) {  // not an error: the set stays usable through the generic path
    drop();
    if (out_bad_index) *out_bad_index = (int64_t)bad;
  }
  return NCG_OK;
}

// interleavedMSMUnsafe's precomputation (curve.ts:907-959: tables once per point set) on the device: window-shifted
// copies of the set, after which ncg_msm_resident* runs the shared-bucket MSM (one bucket fold, no Horner across
// windows).  Uses the endomorphism images when the set is verified, the points themselves otherwise.  Sets below
// 4096 points and ed25519 sets are left as they are (NCG_OK, nothing built).
int ncg_points_precompute(ncg_ctx* ctx, ncg_points* h) {
  if (!ctx || !h || h->ctx != ctx) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: points_precompute: handle does not belong to this context");
  if (h->d_shift || h->n < 4096 || h->curve == NCG_ED25519) return NCG_OK;
  static const bool no_shift = ncg::knob_set("NCG_NO_PRECOMP");
  if (no_shift) return NCG_OK;  // the levels would never be used: pay neither the build nor the memory
  NCG_HIP(ctx, hipSetDevice(ctx->device));
  static const bool no_endo = ncg::knob_set("NCG_NO_ENDO");
  const bool endo = h->d_endo && !no_endo;
  ncg::MsmPlan pl;
  const int c = 16;
  if ((endo ? ncg::msm_make_plan_endo(h->curve, (int)h->n, c, &pl) : ncg::msm_make_plan(h->curve, (int)h->n, c, &pl)) != 0)
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: cannot plan windows");
  const size_t m = (size_t)pl.n, sw = ncg::msm_stored_words_per_point(h->curve);
  if (m * (size_t)pl.nwin > 0x7fffffffu) return NCG_OK;  // entry index space: keep the per-window path
  if (!endo) {
    int rc = points_build_stored(ctx, h, ctx->stream);
    if (rc) return rc;
    if (!h->d_stored) return NCG_OK;
  }
  void *d = nullptr, *tmp = nullptr;
  {  // the levels are nwin copies of the set: leave room for the MSM workspace and whatever else the process allocates
    size_t free_b = 0, total_b = 0;
    const size_t want = m * (size_t)pl.nwin * sw * 4 + ncg::msm_shift_tmp_bytes(h->curve, (int)m);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b / 2) return NCG_OK;  // keep the per-window path
  }
  hipError_t e = hipMalloc(&d, m * (size_t)pl.nwin * sw * 4);
  if (e == hipSuccess) e = hipMalloc(&tmp, ncg::msm_shift_tmp_bytes(h->curve, (int)m));
  if (e != hipSuccess) {  // not fatal: the set keeps the per-window path
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    return NCG_OK;
  }
  e = hipMemcpyAsync(d, endo ? h->d_endo : h->d_stored, m * sw * 4, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = ncg::msm_shift_levels(h->curve, (uint32_t*)d, (int)m, pl.nwin, pl.c, tmp, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: points_precompute: %s", hipGetErrorString(e));
  }
  if (!endo && h->d_stored) {  // level 0 of the copies IS the stored set: the separate array is a duplicate now
    (void)hipFree(h->d_stored);
    h->d_stored = nullptr;
  }
  h->d_shift = d;
  h->shift_c = pl.c;
  h->shift_nwin = pl.nwin;
  h->shift_mode = endo ? 2 : 1;
  h->shift_m = m;
  return NCG_OK;
}
int ncg_points_precomputed(const ncg_points* h) { return h && h->d_shift ? 1 : 0; }

int ncg_points_in_subgroup(const ncg_points* h) { return h && h->d_endo ? 1 : 0; }

void ncg_points_free(ncg_points* h) {
  if (!h) return;
  (void)hipSetDevice(h->ctx->device);
  if (h->d_pts) (void)hipFree(h->d_pts);
  if (h->d_endo) (void)hipFree(h->d_endo);
  if (h->d_stored) (void)hipFree(h->d_stored);
  if (h->d_shift) (void)hipFree(h->d_shift);
  delete h;
}
size_t ncg_points_count(const ncg_points* h) { return h ? h->n : 0; }
int ncg_points_curve(const ncg_points* h) { return h ? h->curve : -1; }
const void* ncg_points_dev(const ncg_points* h) { return h ? h->d_pts : nullptr; }

}  // extern "C"
#pragma GCC visibility pop
// Which window plan and which device point array an MSM on a resident set uses: the precomputed levels (shared-bucket
// mode), the endomorphism images of a verified set, the stored form of the points, or - if that cache could not be
// allocated - the wire points.  The stored form is built on first use (on `st`).
int ncg_resident_plan(ncg_ctx* ctx, const ncg_points* pts, ncg::MsmPlan* pl, const uint32_t** d_pts, hipStream_t st) {
  static const bool no_endo = ncg::knob_set("NCG_NO_ENDO");
  static const bool no_shift = ncg::knob_set("NCG_NO_PRECOMP");
  if (pts->d_shift && !no_shift) {  // precomputed set: every window adds into one bucket set (msm.hpp `shared`)
    const int prc = pts->shift_mode == 2 ? ncg::msm_make_plan_endo(pts->curve, (int)pts->n, pts->shift_c, pl)
                                         : ncg::msm_make_plan(pts->curve, (int)pts->n, pts->shift_c, pl);
    if (prc != 0 || pl->nwin != pts->shift_nwin || (size_t)pl->n != pts->shift_m)
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: the precomputed levels do not match the window plan");
    pl->shared = 1;
    pl->top_tb = 0;       // one bucket set for all windows: the weight of a bucket is its index, no spreading
    pl->top_submask = 0;
    pl->pts_stored = 1;
    *d_pts = (const uint32_t*)pts->d_shift;
    return NCG_OK;
  }
  if (pts->d_endo && !no_endo) {  // verified subgroup set: endomorphism MSM on the expanded images (endo.hpp)
    if (ncg::msm_make_plan_endo(pts->curve, (int)pts->n, 0, pl) != 0)
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: cannot plan windows");
    *d_pts = (const uint32_t*)pts->d_endo;
    return NCG_OK;
  }
  if (ncg::msm_make_plan(pts->curve, (int)pts->n, 0, pl) != 0)
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: cannot plan windows");
  if (pts->d_shift && pts->shift_mode == 1) {  // level 0 of the copies is the stored set
    pl->pts_stored = 1;
    *d_pts = (const uint32_t*)pts->d_shift;
    return NCG_OK;
  }
  int rc = points_build_stored(ctx, const_cast<ncg_points*>(pts), st);  // a cache inside the handle
  if (rc) return rc;
  if (pts->d_stored) {
    pl->pts_stored = 1;
    *d_pts = (const uint32_t*)pts->d_stored;
  } else {
    *d_pts = (const uint32_t*)pts->d_pts;  // wire points: converted per call
  }
  return NCG_OK;
}

#pragma GCC visibility push(default)
extern "C" {

// MSM on a resident set with the scalars already on the device
static int msm_resident_core(ncg_ctx* ctx, const ncg_points* pts, const void* d_sc, void* out_affine, uint8_t* out_is_inf,
                             hipStream_t st) {
  ncg::MsmPlan pl;
  const uint32_t* d_pts = nullptr;
  int rc = ncg_resident_plan(ctx, pts, &pl, &d_pts, st);
  if (rc) return rc;
  rc = msm_ensure_ws(ctx, pts->curve, pl);
  if (rc) return rc;
  uint32_t bad = 0xFFFFFFFFu;
  uint8_t inf_local = 0;
  NCG_HIP(ctx, ncg::msm_run(pts->curve, pl, d_pts, (const uint32_t*)d_sc, ctx->msm_ws, (uint32_t*)out_affine, &inf_local, st, &bad,
                            pl.pts_stored || pl.endo ? nullptr : &ctx->msm_side));
  if (bad != 0xFFFFFFFFu)
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm: invalid scalar at index %u (not below the group order)", bad);
  if (out_is_inf) *out_is_inf = inf_local;
  return NCG_OK;
}

int ncg_msm_resident(ncg_ctx* ctx, const ncg_points* pts, const void* scalars, void* out_affine, uint8_t* out_is_inf) {
  NCG_BEGIN_OR(ctx, handle_rule(ctx, "msm_resident", pts), pts->n, msm_identity(ctx, pts->curve, out_affine, out_is_inf), scalars,
               out_affine);
  HostCall hc(ctx);
  const int sc = hc.in(scalars, pts->n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(msm_resident_core(ctx, pts, hc.dev(sc), out_affine, out_is_inf, ctx->stream));
}

int ncg_msm_resident_dev(ncg_ctx* ctx, const ncg_points* pts, const void* scalars_dev, void* out_affine, uint8_t* out_is_inf,
                         void* stream) {
  NCG_BEGIN_OR(ctx, handle_rule(ctx, "msm_resident", pts), pts->n, msm_identity(ctx, pts->curve, out_affine, out_is_inf), scalars_dev,
               out_affine);
  if (misaligned16(scalars_dev)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: msm_resident: device buffers must be 16-byte aligned");
  return msm_resident_core(ctx, pts, scalars_dev, out_affine, out_is_inf, stream_of(ctx, stream));
}

// batch multiply on a resident set, device buffers: a verified subgroup set takes the endomorphism ladders of
// mulvar_endo.hip (G1: two 128-bit streams along phi; G2: four 64-bit streams along psi), any other set the generic kernel
static int mul_var_resident_core(ncg_ctx* ctx, const ncg_points* pts, const void* d_sc, void* d_out, uint8_t* d_inf, hipStream_t st) {
  const size_t n = pts->n;
  static const bool no_endo = ncg::knob_set("NCG_NO_ENDO");
  const bool bls = pts->curve == NCG_BLS12_381_G1 || pts->curve == NCG_BLS12_381_G2;
  if (pts->d_endo && bls && !no_endo) {
    int rc = ensure_mul_ws(ctx, pts->curve, n, st);
    if (rc) return rc;
    if (pts->curve == NCG_BLS12_381_G1)
      NCG_HIP(ctx, ncg::mul_var_batch_g1_subgroup((const uint32_t*)pts->d_pts, (const uint32_t*)d_sc, (uint32_t*)d_out, d_inf, (int)n,
                                                  (uint32_t*)ctx->mul_ws, st));
    else
      NCG_HIP(ctx, ncg::mul_var_batch_g2_subgroup((const uint32_t*)pts->d_pts, (const uint32_t*)d_sc, (uint32_t*)d_out, d_inf, (int)n,
                                                  (uint32_t*)ctx->mul_ws, st));
    return NCG_OK;
  }
  return ncg_mul_var_batch_dev(ctx, pts->curve, n, pts->d_pts, d_sc, d_out, d_inf, st);
}

int ncg_mul_var_batch_resident_dev(ncg_ctx* ctx, const ncg_points* pts, const void* scalars_dev, void* out_affine_dev,
                                   uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, handle_rule(ctx, "mul_var_batch_resident", pts), pts->n, scalars_dev, out_affine_dev, out_is_inf_dev);
  return mul_var_resident_core(ctx, pts, scalars_dev, out_affine_dev, out_is_inf_dev, stream_of(ctx, stream));
}

int ncg_mul_var_batch_resident(ncg_ctx* ctx, const ncg_points* pts, const void* scalars, void* out_affine,
                               uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, handle_rule(ctx, "mul_var_batch_resident", pts), pts->n, scalars, out_affine);
  const size_t n = pts->n;
  HostCall hc(ctx);
  const int sc = hc.in(scalars, n * 32);
  const int o = hc.out(out_affine, n * (size_t)ncg_point_bytes(pts->curve)), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(mul_var_resident_core(ctx, pts, hc.dev(sc), hc.dev(o), hc.dev<uint8_t>(f), ctx->stream));
}

// decode on the device, then sum through the MSM path with unit scalars; nothing but the encodings
// goes up and one point (plus the verdicts) comes back
int ncg_aggregate_encoded(ncg_ctx* ctx, int curve, size_t n, const void* encoded, int flags, void* out_affine,
                          uint8_t* out_is_inf, int64_t* out_bad_index) {
  if (out_bad_index) *out_bad_index = -1;
  NCG_BEGIN_OR(ctx, encoded_rule(ctx, "aggregate_encoded", curve), n, msm_identity(ctx, curve, out_affine, out_is_inf), encoded,
               out_affine);
  std::vector<uint8_t> ok(n);
  HostCall hc(ctx);
  const int in = hc.in(encoded, n * (size_t)ncg::decode_in_bytes(curve)), dok = hc.out(ok.data(), n);
  const int pts = hc.dev_only(n * (size_t)ncg_point_bytes(curve)), sc = hc.dev_only(n * 32), inf = hc.dev_only(n);
  if (int rc = hc.stage()) return rc;
  if (int rc = ncg_decode_points_batch_dev(ctx, curve, n, hc.dev(in), flags, hc.dev(pts), hc.dev<uint8_t>(dok), hc.dev<uint8_t>(inf),
                                           ctx->stream))
    return rc;
  NCG_HIP(ctx, hipMemsetAsync(hc.dev(sc), 0, n * 32, ctx->stream));
  NCG_HIP(ctx, hipMemset2DAsync(hc.dev(sc), 32, 1, 1, n, ctx->stream));  // scalar 1 in every 32-byte row
  if (int rc = hc.finish(NCG_OK)) return rc;
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) {  // the reference throws while decoding (Point.fromBytes / assertValidity)
      if (out_bad_index) *out_bad_index = (int64_t)i;
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: aggregate_encoded: invalid point encoding at index %zu", i);
    }
  return ncg_msm_dev(ctx, curve, n, hc.dev(pts), hc.dev(sc), out_affine, out_is_inf, ctx->stream);
}

int ncg_normalize_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* points_proj_dev, void* out_affine_dev,
                            uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, normalize_rule(ctx, curve), n, points_proj_dev, out_affine_dev, out_is_inf_dev);
  NCG_HIP(ctx, ncg::normalize_batch(curve, (const uint32_t*)points_proj_dev, (uint32_t*)out_affine_dev, out_is_inf_dev,
                                    (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}

int ncg_normalize_batch(ncg_ctx* ctx, int curve, size_t n, const void* points_proj, void* out_affine,
                        uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, normalize_rule(ctx, curve), n, points_proj, out_affine);
  const size_t pb = (size_t)ncg_point_bytes(curve);
  HostCall hc(ctx);
  const int in = hc.in(points_proj, n * (pb / 2) * 3);
  const int o = hc.out(out_affine, n * pb), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_normalize_batch_dev(ctx, curve, n, hc.dev(in), hc.dev(o), hc.dev<uint8_t>(f), ctx->stream));
}

int ncg_decode_points_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* encoded_dev, int flags,
                                void* out_affine_dev, uint8_t* out_ok_dev, uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, encoded_rule(ctx, "decode_points_batch", curve), n, encoded_dev, out_affine_dev, out_ok_dev, out_is_inf_dev);
  NCG_HIP(ctx, ncg::decode_points_batch(curve, (const uint8_t*)encoded_dev, flags, (uint32_t*)out_affine_dev, out_ok_dev,
                                        out_is_inf_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}

int ncg_decode_points_batch(ncg_ctx* ctx, int curve, size_t n, const void* encoded, int flags, void* out_affine,
                            uint8_t* out_ok, uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, encoded_rule(ctx, "decode_points_batch", curve), n, encoded, out_affine, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(encoded, n * (size_t)ncg::decode_in_bytes(curve));
  const int o = hc.out(out_affine, n * (size_t)ncg_point_bytes(curve)), ok = hc.out(out_ok, n), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_decode_points_batch_dev(ctx, curve, n, hc.dev(in), flags, hc.dev(o), hc.dev<uint8_t>(ok), hc.dev<uint8_t>(f),
                                               ctx->stream));
}

int ncg_encode_points_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* affine_dev, void* out_encoded_dev,
                                uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, encoded_rule(ctx, "encode_points_batch", curve), n, affine_dev, out_encoded_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::encode_points_batch(curve, (const uint32_t*)affine_dev, (uint8_t*)out_encoded_dev, out_ok_dev, (int)n,
                                        stream_of(ctx, stream)));
  return NCG_OK;
}

int ncg_encode_points_batch(ncg_ctx* ctx, int curve, size_t n, const void* affine, void* out_encoded, uint8_t* out_ok) {
  NCG_BEGIN(ctx, encoded_rule(ctx, "encode_points_batch", curve), n, affine, out_encoded, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(affine, n * (size_t)ncg_point_bytes(curve));
  const int o = hc.out(out_encoded, n * (size_t)ncg::decode_in_bytes(curve)), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_encode_points_batch_dev(ctx, curve, n, hc.dev(in), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}

int ncg_map_to_curve_batch_dev(ncg_ctx* ctx, int curve, size_t n, int count, const void* u_dev, void* out_affine_dev,
                               uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, map_rule(ctx, curve, count), n, u_dev, out_affine_dev, out_is_inf_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_mul_ws(ctx, curve, n, st)) return rc;  // Jacobian scratch for the batched affine conversion
  NCG_HIP(ctx, ncg::map_to_curve_batch(curve, (const uint32_t*)u_dev, count, (uint32_t*)out_affine_dev, out_is_inf_dev,
                                       (int)n, (uint32_t*)ctx->mul_ws, st));
  return NCG_OK;
}

int ncg_map_to_curve_batch(ncg_ctx* ctx, int curve, size_t n, int count, const void* u, void* out_affine,
                           uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, map_rule(ctx, curve, count), n, u, out_affine);
  const size_t pb = (size_t)ncg_point_bytes(curve);
  HostCall hc(ctx);
  const int in = hc.in(u, n * (size_t)count * (pb / 2));
  const int o = hc.out(out_affine, n * pb), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_map_to_curve_batch_dev(ctx, curve, n, count, hc.dev(in), hc.dev(o), hc.dev<uint8_t>(f), ctx->stream));
}

// twiddle table for (field, log2n, omega): built on first use, rebuilt if a different root is passed; the two fields
// keep their tables side by side
static int ntt_field_slot(int field) { return field == NCG_FIELD_BN254_FR ? 1 : 0; }
static int ensure_ntt_table(ncg_ctx* ctx, int field, int log2n, const uint32_t* omega) {
  uint32_t*& slot = ctx->ntt_tab[ntt_field_slot(field)][log2n];
  uint32_t(&slot_omega)[8] = ctx->ntt_omega[ntt_field_slot(field)][log2n];
  if (slot && memcmp(slot_omega, omega, 32) == 0) return NCG_OK;
  if (slot) {
    NCG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(slot);
    slot = nullptr;
  }
  uint32_t* tab = nullptr;
  void* tmp = nullptr;
  hipError_t e = hipMalloc((void**)&tab, ncg::ntt_table_bytes(log2n));
  if (e != hipSuccess) return set_err(ctx, NCG_ERR_NOMEM, "noble-gpu: ntt table hipMalloc failed: %s", hipGetErrorString(e));
  e = hipMalloc(&tmp, ncg::ntt_small_bytes(log2n) + 32);
  if (e != hipSuccess) {
    (void)hipFree(tab);
    return set_err(ctx, NCG_ERR_NOMEM, "noble-gpu: ntt table hipMalloc failed: %s", hipGetErrorString(e));
  }
  uint32_t* d_omega = (uint32_t*)tmp;
  uint32_t* d_small = d_omega + 8;
  alignas(16) uint32_t probe[16] = {0}, expect_tw[16] = {0};
  const int tww = ncg::ntt_tw_words();
  e = hipMemcpyAsync(d_omega, omega, 32, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = ncg::ntt_build_table(field, log2n, d_omega, d_small, tab, ctx->stream);
  // primitive-root check: omega^(N/2) == -1 (N = 1: omega == 1); table entries are x 2^261 mod r
  const size_t probe_idx = log2n ? ((size_t)1 << (log2n - 1)) : 0;
  if (e == hipSuccess) e = hipMemcpyAsync(probe, tab + probe_idx * tww, (size_t)tww * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) {
    (void)hipFree(tab);
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: ntt table build failed: %s", hipGetErrorString(e));
  }
  uint32_t expect[8];  // entries are x 2^261 mod r (ntt.hip): K261 for +1, r - K261 for -1, r and K261 of this field
  const uint32_t *fp, *fk;
  ncg::ntt_field_consts(field, &fp, &fk);
  if (log2n == 0) {
    for (int i = 0; i < 8; i++) expect[i] = fk[i];
  } else {
    uint64_t bw = 0;
    for (int i = 0; i < 8; i++) {
      uint64_t d = (uint64_t)fp[i] - fk[i] - bw;
      expect[i] = (uint32_t)d;
      bw = (d >> 32) & 1;
    }
  }
  ncg::ntt_tw_from_canonical(expect, expect_tw);
  if (memcmp(probe, expect_tw, (size_t)tww * 4) != 0) {
    (void)hipFree(tab);
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ntt: omega is not a primitive 2^%d-th root of unity", log2n);
  }
  slot = tab;
  memcpy(slot_omega, omega, 32);
  return NCG_OK;
}

int ncg_ntt_dev(ncg_ctx* ctx, int field, int log2n, size_t batch, const void* omega, const void* in_dev, void* out_dev,
                int flags, void* stream) {
  NCG_BEGIN(ctx, ntt_rule(ctx, field, log2n, batch), batch, omega, in_dev, out_dev);
  if (misaligned16(in_dev) || misaligned16(out_dev)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ntt: device buffers must be 16-byte aligned");
  if (int rc = ensure_ntt_table(ctx, field, log2n, (const uint32_t*)omega)) return rc;
  const bool fold = ((flags >> 1) & 1) == ((flags >> 2) & 1);
  const size_t bytes = (batch << log2n) * 32;
  if (fold && log2n > 10) {
    if (int rc = ncg_grow_buf(ctx, &ctx->ntt_ws, &ctx->ntt_ws_bytes, bytes, bytes, GrowWait::device)) return rc;
  }
  NCG_HIP(ctx, ncg::ntt_run(field, log2n, batch, (const uint32_t*)in_dev, (uint32_t*)out_dev, (uint32_t*)ctx->ntt_ws,
                            ctx->ntt_tab[ntt_field_slot(field)][log2n], log2n, flags, stream_of(ctx, stream)));
  return NCG_OK;
}

int ncg_ntt(ncg_ctx* ctx, int field, int log2n, size_t batch, const void* omega, const void* in, void* out, int flags) {
  NCG_BEGIN(ctx, ntt_rule(ctx, field, log2n, batch), batch, omega, in, out);
  HostCall hc(ctx);
  const int io = hc.inout(in, out, (batch << log2n) * 32);  // batch <= 2^16, log2n <= 28: below 2^49
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ntt_dev(ctx, field, log2n, batch, omega, hc.dev(io), hc.dev(io), flags, ctx->stream));
}

// ---- polynomial arithmetic on field vectors (poly.hip).  The _dev forms work on ctx->poly_ws, never on ctx->scratch.
static int poly_misaligned(ncg_ctx* ctx, std::initializer_list<const void*> bufs) {
  for (const void* p : bufs)
    if (misaligned16(p)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly: device buffers must be 16-byte aligned");
  return NCG_OK;
}
static int poly_ensure_ws(ncg_ctx* ctx, int log2n_mul) {
  const size_t need = ncg::poly_ws_bytes(log2n_mul);
  return ncg_grow_buf(ctx, &ctx->poly_ws, &ctx->poly_ws_bytes, need, need, GrowWait::device);
}
// the evaluations of an empty polynomial are F.ZERO (fft.ts:859, :876): written, not refused, so the output is required even then
static int poly_zero(ncg_ctx* ctx, void* out, size_t bytes, bool dev, void* stream) {
  if (!out) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly: NULL output");
  if (!dev) {
    memset(out, 0, bytes);
    return NCG_OK;
  }
  NCG_HIP(ctx, hipSetDevice(ctx->device));
  NCG_HIP(ctx, hipMemsetAsync(out, 0, bytes, stream_of(ctx, stream)));
  return NCG_OK;
}

int ncg_poly_pointwise_dev(ncg_ctx* ctx, int field, int op, size_t n, const void* a_dev, const void* b_dev, void* out_dev, void* stream) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_POINTWISE, field, op, 0, 1, 0, 0), n, a_dev, b_dev, out_dev);
  if (int rc = poly_misaligned(ctx, {a_dev, b_dev, out_dev})) return rc;
  NCG_HIP(ctx, ncg::poly_pointwise(field, op, n, (const uint32_t*)a_dev, (const uint32_t*)b_dev, (uint32_t*)out_dev, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_poly_pointwise(ncg_ctx* ctx, int field, int op, size_t n, const void* a, const void* b, void* out) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_POINTWISE, field, op, 0, 1, 0, 0), n, a, b, out);
  HostCall hc(ctx);
  const int ia = hc.inout(a, out, n * 32), ib = hc.in(b, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_poly_pointwise_dev(ctx, field, op, n, hc.dev(ia), hc.dev(ib), hc.dev(ia), ctx->stream));
}

int ncg_poly_scale_dev(ncg_ctx* ctx, int field, size_t n, const void* a_dev, const void* scalar, int powers, void* out_dev, void* stream) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_SCALE, field, powers, 0, 1, 0, 0), n, a_dev, scalar, out_dev);
  if (int rc = poly_misaligned(ctx, {a_dev, out_dev})) return rc;
  NCG_HIP(ctx, ncg::poly_scale(field, n, (const uint32_t*)a_dev, (const uint32_t*)scalar, powers, (uint32_t*)out_dev, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_poly_scale(ncg_ctx* ctx, int field, size_t n, const void* a, const void* scalar, int powers, void* out) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_SCALE, field, powers, 0, 1, 0, 0), n, a, scalar, out);
  HostCall hc(ctx);
  const int io = hc.inout(a, out, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_poly_scale_dev(ctx, field, n, hc.dev(io), scalar, powers, hc.dev(io), ctx->stream));
}

int ncg_poly_eval_dev(ncg_ctx* ctx, int field, size_t n, const void* a_dev, const void* basis_dev, void* out32_dev, void* stream) {
  NCG_BEGIN_OR(ctx, poly_rule(ctx, POLY_EVAL, field, 0, 0, 1, 0, 0), n, poly_zero(ctx, out32_dev, 32, true, stream), a_dev, basis_dev, out32_dev);
  if (int rc = poly_misaligned(ctx, {a_dev, basis_dev, out32_dev})) return rc;
  if (int rc = poly_ensure_ws(ctx, -1)) return rc;
  NCG_HIP(ctx, ncg::poly_eval(field, n, (const uint32_t*)a_dev, (const uint32_t*)basis_dev, ctx->poly_ws, (uint32_t*)out32_dev, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_poly_eval(ncg_ctx* ctx, int field, size_t n, const void* a, const void* basis, void* out32) {
  NCG_BEGIN_OR(ctx, poly_rule(ctx, POLY_EVAL, field, 0, 0, 1, 0, 0), n, poly_zero(ctx, out32, 32, false, nullptr), a, basis, out32);
  HostCall hc(ctx);
  const int ia = hc.in(a, n * 32), ib = hc.in(basis, n * 32), o = hc.out(out32, 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_poly_eval_dev(ctx, field, n, hc.dev(ia), hc.dev(ib), hc.dev(o), ctx->stream));
}

int ncg_poly_eval_monomial_dev(ncg_ctx* ctx, int field, size_t n, const void* a_dev, int m, const void* xs, void* out_dev, void* stream) {
  NCG_BEGIN_OR(ctx, poly_rule(ctx, POLY_EVAL_MONOMIAL, field, 0, 0, m, 0, 0), n, poly_zero(ctx, out_dev, (size_t)m * 32, true, stream), a_dev, xs,
               out_dev);
  if (int rc = poly_misaligned(ctx, {a_dev, out_dev})) return rc;
  if (int rc = poly_ensure_ws(ctx, -1)) return rc;
  NCG_HIP(ctx, ncg::poly_eval_monomial(field, n, (const uint32_t*)a_dev, m, (const uint32_t*)xs, ctx->poly_ws, (uint32_t*)out_dev,
                                       stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_poly_eval_monomial(ncg_ctx* ctx, int field, size_t n, const void* a, int m, const void* xs, void* out) {
  NCG_BEGIN_OR(ctx, poly_rule(ctx, POLY_EVAL_MONOMIAL, field, 0, 0, m, 0, 0), n, poly_zero(ctx, out, (size_t)m * 32, false, nullptr), a, xs, out);
  HostCall hc(ctx);
  const int ia = hc.in(a, n * 32), o = hc.out(out, (size_t)m * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_poly_eval_monomial_dev(ctx, field, n, hc.dev(ia), m, xs, hc.dev(o), ctx->stream));
}

int ncg_poly_lagrange_basis_dev(ncg_ctx* ctx, int field, int log2n, const void* omega, const void* x, int brp, void* out_dev, void* stream) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_LAGRANGE, field, 0, log2n, 1, 0, 0), 1, omega, x, out_dev);
  if (int rc = poly_misaligned(ctx, {out_dev})) return rc;
  if (int rc = ensure_ntt_table(ctx, field, log2n, (const uint32_t*)omega)) return rc;
  if (int rc = poly_ensure_ws(ctx, -1)) return rc;
  NCG_HIP(ctx, ncg::poly_lagrange_basis(field, log2n, ctx->ntt_tab[ntt_field_slot(field)][log2n], (const uint32_t*)x, brp ? 1 : 0, ctx->poly_ws,
                                        (uint32_t*)out_dev, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_poly_lagrange_basis(ncg_ctx* ctx, int field, int log2n, const void* omega, const void* x, int brp, void* out) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_LAGRANGE, field, 0, log2n, 1, 0, 0), 1, omega, x, out);
  HostCall hc(ctx);
  const int o = hc.out(out, (size_t)32 << log2n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_poly_lagrange_basis_dev(ctx, field, log2n, omega, x, brp, hc.dev(o), ctx->stream));
}

int ncg_poly_mul_dev(ncg_ctx* ctx, int field, int log2n, const void* omega, size_t na, const void* a_dev, size_t nb, const void* b_dev,
                     void* out_dev, void* stream) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_MUL, field, 0, log2n, 1, na, nb), 1, omega, out_dev);
  if ((na && !a_dev) || (nb && !b_dev)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly_mul: NULL buffer");
  if (int rc = poly_misaligned(ctx, {a_dev, b_dev, out_dev})) return rc;
  if (int rc = ensure_ntt_table(ctx, field, log2n, (const uint32_t*)omega)) return rc;
  if (int rc = poly_ensure_ws(ctx, log2n)) return rc;
  NCG_HIP(ctx, ncg::poly_mul(field, log2n, ctx->ntt_tab[ntt_field_slot(field)][log2n], na, (const uint32_t*)a_dev, nb, (const uint32_t*)b_dev,
                             ctx->poly_ws, (uint32_t*)out_dev, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_poly_mul(ncg_ctx* ctx, int field, int log2n, const void* omega, size_t na, const void* a, size_t nb, const void* b, void* out) {
  NCG_BEGIN(ctx, poly_rule(ctx, POLY_MUL, field, 0, log2n, 1, na, nb), 1, omega, out);
  if ((na && !a) || (nb && !b)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: poly_mul: NULL buffer");
  HostCall hc(ctx);
  const int ia = hc.in(a, na * 32), ib = hc.in(b, nb * 32), o = hc.out(out, (size_t)32 << log2n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_poly_mul_dev(ctx, field, log2n, omega, na, hc.dev(ia), nb, hc.dev(ib), hc.dev(o), ctx->stream));
}

static int ensure_ed_table(ncg_ctx* ctx) {
  if (ctx->ed_btab) return NCG_OK;
  uint32_t host[ncg::ED25519_BTAB_WORDS];
  ncg::ed25519_build_base_table(host);
  NCG_HIP(ctx, hipMalloc((void**)&ctx->ed_btab, sizeof host));
  NCG_HIP(ctx, hipMemcpy(ctx->ed_btab, host, sizeof host, hipMemcpyHostToDevice));
  return NCG_OK;
}

int ncg_ed25519_verify_batch_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* pk32_dev,
                                 const void* k32_dev, int zip215, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ed25519_verify_batch"), n, sig64_dev, pk32_dev, k32_dev, out_ok_dev);
  if (int rc = ensure_ed_table(ctx)) return rc;
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_mul_ws(ctx, NCG_ED25519, n, st)) return rc;  // per-item window tables live in the multiply scratch
  NCG_HIP(ctx, ncg::ed25519_verify_batch((const uint32_t*)sig64_dev, (const uint32_t*)pk32_dev,
                                         (const uint32_t*)k32_dev, ctx->ed_btab, zip215, out_ok_dev, (int)n,
                                         (uint32_t*)ctx->mul_ws, st));
  return NCG_OK;
}

int ncg_ed25519_verify_batch(ncg_ctx* ctx, size_t n, const void* sig64, const void* pk32, const void* k32,
                             int zip215, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("ed25519_verify_batch"), n, sig64, pk32, k32, out_ok);
  HostCall hc(ctx);
  const int sig = hc.in(sig64, n * 64), pk = hc.in(pk32, n * 32), k = hc.in(k32, n * 32), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed25519_verify_batch_dev(ctx, n, hc.dev(sig), hc.dev(pk), hc.dev(k), zip215, hc.dev<uint8_t>(ok), ctx->stream));
}

// ---- ed25519 verify from messages: the challenge hash runs on the device too
int ncg_ed25519_challenge_batch_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* pk32_dev, const void* msgs_dev,
                                    const uint64_t* msg_off_dev, void* out_k32_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ed25519_challenge"), n, sig64_dev, pk32_dev, msg_off_dev, out_k32_dev);
  NCG_HIP(ctx, ncg::ed25519_challenge_batch((const uint8_t*)sig64_dev, (const uint8_t*)pk32_dev, (const uint8_t*)msgs_dev,
                                            msg_off_dev, (uint32_t*)out_k32_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}

int ncg_ed25519_verify_batch_msgs_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* pk32_dev,
                                      const void* msgs_dev, const uint64_t* msg_off_dev, int zip215, uint8_t* out_ok_dev,
                                      void* stream) {
  NCG_BEGIN(ctx, no_rule("ed25519_verify_msgs"), n, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ncg_grow_buf(ctx, &ctx->ed_ks, &ctx->ed_ks_bytes, n * 32, n * 40, GrowWait::stream, st)) return rc;
  if (int rc = ncg_ed25519_challenge_batch_dev(ctx, n, sig64_dev, pk32_dev, msgs_dev, msg_off_dev, ctx->ed_ks, st)) return rc;
  return ncg_ed25519_verify_batch_dev(ctx, n, sig64_dev, pk32_dev, ctx->ed_ks, zip215, out_ok_dev, st);
}

// The message blob of the message-taking host forms: the offsets must not decrease and a non-empty blob needs its buffer;
// the blob goes up from its first message, with the offsets made relative to it in `rel` (declared before `hc`).
static int stage_msgs(HostCall& hc, const char* op, size_t n, const void* msgs, const uint64_t* msg_off, std::vector<uint64_t>& rel,
                      int* d_msg, int* d_off) {
  for (size_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i])
      return set_err(hc.ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: offsets must not decrease (index %zu)", op, i);
  const size_t mbytes = (size_t)(msg_off[n] - msg_off[0]);
  if (mbytes && !msgs) return set_err(hc.ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: NULL message buffer", op);
  rel.resize(n + 1);
  for (size_t i = 0; i <= n; i++) rel[i] = msg_off[i] - msg_off[0];
  *d_off = hc.in(rel.data(), (n + 1) * 8);
  *d_msg = hc.in(mbytes ? (const char*)msgs + msg_off[0] : nullptr, mbytes);
  return NCG_OK;
}

int ncg_ed25519_verify_batch_msgs(ncg_ctx* ctx, size_t n, const void* sig64, const void* pk32, const void* msgs,
                                  const uint64_t* msg_off, int zip215, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("ed25519_verify_msgs"), n, sig64, pk32, msg_off, out_ok);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  const int sig = hc.in(sig64, n * 64), pk = hc.in(pk32, n * 32);
  int msg, off;
  if (int rc = stage_msgs(hc, "ed25519_verify_msgs", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed25519_verify_batch_msgs_dev(ctx, n, hc.dev(sig), hc.dev(pk), hc.dev(msg), hc.dev<const uint64_t>(off), zip215,
                                                     hc.dev<uint8_t>(ok), ctx->stream));
}

// ---- Ed25519 signing (ed25519_sign.hip): getPublicKey, getExtendedPublicKey and sign for ed25519 / ed25519ctx / ed25519ph.
// Expanded rows, public keys and signatures are read and written as 32-bit words (seeds byte by byte): a device pointer to them must be 4-byte
// aligned and is refused otherwise (the host forms stage every buffer at a 256-byte boundary).  The workspace holds scalars,
// prefixes and nonces during a call: it is cleared on the call's stream before the call returns, and so is the staged copy of the
// keys of a host form.
static int ensure_ed_scan_table(ncg_ctx* ctx) {
  if (ctx->ed_scan_tab) return NCG_OK;
  std::vector<uint32_t> host(ncg::ed25519_scan_table_words());
  ncg::ed25519_build_scan_table(host.data());
  uint32_t* tab = nullptr;
  NCG_HIP(ctx, hipMalloc((void**)&tab, host.size() * 4));
  hipError_t e = hipMemcpy(tab, host.data(), host.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(tab);
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: uploading the ed25519 signing table failed: %s", hipGetErrorString(e));
  }
  ctx->ed_scan_tab = tab;
  return NCG_OK;
}
constexpr int ED_SIGN_FLAGS = NCG_ED25519_SIGN_EXPANDED | NCG_ED25519_SIGN_ONE_KEY | NCG_ED25519_SIGN_PREHASH;
// the rule of the EdDSA signers (Ed25519 here, Ed448 below): the flag bits the entry point knows, dom, and the rows it reads as words
static Rule eddsa_sign_rule(ncg_ctx* ctx, const char* op, int flags, int known_flags, const void* dom, size_t dom_len, size_t dom_max,
                            const char* what_rows, std::initializer_list<const void*> word_rows) {
  int rc = NCG_OK;
  if (flags & ~known_flags) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: unknown flag bits 0x%x", op, flags);
  else if (dom_len > dom_max) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: dom_len %zu above %d", op, dom_len, (int)dom_max);
  else if (dom_len && !dom) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: NULL buffer (dom)", op);
  else
    for (const void* p : word_rows)
      if ((uintptr_t)p & 3) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: %s must be 4-byte aligned", op, what_rows);
  return {op, rc};
}
static Rule ed_sign_rule(ncg_ctx* ctx, const char* op, int flags, const void* dom, size_t dom_len, std::initializer_list<const void*> word_rows) {
  return eddsa_sign_rule(ctx, op, flags, ED_SIGN_FLAGS, dom, dom_len, NCG_ED25519_DOM_MAX, "key and signature rows", word_rows);
}
static int ed_sign_ws(ncg_ctx* ctx, size_t words) {
  return ncg_grow_buf(ctx, &ctx->ed_sign_ws, &ctx->ed_sign_ws_bytes, words * 4, words * 4 + (words >> 1) + 4096, GrowWait::device);
}
// seeds (read byte by byte) -> public keys (rows false: 8 words per row at `out`) or expanded rows (rows true: 24 words per row)
static int ed_expand_dev(ncg_ctx* ctx, const char* op, size_t n, const void* seed32_dev, void* out_dev, bool rows, void* stream) {
  NCG_BEGIN(ctx, ed_sign_rule(ctx, op, 0, nullptr, 0, {out_dev}), n, seed32_dev, out_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_ed_scan_table(ctx)) return rc;
  uint32_t* keys = (uint32_t*)out_dev;
  if (!rows) {  // scalar || prefix stay in the workspace, only A goes out
    if (int rc = ed_sign_ws(ctx, n * 24)) return rc;
    keys = (uint32_t*)ctx->ed_sign_ws;
  }
  hipError_t e = ncg::ed25519_expand_batch(ctx->ed_scan_tab, (const uint8_t*)seed32_dev, keys, rows ? keys + 16 : (uint32_t*)out_dev, rows ? 24 : 8,
                                           (int)n, st);
  if (!rows) (void)hipMemsetAsync(ctx->ed_sign_ws, 0, n * 96, st);
  NCG_HIP(ctx, e);
  return NCG_OK;
}
int ncg_ed25519_public_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed32_dev, void* out_pk32_dev, void* stream) {
  return ed_expand_dev(ctx, "ed25519_public_key_batch", n, seed32_dev, out_pk32_dev, false, stream);
}
int ncg_ed25519_expand_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed32_dev, void* out_key96_dev, void* stream) {
  return ed_expand_dev(ctx, "ed25519_expand_key_batch", n, seed32_dev, out_key96_dev, true, stream);
}
// the staged copy of the keys of a host form, cleared on the context's stream on every way out once anything was enqueued
static void ed_clear_staged(HostCall& hc, int slot, size_t bytes) {
  if (hc.enqueued && bytes) (void)hipMemsetAsync(hc.dev(slot), 0, bytes, hc.ctx->stream);
}
static int ed_expand_host(ncg_ctx* ctx, const char* op, size_t n, const void* seed32, void* out, size_t out_bytes) {
  NCG_BEGIN(ctx, no_rule(op), n, seed32, out);
  HostCall hc(ctx);
  const int s = hc.in(seed32, n * 32), o = hc.out(out, n * out_bytes);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, s, n * 32);
    return rc;
  }
  const int rc = out_bytes == 32 ? ncg_ed25519_public_key_batch_dev(ctx, n, hc.dev(s), hc.dev(o), ctx->stream)
                                 : ncg_ed25519_expand_key_batch_dev(ctx, n, hc.dev(s), hc.dev(o), ctx->stream);
  ed_clear_staged(hc, s, n * 32);
  const int frc = hc.finish(rc);
  if (out_bytes == 96 && frc == NCG_OK) (void)hipMemsetAsync(hc.dev(o), 0, n * 96, ctx->stream);   // after the copy back, same stream
  return frc;
}
int ncg_ed25519_public_key_batch(ncg_ctx* ctx, size_t n, const void* seed32, void* out_pk32) {
  return ed_expand_host(ctx, "ed25519_public_key_batch", n, seed32, out_pk32, 32);
}
int ncg_ed25519_expand_key_batch(ncg_ctx* ctx, size_t n, const void* seed32, void* out_key96) {
  return ed_expand_host(ctx, "ed25519_expand_key_batch", n, seed32, out_key96, 96);
}

int ncg_ed25519_sign_batch_dev(ncg_ctx* ctx, size_t n, const void* keys_dev, int flags, const void* dom, size_t dom_len, const void* msgs_dev,
                               const uint64_t* msg_off_dev, void* out_sig64_dev, uint8_t* out_ok_dev, void* stream) {
  // seeds are read byte by byte; expanded rows and signatures as words
  NCG_BEGIN(ctx, ed_sign_rule(ctx, "ed25519_sign_batch", flags, dom, dom_len, {(flags & NCG_ED25519_SIGN_EXPANDED) ? keys_dev : nullptr, out_sig64_dev}),
            n, keys_dev, msg_off_dev, out_sig64_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_ed_scan_table(ctx)) return rc;
  const int expanded = (flags & NCG_ED25519_SIGN_EXPANDED) != 0, one_key = (flags & NCG_ED25519_SIGN_ONE_KEY) != 0;
  const int prehash = (flags & NCG_ED25519_SIGN_PREHASH) != 0;
  const size_t words = ncg::ed25519_sign_ws_words((int)n, expanded ? 0 : (one_key ? 1 : (int)n), prehash);
  if (int rc = ed_sign_ws(ctx, words)) return rc;
  hipError_t e = ncg::ed25519_sign_batch(ctx->ed_scan_tab, keys_dev, expanded, one_key, prehash, (const uint8_t*)dom, (uint32_t)dom_len,
                                         (const uint8_t*)msgs_dev, msg_off_dev, (uint32_t*)out_sig64_dev, out_ok_dev, (int)n,
                                         (uint32_t*)ctx->ed_sign_ws, st);
  (void)hipMemsetAsync(ctx->ed_sign_ws, 0, words * 4, st);
  NCG_HIP(ctx, e);
  return NCG_OK;
}
int ncg_ed25519_sign_batch(ncg_ctx* ctx, size_t n, const void* keys, int flags, const void* dom, size_t dom_len, const void* msgs,
                           const uint64_t* msg_off, void* out_sig64, uint8_t* out_ok) {
  NCG_BEGIN(ctx, ed_sign_rule(ctx, "ed25519_sign_batch", flags, dom, dom_len, {}), n, keys, msg_off, out_sig64, out_ok);
  const size_t kbytes = ((flags & NCG_ED25519_SIGN_ONE_KEY) ? 1 : n) * ((flags & NCG_ED25519_SIGN_EXPANDED) ? 96 : 32);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  const int k = hc.in(keys, kbytes);
  int msg, off;
  if (int rc = stage_msgs(hc, "ed25519_sign_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int sig = hc.out(out_sig64, n * 64), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, k, kbytes);
    return rc;
  }
  const int rc = ncg_ed25519_sign_batch_dev(ctx, n, hc.dev(k), flags, dom, dom_len, hc.dev(msg), hc.dev<const uint64_t>(off), hc.dev(sig),
                                            hc.dev<uint8_t>(ok), ctx->stream);
  ed_clear_staged(hc, k, kbytes);
  return hc.finish(rc);
}

// ---- secp256k1 ECDSA batch verify (weierstrass.ts:1571-1620): SEC1 decode of the keys, the scalar side
// (ecdsa.hip), u1 G by the fixed-base table, u2 P by the variable-base ladder, one pairwise add, compare.
struct SigWs {  // device buffers of the signature pipelines (ECDSA, Schnorr)
  char *pub, *A, *B, *R, *u1, *u2, *pub33, *hash;
  uint8_t *pub_ok, *pub_inf, *pre_ok, *A_inf, *B_inf, *R_inf;
};
static int sig_ws(ncg_ctx* ctx, size_t n, hipStream_t st, SigWs* w) {
  const size_t pt_b = align256(n * 64), sc_b = align256(n * 32), fl_b = align256(n), pk_b = align256(n * 33);
  const size_t need = 4 * pt_b + 3 * sc_b + 6 * fl_b + pk_b;
  if (int rc = ncg_grow_buf(ctx, &ctx->ecdsa_ws, &ctx->ecdsa_ws_bytes, need, need + (need >> 2), GrowWait::stream, st)) return rc;
  char* p = (char*)ctx->ecdsa_ws;
  w->pub = p;    p += pt_b;
  w->A = p;      p += pt_b;
  w->B = p;      p += pt_b;
  w->R = p;      p += pt_b;
  w->u1 = p;     p += sc_b;
  w->u2 = p;     p += sc_b;
  w->pub33 = p;  p += pk_b;
  w->hash = p;   p += sc_b;
  w->pub_ok = (uint8_t*)p;   p += fl_b;
  w->pub_inf = (uint8_t*)p;  p += fl_b;
  w->pre_ok = (uint8_t*)p;   p += fl_b;
  w->A_inf = (uint8_t*)p;    p += fl_b;
  w->B_inf = (uint8_t*)p;    p += fl_b;
  w->R_inf = (uint8_t*)p;
  return NCG_OK;
}
// R = u1 G + u2 P for decoded keys: fixed-base table, variable-base ladder, one pairwise add
static int sig_mul_add(ncg_ctx* ctx, int curve, size_t n, const SigWs& w, hipStream_t st) {
  int rc = ncg_mul_base_batch_dev(ctx, curve, n, w.u1, w.A, w.A_inf, st);
  if (rc) return rc;
  rc = ncg_mul_var_batch_dev(ctx, curve, n, w.pub, w.u2, w.B, w.B_inf, st);  // rejected keys decode to (0,0) = O
  if (rc) return rc;
  return ncg_add_pairs_batch_dev(ctx, curve, n, w.A, w.B, 0, w.R, w.R_inf, st);
}

int ncg_ecdsa_verify_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* sig64_dev, const void* hash32_dev,
                               const void* pub33_dev, int flags, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, secp_rule(ctx, "ecdsa_verify", curve), n, sig64_dev, hash32_dev, pub33_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  SigWs w;
  if (int rc = sig_ws(ctx, n, st, &w)) return rc;
  if (flags & NCG_ECDSA_PUB_UNCOMPRESSED) {  // 65-byte keys: range + curve-equation check, no square root
    NCG_HIP(ctx, ncg::secp_load_uncompressed((const uint8_t*)pub33_dev, (uint32_t*)w.pub, w.pub_ok, w.pub_inf, (int)n, st));
  } else {
    if (int rc = ncg_decode_points_batch_dev(ctx, curve, n, pub33_dev, 0, w.pub, w.pub_ok, w.pub_inf, st)) return rc;
  }
  NCG_HIP(ctx, ncg::ecdsa_prepare((const uint8_t*)sig64_dev, (const uint8_t*)hash32_dev, (int)n, (flags & NCG_ECDSA_LOW_S) != 0,
                                  (uint32_t*)w.u1, (uint32_t*)w.u2, w.pre_ok, st));
  if (int rc = sig_mul_add(ctx, curve, n, w, st)) return rc;
  NCG_HIP(ctx, ncg::ecdsa_finish((const uint8_t*)sig64_dev, (const uint32_t*)w.R, w.R_inf, w.pre_ok, w.pub_ok, w.pub_inf, (int)n,
                                 out_ok_dev, st));
  return NCG_OK;
}

// Q[i] = recoverPublicKey(sig65[i], hash[i]) as an affine wire point, out_ok[i] = 0 where the reference throws
int ncg_ecdsa_recover_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* sig65_dev, const void* hash32_dev,
                                void* out_affine_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, secp_rule(ctx, "ecdsa_recover", curve), n, sig65_dev, hash32_dev, out_affine_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  SigWs w;
  if (int rc = sig_ws(ctx, n, st, &w)) return rc;
  NCG_HIP(ctx, ncg::ecdsa_recover_prepare((const uint8_t*)sig65_dev, (const uint8_t*)hash32_dev, (int)n, (uint32_t*)w.u1, (uint32_t*)w.u2,
                                          (uint8_t*)w.pub33, w.pre_ok, st));
  int rc = ncg_decode_points_batch_dev(ctx, curve, n, w.pub33, 0, w.pub, w.pub_ok, w.pub_inf, st);  // R from (x, parity)
  if (rc) return rc;
  rc = ncg_mul_base_batch_dev(ctx, curve, n, w.u1, w.A, w.A_inf, st);
  if (rc) return rc;
  rc = ncg_mul_var_batch_dev(ctx, curve, n, w.pub, w.u2, w.B, w.B_inf, st);
  if (rc) return rc;
  rc = ncg_add_pairs_batch_dev(ctx, curve, n, w.A, w.B, 0, out_affine_dev, w.R_inf, st);
  if (rc) return rc;
  NCG_HIP(ctx, ncg::ecdsa_recover_finish((uint32_t*)out_affine_dev, w.R_inf, w.pre_ok, w.pub_ok, (int)n, out_ok_dev, st));
  return NCG_OK;
}

int ncg_ecdsa_recover_batch(ncg_ctx* ctx, int curve, size_t n, const void* sig65, const void* hash32, void* out_affine,
                            uint8_t* out_ok) {
  NCG_BEGIN(ctx, secp_rule(ctx, "ecdsa_recover", curve), n, sig65, hash32, out_affine, out_ok);
  HostCall hc(ctx);
  const int sig = hc.in(sig65, n * 65), hash = hc.in(hash32, n * 32), o = hc.out(out_affine, n * 64), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ecdsa_recover_batch_dev(ctx, curve, n, hc.dev(sig), hc.dev(hash), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}

int ncg_schnorr_verify_batch_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* e32_dev, const void* pkx32_dev,
                                 uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("schnorr_verify"), n, sig64_dev, e32_dev, pkx32_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  SigWs w;
  if (int rc = sig_ws(ctx, n, st, &w)) return rc;
  NCG_HIP(ctx, ncg::schnorr_prepare((const uint8_t*)sig64_dev, (const uint8_t*)e32_dev, (const uint8_t*)pkx32_dev, (int)n,
                                    (uint32_t*)w.u1, (uint32_t*)w.u2, (uint8_t*)w.pub33, w.pre_ok, st));
  int rc = ncg_decode_points_batch_dev(ctx, NCG_SECP256K1, n, w.pub33, 0, w.pub, w.pub_ok, w.pub_inf, st);  // lift_x: the even root
  if (rc) return rc;
  rc = sig_mul_add(ctx, NCG_SECP256K1, n, w, st);
  if (rc) return rc;
  NCG_HIP(ctx, ncg::schnorr_finish((const uint8_t*)sig64_dev, (const uint32_t*)w.R, w.R_inf, w.pre_ok, w.pub_ok, w.pub_inf, (int)n,
                                   out_ok_dev, st));
  return NCG_OK;
}

// ---- the same from messages: SHA-256 on the device (csrc/sha256.hpp) - the prehash of ecdsa.verify and the BIP-340
// tagged challenge - then the entry points above
int ncg_ecdsa_verify_batch_msgs_dev(ncg_ctx* ctx, int curve, size_t n, const void* sig64_dev, const void* msgs_dev,
                                    const uint64_t* msg_off_dev, const void* pub_dev, int flags, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, secp_rule(ctx, "ecdsa_verify_msgs", curve), n, sig64_dev, msg_off_dev, pub_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  SigWs w;
  if (int rc = sig_ws(ctx, n, st, &w)) return rc;
  NCG_HIP(ctx, ncg::sha256_msgs((const uint8_t*)msgs_dev, msg_off_dev, nullptr, nullptr, 0, (int)n, (uint8_t*)w.hash, st));
  return ncg_ecdsa_verify_batch_dev(ctx, curve, n, sig64_dev, w.hash, pub_dev, flags, out_ok_dev, st);
}

int ncg_schnorr_verify_batch_msgs_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* msgs_dev,
                                      const uint64_t* msg_off_dev, const void* pkx32_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("schnorr_verify_msgs"), n, sig64_dev, msg_off_dev, pkx32_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  SigWs w;
  if (int rc = sig_ws(ctx, n, st, &w)) return rc;
  NCG_HIP(ctx, ncg::sha256_msgs((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)sig64_dev, (const uint8_t*)pkx32_dev, 1, (int)n,
                                (uint8_t*)w.hash, st));
  return ncg_schnorr_verify_batch_dev(ctx, n, sig64_dev, w.hash, pkx32_dev, out_ok_dev, st);
}

// host-pointer variants: mode 0 = ECDSA (keys: kb bytes per row), mode 1 = Schnorr (32-byte x-only keys)
static int sig_verify_msgs_host(ncg_ctx* ctx, Rule rule, int mode, size_t n, const void* sig64, const void* msgs,
                                const uint64_t* msg_off, const void* keys, size_t kb, int flags, uint8_t* out_ok) {
  NCG_BEGIN(ctx, rule, n, sig64, msg_off, keys, out_ok);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  const int sig = hc.in(sig64, n * 64), key = hc.in(keys, n * kb);
  int msg, off;
  if (int rc = stage_msgs(hc, rule.op, n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  const uint64_t* d_off = hc.dev<const uint64_t>(off);
  return hc.finish(mode == 0 ? ncg_ecdsa_verify_batch_msgs_dev(ctx, NCG_SECP256K1, n, hc.dev(sig), hc.dev(msg), d_off, hc.dev(key), flags,
                                                               hc.dev<uint8_t>(ok), ctx->stream)
                             : ncg_schnorr_verify_batch_msgs_dev(ctx, n, hc.dev(sig), hc.dev(msg), d_off, hc.dev(key), hc.dev<uint8_t>(ok),
                                                                 ctx->stream));
}
int ncg_ecdsa_verify_batch_msgs(ncg_ctx* ctx, int curve, size_t n, const void* sig64, const void* msgs, const uint64_t* msg_off,
                                const void* pub, int flags, uint8_t* out_ok) {
  return sig_verify_msgs_host(ctx, secp_rule(ctx, "ecdsa_verify_msgs", curve), 0, n, sig64, msgs, msg_off, pub,
                              (flags & NCG_ECDSA_PUB_UNCOMPRESSED) ? 65 : 33, flags, out_ok);
}
int ncg_schnorr_verify_batch_msgs(ncg_ctx* ctx, size_t n, const void* sig64, const void* msgs, const uint64_t* msg_off,
                                  const void* pkx32, uint8_t* out_ok) {
  return sig_verify_msgs_host(ctx, no_rule("schnorr_verify_msgs"), 1, n, sig64, msgs, msg_off, pkx32, 32, 0, out_ok);
}

int ncg_schnorr_verify_batch(ncg_ctx* ctx, size_t n, const void* sig64, const void* e32, const void* pkx32, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("schnorr_verify"), n, sig64, e32, pkx32, out_ok);
  HostCall hc(ctx);
  const int sig = hc.in(sig64, n * 64), e = hc.in(e32, n * 32), pk = hc.in(pkx32, n * 32), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_schnorr_verify_batch_dev(ctx, n, hc.dev(sig), hc.dev(e), hc.dev(pk), hc.dev<uint8_t>(ok), ctx->stream));
}

int ncg_ecdsa_verify_batch(ncg_ctx* ctx, int curve, size_t n, const void* sig64, const void* hash32, const void* pub33, int flags,
                           uint8_t* out_ok) {
  NCG_BEGIN(ctx, secp_rule(ctx, "ecdsa_verify", curve), n, sig64, hash32, pub33, out_ok);
  const size_t kb = (flags & NCG_ECDSA_PUB_UNCOMPRESSED) ? 65 : 33;  // bytes per key row
  HostCall hc(ctx);
  const int sig = hc.in(sig64, n * 64), hash = hc.in(hash32, n * 32), pub = hc.in(pub33, n * kb), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ecdsa_verify_batch_dev(ctx, curve, n, hc.dev(sig), hc.dev(hash), hc.dev(pub), flags, hc.dev<uint8_t>(ok), ctx->stream));
}

// ---- secp256k1 signing (secp256k1_sign.hip): getPublicKey, ECDSA sign with RFC 6979 nonces, BIP-340 sign.  Every row is read and
// written byte by byte, so no pointer has an alignment rule.  The workspace holds keys, nonces and the DRBG's state during a call: it
// is cleared on the call's stream before the call returns, and so are the staged copies of the keys and the extra entropy of a
// host form.
static int ensure_secp_scan_table(ncg_ctx* ctx) {
  if (ctx->secp_scan_tab) return NCG_OK;
  std::vector<uint32_t> host(ncg::secp_scan_table_words());
  ncg::secp_build_scan_table(host.data());
  uint32_t* tab = nullptr;
  NCG_HIP(ctx, hipMalloc((void**)&tab, host.size() * 4));
  hipError_t e = hipMemcpy(tab, host.data(), host.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(tab);
    return set_err(ctx, NCG_ERR_HIP, "noble-gpu: uploading the secp256k1 signing table failed: %s", hipGetErrorString(e));
  }
  ctx->secp_scan_tab = tab;
  return NCG_OK;
}
static int secp_sign_ws(ncg_ctx* ctx, size_t words) {
  return ncg_grow_buf(ctx, &ctx->secp_sign_ws, &ctx->secp_sign_ws_bytes, words * 4, words * 4 + (words >> 1) + 4096, GrowWait::device);
}
// the rule of the signing entry points: the curve (where the entry point takes one) and the flag bits it knows
static Rule secp_sign_rule(ncg_ctx* ctx, const char* op, int curve, int flags, int known_flags) {
  Rule r = secp_rule(ctx, op, curve);
  if (r.rc == NCG_OK && (flags & ~known_flags)) r.rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: unknown flag bits 0x%x", op, flags);
  return r;
}
static Rule secp_pk_rule(ncg_ctx* ctx, int flags) {
  return {"secp256k1_public_key_batch", flags >= NCG_SECP_PK_COMPRESSED && flags <= NCG_SECP_PK_XONLY
                                            ? NCG_OK
                                            : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: secp256k1_public_key_batch: unknown flags 0x%x", flags)};
}
static size_t secp_pk_row_bytes(int flags) { return flags == NCG_SECP_PK_UNCOMPRESSED ? 65 : flags == NCG_SECP_PK_XONLY ? 32 : 33; }

int ncg_secp256k1_public_key_batch_dev(ncg_ctx* ctx, size_t n, const void* sk32_dev, int flags, void* out_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, secp_pk_rule(ctx, flags), n, sk32_dev, out_dev, out_ok_dev);
  if (int rc = ensure_secp_scan_table(ctx)) return rc;
  NCG_HIP(ctx, ncg::secp_public_key_batch(ctx->secp_scan_tab, (const uint8_t*)sk32_dev, flags, (uint8_t*)out_dev, out_ok_dev, (int)n,
                                          stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_secp256k1_public_key_batch(ncg_ctx* ctx, size_t n, const void* sk32, int flags, void* out, uint8_t* out_ok) {
  NCG_BEGIN(ctx, secp_pk_rule(ctx, flags), n, sk32, out, out_ok);
  HostCall hc(ctx);
  const int s = hc.in(sk32, n * 32), o = hc.out(out, n * secp_pk_row_bytes(flags)), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, s, n * 32);
    return rc;
  }
  const int rc = ncg_secp256k1_public_key_batch_dev(ctx, n, hc.dev(s), flags, hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream);
  ed_clear_staged(hc, s, n * 32);
  return hc.finish(rc);
}

constexpr int ECDSA_SIGN_FLAGS = NCG_ECDSA_LOW_S | NCG_SECP_SIGN_ONE_KEY;
// hash32_dev, or (msgs_dev, msg_off_dev) with hash32_dev NULL: the prehash then runs first, into the workspace
static int ecdsa_sign_dev(ncg_ctx* ctx, size_t n, const void* sk32_dev, const void* hash32_dev, const void* msgs_dev, const uint64_t* msg_off_dev,
                          const void* extra32_dev, int flags, void* out_sig64_dev, uint8_t* out_recid_dev, uint8_t* out_ok_dev, hipStream_t st) {
  if (int rc = ensure_secp_scan_table(ctx)) return rc;
  const size_t row_words = ncg::secp_sign_ws_words((int)n, 0), words = row_words + (hash32_dev ? 0 : n * 8);
  if (int rc = secp_sign_ws(ctx, words)) return rc;
  uint32_t* ws = (uint32_t*)ctx->secp_sign_ws;
  hipError_t e = hipSuccess;
  if (!hash32_dev) {
    e = ncg::sha256_msgs((const uint8_t*)msgs_dev, msg_off_dev, nullptr, nullptr, 0, (int)n, (uint8_t*)(ws + row_words), st);
    hash32_dev = ws + row_words;
  }
  if (e == hipSuccess)
    e = ncg::ecdsa_sign_batch(ctx->secp_scan_tab, (const uint8_t*)sk32_dev, (flags & NCG_SECP_SIGN_ONE_KEY) != 0, (const uint8_t*)hash32_dev,
                              (const uint8_t*)extra32_dev, (flags & NCG_ECDSA_LOW_S) != 0, (uint8_t*)out_sig64_dev, out_recid_dev, out_ok_dev,
                              (int)n, ws, st);
  (void)hipMemsetAsync(ctx->secp_sign_ws, 0, words * 4, st);
  NCG_HIP(ctx, e);
  return NCG_OK;
}
int ncg_ecdsa_sign_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* sk32_dev, const void* hash32_dev, const void* extra32_dev, int flags,
                             void* out_sig64_dev, uint8_t* out_recid_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, secp_sign_rule(ctx, "ecdsa_sign_batch", curve, flags, ECDSA_SIGN_FLAGS), n, sk32_dev, hash32_dev, out_sig64_dev, out_ok_dev);
  return ecdsa_sign_dev(ctx, n, sk32_dev, hash32_dev, nullptr, nullptr, extra32_dev, flags, out_sig64_dev, out_recid_dev, out_ok_dev,
                        stream_of(ctx, stream));
}
int ncg_ecdsa_sign_batch_msgs_dev(ncg_ctx* ctx, int curve, size_t n, const void* sk32_dev, const void* msgs_dev, const uint64_t* msg_off_dev,
                                  const void* extra32_dev, int flags, void* out_sig64_dev, uint8_t* out_recid_dev, uint8_t* out_ok_dev,
                                  void* stream) {
  NCG_BEGIN(ctx, secp_sign_rule(ctx, "ecdsa_sign_batch_msgs", curve, flags, ECDSA_SIGN_FLAGS), n, sk32_dev, msg_off_dev, out_sig64_dev, out_ok_dev);
  return ecdsa_sign_dev(ctx, n, sk32_dev, nullptr, msgs_dev, msg_off_dev, extra32_dev, flags, out_sig64_dev, out_recid_dev, out_ok_dev,
                        stream_of(ctx, stream));
}
// the host forms of both: hash32, or (msgs, msg_off) with hash32 NULL
static int ecdsa_sign_host(ncg_ctx* ctx, Rule rule, int curve, size_t n, const void* sk32, const void* hash32, const void* msgs,
                           const uint64_t* msg_off, const void* extra32, int flags, void* out_sig64, uint8_t* out_recid, uint8_t* out_ok) {
  NCG_BEGIN(ctx, rule, n, sk32, msg_off ? (const void*)msg_off : hash32, out_sig64, out_ok);
  const size_t kbytes = ((flags & NCG_SECP_SIGN_ONE_KEY) ? 1 : n) * 32, xbytes = extra32 ? n * 32 : 0;
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  const int k = hc.in(sk32, kbytes), x = hc.in(extra32, xbytes);
  int h = -1, msg = -1, off = -1;
  if (msg_off) {
    if (int rc = stage_msgs(hc, rule.op, n, msgs, msg_off, rel, &msg, &off)) return rc;
  } else {
    h = hc.in(hash32, n * 32);
  }
  const int sig = hc.out(out_sig64, n * 64), rec = hc.out(out_recid, n), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, k, kbytes);
    ed_clear_staged(hc, x, xbytes);
    return rc;
  }
  uint8_t* d_rec = out_recid ? hc.dev<uint8_t>(rec) : nullptr;
  const void* d_x = extra32 ? hc.dev(x) : nullptr;
  const int rc = msg_off ? ncg_ecdsa_sign_batch_msgs_dev(ctx, curve, n, hc.dev(k), hc.dev(msg), hc.dev<const uint64_t>(off), d_x, flags, hc.dev(sig),
                                                         d_rec, hc.dev<uint8_t>(ok), ctx->stream)
                         : ncg_ecdsa_sign_batch_dev(ctx, curve, n, hc.dev(k), hc.dev(h), d_x, flags, hc.dev(sig), d_rec, hc.dev<uint8_t>(ok),
                                                    ctx->stream);
  ed_clear_staged(hc, k, kbytes);
  ed_clear_staged(hc, x, xbytes);
  return hc.finish(rc);
}
int ncg_ecdsa_sign_batch(ncg_ctx* ctx, int curve, size_t n, const void* sk32, const void* hash32, const void* extra32, int flags, void* out_sig64,
                         uint8_t* out_recid, uint8_t* out_ok) {
  return ecdsa_sign_host(ctx, secp_sign_rule(ctx, "ecdsa_sign_batch", curve, flags, ECDSA_SIGN_FLAGS), curve, n, sk32, hash32, nullptr, nullptr,
                         extra32, flags, out_sig64, out_recid, out_ok);
}
int ncg_ecdsa_sign_batch_msgs(ncg_ctx* ctx, int curve, size_t n, const void* sk32, const void* msgs, const uint64_t* msg_off, const void* extra32,
                              int flags, void* out_sig64, uint8_t* out_recid, uint8_t* out_ok) {
  const Rule rule = secp_sign_rule(ctx, "ecdsa_sign_batch_msgs", curve, flags, ECDSA_SIGN_FLAGS);
  if (ctx && rule.rc == NCG_OK && n && !msg_off) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ecdsa_sign_batch_msgs: NULL buffer");
  return ecdsa_sign_host(ctx, rule, curve, n, sk32, nullptr, msgs, msg_off, extra32, flags, out_sig64, out_recid, out_ok);
}

int ncg_schnorr_sign_batch_dev(ncg_ctx* ctx, size_t n, const void* sk32_dev, const void* aux32_dev, const void* msgs_dev, const uint64_t* msg_off_dev,
                               int flags, void* out_sig64_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, secp_sign_rule(ctx, "schnorr_sign_batch", NCG_SECP256K1, flags, NCG_SECP_SIGN_ONE_KEY), n, sk32_dev, aux32_dev, msg_off_dev,
            out_sig64_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_secp_scan_table(ctx)) return rc;
  const int one_key = (flags & NCG_SECP_SIGN_ONE_KEY) != 0;
  const size_t words = ncg::secp_sign_ws_words((int)n, one_key ? 1 : (int)n);
  if (int rc = secp_sign_ws(ctx, words)) return rc;
  hipError_t e = ncg::schnorr_sign_batch(ctx->secp_scan_tab, (const uint8_t*)sk32_dev, one_key, (const uint8_t*)aux32_dev, (const uint8_t*)msgs_dev,
                                         msg_off_dev, (uint8_t*)out_sig64_dev, out_ok_dev, (int)n, (uint32_t*)ctx->secp_sign_ws, st);
  (void)hipMemsetAsync(ctx->secp_sign_ws, 0, words * 4, st);
  NCG_HIP(ctx, e);
  return NCG_OK;
}
int ncg_schnorr_sign_batch(ncg_ctx* ctx, size_t n, const void* sk32, const void* aux32, const void* msgs, const uint64_t* msg_off, int flags,
                           void* out_sig64, uint8_t* out_ok) {
  NCG_BEGIN(ctx, secp_sign_rule(ctx, "schnorr_sign_batch", NCG_SECP256K1, flags, NCG_SECP_SIGN_ONE_KEY), n, sk32, aux32, msg_off, out_sig64, out_ok);
  const size_t kbytes = ((flags & NCG_SECP_SIGN_ONE_KEY) ? 1 : n) * 32;
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  const int k = hc.in(sk32, kbytes), a = hc.in(aux32, n * 32);
  int msg, off;
  if (int rc = stage_msgs(hc, "schnorr_sign_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int sig = hc.out(out_sig64, n * 64), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, k, kbytes);
    ed_clear_staged(hc, a, n * 32);
    return rc;
  }
  const int rc = ncg_schnorr_sign_batch_dev(ctx, n, hc.dev(k), hc.dev(a), hc.dev(msg), hc.dev<const uint64_t>(off), flags, hc.dev(sig),
                                            hc.dev<uint8_t>(ok), ctx->stream);
  ed_clear_staged(hc, k, kbytes);
  ed_clear_staged(hc, a, n * 32);
  return hc.finish(rc);
}

// The pieces of secp256k1_sign.hpp on raw words, in the style of ncg_decaf448_check: an op nobody defines reads nothing and leaves
// rows of 16 zero words.  The rows of workspace the DRBG ops use are a device-only slot, cleared before the call returns.
int ncg_secp256k1_sign_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out) {
  int wa, wb, wo;
  ncg::secp_sign_check_row_words(op, &wa, &wb, &wo);
  int rrc = NCG_OK;
  if (ctx && n > (1u << 24)) rrc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: secp256k1_sign_check: batch too large (max 2^24)");
  else if (ctx && wo && (op == 0 || op == 4) && (variant < 0 || (variant >> 1) > 3))
    rrc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: secp256k1_sign_check: variant %d out of range", variant);
  const Rule rule = {"secp256k1_sign_check", rrc};
  NCG_BEGIN(ctx, rule, n, a, b, out);
  if (wo)
    if (int rc = ensure_secp_scan_table(ctx)) return rc;
  const size_t ws_bytes = ncg::secp_sign_ws_words((int)n, 0) * 4;
  HostCall hc(ctx);
  const int da = hc.in(a, n * wa * 4), db = hc.in(b, n * wb * 4);
  const int o = hc.out(out, n * (wo ? wo : 16) * 4, true), w = hc.dev_only(wo ? ws_bytes : 0);
  if (int rc = hc.stage()) return rc;
  hipError_t e = hipSuccess;
  if (wo) {
    e = ncg::secp_sign_check(op, variant, ctx->secp_scan_tab, hc.dev<uint32_t>(w), hc.dev<const uint32_t>(da), hc.dev<const uint32_t>(db),
                             hc.dev<uint32_t>(o), (int)n, ctx->stream);
    (void)hipMemsetAsync(hc.dev(w), 0, ws_bytes, ctx->stream);
    (void)hipMemsetAsync(hc.dev(da), 0, n * wa * 4, ctx->stream);
  }
  NCG_HIP(ctx, e);
  return hc.finish(NCG_OK);
}

// ---- X25519 (x25519.hip).  Rows are 32 bytes, read as 8 LE words: 4-byte aligned like every other byte row of this ABI.
static Rule x25519_rule(ncg_ctx* ctx, int flags) {
  return {"x25519_batch", (flags & ~NCG_X25519_ONE_SCALAR) == 0 ? NCG_OK
                              : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: x25519_batch: unknown flag bits 0x%x", flags)};
}
int ncg_x25519_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, const void* u_dev, int flags, void* out32_dev,
                         uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, x25519_rule(ctx, flags), n, scalars_dev, u_dev, out32_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::x25519_batch((const uint32_t*)scalars_dev, (const uint32_t*)u_dev, flags & NCG_X25519_ONE_SCALAR, (uint32_t*)out32_dev,
                                 out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_x25519_batch(ncg_ctx* ctx, size_t n, const void* scalars, const void* u, int flags, void* out32, uint8_t* out_ok) {
  NCG_BEGIN(ctx, x25519_rule(ctx, flags), n, scalars, u, out32, out_ok);
  HostCall hc(ctx);
  const int sc = hc.in(scalars, (flags & NCG_X25519_ONE_SCALAR) ? 32 : n * 32), du = hc.in(u, n * 32);
  const int o = hc.out(out32, n * 32), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_x25519_batch_dev(ctx, n, hc.dev(sc), hc.dev(du), flags, hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_x25519_base_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, void* out32_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("x25519_base_batch"), n, scalars_dev, out32_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  const size_t need = ncg::x25519_base_tmp_words((int)n) * 4;
  if (int rc = ncg_grow_buf(ctx, &ctx->mul_ws, &ctx->mul_ws_bytes, need, need, GrowWait::stream, st, true)) return rc;
  if (int rc = ensure_ed_base_table(ctx)) return rc;
  NCG_HIP(ctx, ncg::x25519_base_batch(ctx->base_tab[NCG_ED25519], (const uint32_t*)scalars_dev, (uint32_t*)out32_dev, out_ok_dev, (int)n,
                                      (uint32_t*)ctx->mul_ws, st));
  return NCG_OK;
}
int ncg_x25519_base_batch(ncg_ctx* ctx, size_t n, const void* scalars, void* out32, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("x25519_base_batch"), n, scalars, out32, out_ok);
  HostCall hc(ctx);
  const int sc = hc.in(scalars, n * 32), o = hc.out(out32, n * 32), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_x25519_base_batch_dev(ctx, n, hc.dev(sc), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_ed25519_to_montgomery_batch_dev(ncg_ctx* ctx, size_t n, const void* pk32_dev, void* out32_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ed25519_to_montgomery_batch"), n, pk32_dev, out32_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::ed25519_to_montgomery_batch((const uint32_t*)pk32_dev, (uint32_t*)out32_dev, out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed25519_to_montgomery_batch(ncg_ctx* ctx, size_t n, const void* pk32, void* out32, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("ed25519_to_montgomery_batch"), n, pk32, out32, out_ok);
  HostCall hc(ctx);
  const int pk = hc.in(pk32, n * 32), o = hc.out(out32, n * 32), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed25519_to_montgomery_batch_dev(ctx, n, hc.dev(pk), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}

// ---- X448 and Ed448 (ed448.hip).  56-byte rows (scalars, u coordinates, the halves of an affine point) are read as 14 LE words: a
// device pointer to them must be 4-byte aligned and is refused otherwise; encodings (57 bytes) and signatures (114) are packed and
// read byte by byte.  The host forms stage every buffer at a 256-byte boundary, so host memory may sit at any address.
static Rule ed448_rule(ncg_ctx* ctx, const char* op, int flags, int known_flags, std::initializer_list<const void*> word_rows) {
  int rc = NCG_OK;
  if (flags & ~known_flags) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: unknown flag bits 0x%x", op, flags);
  else
    for (const void* p : word_rows)
      if ((uintptr_t)p & 3) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: 56-byte rows must be 4-byte aligned", op);
  return {op, rc};
}
static Rule ed448_flags_rule(ncg_ctx* ctx, const char* op, int flags, int known_flags) { return ed448_rule(ctx, op, flags, known_flags, {}); }

int ncg_x448_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, const void* u_dev, int flags, void* out56_dev, uint8_t* out_ok_dev,
                       void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "x448_batch", flags, NCG_X448_ONE_SCALAR, {scalars_dev, u_dev, out56_dev}), n, scalars_dev, u_dev, out56_dev,
            out_ok_dev);
  NCG_HIP(ctx, ncg::x448_batch((const uint32_t*)scalars_dev, (const uint32_t*)u_dev, flags & NCG_X448_ONE_SCALAR, (uint32_t*)out56_dev, out_ok_dev,
                               (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_x448_batch(ncg_ctx* ctx, size_t n, const void* scalars, const void* u, int flags, void* out56, uint8_t* out_ok) {
  NCG_BEGIN(ctx, ed448_flags_rule(ctx, "x448_batch", flags, NCG_X448_ONE_SCALAR), n, scalars, u, out56, out_ok);
  HostCall hc(ctx);
  const int sc = hc.in(scalars, (flags & NCG_X448_ONE_SCALAR) ? 56 : n * 56), du = hc.in(u, n * 56);
  const int o = hc.out(out56, n * 56), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_x448_batch_dev(ctx, n, hc.dev(sc), hc.dev(du), flags, hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_x448_base_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, void* out56_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "x448_base_batch", 0, 0, {scalars_dev, out56_dev}), n, scalars_dev, out56_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::x448_batch((const uint32_t*)scalars_dev, nullptr, 0, (uint32_t*)out56_dev, out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_x448_base_batch(ncg_ctx* ctx, size_t n, const void* scalars, void* out56, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("x448_base_batch"), n, scalars, out56, out_ok);
  HostCall hc(ctx);
  const int sc = hc.in(scalars, n * 56), o = hc.out(out56, n * 56), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_x448_base_batch_dev(ctx, n, hc.dev(sc), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_ed448_decode_batch_dev(ncg_ctx* ctx, size_t n, const void* enc57_dev, void* out_affine112_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "ed448_decode_batch", 0, 0, {out_affine112_dev}), n, enc57_dev, out_affine112_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::ed448_decode_batch((const uint8_t*)enc57_dev, (uint32_t*)out_affine112_dev, out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_decode_batch(ncg_ctx* ctx, size_t n, const void* enc57, void* out_affine112, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("ed448_decode_batch"), n, enc57, out_affine112, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(enc57, n * 57), o = hc.out(out_affine112, n * 112), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_decode_batch_dev(ctx, n, hc.dev(in), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_ed448_encode_batch_dev(ncg_ctx* ctx, size_t n, const void* affine112_dev, void* out57_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "ed448_encode_batch", 0, 0, {affine112_dev}), n, affine112_dev, out57_dev);
  NCG_HIP(ctx, ncg::ed448_encode_batch((const uint32_t*)affine112_dev, (uint8_t*)out57_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_encode_batch(ncg_ctx* ctx, size_t n, const void* affine112, void* out57) {
  NCG_BEGIN(ctx, no_rule("ed448_encode_batch"), n, affine112, out57);
  HostCall hc(ctx);
  const int in = hc.in(affine112, n * 112), o = hc.out(out57, n * 57);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_encode_batch_dev(ctx, n, hc.dev(in), hc.dev(o), ctx->stream));
}
int ncg_ed448_add_pairs_batch_dev(ncg_ctx* ctx, size_t n, const void* a112_dev, const void* b112_dev, int subtract, void* out112_dev,
                                  void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "ed448_add_pairs_batch", 0, 0, {a112_dev, b112_dev, out112_dev}), n, a112_dev, b112_dev, out112_dev);
  NCG_HIP(ctx, ncg::ed448_add_pairs_batch((const uint32_t*)a112_dev, (const uint32_t*)b112_dev, subtract != 0, (uint32_t*)out112_dev, (int)n,
                                          stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_add_pairs_batch(ncg_ctx* ctx, size_t n, const void* a112, const void* b112, int subtract, void* out112) {
  NCG_BEGIN(ctx, no_rule("ed448_add_pairs_batch"), n, a112, b112, out112);
  HostCall hc(ctx);
  const int da = hc.in(a112, n * 112), db = hc.in(b112, n * 112), o = hc.out(out112, n * 112);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_add_pairs_batch_dev(ctx, n, hc.dev(da), hc.dev(db), subtract, hc.dev(o), ctx->stream));
}
int ncg_ed448_mul_batch_dev(ncg_ctx* ctx, size_t n, const void* enc57_dev, const void* k56_dev, int flags, void* out57_dev, uint8_t* out_ok_dev,
                            void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "ed448_mul_batch", flags, NCG_ED448_ONE_SCALAR, {k56_dev}), n, enc57_dev, k56_dev, out57_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::ed448_mul_batch((const uint8_t*)enc57_dev, (const uint32_t*)k56_dev, flags & NCG_ED448_ONE_SCALAR, (uint8_t*)out57_dev,
                                    out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_mul_batch(ncg_ctx* ctx, size_t n, const void* enc57, const void* k56, int flags, void* out57, uint8_t* out_ok) {
  NCG_BEGIN(ctx, ed448_flags_rule(ctx, "ed448_mul_batch", flags, NCG_ED448_ONE_SCALAR), n, enc57, k56, out57, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(enc57, n * 57), k = hc.in(k56, (flags & NCG_ED448_ONE_SCALAR) ? 56 : n * 56);
  const int o = hc.out(out57, n * 57), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_mul_batch_dev(ctx, n, hc.dev(in), hc.dev(k), flags, hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_ed448_mul_base_batch_dev(ncg_ctx* ctx, size_t n, const void* k56_dev, void* out57_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "ed448_mul_base_batch", 0, 0, {k56_dev}), n, k56_dev, out57_dev);
  NCG_HIP(ctx, ncg::ed448_mul_batch(nullptr, (const uint32_t*)k56_dev, 0, (uint8_t*)out57_dev, nullptr, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_mul_base_batch(ncg_ctx* ctx, size_t n, const void* k56, void* out57) {
  NCG_BEGIN(ctx, no_rule("ed448_mul_base_batch"), n, k56, out57);
  HostCall hc(ctx);
  const int k = hc.in(k56, n * 56), o = hc.out(out57, n * 57);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_mul_base_batch_dev(ctx, n, hc.dev(k), hc.dev(o), ctx->stream));
}
int ncg_ed448_to_montgomery_batch_dev(ncg_ctx* ctx, size_t n, const void* pk57_dev, void* out56_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "ed448_to_montgomery_batch", 0, 0, {out56_dev}), n, pk57_dev, out56_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::ed448_to_montgomery_batch((const uint8_t*)pk57_dev, (uint32_t*)out56_dev, out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_to_montgomery_batch(ncg_ctx* ctx, size_t n, const void* pk57, void* out56, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("ed448_to_montgomery_batch"), n, pk57, out56, out_ok);
  HostCall hc(ctx);
  const int pk = hc.in(pk57, n * 57), o = hc.out(out56, n * 56), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_to_montgomery_batch_dev(ctx, n, hc.dev(pk), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_ed448_verify_batch_dev(ncg_ctx* ctx, size_t n, const void* sig114_dev, const void* pk57_dev, const void* k56_dev, uint8_t* out_ok_dev,
                               void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "ed448_verify_batch", 0, 0, {k56_dev}), n, sig114_dev, pk57_dev, k56_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::ed448_verify_batch((const uint8_t*)sig114_dev, (const uint8_t*)pk57_dev, (const uint32_t*)k56_dev, out_ok_dev, (int)n,
                                       stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_verify_batch(ncg_ctx* ctx, size_t n, const void* sig114, const void* pk57, const void* k56, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("ed448_verify_batch"), n, sig114, pk57, k56, out_ok);
  HostCall hc(ctx);
  const int sig = hc.in(sig114, n * 114), pk = hc.in(pk57, n * 57), k = hc.in(k56, n * 56), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_verify_batch_dev(ctx, n, hc.dev(sig), hc.dev(pk), hc.dev(k), hc.dev<uint8_t>(ok), ctx->stream));
}

// ---- SHAKE256, Ed448 signing and verification from messages (ed448_sign.hip).  Seeds, public keys and signatures are packed bytes at
// any address; expanded key rows and challenges are read and written as words and refused when misaligned on the device.  The
// workspace holds scalars, prefixes and nonces during a signing call: it is cleared on the call's stream before the call returns,
// and so is the staged copy of the keys of a host form.
constexpr int ED448_SIGN_FLAGS = NCG_ED448_SIGN_EXPANDED | NCG_ED448_SIGN_ONE_KEY | NCG_ED448_PREHASH;
static Rule ed448_sign_rule(ncg_ctx* ctx, const char* op, int flags, int known_flags, const void* dom, size_t dom_len,
                            std::initializer_list<const void*> word_rows) {
  return eddsa_sign_rule(ctx, op, flags, known_flags, dom, dom_len, NCG_ED448_DOM_MAX, "key rows and 56-byte rows", word_rows);
}
static Rule shake256_rule(ncg_ctx* ctx, size_t out_len) {
  return {"shake256_batch", out_len >= 1 && out_len <= 65535
                                ? NCG_OK
                                : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: shake256_batch: out_len %zu out of range 1..65535", out_len)};
}
static int ed448_ws(ncg_ctx* ctx, size_t words) {
  return ncg_grow_buf(ctx, &ctx->ed448_ws, &ctx->ed448_ws_bytes, words * 4, words * 4 + (words >> 1) + 4096, GrowWait::device);
}
int ncg_shake256_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, size_t out_len, void* out_dev,
                           void* stream) {
  NCG_BEGIN(ctx, shake256_rule(ctx, out_len), n, msg_off_dev, out_dev);
  NCG_HIP(ctx, ncg::shake256_batch((const uint8_t*)msgs_dev, msg_off_dev, (uint32_t)out_len, (uint8_t*)out_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_shake256_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, size_t out_len, void* out) {
  NCG_BEGIN(ctx, shake256_rule(ctx, out_len), n, msg_off, out);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "shake256_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out, n * out_len);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_shake256_batch_dev(ctx, n, hc.dev(msg), hc.dev<const uint64_t>(off), out_len, hc.dev(o), ctx->stream));
}

int ncg_ed448_challenge_batch_dev(ncg_ctx* ctx, size_t n, const void* sig114_dev, const void* pk57_dev, int flags, const void* dom,
                                  size_t dom_len, const void* msgs_dev, const uint64_t* msg_off_dev, void* out_k56_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_sign_rule(ctx, "ed448_challenge_batch", flags, NCG_ED448_PREHASH, dom, dom_len, {out_k56_dev}), n, sig114_dev, pk57_dev,
            msg_off_dev, out_k56_dev);
  const int prehash = (flags & NCG_ED448_PREHASH) != 0;
  if (int rc = ed448_ws(ctx, ncg::ed448_challenge_ws_words((int)n, prehash))) return rc;
  NCG_HIP(ctx, ncg::ed448_challenge_batch((const uint8_t*)sig114_dev, (const uint8_t*)pk57_dev, prehash, (const uint8_t*)dom, (uint32_t)dom_len,
                                          (const uint8_t*)msgs_dev, msg_off_dev, (uint32_t*)out_k56_dev, (int)n, (uint32_t*)ctx->ed448_ws,
                                          stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_verify_batch_msgs_dev(ncg_ctx* ctx, size_t n, const void* sig114_dev, const void* pk57_dev, int flags, const void* dom,
                                    size_t dom_len, const void* msgs_dev, const uint64_t* msg_off_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_sign_rule(ctx, "ed448_verify_msgs", flags, NCG_ED448_PREHASH, dom, dom_len, {}), n, sig114_dev, pk57_dev, msg_off_dev,
            out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  const int prehash = (flags & NCG_ED448_PREHASH) != 0;
  const size_t cw = ncg::ed448_challenge_ws_words((int)n, prehash);   // the challenges follow the workspace of their hash
  if (int rc = ed448_ws(ctx, cw + n * 14)) return rc;
  uint32_t* ws = (uint32_t*)ctx->ed448_ws;
  NCG_HIP(ctx, ncg::ed448_challenge_batch((const uint8_t*)sig114_dev, (const uint8_t*)pk57_dev, prehash, (const uint8_t*)dom, (uint32_t)dom_len,
                                          (const uint8_t*)msgs_dev, msg_off_dev, ws + cw, (int)n, ws, st));
  return ncg_ed448_verify_batch_dev(ctx, n, sig114_dev, pk57_dev, ws + cw, out_ok_dev, st);
}
int ncg_ed448_verify_batch_msgs(ncg_ctx* ctx, size_t n, const void* sig114, const void* pk57, int flags, const void* dom, size_t dom_len,
                                const void* msgs, const uint64_t* msg_off, uint8_t* out_ok) {
  NCG_BEGIN(ctx, ed448_sign_rule(ctx, "ed448_verify_msgs", flags, NCG_ED448_PREHASH, dom, dom_len, {}), n, sig114, pk57, msg_off, out_ok);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  const int sig = hc.in(sig114, n * 114), pk = hc.in(pk57, n * 57);
  int msg, off;
  if (int rc = stage_msgs(hc, "ed448_verify_msgs", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_verify_batch_msgs_dev(ctx, n, hc.dev(sig), hc.dev(pk), flags, dom, dom_len, hc.dev(msg), hc.dev<const uint64_t>(off),
                                                   hc.dev<uint8_t>(ok), ctx->stream));
}

// seeds -> public keys (rows false: 57 packed bytes per row at `out`) or expanded rows (rows true: NCG_ED448_KEY_BYTES per row)
static int ed448_expand_dev(ncg_ctx* ctx, const char* op, size_t n, const void* seed57_dev, void* out_dev, bool rows, void* stream) {
  NCG_BEGIN(ctx, ed448_sign_rule(ctx, op, 0, 0, nullptr, 0, {rows ? out_dev : nullptr}), n, seed57_dev, out_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint32_t* keys = (uint32_t*)out_dev;
  if (!rows) {  // scalar || prefix stay in the workspace, only A goes out
    if (int rc = ed448_ws(ctx, n * 43)) return rc;
    keys = (uint32_t*)ctx->ed448_ws;
  }
  hipError_t e = ncg::ed448_expand_batch((const uint8_t*)seed57_dev, keys, rows ? (uint8_t*)keys + 113 : (uint8_t*)out_dev,
                                         rows ? NCG_ED448_KEY_BYTES : 57, (int)n, st);
  if (!rows) (void)hipMemsetAsync(ctx->ed448_ws, 0, n * NCG_ED448_KEY_BYTES, st);
  NCG_HIP(ctx, e);
  return NCG_OK;
}
int ncg_ed448_public_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed57_dev, void* out_pk57_dev, void* stream) {
  return ed448_expand_dev(ctx, "ed448_public_key_batch", n, seed57_dev, out_pk57_dev, false, stream);
}
int ncg_ed448_expand_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed57_dev, void* out_key172_dev, void* stream) {
  return ed448_expand_dev(ctx, "ed448_expand_key_batch", n, seed57_dev, out_key172_dev, true, stream);
}
static int ed448_expand_host(ncg_ctx* ctx, const char* op, size_t n, const void* seed57, void* out, size_t out_bytes) {
  NCG_BEGIN(ctx, no_rule(op), n, seed57, out);
  HostCall hc(ctx);
  const int s = hc.in(seed57, n * 57), o = hc.out(out, n * out_bytes);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, s, n * 57);
    return rc;
  }
  const int rc = out_bytes == 57 ? ncg_ed448_public_key_batch_dev(ctx, n, hc.dev(s), hc.dev(o), ctx->stream)
                                 : ncg_ed448_expand_key_batch_dev(ctx, n, hc.dev(s), hc.dev(o), ctx->stream);
  ed_clear_staged(hc, s, n * 57);
  const int frc = hc.finish(rc);
  if (out_bytes != 57 && frc == NCG_OK) (void)hipMemsetAsync(hc.dev(o), 0, n * out_bytes, ctx->stream);   // after the copy back, same stream
  return frc;
}
int ncg_ed448_public_key_batch(ncg_ctx* ctx, size_t n, const void* seed57, void* out_pk57) {
  return ed448_expand_host(ctx, "ed448_public_key_batch", n, seed57, out_pk57, 57);
}
int ncg_ed448_expand_key_batch(ncg_ctx* ctx, size_t n, const void* seed57, void* out_key172) {
  return ed448_expand_host(ctx, "ed448_expand_key_batch", n, seed57, out_key172, NCG_ED448_KEY_BYTES);
}

int ncg_ed448_sign_batch_dev(ncg_ctx* ctx, size_t n, const void* keys_dev, int flags, const void* dom, size_t dom_len, const void* msgs_dev,
                             const uint64_t* msg_off_dev, void* out_sig114_dev, uint8_t* out_ok_dev, void* stream) {
  // seeds and signatures are read and written byte by byte; expanded rows as words
  NCG_BEGIN(ctx, ed448_sign_rule(ctx, "ed448_sign_batch", flags, ED448_SIGN_FLAGS, dom, dom_len,
                                 {(flags & NCG_ED448_SIGN_EXPANDED) ? keys_dev : nullptr}),
            n, keys_dev, msg_off_dev, out_sig114_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  const int expanded = (flags & NCG_ED448_SIGN_EXPANDED) != 0, one_key = (flags & NCG_ED448_SIGN_ONE_KEY) != 0;
  const int prehash = (flags & NCG_ED448_PREHASH) != 0;
  const size_t words = ncg::ed448_sign_ws_words((int)n, expanded ? 0 : (one_key ? 1 : (int)n), prehash);
  if (int rc = ed448_ws(ctx, words)) return rc;
  hipError_t e = ncg::ed448_sign_batch(keys_dev, expanded, one_key, prehash, (const uint8_t*)dom, (uint32_t)dom_len, (const uint8_t*)msgs_dev,
                                       msg_off_dev, (uint8_t*)out_sig114_dev, out_ok_dev, (int)n, (uint32_t*)ctx->ed448_ws, st);
  (void)hipMemsetAsync(ctx->ed448_ws, 0, words * 4, st);
  NCG_HIP(ctx, e);
  return NCG_OK;
}
int ncg_ed448_sign_batch(ncg_ctx* ctx, size_t n, const void* keys, int flags, const void* dom, size_t dom_len, const void* msgs,
                         const uint64_t* msg_off, void* out_sig114, uint8_t* out_ok) {
  NCG_BEGIN(ctx, ed448_sign_rule(ctx, "ed448_sign_batch", flags, ED448_SIGN_FLAGS, dom, dom_len, {}), n, keys, msg_off, out_sig114, out_ok);
  const size_t kbytes = ((flags & NCG_ED448_SIGN_ONE_KEY) ? 1 : n) * ((flags & NCG_ED448_SIGN_EXPANDED) ? NCG_ED448_KEY_BYTES : 57);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  const int k = hc.in(keys, kbytes);
  int msg, off;
  if (int rc = stage_msgs(hc, "ed448_sign_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int sig = hc.out(out_sig114, n * 114), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, k, kbytes);
    return rc;
  }
  const int rc = ncg_ed448_sign_batch_dev(ctx, n, hc.dev(k), flags, dom, dom_len, hc.dev(msg), hc.dev<const uint64_t>(off), hc.dev(sig),
                                          hc.dev<uint8_t>(ok), ctx->stream);
  ed_clear_staged(hc, k, kbytes);
  return hc.finish(rc);
}

// The pieces of keccak.hpp / ed448_sign.hpp on raw words, in the style of ncg_fe448_check: an op nobody defines reads nothing and
// leaves rows of 16 zero words.  Op 3 takes a key row and a nonce: the staged inputs and the workspace are cleared before the call
// returns.
int ncg_ed448_sign_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out) {
  (void)variant;  // no op has variants
  const Rule rule = {"ed448_sign_check", !ctx || n <= (1u << 24) ? NCG_OK
                                             : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ed448_sign_check: batch too large (max 2^24)")};
  NCG_BEGIN(ctx, rule, n, a, b, out);
  int wa, wb, wo;
  ncg::ed448_sign_check_row_words(op, &wa, &wb, &wo);
  const size_t ws_bytes = wo ? ncg::ed448_sign_check_ws_words() * 4 : 0;
  HostCall hc(ctx);
  const int da = hc.in(a, n * wa * 4), db = hc.in(b, n * wb * 4);
  const int o = hc.out(out, n * (wo ? wo : 16) * 4, true), w = hc.dev_only(ws_bytes);
  if (int rc = hc.stage()) return rc;
  hipError_t e = hipSuccess;
  if (wo) {
    e = ncg::ed448_sign_check(op, hc.dev<const uint32_t>(da), hc.dev<const uint32_t>(db), hc.dev<uint32_t>(o), (int)n, hc.dev<uint32_t>(w),
                              ctx->stream);
    (void)hipMemsetAsync(hc.dev(da), 0, n * wa * 4, ctx->stream);
    if (wb) (void)hipMemsetAsync(hc.dev(db), 0, n * wb * 4, ctx->stream);
  }
  NCG_HIP(ctx, e);
  return hc.finish(NCG_OK);
}

// ---- decaf448 (decaf448.hip).  Every buffer but the flag bytes is made of 56-byte rows read as 14 LE words: the alignment rule of
// the Ed448 family holds for all of them.  Edwards representatives are Ed448 affine points (x || y, 112 bytes).
int ncg_decaf448_decode_batch_dev(ncg_ctx* ctx, size_t n, const void* enc56_dev, void* out_affine112_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "decaf448_decode_batch", 0, 0, {enc56_dev, out_affine112_dev}), n, enc56_dev, out_affine112_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::decaf448_decode_batch((const uint32_t*)enc56_dev, (uint32_t*)out_affine112_dev, out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_decaf448_decode_batch(ncg_ctx* ctx, size_t n, const void* enc56, void* out_affine112, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("decaf448_decode_batch"), n, enc56, out_affine112, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(enc56, n * 56), o = hc.out(out_affine112, n * 112), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_decaf448_decode_batch_dev(ctx, n, hc.dev(in), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_decaf448_encode_batch_dev(ncg_ctx* ctx, size_t n, const void* affine112_dev, void* out56_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "decaf448_encode_batch", 0, 0, {affine112_dev, out56_dev}), n, affine112_dev, out56_dev);
  NCG_HIP(ctx, ncg::decaf448_encode_batch((const uint32_t*)affine112_dev, (uint32_t*)out56_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_decaf448_encode_batch(ncg_ctx* ctx, size_t n, const void* affine112, void* out56) {
  NCG_BEGIN(ctx, no_rule("decaf448_encode_batch"), n, affine112, out56);
  HostCall hc(ctx);
  const int in = hc.in(affine112, n * 112), o = hc.out(out56, n * 56);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_decaf448_encode_batch_dev(ctx, n, hc.dev(in), hc.dev(o), ctx->stream));
}
int ncg_decaf448_equals_batch_dev(ncg_ctx* ctx, size_t n, const void* a112_dev, const void* b112_dev, uint8_t* out_eq_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "decaf448_equals_batch", 0, 0, {a112_dev, b112_dev}), n, a112_dev, b112_dev, out_eq_dev);
  NCG_HIP(ctx, ncg::decaf448_equals_batch((const uint32_t*)a112_dev, (const uint32_t*)b112_dev, out_eq_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_decaf448_equals_batch(ncg_ctx* ctx, size_t n, const void* a112, const void* b112, uint8_t* out_eq) {
  NCG_BEGIN(ctx, no_rule("decaf448_equals_batch"), n, a112, b112, out_eq);
  HostCall hc(ctx);
  const int da = hc.in(a112, n * 112), db = hc.in(b112, n * 112), o = hc.out(out_eq, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_decaf448_equals_batch_dev(ctx, n, hc.dev(da), hc.dev(db), hc.dev<uint8_t>(o), ctx->stream));
}
int ncg_decaf448_from_uniform_batch_dev(ncg_ctx* ctx, size_t n, const void* uniform112_dev, void* out56_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "decaf448_from_uniform_batch", 0, 0, {uniform112_dev, out56_dev}), n, uniform112_dev, out56_dev);
  NCG_HIP(ctx, ncg::decaf448_from_uniform_batch((const uint32_t*)uniform112_dev, (uint32_t*)out56_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_decaf448_from_uniform_batch(ncg_ctx* ctx, size_t n, const void* uniform112, void* out56) {
  NCG_BEGIN(ctx, no_rule("decaf448_from_uniform_batch"), n, uniform112, out56);
  HostCall hc(ctx);
  const int in = hc.in(uniform112, n * 112), o = hc.out(out56, n * 56);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_decaf448_from_uniform_batch_dev(ctx, n, hc.dev(in), hc.dev(o), ctx->stream));
}
int ncg_decaf448_mul_batch_dev(ncg_ctx* ctx, size_t n, const void* enc56_dev, const void* k56_dev, int flags, void* out56_dev,
                               uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "decaf448_mul_batch", flags, NCG_DECAF448_ONE_SCALAR, {enc56_dev, k56_dev, out56_dev}), n, enc56_dev, k56_dev,
            out56_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::decaf448_mul_batch((const uint32_t*)enc56_dev, (const uint32_t*)k56_dev, flags & NCG_DECAF448_ONE_SCALAR, (uint32_t*)out56_dev,
                                       out_ok_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_decaf448_mul_batch(ncg_ctx* ctx, size_t n, const void* enc56, const void* k56, int flags, void* out56, uint8_t* out_ok) {
  NCG_BEGIN(ctx, ed448_flags_rule(ctx, "decaf448_mul_batch", flags, NCG_DECAF448_ONE_SCALAR), n, enc56, k56, out56, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(enc56, n * 56), k = hc.in(k56, (flags & NCG_DECAF448_ONE_SCALAR) ? 56 : n * 56);
  const int o = hc.out(out56, n * 56), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_decaf448_mul_batch_dev(ctx, n, hc.dev(in), hc.dev(k), flags, hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_decaf448_mul_base_batch_dev(ncg_ctx* ctx, size_t n, const void* k56_dev, void* out56_dev, void* stream) {
  NCG_BEGIN(ctx, ed448_rule(ctx, "decaf448_mul_base_batch", 0, 0, {k56_dev, out56_dev}), n, k56_dev, out56_dev);
  NCG_HIP(ctx, ncg::decaf448_mul_batch(nullptr, (const uint32_t*)k56_dev, 0, (uint32_t*)out56_dev, nullptr, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_decaf448_mul_base_batch(ncg_ctx* ctx, size_t n, const void* k56, void* out56) {
  NCG_BEGIN(ctx, no_rule("decaf448_mul_base_batch"), n, k56, out56);
  HostCall hc(ctx);
  const int k = hc.in(k56, n * 56), o = hc.out(out56, n * 56);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_decaf448_mul_base_batch_dev(ctx, n, hc.dev(k), hc.dev(o), ctx->stream));
}

// ---- ristretto255 (ristretto.hip).  Encodings and scalars are rows of 32 bytes read as 8 LE words, Edwards representatives are
// ed25519 wire points.  The _dev forms keep what lies between their kernels in ctx->rist_ws, never in ctx->scratch.
static int ensure_rist_ws(ncg_ctx* ctx, size_t bytes, hipStream_t st) {
  return ncg_grow_buf(ctx, &ctx->rist_ws, &ctx->rist_ws_bytes, bytes, bytes + (bytes >> 2), GrowWait::stream, st);
}
int ncg_ristretto_decode_batch_dev(ncg_ctx* ctx, size_t n, const void* enc_dev, void* out_affine_dev, uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ristretto_decode_batch"), n, enc_dev, out_affine_dev, out_ok_dev);
  NCG_HIP(ctx, ncg::ristretto_decode_batch((const uint32_t*)enc_dev, (uint32_t*)out_affine_dev, out_ok_dev, 0, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ristretto_decode_batch(ncg_ctx* ctx, size_t n, const void* enc, void* out_affine, uint8_t* out_ok) {
  NCG_BEGIN(ctx, no_rule("ristretto_decode_batch"), n, enc, out_affine, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(enc, n * 32), o = hc.out(out_affine, n * 64), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_decode_batch_dev(ctx, n, hc.dev(in), hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
int ncg_ristretto_encode_batch_dev(ncg_ctx* ctx, size_t n, const void* affine_dev, void* out32_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ristretto_encode_batch"), n, affine_dev, out32_dev);
  NCG_HIP(ctx, ncg::ristretto_encode_batch((const uint32_t*)affine_dev, (uint32_t*)out32_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ristretto_encode_batch(ncg_ctx* ctx, size_t n, const void* affine, void* out32) {
  NCG_BEGIN(ctx, no_rule("ristretto_encode_batch"), n, affine, out32);
  HostCall hc(ctx);
  const int in = hc.in(affine, n * 64), o = hc.out(out32, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_encode_batch_dev(ctx, n, hc.dev(in), hc.dev(o), ctx->stream));
}
int ncg_ristretto_equals_batch_dev(ncg_ctx* ctx, size_t n, const void* a_dev, const void* b_dev, uint8_t* out_eq_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ristretto_equals_batch"), n, a_dev, b_dev, out_eq_dev);
  NCG_HIP(ctx, ncg::ristretto_equals_batch((const uint32_t*)a_dev, (const uint32_t*)b_dev, out_eq_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ristretto_equals_batch(ncg_ctx* ctx, size_t n, const void* a, const void* b, uint8_t* out_eq) {
  NCG_BEGIN(ctx, no_rule("ristretto_equals_batch"), n, a, b, out_eq);
  HostCall hc(ctx);
  const int da = hc.in(a, n * 64), db = hc.in(b, n * 64), o = hc.out(out_eq, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_equals_batch_dev(ctx, n, hc.dev(da), hc.dev(db), hc.dev<uint8_t>(o), ctx->stream));
}
// out_affine_dev / out_affine may be NULL: the encodings alone
int ncg_ristretto_from_uniform_batch_dev(ncg_ctx* ctx, size_t n, const void* bytes64_dev, void* out32_dev, void* out_affine_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ristretto_from_uniform_batch"), n, bytes64_dev, out32_dev);
  NCG_HIP(ctx, ncg::ristretto_from_uniform_batch((const uint32_t*)bytes64_dev, (uint32_t*)out32_dev, (uint32_t*)out_affine_dev, (int)n,
                                                 stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ristretto_from_uniform_batch(ncg_ctx* ctx, size_t n, const void* bytes64, void* out32, void* out_affine) {
  NCG_BEGIN(ctx, no_rule("ristretto_from_uniform_batch"), n, bytes64, out32);
  HostCall hc(ctx);
  const int in = hc.in(bytes64, n * 64), o = hc.out(out32, n * 32), aff = out_affine ? hc.out(out_affine, n * 64) : -1;
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_from_uniform_batch_dev(ctx, n, hc.dev(in), hc.dev(o), aff < 0 ? nullptr : hc.dev(aff), ctx->stream));
}

static Rule ristretto_mul_rule(ncg_ctx* ctx, int flags) {
  return {"ristretto_mul_batch", (flags & ~NCG_RISTRETTO_ONE_SCALAR) == 0 ? NCG_OK
                                     : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ristretto_mul_batch: unknown flag bits 0x%x", flags)};
}
// decode (a rejected row becomes the identity), the ed25519 variable-base multiply, encode: three launches, only bytes cross
int ncg_ristretto_mul_batch_dev(ncg_ctx* ctx, size_t n, const void* enc_dev, const void* scalars_dev, int flags, void* out32_dev,
                                uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, ristretto_mul_rule(ctx, flags), n, enc_dev, scalars_dev, out32_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  const bool one = (flags & NCG_RISTRETTO_ONE_SCALAR) != 0;
  const size_t pts_b = align256(n * 64), inf_b = align256(n);
  if (int rc = ensure_rist_ws(ctx, 2 * pts_b + inf_b + (one ? n * 32 : 0), st)) return rc;
  char* d_pts = (char*)ctx->rist_ws;
  char* d_prod = d_pts + pts_b;
  char* d_inf = d_prod + pts_b;
  const void* d_sc = scalars_dev;
  NCG_HIP(ctx, ncg::ristretto_decode_batch((const uint32_t*)enc_dev, (uint32_t*)d_pts, out_ok_dev, 1, (int)n, st));
  if (one) {  // the multiply reads one scalar per item
    NCG_HIP(ctx, ncg::ristretto_broadcast_scalar((const uint32_t*)scalars_dev, (uint32_t*)(d_inf + inf_b), (int)n, st));
    d_sc = d_inf + inf_b;
  }
  if (int rc = ncg_mul_var_batch_dev(ctx, NCG_ED25519, n, d_pts, d_sc, d_prod, (uint8_t*)d_inf, st)) return rc;
  NCG_HIP(ctx, ncg::ristretto_encode_batch((const uint32_t*)d_prod, (uint32_t*)out32_dev, (int)n, st));
  return NCG_OK;
}
int ncg_ristretto_mul_batch(ncg_ctx* ctx, size_t n, const void* enc, const void* scalars, int flags, void* out32, uint8_t* out_ok) {
  NCG_BEGIN(ctx, ristretto_mul_rule(ctx, flags), n, enc, scalars, out32, out_ok);
  HostCall hc(ctx);
  const int in = hc.in(enc, n * 32), sc = hc.in(scalars, (flags & NCG_RISTRETTO_ONE_SCALAR) ? 32 : n * 32);
  const int o = hc.out(out32, n * 32), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_mul_batch_dev(ctx, n, hc.dev(in), hc.dev(sc), flags, hc.dev(o), hc.dev<uint8_t>(ok), ctx->stream));
}
// the fixed-base table walk, then the encoder on its projective rows: no inversion
int ncg_ristretto_mul_base_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, void* out32_dev, void* stream) {
  NCG_BEGIN(ctx, no_rule("ristretto_mul_base_batch"), n, scalars_dev, out32_dev);
  const hipStream_t st = stream_of(ctx, stream);
  if (int rc = ensure_rist_ws(ctx, ncg::ristretto_proj_words((int)n) * 4, st)) return rc;
  if (int rc = ensure_ed_base_table(ctx)) return rc;
  NCG_HIP(ctx, ncg::ed25519_mul_base_proj(ctx->base_tab[NCG_ED25519], (const uint32_t*)scalars_dev, (uint32_t*)ctx->rist_ws, (int)n, st));
  NCG_HIP(ctx, ncg::ristretto_encode_proj_batch((const uint32_t*)ctx->rist_ws, (uint32_t*)out32_dev, (int)n, st));
  return NCG_OK;
}
int ncg_ristretto_mul_base_batch(ncg_ctx* ctx, size_t n, const void* scalars, void* out32) {
  NCG_BEGIN(ctx, no_rule("ristretto_mul_base_batch"), n, scalars, out32);
  HostCall hc(ctx);
  const int sc = hc.in(scalars, n * 32), o = hc.out(out32, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_mul_base_batch_dev(ctx, n, hc.dev(sc), hc.dev(o), ctx->stream));
}

// An empty sum is the identity, whose encoding is 32 zero bytes: written, not refused, as ncg_msm writes (0, 1).
static int ristretto_msm_identity(ncg_ctx* ctx, void* out32) {
  if (!out32) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ristretto_msm: NULL output");
  memset(out32, 0, 32);
  return NCG_OK;
}
// decode on the device, the ed25519 MSM on the decoded points where they lie, the one resulting point encoded by the lane
// function on the host (the MSM hands its result over in host memory)
int ncg_ristretto_msm_dev(ncg_ctx* ctx, size_t n, const void* enc_dev, const void* scalars_dev, void* out32, int64_t* out_bad_index,
                          void* stream) {
  if (out_bad_index) *out_bad_index = -1;
  NCG_BEGIN_OR(ctx, no_rule("ristretto_msm"), n, ristretto_msm_identity(ctx, out32), enc_dev, scalars_dev, out32);
  const hipStream_t st = stream_of(ctx, stream);
  const size_t pts_b = align256(n * 64);
  if (int rc = ensure_rist_ws(ctx, pts_b + n, st)) return rc;
  char* d_pts = (char*)ctx->rist_ws;
  uint8_t* d_ok = (uint8_t*)(d_pts + pts_b);
  NCG_HIP(ctx, ncg::ristretto_decode_batch((const uint32_t*)enc_dev, (uint32_t*)d_pts, d_ok, 0, (int)n, st));
  std::vector<uint8_t> ok(n);
  NCG_HIP(ctx, hipMemcpyAsync(ok.data(), d_ok, n, hipMemcpyDeviceToHost, st));
  NCG_HIP(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) {  // the reference throws in fromBytes
      if (out_bad_index) *out_bad_index = (int64_t)i;
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ristretto_msm: invalid ristretto255 encoding at index %zu", i);
    }
  uint32_t aff[16], enc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint8_t inf = 0;
  if (int rc = ncg_msm_dev(ctx, NCG_ED25519, n, d_pts, scalars_dev, aff, &inf, st)) return rc;
  if (!inf) ncg::ristretto_encode_host(aff, enc, 1);
  memcpy(out32, enc, 32);
  return NCG_OK;
}
int ncg_ristretto_msm(ncg_ctx* ctx, size_t n, const void* enc, const void* scalars, void* out32, int64_t* out_bad_index) {
  if (out_bad_index) *out_bad_index = -1;
  NCG_BEGIN_OR(ctx, no_rule("ristretto_msm"), n, ristretto_msm_identity(ctx, out32), enc, scalars, out32);
  HostCall hc(ctx);
  const int in = hc.in(enc, n * 32), sc = hc.in(scalars, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_msm_dev(ctx, n, hc.dev(in), hc.dev(sc), out32, out_bad_index, ctx->stream));
}

// ---- OPRF over ristretto255 (oprf.hip).  The strings of a call, the one scalar inverted and the rows of the proof calls live in
// ctx->oprf_ws, which is cleared on the call's stream before the call returns, and so is the staged copy of the scalars of a host
// form.  The scalar rows of a _dev form are read as words: 4-byte aligned or refused.
// the row index of a kernel is an int, and the last block of 256 lanes runs past n: the largest batch leaves room for it
constexpr size_t OPRF_NO_LIMIT = 0x7fffffffu - 255;
constexpr size_t OPRF_PROOF_WS = 1024;   // behind the header: the rows of a proof call (M | k r | Z t3 t2, or G B M Z | s c)
static Rule oprf_rule(ncg_ctx* ctx, const char* op, int suite, int mode, int flags, size_t n_max, size_t n, const void* info, size_t info_len,
                      std::initializer_list<const void*> word_rows) {
  int rc = NCG_OK;
  if (suite != NCG_OPRF_RISTRETTO255_SHA512) rc = set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: %s: unsupported suite %d", op, suite);
  else if (mode < 0 || mode > 2) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: mode %d is not 0, 1 or 2", op, mode);
  else if (flags & ~(NCG_OPRF_ONE_SCALAR | NCG_OPRF_INVERT)) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: unknown flag bits 0x%x", op, flags);
  else if (n > n_max && n_max == 65535) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: %zu rows, the row index must fit 16 bits", op, n);
  else if (n > n_max) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: batch too large", op);
  else if (mode != 2 && (info || info_len)) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: info is read only in mode 2", op);
  else if (info_len > 65535) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: info_len %zu above 65535", op, info_len);
  else if (info_len && !info) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: NULL buffer (info)", op);
  else
    for (const void* p : word_rows)
      if ((uintptr_t)p & 3) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: element and scalar rows must be 4-byte aligned", op);
  return {op, rc};
}
static Rule xmd_rule(ncg_ctx* ctx, const char* op, size_t n, const void* dst, size_t dst_len, size_t out_len,
                     std::initializer_list<const void*> word_rows) {
  int rc = NCG_OK;
  if (n > OPRF_NO_LIMIT) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: batch too large", op);
  else if (dst_len < 1 || dst_len > 255) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: dst_len %zu outside 1..255", op, dst_len);
  else if (!dst) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: NULL buffer (dst)", op);
  else if (out_len < 1 || out_len > 256) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: out_len %zu outside 1..256", op, out_len);
  else
    for (const void* p : word_rows)
      if ((uintptr_t)p & 3) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: output rows must be 4-byte aligned", op);
  return {op, rc};
}
static int oprf_ws(ncg_ctx* ctx, size_t info_len, size_t extra, uint8_t** ws, size_t* bytes) {
  *bytes = ncg::oprf_ws_bytes(info_len) + extra;
  if (int rc = ncg_grow_buf(ctx, &ctx->oprf_ws, &ctx->oprf_ws_bytes, *bytes, *bytes + 4096, GrowWait::device)) return rc;
  *ws = (uint8_t*)ctx->oprf_ws;
  return NCG_OK;
}
// the end of a _dev form: the workspace cleared on the call's stream, then the launch status
static int oprf_done(ncg_ctx* ctx, hipError_t e, size_t ws_bytes, hipStream_t st) {
  (void)hipMemsetAsync(ctx->oprf_ws, 0, ws_bytes, st);
  NCG_HIP(ctx, e);
  return NCG_OK;
}
// the inputs of the host forms: at most 65535 bytes each, where the reference's inputBytes throws
static int oprf_input_lengths(ncg_ctx* ctx, const char* op, size_t n, const uint64_t* off) {
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] >= off[i] && off[i + 1] - off[i] > 65535)
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: input %zu is longer than 65535 bytes", op, i);
  return NCG_OK;
}

int ncg_xmd_sha512_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst, size_t dst_len,
                             size_t out_len, void* out_dev, void* stream) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "xmd_sha512_batch", n, dst, dst_len, out_len, {}), n, msg_off_dev, out_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, 0, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_xmd_batch((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, (uint32_t)out_len,
                                            (uint8_t*)out_dev, (int)n, ws, st), wb, st);
}
int ncg_xmd_sha512_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len, size_t out_len,
                         void* out) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "xmd_sha512_batch", n, dst, dst_len, out_len, {}), n, msg_off, out);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "xmd_sha512_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out, n * out_len);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_xmd_sha512_batch_dev(ctx, n, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, out_len, hc.dev(o), ctx->stream));
}
int ncg_ristretto_hash_to_group_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                          size_t dst_len, void* out32_dev, void* out_affine_dev, void* stream) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "ristretto_hash_to_group_batch", n, dst, dst_len, 64, {out32_dev, out_affine_dev}), n, msg_off_dev, out32_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, 0, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_hash_to_group_batch((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len,
                                                      (uint32_t*)out32_dev, (uint32_t*)out_affine_dev, (int)n, ws, st), wb, st);
}
int ncg_ristretto_hash_to_group_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                                      void* out32, void* out_affine) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "ristretto_hash_to_group_batch", n, dst, dst_len, 64, {}), n, msg_off, out32);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "ristretto_hash_to_group_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out32, n * 32), aff = out_affine ? hc.out(out_affine, n * 64) : -1;
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_hash_to_group_batch_dev(ctx, n, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o),
                                                         aff < 0 ? nullptr : hc.dev(aff), ctx->stream));
}
int ncg_ristretto_hash_to_scalar_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                           size_t dst_len, void* out32_dev, void* stream) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "ristretto_hash_to_scalar_batch", n, dst, dst_len, 64, {out32_dev}), n, msg_off_dev, out32_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, 0, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_hash_to_scalar_batch((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len,
                                                       (uint32_t*)out32_dev, (int)n, ws, st), wb, st);
}
int ncg_ristretto_hash_to_scalar_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                                       void* out32) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "ristretto_hash_to_scalar_batch", n, dst, dst_len, 64, {}), n, msg_off, out32);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "ristretto_hash_to_scalar_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out32, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ristretto_hash_to_scalar_batch_dev(ctx, n, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o), ctx->stream));
}

int ncg_oprf_blind_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs_dev, const uint64_t* off_dev,
                             const void* blinds32_dev, void* out_blinded32_dev, uint8_t* out_status_dev, void* stream) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_blind_batch", suite, mode, 0, OPRF_NO_LIMIT, n, nullptr, 0, {blinds32_dev, out_blinded32_dev}), n, off_dev,
            blinds32_dev, out_blinded32_dev, out_status_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, 0, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_blind_batch(mode, (const uint8_t*)inputs_dev, off_dev, (const uint32_t*)blinds32_dev, (uint32_t*)out_blinded32_dev,
                                              out_status_dev, (int)n, ws, st), wb, st);
}
int ncg_oprf_blind_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs, const uint64_t* off, const void* blinds32,
                         void* out_blinded32, uint8_t* out_status) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_blind_batch", suite, mode, 0, OPRF_NO_LIMIT, n, nullptr, 0, {}), n, off, blinds32, out_blinded32, out_status);
  if (int rc = oprf_input_lengths(ctx, "oprf_blind_batch", n, off)) return rc;
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, o_;
  if (int rc = stage_msgs(hc, "oprf_blind_batch", n, inputs, off, rel, &msg, &o_)) return rc;
  const int b = hc.in(blinds32, n * 32), o = hc.out(out_blinded32, n * 32), s = hc.out(out_status, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, b, n * 32);
    return rc;
  }
  const int rc = ncg_oprf_blind_batch_dev(ctx, suite, mode, n, hc.dev(msg), hc.dev<const uint64_t>(o_), hc.dev(b), hc.dev(o), hc.dev<uint8_t>(s),
                                          ctx->stream);
  ed_clear_staged(hc, b, n * 32);
  return hc.finish(rc);
}
int ncg_oprf_mul_batch_dev(ncg_ctx* ctx, int suite, size_t n, const void* elements32_dev, const void* scalars32_dev, int flags, void* out32_dev,
                           uint8_t* out_status_dev, void* stream) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_mul_batch", suite, 0, flags, OPRF_NO_LIMIT, n, nullptr, 0, {elements32_dev, scalars32_dev, out32_dev}), n,
            elements32_dev, scalars32_dev, out32_dev, out_status_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, 0, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_mul_batch((const uint32_t*)elements32_dev, (const uint32_t*)scalars32_dev, flags, (uint32_t*)out32_dev,
                                            out_status_dev, (int)n, ws, st), wb, st);
}
int ncg_oprf_mul_batch(ncg_ctx* ctx, int suite, size_t n, const void* elements32, const void* scalars32, int flags, void* out32,
                       uint8_t* out_status) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_mul_batch", suite, 0, flags, OPRF_NO_LIMIT, n, nullptr, 0, {}), n, elements32, scalars32, out32, out_status);
  const size_t sbytes = (flags & NCG_OPRF_ONE_SCALAR) ? 32 : n * 32;
  HostCall hc(ctx);
  const int e = hc.in(elements32, n * 32), k = hc.in(scalars32, sbytes), o = hc.out(out32, n * 32), s = hc.out(out_status, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, k, sbytes);
    return rc;
  }
  const int rc = ncg_oprf_mul_batch_dev(ctx, suite, n, hc.dev(e), hc.dev(k), flags, hc.dev(o), hc.dev<uint8_t>(s), ctx->stream);
  ed_clear_staged(hc, k, sbytes);
  return hc.finish(rc);
}
int ncg_oprf_finalize_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs_dev, const uint64_t* off_dev, const void* info,
                                size_t info_len, const void* blinds32_dev, const void* evaluated32_dev, void* out64_dev, uint8_t* out_status_dev,
                                void* stream) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_finalize_batch", suite, mode, 0, OPRF_NO_LIMIT, n, info, info_len, {blinds32_dev, evaluated32_dev}), n, off_dev,
            blinds32_dev, evaluated32_dev, out64_dev, out_status_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, info_len, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_finalize_batch(mode, (const uint8_t*)inputs_dev, off_dev, (const uint8_t*)info, (uint32_t)info_len,
                                                 (const uint32_t*)blinds32_dev, (const uint32_t*)evaluated32_dev, (uint8_t*)out64_dev,
                                                 out_status_dev, (int)n, ws, st), wb, st);
}
int ncg_oprf_finalize_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs, const uint64_t* off, const void* info,
                            size_t info_len, const void* blinds32, const void* evaluated32, void* out64, uint8_t* out_status) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_finalize_batch", suite, mode, 0, OPRF_NO_LIMIT, n, info, info_len, {}), n, off, blinds32, evaluated32, out64,
            out_status);
  if (int rc = oprf_input_lengths(ctx, "oprf_finalize_batch", n, off)) return rc;
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, o_;
  if (int rc = stage_msgs(hc, "oprf_finalize_batch", n, inputs, off, rel, &msg, &o_)) return rc;
  const int b = hc.in(blinds32, n * 32), e = hc.in(evaluated32, n * 32), o = hc.out(out64, n * 64), s = hc.out(out_status, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, b, n * 32);
    return rc;
  }
  const int rc = ncg_oprf_finalize_batch_dev(ctx, suite, mode, n, hc.dev(msg), hc.dev<const uint64_t>(o_), info, info_len, hc.dev(b), hc.dev(e),
                                             hc.dev(o), hc.dev<uint8_t>(s), ctx->stream);
  ed_clear_staged(hc, b, n * 32);
  return hc.finish(rc);
}
int ncg_oprf_evaluate_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs_dev, const uint64_t* off_dev, const void* info,
                                size_t info_len, const void* scalar32_dev, int flags, void* out64_dev, uint8_t* out_status_dev, void* stream) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_evaluate_batch", suite, mode, flags, OPRF_NO_LIMIT, n, info, info_len, {scalar32_dev}), n, off_dev,
            scalar32_dev, out64_dev, out_status_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, info_len, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_evaluate_batch(mode, (const uint8_t*)inputs_dev, off_dev, (const uint8_t*)info, (uint32_t)info_len,
                                                 (const uint32_t*)scalar32_dev, flags, (uint8_t*)out64_dev, out_status_dev, (int)n, ws, st), wb, st);
}
int ncg_oprf_evaluate_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs, const uint64_t* off, const void* info,
                            size_t info_len, const void* scalar32, int flags, void* out64, uint8_t* out_status) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_evaluate_batch", suite, mode, flags, OPRF_NO_LIMIT, n, info, info_len, {}), n, off, scalar32, out64, out_status);
  if (int rc = oprf_input_lengths(ctx, "oprf_evaluate_batch", n, off)) return rc;
  const size_t sbytes = (flags & NCG_OPRF_ONE_SCALAR) ? 32 : n * 32;
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, o_;
  if (int rc = stage_msgs(hc, "oprf_evaluate_batch", n, inputs, off, rel, &msg, &o_)) return rc;
  const int k = hc.in(scalar32, sbytes), o = hc.out(out64, n * 64), s = hc.out(out_status, n);
  if (int rc = hc.stage()) {
    ed_clear_staged(hc, k, sbytes);
    return rc;
  }
  const int rc = ncg_oprf_evaluate_batch_dev(ctx, suite, mode, n, hc.dev(msg), hc.dev<const uint64_t>(o_), info, info_len, hc.dev(k), flags,
                                             hc.dev(o), hc.dev<uint8_t>(s), ctx->stream);
  ed_clear_staged(hc, k, sbytes);
  return hc.finish(rc);
}
int ncg_oprf_composite_scalars_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32_dev, const void* D32_dev,
                                         void* out32_dev, uint8_t* out_status_dev, void* stream) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_composite_scalars_batch", suite, mode, 0, 65535, n, nullptr, 0, {C32_dev, D32_dev, out32_dev}), n, B32, C32_dev,
            D32_dev, out32_dev, out_status_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, 0, 0, &ws, &wb)) return rc;
  return oprf_done(ctx, ncg::oprf_composite_batch(mode, (const uint8_t*)B32, (const uint32_t*)C32_dev, (const uint32_t*)D32_dev,
                                                  (uint32_t*)out32_dev, out_status_dev, (int)n, ws, st), wb, st);
}
int ncg_oprf_composite_scalars_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32, const void* D32, void* out32,
                                     uint8_t* out_status) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_composite_scalars_batch", suite, mode, 0, 65535, n, nullptr, 0, {}), n, B32, C32, D32, out32, out_status);
  HostCall hc(ctx);
  const int c = hc.in(C32, n * 32), d = hc.in(D32, n * 32), o = hc.out(out32, n * 32), s = hc.out(out_status, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_oprf_composite_scalars_batch_dev(ctx, suite, mode, n, B32, hc.dev(c), hc.dev(d), hc.dev(o), hc.dev<uint8_t>(s), ctx->stream));
}

// The composites of a proof call: d on the device, every row of C and D accepted (or the call fails on the first one that is not),
// then M = sum d_i C_i and, where Z32 is given, Z = sum d_i D_i by the ristretto MSM.  d stays at ws + OPRF_PROOF_WS + 1024.
static int oprf_composites(ncg_ctx* ctx, const char* op, int mode, size_t n, const void* B32, const void* C32_dev, const void* D32_dev, uint8_t* ws,
                           uint8_t* M32, uint8_t* Z32, hipStream_t st) {
  uint32_t bw[8], baff[16];
  uint8_t bok = 0;
  memcpy(bw, B32, 32);
  ncg::ristretto_decode_host(bw, baff, &bok, 0, 1);
  bool bzero = true;
  for (int i = 0; i < 8; i++) bzero = bzero && bw[i] == 0;
  if (!bok || bzero) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: the public key %s", op, bzero ? "is the identity" : "does not decode");
  uint32_t* d_d = (uint32_t*)(ws + OPRF_PROOF_WS + 1024);
  uint8_t* d_st = (uint8_t*)(d_d + n * 8);
  NCG_HIP(ctx, ncg::oprf_composite_batch(mode, (const uint8_t*)B32, (const uint32_t*)C32_dev, (const uint32_t*)D32_dev, d_d, d_st, (int)n, ws, st));
  std::vector<uint8_t> status(n);
  NCG_HIP(ctx, hipMemcpyAsync(status.data(), d_st, n, hipMemcpyDeviceToHost, st));
  NCG_HIP(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++)
    if (status[i])
      return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: row %zu: an element %s", op, i,
                     status[i] == 2 ? "is the identity" : "does not decode");
  if (int rc = ncg_ristretto_msm_dev(ctx, n, C32_dev, d_d, M32, nullptr, st)) return rc;
  if (Z32)
    if (int rc = ncg_ristretto_msm_dev(ctx, n, D32_dev, d_d, Z32, nullptr, st)) return rc;
  return NCG_OK;
}
static size_t oprf_proof_ws_extra(size_t n) { return OPRF_PROOF_WS + 1024 + n * 32 + align256(n); }
int ncg_oprf_generate_proof_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* k32, const void* B32, const void* C32_dev,
                                const void* D32_dev, const void* r32, void* out_proof64, void* stream) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_generate_proof", suite, mode, 0, 65535, n, nullptr, 0, {C32_dev, D32_dev}), n, k32, B32, C32_dev, D32_dev, r32,
            out_proof64);
  const hipStream_t st = stream_of(ctx, stream);
  uint32_t kr[16], pts[40], c[8], s[8];   // pts: B M Z t2 t3
  memcpy(kr, k32, 32);
  memcpy(kr + 8, r32, 32);
  auto wipe = [&] {
    for (int i = 0; i < 16; i++) ((volatile uint32_t*)kr)[i] = 0;
  };
  if (!ncg::oprf_scalar_ok_host(kr, 0) || !ncg::oprf_scalar_ok_host(kr + 8, 0)) {
    wipe();
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: oprf_generate_proof: the key and the nonce must be below L and not zero");
  }
  uint8_t* ws = nullptr;
  size_t wb = 0;
  int rc = ensure_ed_scan_table(ctx);
  if (rc == NCG_OK) rc = oprf_ws(ctx, 0, oprf_proof_ws_extra(n), &ws, &wb);
  if (rc != NCG_OK) {
    wipe();
    return rc;
  }
  memcpy(pts, B32, 32);
  rc = oprf_composites(ctx, "oprf_generate_proof", mode, n, B32, C32_dev, D32_dev, ws, (uint8_t*)(pts + 8), nullptr, st);
  if (rc == NCG_OK) {
    uint8_t* pw = ws + OPRF_PROOF_WS;   // M (32) | k r (64) | Z t3 t2 (96)
    uint32_t zt[24];
    hipError_t e = ncg::oprf_put(pw, (const uint8_t*)(pts + 8), 32, st);
    if (e == hipSuccess) e = ncg::oprf_put(pw + 32, (const uint8_t*)kr, 64, st);
    if (e == hipSuccess)
      e = ncg::oprf_proof_points(ctx->ed_scan_tab, (const uint32_t*)pw, (const uint32_t*)(pw + 32), (uint32_t*)(pw + 96), st);
    if (e == hipSuccess) e = hipMemcpyAsync(zt, pw + 96, 96, hipMemcpyDeviceToHost, st);
    (void)hipMemsetAsync(ctx->oprf_ws, 0, wb, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      wipe();
      NCG_HIP(ctx, e);
    }
    memcpy(pts + 16, zt, 32);        // Z
    memcpy(pts + 24, zt + 16, 32);   // t2
    memcpy(pts + 32, zt + 8, 32);    // t3
    ncg::oprf_challenge_host(mode, (const uint8_t*)pts, c);
    ncg::oprf_proof_s_host(c, kr, kr + 8, s);
    memcpy(out_proof64, c, 32);
    memcpy((char*)out_proof64 + 32, s, 32);
  } else {
    (void)hipMemsetAsync(ctx->oprf_ws, 0, wb, st);
  }
  wipe();
  return rc;
}
int ncg_oprf_generate_proof(ncg_ctx* ctx, int suite, int mode, size_t n, const void* k32, const void* B32, const void* C32, const void* D32,
                            const void* r32, void* out_proof64) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_generate_proof", suite, mode, 0, 65535, n, nullptr, 0, {}), n, k32, B32, C32, D32, r32, out_proof64);
  HostCall hc(ctx);
  const int c = hc.in(C32, n * 32), d = hc.in(D32, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_oprf_generate_proof_dev(ctx, suite, mode, n, k32, B32, hc.dev(c), hc.dev(d), r32, out_proof64, ctx->stream));
}
int ncg_oprf_verify_proof_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32_dev, const void* D32_dev,
                              const void* proof64, uint8_t* out_ok, void* stream) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_verify_proof", suite, mode, 0, 65535, n, nullptr, 0, {C32_dev, D32_dev}), n, B32, C32_dev, D32_dev, proof64,
            out_ok);
  const hipStream_t st = stream_of(ctx, stream);
  *out_ok = 0;
  uint32_t cs[16], sc[16], pts[40], c2[8];   // pts: B M Z t2 t3
  memcpy(cs, proof64, 64);
  uint8_t* ws;
  size_t wb;
  if (int rc = oprf_ws(ctx, 0, oprf_proof_ws_extra(n), &ws, &wb)) return rc;
  memcpy(pts, B32, 32);
  int rc = oprf_composites(ctx, "oprf_verify_proof", mode, n, B32, C32_dev, D32_dev, ws, (uint8_t*)(pts + 8), (uint8_t*)(pts + 16), st);
  if (rc == NCG_OK && ncg::oprf_scalar_ok_host(cs, 1) && ncg::oprf_scalar_ok_host(cs + 8, 1)) {   // Fn.fromBytes: below L, zero allowed
    // t2 = s G + c B and t3 = s M + c Z: two MSMs of two terms on rows laid out in the workspace
    static const uint8_t G[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                  0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    uint8_t rows[128];
    memcpy(rows, G, 32);
    memcpy(rows + 32, B32, 32);
    memcpy(rows + 64, pts + 8, 64);
    memcpy(sc, cs + 8, 32);   // s first
    memcpy(sc + 8, cs, 32);
    uint8_t* pw = ws + OPRF_PROOF_WS;   // G B M Z (128) | s c (64)
    hipError_t e = ncg::oprf_put(pw, rows, 128, st);
    if (e == hipSuccess) e = ncg::oprf_put(pw + 128, (const uint8_t*)sc, 64, st);
    NCG_HIP(ctx, e);
    rc = ncg_ristretto_msm_dev(ctx, 2, pw, pw + 128, pts + 24, nullptr, st);
    if (rc == NCG_OK) rc = ncg_ristretto_msm_dev(ctx, 2, pw + 64, pw + 128, pts + 32, nullptr, st);
    if (rc == NCG_OK) {
      ncg::oprf_challenge_host(mode, (const uint8_t*)pts, c2);
      *out_ok = memcmp(c2, cs, 32) == 0 ? 1 : 0;
    }
  }
  (void)hipMemsetAsync(ctx->oprf_ws, 0, wb, st);
  return rc;
}
int ncg_oprf_verify_proof(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32, const void* D32, const void* proof64,
                          uint8_t* out_ok) {
  NCG_BEGIN(ctx, oprf_rule(ctx, "oprf_verify_proof", suite, mode, 0, 65535, n, nullptr, 0, {}), n, B32, C32, D32, proof64, out_ok);
  HostCall hc(ctx);
  const int c = hc.in(C32, n * 32), d = hc.in(D32, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_oprf_verify_proof_dev(ctx, suite, mode, n, B32, hc.dev(c), hc.dev(d), proof64, out_ok, ctx->stream));
}
// The pieces of oprf.hpp on raw words, in the style of ncg_decaf448_check
int ncg_oprf_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out) {
  int rrc = NCG_OK;
  if (ctx && n > (1u << 24)) rrc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: oprf_check: batch too large (max 2^24)");
  else if (ctx && op == 3 && (variant < 2 || variant > 32)) rrc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: oprf_check: variant %d outside 2..32", variant);
  const Rule rule = {"oprf_check", rrc};
  NCG_BEGIN(ctx, rule, n, a, b, out);
  int wa, wb, wo;
  ncg::oprf_check_words(op, &wa, &wb, &wo);
  HostCall hc(ctx);
  const int da = hc.in(a, n * wa * 4), db = hc.in(b, n * wb * 4);
  const int o = hc.out(out, n * (wo ? wo : 8) * 4, true);
  if (int rc = hc.stage()) return rc;
  if (wo) NCG_HIP(ctx, ncg::oprf_check(op, variant, hc.dev<const uint32_t>(da), hc.dev<const uint32_t>(db), hc.dev<uint32_t>(o), (int)n, ctx->stream));
  return hc.finish(NCG_OK);
}

// ---- RFC 9380 hash-to-curve for secp256k1 and edwards25519 (h2c_suites.hip).  The hand-offs of a call live in ctx->h2c_ws, never in
// ctx->scratch (the host forms stage there).  The limits and the DST rules are xmd_rule's; nothing here is secret, nothing is cleared.
static Rule h2c_rule(ncg_ctx* ctx, const char* op, int suite, int count, size_t n, const void* dst, size_t dst_len,
                     std::initializer_list<const void*> word_rows) {
  if (suite != NCG_H2C_SECP256K1_XMD_SHA256_SSWU && suite != NCG_H2C_EDWARDS25519_XMD_SHA512_ELL2)
    return {op, set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: %s: unsupported suite %d", op, suite)};
  if (count != NCG_H2C_NU && count != NCG_H2C_RO) return {op, set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: count must be 1 or 2", op)};
  return xmd_rule(ctx, op, n, dst, dst_len, 48 * (size_t)count, word_rows);
}
// the maps take no DST
static Rule h2c_map_rule(ncg_ctx* ctx, int suite, int count, size_t n, std::initializer_list<const void*> word_rows) {
  static const uint8_t none[1] = {0};
  return h2c_rule(ctx, "h2c_map_batch", suite, count, n, none, 1, word_rows);
}
static int h2c_ws(ncg_ctx* ctx, size_t bytes, hipStream_t st, uint8_t** ws) {
  if (int rc = ncg_grow_buf(ctx, &ctx->h2c_ws, &ctx->h2c_ws_bytes, bytes, bytes + (bytes >> 2) + 4096, GrowWait::device)) return rc;
  *ws = (uint8_t*)ctx->h2c_ws;
  return NCG_OK;
}

int ncg_h2c_hash_batch_dev(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                           size_t dst_len, void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream) {
  NCG_BEGIN(ctx, h2c_rule(ctx, "h2c_hash_batch", suite, count, n, dst, dst_len, {out_affine_dev}), n, msg_off_dev, out_affine_dev, out_is_inf_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, ncg::h2c_suites_ws_bytes(suite, n, count), st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c_suites_hash(suite, (const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, count,
                                    (uint32_t*)out_affine_dev, out_is_inf_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_h2c_hash_batch(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                       void* out_affine, uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, h2c_rule(ctx, "h2c_hash_batch", suite, count, n, dst, dst_len, {}), n, msg_off, out_affine, out_is_inf);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "h2c_hash_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out_affine, n * 64), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_h2c_hash_batch_dev(ctx, suite, n, count, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o),
                                          hc.dev<uint8_t>(f), ctx->stream));
}
int ncg_h2c_map_batch_dev(ncg_ctx* ctx, int suite, size_t n, int count, const void* u48_dev, void* out_affine_dev, uint8_t* out_is_inf_dev,
                          void* stream) {
  NCG_BEGIN(ctx, h2c_map_rule(ctx, suite, count, n, {u48_dev, out_affine_dev}), n, u48_dev, out_affine_dev, out_is_inf_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, ncg::h2c_suites_ws_bytes(suite, n, count), st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c_suites_map(suite, (const uint32_t*)u48_dev, 12, count, (uint32_t*)out_affine_dev, out_is_inf_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_h2c_map_batch(ncg_ctx* ctx, int suite, size_t n, int count, const void* u48, void* out_affine, uint8_t* out_is_inf) {
  NCG_BEGIN(ctx, h2c_map_rule(ctx, suite, count, n, {}), n, u48, out_affine, out_is_inf);
  HostCall hc(ctx);
  const int in = hc.in(u48, n * (size_t)count * 48);
  const int o = hc.out(out_affine, n * 64), f = hc.out(out_is_inf, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_h2c_map_batch_dev(ctx, suite, n, count, hc.dev(in), hc.dev(o), hc.dev<uint8_t>(f), ctx->stream));
}
int ncg_h2c_hash_to_scalar_batch_dev(ncg_ctx* ctx, int suite, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                     size_t dst_len, void* out32_dev, void* stream) {
  NCG_BEGIN(ctx, h2c_rule(ctx, "h2c_hash_to_scalar_batch", suite, 1, n, dst, dst_len, {out32_dev}), n, msg_off_dev, out32_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, ncg::h2c_suites_ws_bytes(suite, n, 1), st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c_suites_hash_to_scalar(suite, (const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len,
                                              (uint32_t*)out32_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_h2c_hash_to_scalar_batch(ncg_ctx* ctx, int suite, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                                 void* out32) {
  NCG_BEGIN(ctx, h2c_rule(ctx, "h2c_hash_to_scalar_batch", suite, 1, n, dst, dst_len, {}), n, msg_off, out32);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "h2c_hash_to_scalar_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out32, n * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_h2c_hash_to_scalar_batch_dev(ctx, suite, n, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o), ctx->stream));
}
int ncg_h2c_hash_to_field_batch_dev(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev,
                                    const void* dst, size_t dst_len, void* out_u_dev, void* stream) {
  NCG_BEGIN(ctx, h2c_rule(ctx, "h2c_hash_to_field_batch", suite, count, n, dst, dst_len, {out_u_dev}), n, msg_off_dev, out_u_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, ncg::h2c_suites_ws_bytes(suite, n, count), st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c_suites_hash_to_field(suite, (const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, count,
                                             (uint32_t*)out_u_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_h2c_hash_to_field_batch(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs, const uint64_t* msg_off, const void* dst,
                                size_t dst_len, void* out_u) {
  NCG_BEGIN(ctx, h2c_rule(ctx, "h2c_hash_to_field_batch", suite, count, n, dst, dst_len, {}), n, msg_off, out_u);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "h2c_hash_to_field_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out_u, n * (size_t)count * 32);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_h2c_hash_to_field_batch_dev(ctx, suite, n, count, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o),
                                                   ctx->stream));
}
int ncg_xmd_sha256_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst, size_t dst_len,
                             size_t out_len, void* out_dev, void* stream) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "xmd_sha256_batch", n, dst, dst_len, out_len, {}), n, msg_off_dev, out_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, 256, st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c_xmd_sha256_batch((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, (uint32_t)out_len,
                                         (uint8_t*)out_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_xmd_sha256_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len, size_t out_len,
                         void* out) {
  NCG_BEGIN(ctx, xmd_rule(ctx, "xmd_sha256_batch", n, dst, dst_len, out_len, {}), n, msg_off, out);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "xmd_sha256_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out, n * out_len);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_xmd_sha256_batch_dev(ctx, n, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, out_len, hc.dev(o), ctx->stream));
}
// The pieces of h2c_suites.hpp on raw words, in the style of ncg_oprf_check: rows of 24 words in and out
int ncg_h2c_check(ncg_ctx* ctx, int op, size_t n, const void* a, void* out) {
  const Rule rule = {"h2c_check", !ctx || n <= (1u << 24) ? NCG_OK
                                      : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: h2c_check: batch too large (max 2^24)")};
  NCG_BEGIN(ctx, rule, n, a, out);
  HostCall hc(ctx);
  const int da = hc.in(a, n * 96);
  const int o = hc.out(out, n * 96, true);
  if (int rc = hc.stage()) return rc;
  NCG_HIP(ctx, ncg::h2c_check(op, hc.dev<const uint32_t>(da), hc.dev<uint32_t>(o), (int)n, ctx->stream));
  return hc.finish(NCG_OK);
}

// ---- RFC 9380 for edwards448 and decaf448 (h2c448.hip).  The hand-offs of a call live in ctx->h2c_ws like those of the 255-bit
// suites: one call at a time per context.  Nothing here is secret, nothing is cleared.
// the batch limit, count and the alignment of the rows of words: all a map call has to obey
static Rule h2c448_rows_rule(ncg_ctx* ctx, const char* op, int count, size_t n, std::initializer_list<const void*> word_rows) {
  int rc = NCG_OK;
  if (n > 0x7fffffffu) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: batch too large", op);
  else if (count != NCG_H2C_NU && count != NCG_H2C_RO) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: count must be 1 or 2", op);
  else
    for (const void* p : word_rows)
      if ((uintptr_t)p & 3) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: 56-byte rows must be 4-byte aligned", op);
  return {op, rc};
}
// the calls that hash: the DST as well (out_len: 1 where the call fixes the length itself)
static Rule h2c448_rule(ncg_ctx* ctx, const char* op, int count, size_t n, const void* dst, size_t dst_len, size_t out_len,
                        std::initializer_list<const void*> word_rows) {
  Rule r = h2c448_rows_rule(ctx, op, count, n, word_rows);
  if (r.rc) return r;
  if (dst_len < 1 || dst_len > 255) r.rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: dst_len %zu outside 1..255", op, dst_len);
  else if (!dst) r.rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: NULL buffer (dst)", op);
  else if (out_len < 1 || out_len > 65535) r.rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: %s: out_len %zu outside 1..65535", op, out_len);
  return r;
}

int ncg_xof_shake256_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst, size_t dst_len,
                               size_t out_len, void* out_dev, void* stream) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, "xof_shake256_batch", 1, n, dst, dst_len, out_len, {}), n, msg_off_dev, out_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, 512, st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c448_xof_batch((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, (uint32_t)out_len,
                                     (uint8_t*)out_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_xof_shake256_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len, size_t out_len,
                           void* out) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, "xof_shake256_batch", 1, n, dst, dst_len, out_len, {}), n, msg_off, out);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "xof_shake256_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out, n * out_len);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_xof_shake256_batch_dev(ctx, n, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, out_len, hc.dev(o), ctx->stream));
}
int ncg_ed448_h2c_hash_batch_dev(ncg_ctx* ctx, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                 size_t dst_len, void* out_affine112_dev, void* stream) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, "ed448_h2c_hash_batch", count, n, dst, dst_len, 1, {out_affine112_dev}), n, msg_off_dev, out_affine112_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, ncg::h2c448_ws_bytes(n), st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c448_hash((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, count,
                                (uint32_t*)out_affine112_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_ed448_h2c_hash_batch(ncg_ctx* ctx, size_t n, int count, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                             void* out_affine112) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, "ed448_h2c_hash_batch", count, n, dst, dst_len, 1, {}), n, msg_off, out_affine112);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "ed448_h2c_hash_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out_affine112, n * 112);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_h2c_hash_batch_dev(ctx, n, count, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o), ctx->stream));
}
int ncg_ed448_h2c_map_batch_dev(ncg_ctx* ctx, size_t n, int count, const void* u56_dev, void* out_affine112_dev, void* stream) {
  NCG_BEGIN(ctx, h2c448_rows_rule(ctx, "ed448_h2c_map_batch", count, n, {u56_dev, out_affine112_dev}), n, u56_dev, out_affine112_dev);
  NCG_HIP(ctx, ncg::h2c448_map((const uint32_t*)u56_dev, count, (uint32_t*)out_affine112_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_ed448_h2c_map_batch(ncg_ctx* ctx, size_t n, int count, const void* u56, void* out_affine112) {
  NCG_BEGIN(ctx, h2c448_rows_rule(ctx, "ed448_h2c_map_batch", count, n, {}), n, u56, out_affine112);
  HostCall hc(ctx);
  const int in = hc.in(u56, n * (size_t)count * 56);
  const int o = hc.out(out_affine112, n * 112);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_h2c_map_batch_dev(ctx, n, count, hc.dev(in), hc.dev(o), ctx->stream));
}
int ncg_ed448_h2c_hash_to_field_batch_dev(ncg_ctx* ctx, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                          size_t dst_len, void* out_u56_dev, void* stream) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, "ed448_h2c_hash_to_field_batch", count, n, dst, dst_len, 1, {out_u56_dev}), n, msg_off_dev, out_u56_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, ncg::h2c448_ws_bytes(n), st, &ws)) return rc;
  NCG_HIP(ctx, ncg::h2c448_hash_to_field((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, count,
                                         (uint32_t*)out_u56_dev, (int)n, ws, st));
  return NCG_OK;
}
int ncg_ed448_h2c_hash_to_field_batch(ncg_ctx* ctx, size_t n, int count, const void* msgs, const uint64_t* msg_off, const void* dst,
                                      size_t dst_len, void* out_u56) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, "ed448_h2c_hash_to_field_batch", count, n, dst, dst_len, 1, {}), n, msg_off, out_u56);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, "ed448_h2c_hash_to_field_batch", n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out_u56, n * (size_t)count * 56);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_ed448_h2c_hash_to_field_batch_dev(ctx, n, count, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o),
                                                         ctx->stream));
}
// the three calls that hash every message to one 56-byte row
typedef hipError_t (*H2c448RowFn)(const uint8_t*, const uint64_t*, const uint8_t*, uint32_t, uint32_t*, int, uint8_t*, hipStream_t);
static int h2c448_rows_dev(ncg_ctx* ctx, const char* op, H2c448RowFn fn, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev,
                           const void* dst, size_t dst_len, void* out56_dev, void* stream) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, op, 1, n, dst, dst_len, 1, {out56_dev}), n, msg_off_dev, out56_dev);
  const hipStream_t st = stream_of(ctx, stream);
  uint8_t* ws;
  if (int rc = h2c_ws(ctx, ncg::h2c448_ws_bytes(n), st, &ws)) return rc;
  NCG_HIP(ctx, fn((const uint8_t*)msgs_dev, msg_off_dev, (const uint8_t*)dst, (uint32_t)dst_len, (uint32_t*)out56_dev, (int)n, ws, st));
  return NCG_OK;
}
static int h2c448_rows_host(ncg_ctx* ctx, const char* op, H2c448RowFn fn, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst,
                            size_t dst_len, void* out56) {
  NCG_BEGIN(ctx, h2c448_rule(ctx, op, 1, n, dst, dst_len, 1, {}), n, msg_off, out56);
  std::vector<uint64_t> rel;
  HostCall hc(ctx);
  int msg, off;
  if (int rc = stage_msgs(hc, op, n, msgs, msg_off, rel, &msg, &off)) return rc;
  const int o = hc.out(out56, n * 56);
  if (int rc = hc.stage()) return rc;
  return hc.finish(h2c448_rows_dev(ctx, op, fn, n, hc.dev(msg), hc.dev<const uint64_t>(off), dst, dst_len, hc.dev(o), ctx->stream));
}
int ncg_ed448_h2c_hash_to_scalar_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                           size_t dst_len, void* out56_dev, void* stream) {
  return h2c448_rows_dev(ctx, "ed448_h2c_hash_to_scalar_batch", ncg::h2c448_hash_to_scalar, n, msgs_dev, msg_off_dev, dst, dst_len, out56_dev, stream);
}
int ncg_ed448_h2c_hash_to_scalar_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                                       void* out56) {
  return h2c448_rows_host(ctx, "ed448_h2c_hash_to_scalar_batch", ncg::h2c448_hash_to_scalar, n, msgs, msg_off, dst, dst_len, out56);
}
int ncg_decaf448_hash_to_group_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                         size_t dst_len, void* out56_dev, void* stream) {
  return h2c448_rows_dev(ctx, "decaf448_hash_to_group_batch", ncg::decaf448_hash_to_group, n, msgs_dev, msg_off_dev, dst, dst_len, out56_dev, stream);
}
int ncg_decaf448_hash_to_group_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                                     void* out56) {
  return h2c448_rows_host(ctx, "decaf448_hash_to_group_batch", ncg::decaf448_hash_to_group, n, msgs, msg_off, dst, dst_len, out56);
}
int ncg_decaf448_hash_to_scalar_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                          size_t dst_len, void* out56_dev, void* stream) {
  return h2c448_rows_dev(ctx, "decaf448_hash_to_scalar_batch", ncg::decaf448_hash_to_scalar, n, msgs_dev, msg_off_dev, dst, dst_len, out56_dev, stream);
}
int ncg_decaf448_hash_to_scalar_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                                      void* out56) {
  return h2c448_rows_host(ctx, "decaf448_hash_to_scalar_batch", ncg::decaf448_hash_to_scalar, n, msgs, msg_off, dst, dst_len, out56);
}
// The pieces of h2c448.hpp on raw words, in the style of ncg_h2c_check: rows of 42 words in and out
int ncg_h2c448_check(ncg_ctx* ctx, int op, size_t n, const void* a, void* out) {
  const Rule rule = {"h2c448_check", !ctx || n <= (1u << 24) ? NCG_OK
                                         : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: h2c448_check: batch too large (max 2^24)")};
  NCG_BEGIN(ctx, rule, n, a, out);
  HostCall hc(ctx);
  const int da = hc.in(a, n * 168);
  const int o = hc.out(out, n * 168, true);
  if (int rc = hc.stage()) return rc;
  NCG_HIP(ctx, ncg::h2c448_check(op, hc.dev<const uint32_t>(da), hc.dev<uint32_t>(o), (int)n, ctx->stream));
  return hc.finish(NCG_OK);
}

// ---- bls12-381 pairings (pairing.hip).  The _dev form keeps the verdict word, the group offsets and the Miller values in
// ctx->pair_ws, never in ctx->scratch.
static Rule pairing_rule(ncg_ctx* ctx, size_t n_pairs, size_t n_groups, const uint32_t* off, int flags) {
  int rc = NCG_OK;
  if (flags & ~NCG_PAIRING_CHECK_SUBGROUP) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: unknown flag bits 0x%x", flags);
  else if (n_pairs > 0x7fffffffu || n_groups > 0x7fffffffu) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: batch too large");
  else if (n_groups && !off) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: NULL buffer");
  else if (n_groups) {
    bool ok = off[0] == 0 && off[n_groups] == n_pairs;
    for (size_t g = 0; ok && g < n_groups; g++) ok = off[g] <= off[g + 1];
    if (!ok)
      rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: group offsets must ascend from 0 to the number of pairs");
  } else if (n_pairs) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: pairs without a group");
  return {"pairing_batch", rc};
}
// the reference's message for each refusal (bls.ts:685; weierstrass.ts:748-766 assertValidity)
static const char* pairing_bad_message(uint32_t code) {
  switch (code) {
    case 1: return "pairing is not available for ZERO point";
    case 3:
    case 5: return "bad point: not in prime-order subgroup";
    default: return "bad point: equation left != right";
  }
}
int ncg_pairing_batch_dev(ncg_ctx* ctx, size_t n_pairs, const void* g1_affine_dev, const void* g2_affine_dev, size_t n_groups,
                          const uint32_t* group_offsets, int flags, void* out_gt_dev, uint8_t* out_is_one_dev, int64_t* out_bad_index,
                          void* stream) {
  if (out_bad_index) *out_bad_index = -1;
  NCG_BEGIN(ctx, pairing_rule(ctx, n_pairs, n_groups, group_offsets, flags), n_groups, out_is_one_dev);
  if (n_pairs && (!g1_affine_dev || !g2_affine_dev)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: NULL buffer");
  const hipStream_t st = stream_of(ctx, stream);
  const size_t off_b = align256((n_groups + 1) * 4);
  if (int rc = ncg_grow_buf(ctx, &ctx->pair_ws, &ctx->pair_ws_bytes, 256 + off_b + n_pairs * ncg::PAIRING_WS_WORDS * 4,
                            256 + off_b + n_pairs * ncg::PAIRING_WS_WORDS * 4, GrowWait::stream, st))
    return rc;
  unsigned long long* d_bad = (unsigned long long*)ctx->pair_ws;
  uint32_t* d_off = (uint32_t*)((char*)ctx->pair_ws + 256);
  uint32_t* d_f = (uint32_t*)((char*)ctx->pair_ws + 256 + off_b);
  NCG_HIP(ctx, hipMemcpyAsync(d_off, group_offsets, (n_groups + 1) * 4, hipMemcpyHostToDevice, st));
  NCG_HIP(ctx, ncg::pairing_miller((const uint32_t*)g1_affine_dev, (const uint32_t*)g2_affine_dev, flags & NCG_PAIRING_CHECK_SUBGROUP, d_f, d_bad, (int)n_pairs, st));
  unsigned long long bad = 0;
  NCG_HIP(ctx, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
  NCG_HIP(ctx, hipStreamSynchronize(st));  // (also: group_offsets has been read)
  if (bad != ~0ull) {
    if (out_bad_index) *out_bad_index = (int64_t)(bad >> 8);
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: %s (%s operand) at index %llu", pairing_bad_message((uint32_t)(bad & 0xff)),
                   (bad & 0xff) == 1 ? "G1 or G2" : (bad & 0xff) <= 3 ? "G1" : "G2", bad >> 8);
  }
  uint32_t largest = 0;
  for (size_t g = 0; g < n_groups; g++) largest = std::max(largest, group_offsets[g + 1] - group_offsets[g]);
  NCG_HIP(ctx, ncg::pairing_finish(d_f, d_off, (int)n_groups, (int)n_pairs, largest, (uint32_t*)out_gt_dev, out_is_one_dev, st));
  NCG_HIP(ctx, hipStreamSynchronize(st));
  return NCG_OK;
}
int ncg_pairing_batch(ncg_ctx* ctx, size_t n_pairs, const void* g1_affine, const void* g2_affine, size_t n_groups,
                      const uint32_t* group_offsets, int flags, void* out_gt, uint8_t* out_is_one, int64_t* out_bad_index) {
  if (out_bad_index) *out_bad_index = -1;
  NCG_BEGIN(ctx, pairing_rule(ctx, n_pairs, n_groups, group_offsets, flags), n_groups, out_is_one);
  if (n_pairs && (!g1_affine || !g2_affine)) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: pairing_batch: NULL buffer");
  HostCall hc(ctx);
  const int a = hc.in(g1_affine, n_pairs * 96), b = hc.in(g2_affine, n_pairs * 192);
  const int gt = out_gt ? hc.out(out_gt, n_groups * 576) : -1, one = hc.out(out_is_one, n_groups);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_pairing_batch_dev(ctx, n_pairs, hc.dev(a), hc.dev(b), n_groups, group_offsets, flags, gt < 0 ? nullptr : hc.dev(gt),
                                         hc.dev<uint8_t>(one), out_bad_index, ctx->stream));
}

// ---- BLS signature verification for a batch (pairing.hip k_bls_pairs): decode with the subgroup checks, map the messages, two
// pairs per row through the pairing path, is_one - five device steps, only bytes cross.  Everything between them lives in ctx->bls_ws.
static Rule bls_rule(ncg_ctx* ctx, int scheme, size_t n) {
  int rc = NCG_OK;
  if (scheme != 0 && scheme != 1) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: bls_verify_batch: scheme must be 0 (long) or 1 (short), got %d", scheme);
  else if (n > 0x3fffffffu) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: bls_verify_batch: batch too large");
  return {"bls_verify_batch", rc};
}
int ncg_bls_verify_batch_dev(ncg_ctx* ctx, int scheme, size_t n, const void* pk_enc_dev, const void* sig_enc_dev, const void* u_dev,
                             uint8_t* out_ok_dev, void* stream) {
  NCG_BEGIN(ctx, bls_rule(ctx, scheme, n), n, pk_enc_dev, sig_enc_dev, u_dev, out_ok_dev);
  const hipStream_t st = stream_of(ctx, stream);
  const int pk_curve = scheme == 0 ? NCG_BLS12_381_G1 : NCG_BLS12_381_G2, sig_curve = scheme == 0 ? NCG_BLS12_381_G2 : NCG_BLS12_381_G1;
  const size_t pkb = align256(n * (size_t)ncg_point_bytes(pk_curve)), sgb = align256(n * (size_t)ncg_point_bytes(sig_curve)), fb = align256(n);
  const size_t g1b = align256(2 * n * 96), g2b = align256(2 * n * 192);
  const size_t total = pkb + 2 * sgb + 7 * fb + g1b + g2b;
  if (int rc = ncg_grow_buf(ctx, &ctx->bls_ws, &ctx->bls_ws_bytes, total, total, GrowWait::stream, st)) return rc;
  char* p = (char*)ctx->bls_ws;
  uint32_t* d_pk = (uint32_t*)p;  p += pkb;
  uint32_t* d_sig = (uint32_t*)p; p += sgb;
  uint32_t* d_hm = (uint32_t*)p;  p += sgb;
  uint8_t* fl[7];
  for (int k = 0; k < 7; k++) { fl[k] = (uint8_t*)p; p += fb; }   // pk ok / inf, sig ok / inf, hm inf, bad, is_one
  uint32_t* d_g1 = (uint32_t*)p;  p += g1b;
  uint32_t* d_g2 = (uint32_t*)p;
  if (int rc = ncg_decode_points_batch_dev(ctx, pk_curve, n, pk_enc_dev, 0, d_pk, fl[0], fl[1], st)) return rc;
  if (int rc = ncg_decode_points_batch_dev(ctx, sig_curve, n, sig_enc_dev, 0, d_sig, fl[2], fl[3], st)) return rc;
  if (int rc = ncg_map_to_curve_batch_dev(ctx, sig_curve, n, 2, u_dev, d_hm, fl[4], st)) return rc;
  NCG_HIP(ctx, ncg::bls_build_pairs(scheme, d_pk, fl[0], fl[1], d_sig, fl[2], fl[3], d_hm, fl[4], d_g1, d_g2, fl[5], (int)n, st));
  std::vector<uint32_t> off(n + 1);
  for (size_t i = 0; i <= n; i++) off[i] = (uint32_t)(2 * i);
  // (every point is a decoded or mapped subgroup member or a generator: the pairing refuses nothing here)
  if (int rc = ncg_pairing_batch_dev(ctx, 2 * n, d_g1, d_g2, n, off.data(), 0, nullptr, fl[6], nullptr, st)) return rc;
  NCG_HIP(ctx, ncg::bls_verdict(fl[6], fl[5], out_ok_dev, (int)n, st));
  NCG_HIP(ctx, hipStreamSynchronize(st));
  return NCG_OK;
}
int ncg_bls_verify_batch(ncg_ctx* ctx, int scheme, size_t n, const void* pk_enc, const void* sig_enc, const void* u, uint8_t* out_ok) {
  NCG_BEGIN(ctx, bls_rule(ctx, scheme, n), n, pk_enc, sig_enc, u, out_ok);
  HostCall hc(ctx);
  const int pk = hc.in(pk_enc, n * (scheme == 0 ? 48 : 96)), sg = hc.in(sig_enc, n * (scheme == 0 ? 96 : 48));
  const int du = hc.in(u, n * (scheme == 0 ? 192 : 96)), ok = hc.out(out_ok, n);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_bls_verify_batch_dev(ctx, scheme, n, hc.dev(pk), hc.dev(sg), hc.dev(du), hc.dev<uint8_t>(ok), ctx->stream));
}

static Rule fp12_rule(ncg_ctx* ctx, int op) {
  return {"fp12_batch", op >= NCG_FP12_MUL && op <= NCG_FP12_IS_ONE ? NCG_OK : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: fp12_batch: unknown op %d", op)};
}
static size_t fp12_b_bytes(int op) { return op == NCG_FP12_MUL ? 576 : op == NCG_FP12_MUL014 ? 288 : 0; }
int ncg_fp12_batch_dev(ncg_ctx* ctx, int op, size_t n, const void* a_dev, const void* b_dev, void* out_dev, void* stream) {
  NCG_BEGIN(ctx, fp12_rule(ctx, op), n, a_dev, out_dev);
  if (fp12_b_bytes(op) && !b_dev) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: fp12_batch: NULL buffer");
  NCG_HIP(ctx, ncg::fp12_batch(op, (const uint32_t*)a_dev, (const uint32_t*)b_dev, out_dev, (int)n, stream_of(ctx, stream)));
  return NCG_OK;
}
int ncg_fp12_batch(ncg_ctx* ctx, int op, size_t n, const void* a, const void* b, void* out) {
  NCG_BEGIN(ctx, fp12_rule(ctx, op), n, a, out);
  if (fp12_b_bytes(op) && !b) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: fp12_batch: NULL buffer");
  HostCall hc(ctx);
  const int da = hc.in(a, n * 576), db = fp12_b_bytes(op) ? hc.in(b, n * fp12_b_bytes(op)) : -1;
  const int o = hc.out(out, op == NCG_FP12_IS_ONE ? n : n * 576);
  if (int rc = hc.stage()) return rc;
  return hc.finish(ncg_fp12_batch_dev(ctx, op, n, hc.dev(da), db < 0 ? nullptr : hc.dev(db), hc.dev(o), ctx->stream));
}

static Rule field_rule(ncg_ctx* ctx, int field, size_t n) {
  int rc = NCG_OK;
  if (!ncg::selfcheck_field(field)) rc = set_err(ctx, NCG_ERR_UNSUPPORTED, "noble-gpu: field_check: unknown field %d", field);
  else if (n > (1u << 24)) rc = set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: field_check: batch too large (max 2^24)");
  return {"field_check", rc};
}
int ncg_field_check(ncg_ctx* ctx, int field, int op, int variant, size_t n, const void* a, const void* b, void* out) {
  NCG_BEGIN(ctx, field_rule(ctx, field, n), n, a, b, out);
  HostCall hc(ctx);
  const ncg::SelfCheckField& f = *ncg::selfcheck_field(field);  // selfcheck.hpp: words per row
  const int da = hc.in(a, n * f.wa * 4), db = hc.in(b, n * f.wb * 4);
  const int o = hc.out(out, n * f.wo * 4, true);
  if (int rc = hc.stage()) return rc;
  NCG_HIP(ctx, ncg::field_check_run(field, op, variant, hc.dev<const uint32_t>(da), hc.dev<const uint32_t>(db), hc.dev<uint32_t>(o), (int)n,
                                    ctx->stream));
  return hc.finish(NCG_OK);
}

// The pieces of fe448.hpp / ed448.hpp on raw limbs.  Its own entry point: the table of ncg_field_check is closed.  An op nobody
// defines reads nothing and leaves rows of 16 zero words.
int ncg_fe448_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out) {
  const Rule rule = {"fe448_check", !ctx || n <= (1u << 24) ? NCG_OK
                                        : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: fe448_check: batch too large (max 2^24)")};
  NCG_BEGIN(ctx, rule, n, a, b, out);
  int wa, wb, wo;
  ncg::fe448_check_row_words(op, &wa, &wb, &wo);
  HostCall hc(ctx);
  const int da = hc.in(a, n * wa * 4), db = hc.in(b, n * wb * 4);
  const int o = hc.out(out, n * (wo ? wo : 16) * 4, true);
  if (int rc = hc.stage()) return rc;
  if (wo)
    NCG_HIP(ctx, ncg::fe448_check(op, variant, hc.dev<const uint32_t>(da), hc.dev<const uint32_t>(db), hc.dev<uint32_t>(o), (int)n, ctx->stream));
  return hc.finish(NCG_OK);
}

// The pieces of decaf448.hpp on raw limbs, in the same style: an op nobody defines reads nothing and leaves rows of 16 zero words.
int ncg_decaf448_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out) {
  (void)variant;  // no op has variants yet
  const Rule rule = {"decaf448_check", !ctx || n <= (1u << 24) ? NCG_OK
                                           : set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: decaf448_check: batch too large (max 2^24)")};
  NCG_BEGIN(ctx, rule, n, a, b, out);
  int wa, wb, wo;
  ncg::decaf448_check_row_words(op, &wa, &wb, &wo);
  HostCall hc(ctx);
  const int da = hc.in(a, n * wa * 4), db = hc.in(b, n * wb * 4);
  const int o = hc.out(out, n * (wo ? wo : 16) * 4, true);
  if (int rc = hc.stage()) return rc;
  if (wo) NCG_HIP(ctx, ncg::decaf448_check(op, hc.dev<const uint32_t>(da), hc.dev<const uint32_t>(db), hc.dev<uint32_t>(o), (int)n, ctx->stream));
  return hc.finish(NCG_OK);
}

int ncg_ubench(ncg_ctx* ctx, int kind, int blocks, int threads, int iters, float* out_ms) {
  if (!ctx || !out_ms) return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ubench: NULL arg");
  if (blocks <= 0 || threads <= 0 || threads > 256 || iters <= 0)
    return set_err(ctx, NCG_ERR_INVALID_ARG, "noble-gpu: ubench: bad geometry");
  NCG_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->ub_in) {
    NCG_HIP(ctx, hipMalloc((void**)&ctx->ub_in, 1024 * 4));
    uint32_t h[1024];
    uint32_t x = 0x9e3779b9u;
    for (int i = 0; i < 1024; i++) {
      x ^= x << 13;
      x ^= x >> 17;
      x ^= x << 5;
      h[i] = x;
    }
    NCG_HIP(ctx, hipMemcpy(ctx->ub_in, h, sizeof h, hipMemcpyHostToDevice));
  }
  const size_t bytes = (size_t)blocks * threads * 4;
  if (int rc = ncg_grow_buf(ctx, (void**)&ctx->ub_out, &ctx->ub_out_bytes, bytes, bytes)) return rc;
  NCG_HIP(ctx, ncg::ubench_run(kind, blocks, threads, iters, ctx->ub_out, ctx->ub_in, ctx->stream, out_ms));
  return NCG_OK;
}

}  // extern "C"
#pragma GCC visibility pop
