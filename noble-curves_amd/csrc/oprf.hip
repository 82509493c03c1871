// Batch ristretto255-SHA512 OPRF (RFC 9497; createOPRF of src/abstract/oprf.ts): the lane code of oprf.hpp, one row per lane.
// The rows with a point in them run in blocks of 64 like the other ed25519 field kernels, the rows that only hash in blocks of 256
// like the SHA-512 kernels of ed25519_sign.hip.
//   k_oprf_put            bytes of a kernel argument into the workspace: DST', "Seed-" || ctx, info (host pointers in both forms)
//   k_oprf_xmd            expand_message_xmd over SHA-512
//   k_oprf_hash_to_group  xmd -> two Elligator maps -> sum -> encode [and the affine representative]
//   k_oprf_hash_to_scalar xmd -> mod L
//   k_oprf_prep_scalar    the one scalar of a call, inverted once
//   k_oprf_blind / k_oprf_mul / k_oprf_finalize / k_oprf_evaluate / k_oprf_composite: the fused rows of oprf.hpp
//   k_oprf_seed           the seed of the composites, one lane
#include "host_api.hpp"
#include "oprf.hpp"

namespace ncg {

// two waves per SIMD asked of the compiler: the doubled and the added point (2 x 36 limbs), the Niels form of P (36) and the scalar
// are live across the products of ristretto_mul_secret's loop, which does not fit the 168 registers of three waves without
// spilling (DESIGN.md section 8 has the register counts); the rows that only hash and map end up at three waves anyway
constexpr int OPRF_MINW = 2;

// blocks of b lanes for n rows; n may be anything up to 2^31 - 1, so the sum is taken in 64 bits
static dim3 oprf_grid(int n, int b) { return dim3((unsigned)(((long long)n + b - 1) / b)); }

struct OprfBytesArg {
  uint8_t b[OPRF_PUT_CHUNK];
};
__global__ void __launch_bounds__(256) k_oprf_put(OprfBytesArg arg, uint8_t* __restrict__ out, uint32_t len) {
  for (uint32_t i = threadIdx.x; i < len; i += 256) out[i] = arg.b[i];
}

struct OprfMsgs {
  const uint8_t* msgs;
  const uint64_t* off;
  NCG_DI const uint8_t* at(int i, uint64_t* len) const {
    const uint64_t lo = off[i];
    *len = off[i + 1] - lo;
    return msgs + lo;
  }
};

__global__ void __launch_bounds__(256) k_oprf_xmd(OprfMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t out_len,
                                                   uint8_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  xmd_sha512_lane(msg, len, dstp, dstp_len, out_len, out + (size_t)i * out_len);
}
NCG_DI void oprf_hash_to_group_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                   uint32_t* __restrict__ out, uint32_t* __restrict__ out_affine) {
  const EdExt<FEd> p = ristretto_hash_to_group(msg, len, dstp, dstp_len);
  uint32_t r[8];
  ristretto_encode_ext(p.X, p.Y, p.Z, p.T, r);
  oprf_store8_masked(out, r, ~0u);
  if (out_affine) {
    const FEd zi = f_inv(p.Z);
    fe9_to_wire(out_affine, p.X * zi);
    fe9_to_wire(out_affine + 8, p.Y * zi);
  }
}
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_hash_to_group(OprfMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                                                       uint32_t* __restrict__ out, uint32_t* __restrict__ out_affine, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  oprf_hash_to_group_row(msg, len, dstp, dstp_len, out + (size_t)i * 8, out_affine ? out_affine + (size_t)i * 16 : nullptr);
}
NCG_DI void oprf_hash_to_scalar_row(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                    uint32_t* __restrict__ out) {
  const OSeg seg[1] = {oseg_mem(msg, len)};
  uint32_t k[8];
  ristretto_hash_to_scalar<1>(k, seg, dstp, dstp_len);
  oprf_store8_masked(out, k, ~0u);
}
__global__ void __launch_bounds__(256) k_oprf_hash_to_scalar(OprfMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                                              uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  oprf_hash_to_scalar_row(msg, len, dstp, dstp_len, out + (size_t)i * 8);
}
// 1 / scalar, or zero - which every row then refuses - where the scalar is zero or not below L
NCG_DI void oprf_prep_scalar_row(const uint32_t* __restrict__ scalar, uint32_t* __restrict__ out) {
  uint32_t k[8];
  const uint32_t ok = oprf_row_scalar(k, scalar, true);
  oprf_store8_masked(out, k, ok);
}
__global__ void __launch_bounds__(64) k_oprf_prep_scalar(const uint32_t* __restrict__ scalar, uint32_t* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) oprf_prep_scalar_row(scalar, out);
}
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_blind(OprfMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                                               const uint32_t* __restrict__ blinds, uint32_t* __restrict__ out,
                                                               uint8_t* __restrict__ status, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  status[i] = oprf_blind_row(msg, len, dstp, dstp_len, blinds + (size_t)i * 8, out + (size_t)i * 8);
}
// scalar_stride: 8, or 0 when one scalar serves every row
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_mul(const uint32_t* __restrict__ elements, const uint32_t* __restrict__ scalars,
                                                             int scalar_stride, int invert, uint32_t* __restrict__ out,
                                                             uint8_t* __restrict__ status, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  status[i] = oprf_mul_row(elements + (size_t)i * 8, scalars + (size_t)i * scalar_stride, invert != 0, out + (size_t)i * 8);
}
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_finalize(OprfMsgs m, const uint8_t* __restrict__ info, uint32_t info_len,
                                                                  const uint32_t* __restrict__ blinds, const uint32_t* __restrict__ evaluated,
                                                                  uint8_t* __restrict__ out64, uint8_t* __restrict__ status, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  status[i] = oprf_finalize_row(msg, len, info, info_len, blinds + (size_t)i * 8, evaluated + (size_t)i * 8, out64 + (size_t)i * 64);
}
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_evaluate(OprfMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                                                  const uint8_t* __restrict__ info, uint32_t info_len,
                                                                  const uint32_t* __restrict__ scalars, int scalar_stride, int invert,
                                                                  uint8_t* __restrict__ out64, uint8_t* __restrict__ status, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  status[i] = oprf_evaluate_row(msg, len, dstp, dstp_len, info, info_len, scalars + (size_t)i * scalar_stride, invert != 0,
                                out64 + (size_t)i * 64);
}
__global__ void __launch_bounds__(64) k_oprf_seed(const uint8_t* __restrict__ B32, const uint8_t* __restrict__ sdst, uint32_t sdst_len,
                                                   uint8_t* __restrict__ seed64) {
  if (blockIdx.x == 0 && threadIdx.x == 0) oprf_seed_lane(B32, sdst, sdst_len, seed64);
}
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_composite(const uint8_t* __restrict__ seed64, const uint32_t* __restrict__ C,
                                                                   const uint32_t* __restrict__ D, const uint8_t* __restrict__ dstp,
                                                                   uint32_t dstp_len, uint32_t* __restrict__ out, uint8_t* __restrict__ status,
                                                                   int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  status[i] = oprf_composite_row(seed64, (uint32_t)i, C + (size_t)i * 8, D + (size_t)i * 8, dstp, dstp_len, out + (size_t)i * 8);
}
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_check(int op, int variant, int wa, int wb, int wo, const uint32_t* __restrict__ a,
                                                               const uint32_t* __restrict__ b, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  (void)oprf_check_op(op, variant, a + (size_t)i * wa, b + (size_t)i * wb, out + (size_t)i * wo);
}

// ---- the strings of a mode: ctx = "OPRFV1-" || mode || "-ristretto255-SHA512" behind a prefix; with_len: DST' (the length byte)
size_t oprf_dst(const char* prefix, int mode, int with_len, uint8_t* out) {
  static const char name[] = "-ristretto255-SHA512";
  size_t k = 0;
  for (const char* p = prefix; *p; p++) out[k++] = (uint8_t)*p;
  for (const char* p = "OPRFV1-"; *p; p++) out[k++] = (uint8_t)*p;
  out[k++] = (uint8_t)mode;
  for (const char* p = name; *p; p++) out[k++] = (uint8_t)*p;
  if (with_len) {
    out[k] = (uint8_t)k;
    k++;
  }
  return k;
}

// ---- launchers.  ws: oprf_ws_bytes(info_len) bytes of device memory; the strings go in through kernel arguments
size_t oprf_ws_bytes(size_t info_len) { return OPRF_WS_INFO + ((info_len + 255) & ~(size_t)255); }
hipError_t oprf_put(uint8_t* d_out, const uint8_t* host, size_t len, hipStream_t st) {
  for (size_t done = 0; done < len; done += OPRF_PUT_CHUNK) {
    OprfBytesArg arg;
    const size_t part = len - done < OPRF_PUT_CHUNK ? len - done : (size_t)OPRF_PUT_CHUNK;
    for (size_t i = 0; i < OPRF_PUT_CHUNK; i++) arg.b[i] = i < part ? host[done + i] : 0;
    hipLaunchKernelGGL(k_oprf_put, dim3(1), dim3(256), 0, st, arg, d_out + done, (uint32_t)part);
    for (size_t i = 0; i < OPRF_PUT_CHUNK; i++) ((volatile uint8_t*)arg.b)[i] = 0;   // it may have held a key; the runtime's own copy of the argument is beyond reach
  }
  return hipGetLastError();
}
static hipError_t oprf_put_dst(uint8_t* ws, const uint8_t* dst, uint32_t dst_len, hipStream_t st) {  // DST' = DST || len
  uint8_t buf[256];
  for (uint32_t i = 0; i < dst_len; i++) buf[i] = dst[i];
  buf[dst_len] = (uint8_t)dst_len;
  return oprf_put(ws + OPRF_WS_DST, buf, dst_len + 1, st);
}
static hipError_t oprf_put_mode_dst(uint8_t* ws, const char* prefix, int mode, hipStream_t st, uint32_t* dstp_len) {
  uint8_t buf[256];
  *dstp_len = (uint32_t)oprf_dst(prefix, mode, 1, buf);
  return oprf_put(ws + OPRF_WS_DST, buf, *dstp_len, st);
}
// the scalars a row kernel reads: as given, or the one scalar inverted once into the workspace
static hipError_t oprf_scalars(uint8_t* ws, const uint32_t*& scalars, int flags, int* stride, int* invert, hipStream_t st) {
  const bool one = (flags & OPRF_FLAG_ONE_SCALAR) != 0;
  *stride = one ? 0 : 8;
  *invert = (flags & OPRF_FLAG_INVERT) != 0;
  if (one && *invert) {
    uint32_t* d_k = (uint32_t*)(ws + OPRF_WS_SCALAR);
    hipLaunchKernelGGL(k_oprf_prep_scalar, dim3(1), dim3(64), 0, st, scalars, d_k);
    scalars = d_k;
    *invert = 0;
  }
  return hipGetLastError();
}

hipError_t oprf_xmd_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t out_len, uint8_t* out,
                          int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (hipError_t e = oprf_put_dst(ws, dst_host, dst_len, st)) return e;
  hipLaunchKernelGGL(k_oprf_xmd, oprf_grid(n, 256), dim3(256), 0, st, OprfMsgs{msgs, off}, ws + OPRF_WS_DST, dst_len + 1, out_len, out, n);
  return hipGetLastError();
}
hipError_t oprf_hash_to_group_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out,
                                    uint32_t* out_affine, int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (hipError_t e = oprf_put_dst(ws, dst_host, dst_len, st)) return e;
  hipLaunchKernelGGL(k_oprf_hash_to_group, oprf_grid(n, 64), dim3(64), 0, st, OprfMsgs{msgs, off}, ws + OPRF_WS_DST, dst_len + 1, out,
                     out_affine, n);
  return hipGetLastError();
}
hipError_t oprf_hash_to_scalar_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                     uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (hipError_t e = oprf_put_dst(ws, dst_host, dst_len, st)) return e;
  hipLaunchKernelGGL(k_oprf_hash_to_scalar, oprf_grid(n, 256), dim3(256), 0, st, OprfMsgs{msgs, off}, ws + OPRF_WS_DST, dst_len + 1, out, n);
  return hipGetLastError();
}
hipError_t oprf_blind_batch(int mode, const uint8_t* inputs, const uint64_t* off, const uint32_t* blinds, uint32_t* out, uint8_t* status, int n,
                            uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint32_t dl;
  if (hipError_t e = oprf_put_mode_dst(ws, "HashToGroup-", mode, st, &dl)) return e;
  hipLaunchKernelGGL(k_oprf_blind, oprf_grid(n, 64), dim3(64), 0, st, OprfMsgs{inputs, off}, ws + OPRF_WS_DST, dl, blinds, out, status, n);
  return hipGetLastError();
}
hipError_t oprf_mul_batch(const uint32_t* elements, const uint32_t* scalars, int flags, uint32_t* out, uint8_t* status, int n, uint8_t* ws,
                          hipStream_t st) {
  if (n <= 0) return hipSuccess;
  int stride, invert;
  if (hipError_t e = oprf_scalars(ws, scalars, flags, &stride, &invert, st)) return e;
  hipLaunchKernelGGL(k_oprf_mul, oprf_grid(n, 64), dim3(64), 0, st, elements, scalars, stride, invert, out, status, n);
  return hipGetLastError();
}
// info_host: null outside mode 2
static hipError_t oprf_put_info(uint8_t* ws, const uint8_t* info_host, uint32_t info_len, bool has_info, hipStream_t st, const uint8_t** d_info) {
  *d_info = has_info ? ws + OPRF_WS_INFO : nullptr;
  return has_info ? oprf_put(ws + OPRF_WS_INFO, info_host, info_len, st) : hipSuccess;
}
hipError_t oprf_finalize_batch(int mode, const uint8_t* inputs, const uint64_t* off, const uint8_t* info_host, uint32_t info_len,
                               const uint32_t* blinds, const uint32_t* evaluated, uint8_t* out64, uint8_t* status, int n, uint8_t* ws,
                               hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const uint8_t* d_info;
  if (hipError_t e = oprf_put_info(ws, info_host, info_len, mode == 2, st, &d_info)) return e;
  hipLaunchKernelGGL(k_oprf_finalize, oprf_grid(n, 64), dim3(64), 0, st, OprfMsgs{inputs, off}, d_info, info_len, blinds, evaluated, out64,
                     status, n);
  return hipGetLastError();
}
hipError_t oprf_evaluate_batch(int mode, const uint8_t* inputs, const uint64_t* off, const uint8_t* info_host, uint32_t info_len,
                               const uint32_t* scalars, int flags, uint8_t* out64, uint8_t* status, int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint32_t dl;
  const uint8_t* d_info;
  int stride, invert;
  if (hipError_t e = oprf_put_mode_dst(ws, "HashToGroup-", mode, st, &dl)) return e;
  if (hipError_t e = oprf_put_info(ws, info_host, info_len, mode == 2, st, &d_info)) return e;
  if (hipError_t e = oprf_scalars(ws, scalars, flags, &stride, &invert, st)) return e;
  hipLaunchKernelGGL(k_oprf_evaluate, oprf_grid(n, 64), dim3(64), 0, st, OprfMsgs{inputs, off}, ws + OPRF_WS_DST, dl, d_info, info_len, scalars,
                     stride, invert, out64, status, n);
  return hipGetLastError();
}
// B: the 32 bytes of the public key, on the HOST
hipError_t oprf_composite_batch(int mode, const uint8_t* B_host, const uint32_t* C, const uint32_t* D, uint32_t* out, uint8_t* status, int n,
                                uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint32_t dl;
  uint8_t sdst[64];
  const uint32_t sl = (uint32_t)oprf_dst("Seed-", mode, 0, sdst);
  if (hipError_t e = oprf_put_mode_dst(ws, "HashToScalar-", mode, st, &dl)) return e;
  if (hipError_t e = oprf_put(ws + OPRF_WS_SDST, sdst, sl, st)) return e;
  if (hipError_t e = oprf_put(ws + OPRF_WS_B, B_host, 32, st)) return e;
  hipLaunchKernelGGL(k_oprf_seed, dim3(1), dim3(64), 0, st, ws + OPRF_WS_B, ws + OPRF_WS_SDST, sl, ws + OPRF_WS_SEED);
  hipLaunchKernelGGL(k_oprf_composite, oprf_grid(n, 64), dim3(64), 0, st, ws + OPRF_WS_SEED, C, D, ws + OPRF_WS_DST, dl, out, status, n);
  return hipGetLastError();
}
// the three secret multiplies of generateProof, one block each (lane 0): Z = k M, t3 = r M, t2 = r B.  M: the 8 words of the
// composite; kr: k then r; out: Z, t3, t2 (24 words).  M was put together from accepted rows and k, r were checked by the caller, so
// the rows have no status: an M that is the identity gives zero rows, the identity's encoding, as the reference's multiply of ZERO does.
NCG_DI void oprf_proof_point_row(const uint32_t* __restrict__ table, const uint32_t* __restrict__ M, const uint32_t* __restrict__ kr, int b,
                                 uint32_t* __restrict__ out) {
  if (b < 2) (void)oprf_mul_row(M, kr + 8 * b, false, out + 8 * b);
  else oprf_mul_base_row(table, kr + 8, out + 16);
}
__global__ void __launch_bounds__(64, OPRF_MINW) k_oprf_proof_points(const uint32_t* __restrict__ table, const uint32_t* __restrict__ M,
                                                                      const uint32_t* __restrict__ kr, uint32_t* __restrict__ out) {
  if (threadIdx.x != 0) return;
  oprf_proof_point_row(table, M, kr, (int)blockIdx.x, out);
}
hipError_t oprf_proof_points(const uint32_t* table, const uint32_t* M, const uint32_t* kr, uint32_t* out, hipStream_t st) {
  hipLaunchKernelGGL(k_oprf_proof_points, dim3(3), dim3(64), 0, st, table, M, kr, out);
  return hipGetLastError();
}
void oprf_proof_points_host(const uint32_t* table, const uint32_t* M, const uint32_t* kr, uint32_t* out) {
  for (int b = 0; b < 3; b++) oprf_proof_point_row(table, M, kr, b, out);
}
// the host side of a proof: the scalars are host memory in both forms of the proof calls, and these are a few hundred operations
int oprf_scalar_ok_host(const uint32_t* k, int allow_zero) {
  uint32_t w[8];
  oprf_load8(w, k);
  if (allow_zero && oprf_nonzero_mask(w) == 0) return 1;
  return sc_valid_mask(w) != 0;
}
void oprf_challenge_host(int mode, const uint8_t* pts160, uint32_t* c) {
  uint8_t dp[256];
  const uint32_t dl = (uint32_t)oprf_dst("HashToScalar-", mode, 1, dp);
  uint32_t k[8];
  oprf_challenge_lane(pts160, dp, dl, k);
  oprf_store8_masked(c, k, ~0u);
}
void oprf_proof_s_host(const uint32_t* c, const uint32_t* k, const uint32_t* r, uint32_t* s) {  // r - c k mod L
  uint32_t cw[8], kw[8], rw[8], ck[8], sw[8];
  oprf_load8(cw, c);
  oprf_load8(kw, k);
  oprf_load8(rw, r);
  sc_mul(ck, cw, kw);
  sc_sub(sw, rw, ck);
  oprf_store8_masked(s, sw, ~0u);
  for (int i = 0; i < 8; i++) ((volatile uint32_t*)kw)[i] = ((volatile uint32_t*)rw)[i] = ((volatile uint32_t*)ck)[i] = 0;
}
void oprf_check_words(int op, int* wa, int* wb, int* wo) { oprf_check_row_words(op, wa, wb, wo); }
hipError_t oprf_check(int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  int wa, wb, wo;
  oprf_check_row_words(op, &wa, &wb, &wo);
  hipLaunchKernelGGL(k_oprf_check, oprf_grid(n, 64), dim3(64), 0, st, op, variant, wa, wb, wo, d_a, d_b, d_out, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same row functions, one row after the other.  dst / info as the device kernels see them.
static uint32_t oprf_dstp_host(const uint8_t* dst, uint32_t dst_len, uint8_t (&buf)[256]) {
  for (uint32_t i = 0; i < dst_len; i++) buf[i] = dst[i];
  buf[dst_len] = (uint8_t)dst_len;
  return dst_len + 1;
}
void oprf_xmd_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out) {
  uint8_t dp[256];
  const uint32_t dl = oprf_dstp_host(dst, dst_len, dp);
  xmd_sha512_lane(msg, len, dp, dl, out_len, out);
}
void oprf_hash_to_group_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out, uint32_t* out_affine) {
  uint8_t dp[256];
  const uint32_t dl = oprf_dstp_host(dst, dst_len, dp);
  oprf_hash_to_group_row(msg, len, dp, dl, out, out_affine);
}
void oprf_hash_to_scalar_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out) {
  uint8_t dp[256];
  const uint32_t dl = oprf_dstp_host(dst, dst_len, dp);
  oprf_hash_to_scalar_row(msg, len, dp, dl, out);
}
uint8_t oprf_blind_host(int mode, const uint8_t* input, uint64_t len, const uint32_t* blind, uint32_t* out) {
  uint8_t dp[256];
  const uint32_t dl = (uint32_t)oprf_dst("HashToGroup-", mode, 1, dp);
  return oprf_blind_row(input, len, dp, dl, blind, out);
}
uint8_t oprf_mul_host(const uint32_t* element, const uint32_t* scalar, int invert, uint32_t* out) {
  return oprf_mul_row(element, scalar, invert != 0, out);
}
uint8_t oprf_finalize_host(int mode, const uint8_t* input, uint64_t len, const uint8_t* info, uint32_t info_len, const uint32_t* blind,
                           const uint32_t* evaluated, uint8_t* out64) {
  static const uint8_t none[1] = {0};
  return oprf_finalize_row(input, len, mode == 2 ? (info ? info : none) : nullptr, info_len, blind, evaluated, out64);
}
uint8_t oprf_evaluate_host(int mode, const uint8_t* input, uint64_t len, const uint8_t* info, uint32_t info_len, const uint32_t* scalar,
                           int invert, uint8_t* out64) {
  static const uint8_t none[1] = {0};
  uint8_t dp[256];
  const uint32_t dl = (uint32_t)oprf_dst("HashToGroup-", mode, 1, dp);
  return oprf_evaluate_row(input, len, dp, dl, mode == 2 ? (info ? info : none) : nullptr, info_len, scalar, invert != 0, out64);
}
void oprf_composite_host(int mode, const uint8_t* B32, const uint32_t* C, const uint32_t* D, uint32_t* out, uint8_t* status, int n) {
  uint8_t dp[256], sdst[64], seed[64];
  const uint32_t dl = (uint32_t)oprf_dst("HashToScalar-", mode, 1, dp);
  const uint32_t sl = (uint32_t)oprf_dst("Seed-", mode, 0, sdst);
  oprf_seed_lane(B32, sdst, sl, seed);
  for (int i = 0; i < n; i++) status[i] = oprf_composite_row(seed, (uint32_t)i, C + (size_t)i * 8, D + (size_t)i * 8, dp, dl, out + (size_t)i * 8);
}
int oprf_check_host(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out) { return oprf_check_op(op, variant, a, b, out); }

}  // namespace ncg
