// Batch RFC 9380 for edwards448 (edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_) and the hash side of decaf448: the lane code of h2c448.hpp,
// one row per lane in blocks of 64.  The hash kernels hold the Keccak state, the map kernel the field temporaries: separate kernels.
//   k_h2c448_xof               expand_message_xof over SHAKE256 alone, any output length
//   k_h2c448_hash_to_field     xof(count * 84) -> count elements mod p (14 words each)
//   k_h2c448_hash_to_scalar    xof(84) -> one element mod n
//   k_decaf448_hash_to_scalar  xof(64), little-endian, mod n
//   k_h2c448_map               count elements -> Elligator 2, the map to Edwards form, the sum, the cofactor, one inversion: x || y
//   decaf448 hash_to_group     k_h2c448_xof(112) into the workspace, then k_decaf448_from_uniform (decaf448.hip)
// Hand-offs in the workspace: the tail `len_be2 || DST || len(DST)` that all rows share | the uniform bytes | the reduced elements.
#include "h2c448.hpp"
#include "host_api.hpp"

namespace ncg {

struct H2c448Msgs {
  const uint8_t* msgs;
  const uint64_t* off;
  NCG_DI const uint8_t* at(int i, uint64_t* len) const {
    const uint64_t lo = off[i];
    *len = off[i + 1] - lo;
    return msgs + lo;
  }
};
static dim3 h2c448_grid(int n) { return dim3((unsigned)(((long long)n + 63) / 64)); }

__global__ void __launch_bounds__(64) k_h2c448_xof(H2c448Msgs m, const uint8_t* __restrict__ tail, uint32_t tail_len, uint32_t out_len,
                                                    uint8_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  h2c448_xof_row(msg, len, tail, tail_len, out_len, out + (size_t)i * out_len);
}
__global__ void __launch_bounds__(64) k_h2c448_hash_to_field(H2c448Msgs m, const uint8_t* __restrict__ tail, uint32_t tail_len, int count,
                                                              uint8_t* __restrict__ uniform, uint32_t* __restrict__ out_u, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  h2c448_hash_to_field_row(msg, len, tail, tail_len, count, uniform + (size_t)i * count * H2C448_L, out_u + (size_t)i * count * 14);
}
__global__ void __launch_bounds__(64) k_h2c448_hash_to_scalar(H2c448Msgs m, const uint8_t* __restrict__ tail, uint32_t tail_len,
                                                               uint8_t* __restrict__ uniform, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  h2c448_hash_to_scalar_row(msg, len, tail, tail_len, uniform + (size_t)i * H2C448_L, out + (size_t)i * 14);
}
__global__ void __launch_bounds__(64) k_decaf448_hash_to_scalar(H2c448Msgs m, const uint8_t* __restrict__ tail, uint32_t tail_len,
                                                                 uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  decaf448_hash_to_scalar_row(msg, len, tail, tail_len, out + (size_t)i * 14);
}
__global__ void __launch_bounds__(64) k_h2c448_map(const uint32_t* __restrict__ u, int count, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  h2c448_map_row(u + (size_t)i * count * 14, count, out + (size_t)i * 28);
}
__global__ void __launch_bounds__(64) k_h2c448_check(int op, const uint32_t* __restrict__ a, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  (void)h2c448_check_op(op, a + (size_t)i * H2C448_CHECK_WORDS, out + (size_t)i * H2C448_CHECK_WORDS);
}

// ---- the workspace of a call
static size_t h2c448_al(size_t b) { return (b + 255) & ~(size_t)255; }
struct H2c448Ws {
  size_t uniform, u, total;
  H2c448Ws(size_t n, size_t uniform_row) {
    uniform = 512;  // behind the tail
    u = uniform + h2c448_al(n * uniform_row);
    total = u + h2c448_al(n * 2 * 56);
  }
};
size_t h2c448_ws_bytes(size_t n) { return H2c448Ws(n, 2 * H2C448_L).total; }

static hipError_t h2c448_put_tail(uint8_t* ws, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, hipStream_t st, uint32_t* tail_len) {
  uint8_t buf[H2C448_TAIL_MAX];
  *tail_len = xof448_tail(buf, dst, dst_len, out_len);
  return oprf_put(ws, buf, *tail_len, st);
}

hipError_t h2c448_xof_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t out_len, uint8_t* out,
                            int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint32_t tl;
  if (hipError_t e = h2c448_put_tail(ws, dst_host, dst_len, out_len, st, &tl)) return e;
  hipLaunchKernelGGL(k_h2c448_xof, h2c448_grid(n), dim3(64), 0, st, H2c448Msgs{msgs, off}, ws, tl, out_len, out, n);
  return hipGetLastError();
}
// out_u: n * count reduced elements (14 words each), or null to keep them in the workspace
hipError_t h2c448_hash_to_field(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count, uint32_t* out_u,
                                int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const H2c448Ws w((size_t)n, 2 * H2C448_L);
  uint32_t tl;
  if (hipError_t e = h2c448_put_tail(ws, dst_host, dst_len, (uint32_t)count * H2C448_L, st, &tl)) return e;
  hipLaunchKernelGGL(k_h2c448_hash_to_field, h2c448_grid(n), dim3(64), 0, st, H2c448Msgs{msgs, off}, ws, tl, count, ws + w.uniform,
                     out_u ? out_u : (uint32_t*)(ws + w.u), n);
  return hipGetLastError();
}
hipError_t h2c448_map(const uint32_t* u, int count, uint32_t* out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_h2c448_map, h2c448_grid(n), dim3(64), 0, st, u, count, out, n);
  return hipGetLastError();
}
hipError_t h2c448_hash(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count, uint32_t* out, int n,
                       uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (hipError_t e = h2c448_hash_to_field(msgs, off, dst_host, dst_len, count, nullptr, n, ws, st)) return e;
  return h2c448_map((const uint32_t*)(ws + H2c448Ws((size_t)n, 2 * H2C448_L).u), count, out, n, st);
}
hipError_t h2c448_hash_to_scalar(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                 uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const H2c448Ws w((size_t)n, 2 * H2C448_L);
  uint32_t tl;
  if (hipError_t e = h2c448_put_tail(ws, dst_host, dst_len, H2C448_L, st, &tl)) return e;
  hipLaunchKernelGGL(k_h2c448_hash_to_scalar, h2c448_grid(n), dim3(64), 0, st, H2c448Msgs{msgs, off}, ws, tl, ws + w.uniform, out, n);
  return hipGetLastError();
}
// xof(112) into the workspace (4-byte aligned rows of 28 words), then the kernel of ncg_decaf448_from_uniform_batch
hipError_t decaf448_hash_to_group(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                  uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const H2c448Ws w((size_t)n, 2 * H2C448_L);
  if (hipError_t e = h2c448_xof_batch(msgs, off, dst_host, dst_len, 112, ws + w.uniform, n, ws, st)) return e;
  return decaf448_from_uniform_batch((const uint32_t*)(ws + w.uniform), out, n, st);
}
hipError_t decaf448_hash_to_scalar(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t* out, int n,
                                   uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint32_t tl;
  if (hipError_t e = h2c448_put_tail(ws, dst_host, dst_len, 64, st, &tl)) return e;
  hipLaunchKernelGGL(k_decaf448_hash_to_scalar, h2c448_grid(n), dim3(64), 0, st, H2c448Msgs{msgs, off}, ws, tl, out, n);
  return hipGetLastError();
}
hipError_t h2c448_check(int op, const uint32_t* d_a, uint32_t* d_out, int n, hipStream_t st) {
  if (n <= 0 || op < 0 || op >= H2C448_CHECK_OPS) return hipSuccess;
  hipLaunchKernelGGL(k_h2c448_check, h2c448_grid(n), dim3(64), 0, st, op, d_a, d_out, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same row functions, one row per call
void h2c448_xof_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out) {
  uint8_t tail[H2C448_TAIL_MAX];
  const uint32_t tl = xof448_tail(tail, dst, dst_len, out_len);
  h2c448_xof_row(msg, len, tail, tl, out_len, out);
}
void h2c448_hash_to_field_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out_u) {
  uint8_t tail[H2C448_TAIL_MAX], uniform[2 * H2C448_L];
  const uint32_t tl = xof448_tail(tail, dst, dst_len, (uint32_t)count * H2C448_L);
  h2c448_hash_to_field_row(msg, len, tail, tl, count, uniform, out_u);
}
void h2c448_hash_to_scalar_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14) {
  uint8_t tail[H2C448_TAIL_MAX], uniform[H2C448_L];
  const uint32_t tl = xof448_tail(tail, dst, dst_len, H2C448_L);
  h2c448_hash_to_scalar_row(msg, len, tail, tl, uniform, out14);
}
void h2c448_map_host(const uint32_t* u, int count, uint32_t* out28) { h2c448_map_row(u, count, out28); }
void h2c448_hash_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out28) {
  uint32_t u[28];
  h2c448_hash_to_field_host(msg, len, dst, dst_len, count, u);
  h2c448_map_row(u, count, out28);
}
void decaf448_hash_to_group_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14) {
  uint8_t uniform[112];
  uint32_t w[28];
  h2c448_xof_host(msg, len, dst, dst_len, 112, uniform);
  for (int i = 0; i < 28; i++)
    w[i] = (uint32_t)uniform[4 * i] | ((uint32_t)uniform[4 * i + 1] << 8) | ((uint32_t)uniform[4 * i + 2] << 16) | ((uint32_t)uniform[4 * i + 3] << 24);
  decaf_from_uniform_row(w, out14);
}
void decaf448_hash_to_scalar_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out14) {
  uint8_t tail[H2C448_TAIL_MAX];
  const uint32_t tl = xof448_tail(tail, dst, dst_len, 64);
  decaf448_hash_to_scalar_row(msg, len, tail, tl, out14);
}
int h2c448_check_host(int op, const uint32_t* a, uint32_t* out) { return h2c448_check_op(op, a, out); }

}  // namespace ncg
