// Batch RFC 9380 hash-to-curve for secp256k1 (secp256k1_XMD:SHA-256_SSWU_) and edwards25519 (edwards25519_XMD:SHA-512_ELL2_): the lane
// code of h2c_suites.hpp, one item per lane, split so that the hash, the map and the sum do not hold each other's registers:
//   k_h2c_hash_to_field   xmd -> count elements mod p (blocks of 256, like the other kernels that only hash)
//   k_h2c_hash_to_scalar  xmd -> one element mod n / mod L
//   k_h2c_xmd_sha256      expand_message_xmd over SHA-256 alone
//   k_h2c_map_secp        one lane per FIELD ELEMENT (2 n lanes for hashToCurve): SWU + 3-isogeny -> Jacobian point of E
//   k_h2c_map_ed          one lane per field element: Elligator 2 + the map to Edwards form -> extended point
//   k_h2c_sum_secp        Q0 + Q1 (Jacobian)                 then k_jac_batch_affine (mulvar.hpp): one inversion per 8 rows
//   k_h2c_sum_ed          8 (Q0 [+ Q1]) -> (X, Y, Z)          then ed25519_proj_to_affine (ed25519.hip), likewise
// Hand-offs in the workspace: DST' | the uniform bytes | the reduced elements (8 words) | the mapped points (27 / 36 stored words per
// element) | the summed points (27 stored words per row).  With count = 1 the secp256k1 map writes the summed slot itself.
#include "h2c_suites.hpp"
#include "host_api.hpp"
#include "mulvar.hpp"

namespace ncg {

struct H2cMsgs {
  const uint8_t* msgs;
  const uint64_t* off;
  NCG_DI const uint8_t* at(int i, uint64_t* len) const {
    const uint64_t lo = off[i];
    *len = off[i + 1] - lo;
    return msgs + lo;
  }
};
// blocks of b lanes for `total` lanes (up to 2 (2^31 - 256): the count is taken in 64 bits)
static dim3 h2c_grid(size_t total, int b) { return dim3((unsigned)((total + b - 1) / b)); }

template <int SUITE>
__global__ void __launch_bounds__(256) k_h2c_hash_to_field(H2cMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len, int count,
                                                            uint8_t* __restrict__ uniform, uint32_t* __restrict__ out_u, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  h2c_hash_to_field_row<SUITE>(msg, len, dstp, dstp_len, count, uniform + (size_t)i * count * 48, out_u + (size_t)i * count * 8);
}
template <int SUITE>
__global__ void __launch_bounds__(256) k_h2c_hash_to_scalar(H2cMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                                             uint8_t* __restrict__ uniform, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  h2c_hash_to_scalar_row<SUITE>(msg, len, dstp, dstp_len, uniform + (size_t)i * 48, out + (size_t)i * 8);
}
__global__ void __launch_bounds__(256) k_h2c_xmd_sha256(H2cMsgs m, const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t out_len,
                                                         uint8_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  xmd_sha256_lane(msg, len, dstp, dstp_len, out_len, out + (size_t)i * out_len);
}
// The maps are one power chain each with a few dozen products around it: the values live across the chain are the ones the
// tail needs (u, tv1, tv3, tv4, gx on secp256k1; u, tv1, xd, gxd, gx1, tv3 on edwards25519), nine limbs each
__global__ void __launch_bounds__(64, 3) k_h2c_map_secp(const uint32_t* __restrict__ u, int in_words, uint32_t* __restrict__ stage, size_t total) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= total) return;
  secp_map_row(u + t * in_words, in_words, stage + t * SECP_JAC_WORDS);
}
__global__ void __launch_bounds__(64) k_h2c_map_ed(const uint32_t* __restrict__ u, int in_words, uint32_t* __restrict__ stage, size_t total) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= total) return;
  ed_map_row(u + t * in_words, in_words, stage + t * ED_EXT_WORDS);
}
__global__ void __launch_bounds__(64) k_h2c_sum_secp(const uint32_t* __restrict__ stage, int count, uint32_t* __restrict__ jac, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  secp_sum_row(stage + (size_t)i * count * SECP_JAC_WORDS, count, jac + (size_t)i * SECP_JAC_WORDS);
}
__global__ void __launch_bounds__(64) k_h2c_sum_ed(const uint32_t* __restrict__ stage, int count, uint32_t* __restrict__ proj, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed_sum_row(stage + (size_t)i * count * ED_EXT_WORDS, count, proj + (size_t)i * 27);
}
__global__ void __launch_bounds__(64) k_h2c_check(int op, const uint32_t* __restrict__ a, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  (void)h2c_check_op(op, a + (size_t)i * H2C_CHECK_WORDS, out + (size_t)i * H2C_CHECK_WORDS);
}

// ---- the workspace of a call
static size_t h2c_al(size_t b) { return (b + 255) & ~(size_t)255; }
struct H2cWs {
  size_t uniform, u, stage, fin, total;
  H2cWs(int suite, size_t n, int count) {
    const size_t sw = suite == H2C_SECP256K1_XMD_SHA256_SSWU ? SECP_JAC_WORDS : ED_EXT_WORDS;
    uniform = 256;                                   // behind DST'
    u = uniform + h2c_al(n * count * 48);
    stage = u + h2c_al(n * count * 32);
    fin = stage + h2c_al(n * count * sw * 4);
    total = fin + h2c_al(n * 27 * 4);
  }
};
size_t h2c_suites_ws_bytes(int suite, size_t n, int count) { return H2cWs(suite, n, count).total; }

static hipError_t h2c_put_dst(uint8_t* ws, const uint8_t* dst, uint32_t dst_len, hipStream_t st) {  // DST' = DST || len
  uint8_t buf[256];
  for (uint32_t i = 0; i < dst_len; i++) buf[i] = dst[i];
  buf[dst_len] = (uint8_t)dst_len;
  return oprf_put(ws, buf, dst_len + 1, st);
}

// u: n * count elements of in_words words (device) -> affine wire points and flags
hipError_t h2c_suites_map(int suite, const uint32_t* u, int in_words, int count, uint32_t* out, uint8_t* inf, int n, uint8_t* ws,
                          hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const H2cWs w(suite, (size_t)n, count);
  const size_t total = (size_t)n * count;
  uint32_t* stage = (uint32_t*)(ws + w.stage);
  uint32_t* fin = (uint32_t*)(ws + w.fin);
  if (suite == H2C_SECP256K1_XMD_SHA256_SSWU) {
    hipLaunchKernelGGL(k_h2c_map_secp, h2c_grid(total, 64), dim3(64), 0, st, u, in_words, count == 1 ? fin : stage, total);
    if (count == 2) hipLaunchKernelGGL(k_h2c_sum_secp, h2c_grid((size_t)n, 64), dim3(64), 0, st, stage, count, fin, n);
    hipLaunchKernelGGL((k_jac_batch_affine<CurveSecp, 8>), dim3(((n + 7) / 8 + 255) / 256), dim3(256), 0, st, fin, out, inf, n);
    return hipGetLastError();
  }
  if (suite == H2C_EDWARDS25519_XMD_SHA512_ELL2) {
    hipLaunchKernelGGL(k_h2c_map_ed, h2c_grid(total, 64), dim3(64), 0, st, u, in_words, stage, total);
    hipLaunchKernelGGL(k_h2c_sum_ed, h2c_grid((size_t)n, 64), dim3(64), 0, st, stage, count, fin, n);
    if (hipError_t e = hipGetLastError()) return e;
    return ed25519_proj_to_affine(fin, out, inf, n, st);
  }
  return hipErrorInvalidValue;
}
// out_u: n * count reduced elements (8 words each), or null to keep them in the workspace
hipError_t h2c_suites_hash_to_field(int suite, const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count,
                                    uint32_t* out_u, int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const H2cWs w(suite, (size_t)n, count);
  if (hipError_t e = h2c_put_dst(ws, dst_host, dst_len, st)) return e;
  uint32_t* u = out_u ? out_u : (uint32_t*)(ws + w.u);
  if (suite == H2C_SECP256K1_XMD_SHA256_SSWU)
    hipLaunchKernelGGL(k_h2c_hash_to_field<H2C_SECP256K1_XMD_SHA256_SSWU>, h2c_grid((size_t)n, 256), dim3(256), 0, st, H2cMsgs{msgs, off}, ws,
                       dst_len + 1, count, ws + w.uniform, u, n);
  else if (suite == H2C_EDWARDS25519_XMD_SHA512_ELL2)
    hipLaunchKernelGGL(k_h2c_hash_to_field<H2C_EDWARDS25519_XMD_SHA512_ELL2>, h2c_grid((size_t)n, 256), dim3(256), 0, st, H2cMsgs{msgs, off}, ws,
                       dst_len + 1, count, ws + w.uniform, u, n);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t h2c_suites_hash(int suite, const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, int count,
                           uint32_t* out, uint8_t* inf, int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (hipError_t e = h2c_suites_hash_to_field(suite, msgs, off, dst_host, dst_len, count, nullptr, n, ws, st)) return e;
  return h2c_suites_map(suite, (const uint32_t*)(ws + H2cWs(suite, (size_t)n, count).u), 8, count, out, inf, n, ws, st);
}
hipError_t h2c_suites_hash_to_scalar(int suite, const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len,
                                     uint32_t* out, int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const H2cWs w(suite, (size_t)n, 1);
  if (hipError_t e = h2c_put_dst(ws, dst_host, dst_len, st)) return e;
  if (suite == H2C_SECP256K1_XMD_SHA256_SSWU)
    hipLaunchKernelGGL(k_h2c_hash_to_scalar<H2C_SECP256K1_XMD_SHA256_SSWU>, h2c_grid((size_t)n, 256), dim3(256), 0, st, H2cMsgs{msgs, off}, ws,
                       dst_len + 1, ws + w.uniform, out, n);
  else if (suite == H2C_EDWARDS25519_XMD_SHA512_ELL2)
    hipLaunchKernelGGL(k_h2c_hash_to_scalar<H2C_EDWARDS25519_XMD_SHA512_ELL2>, h2c_grid((size_t)n, 256), dim3(256), 0, st, H2cMsgs{msgs, off}, ws,
                       dst_len + 1, ws + w.uniform, out, n);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
// ws: 256 bytes (DST')
hipError_t h2c_xmd_sha256_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* dst_host, uint32_t dst_len, uint32_t out_len,
                                uint8_t* out, int n, uint8_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (hipError_t e = h2c_put_dst(ws, dst_host, dst_len, st)) return e;
  hipLaunchKernelGGL(k_h2c_xmd_sha256, h2c_grid((size_t)n, 256), dim3(256), 0, st, H2cMsgs{msgs, off}, ws, dst_len + 1, out_len, out, n);
  return hipGetLastError();
}
hipError_t h2c_check(int op, const uint32_t* d_a, uint32_t* d_out, int n, hipStream_t st) {
  if (n <= 0 || op < 0 || op >= H2C_CHECK_OPS) return hipSuccess;
  hipLaunchKernelGGL(k_h2c_check, h2c_grid((size_t)n, 64), dim3(64), 0, st, op, d_a, d_out, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same row functions, one row after the other; the affine conversion is one inversion per row here
static uint32_t h2c_dstp_host(const uint8_t* dst, uint32_t dst_len, uint8_t (&buf)[256]) {
  for (uint32_t i = 0; i < dst_len; i++) buf[i] = dst[i];
  buf[dst_len] = (uint8_t)dst_len;
  return dst_len + 1;
}
void h2c_xmd_sha256_host(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t out_len, uint8_t* out) {
  uint8_t dp[256];
  const uint32_t dl = h2c_dstp_host(dst, dst_len, dp);
  xmd_sha256_lane(msg, len, dp, dl, out_len, out);
}
int h2c_hash_to_field_host(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out_u) {
  uint8_t dp[256], uniform[96];
  const uint32_t dl = h2c_dstp_host(dst, dst_len, dp);
  if (suite == H2C_SECP256K1_XMD_SHA256_SSWU) h2c_hash_to_field_row<H2C_SECP256K1_XMD_SHA256_SSWU>(msg, len, dp, dl, count, uniform, out_u);
  else if (suite == H2C_EDWARDS25519_XMD_SHA512_ELL2) h2c_hash_to_field_row<H2C_EDWARDS25519_XMD_SHA512_ELL2>(msg, len, dp, dl, count, uniform, out_u);
  else return -1;
  return 0;
}
int h2c_hash_to_scalar_host(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, uint32_t* out8) {
  uint8_t dp[256], uniform[48];
  const uint32_t dl = h2c_dstp_host(dst, dst_len, dp);
  if (suite == H2C_SECP256K1_XMD_SHA256_SSWU) h2c_hash_to_scalar_row<H2C_SECP256K1_XMD_SHA256_SSWU>(msg, len, dp, dl, uniform, out8);
  else if (suite == H2C_EDWARDS25519_XMD_SHA512_ELL2) h2c_hash_to_scalar_row<H2C_EDWARDS25519_XMD_SHA512_ELL2>(msg, len, dp, dl, uniform, out8);
  else return -1;
  return 0;
}
// u: count elements of in_words words -> one affine wire point (16 words) and its flag
int h2c_map_host(int suite, const uint32_t* u, int in_words, int count, uint32_t* out, uint8_t* inf) {
  uint32_t fin[27];
  if (suite == H2C_SECP256K1_XMD_SHA256_SSWU) {
    uint32_t stage[2 * SECP_JAC_WORDS];
    for (int j = 0; j < count; j++) secp_map_row(u + j * in_words, in_words, stage + j * SECP_JAC_WORDS);
    secp_sum_row(stage, count, fin);
    const Jac<FeSecp> R = secp_load_jac(fin);
    const Affine<FeSecp> a = jac_to_affine(R, f_inv(R.Z));
    store_affine_wire<FeSecp>(out, a);
    *inf = R.is_inf() ? 1 : 0;
    return 0;
  }
  if (suite == H2C_EDWARDS25519_XMD_SHA512_ELL2) {
    uint32_t stage[2 * ED_EXT_WORDS];
    for (int j = 0; j < count; j++) ed_map_row(u + j * in_words, in_words, stage + j * ED_EXT_WORDS);
    ed_sum_row(stage, count, fin);
    const FEd zi = f_inv(FieldIO<FEd>::load(fin + 18));
    const FEd x = FieldIO<FEd>::load(fin) * zi, y = FieldIO<FEd>::load(fin + 9) * zi;
    fe9_to_wire(out, x);
    fe9_to_wire(out + 8, y);
    *inf = (f_eqz(x) && f_eq(y, FEd::one())) ? 1 : 0;
    return 0;
  }
  return -1;
}
int h2c_hash_host(int suite, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint32_t dst_len, int count, uint32_t* out, uint8_t* inf) {
  uint32_t u[16];
  if (h2c_hash_to_field_host(suite, msg, len, dst, dst_len, count, u)) return -1;
  return h2c_map_host(suite, u, 8, count, out, inf);
}
int h2c_check_host(int op, const uint32_t* a, uint32_t* out) { return h2c_check_op(op, a, out); }

}  // namespace ncg
