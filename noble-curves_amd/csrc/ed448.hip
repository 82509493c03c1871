// Batch X448 and Ed448 (src/ed448.ts of the reference): one item per lane, the lane code of ed448.hpp.  The ladder and the
// multiplications keep their whole state in registers: no table in memory, no LDS, no memory traffic between the loads of the
// inputs and the store of the result.  56-byte rows are read as 14 LE words (4-byte aligned); 57- and 114-byte rows are packed
// and read byte by byte.
#include "host_api.hpp"
#include "ed448.hpp"

namespace ncg {

NCG_DI void x448_store(uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, const uint32_t (&r)[14], bool ok) {
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = r[i];
  *out_ok = ok ? 1 : 0;
}

// x448.scalarMult per row; u = NULL: the base point u = 5 (getPublicKey)
NCG_DI void x448_row(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ u, uint32_t* __restrict__ out,
                     uint8_t* __restrict__ out_ok, int i, int one_scalar) {
  uint32_t r[14];
  const bool ok = x448_lane(scalars + (one_scalar ? 0 : (size_t)i * 14), u ? u + (size_t)i * 14 : nullptr, r);
  x448_store(out + (size_t)i * 14, out_ok + i, r, ok);
}

__global__ void __launch_bounds__(64)
k_x448(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ u, uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, int n,
       int one_scalar) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  x448_row(scalars, u, out, out_ok, i, one_scalar);
}

__global__ void __launch_bounds__(64)
k_ed448_decode(const uint8_t* __restrict__ enc, uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out_ok[i] = ed448_decode_lane(enc + (size_t)i * 57, out + (size_t)i * 28) ? 1 : 0;
}

__global__ void __launch_bounds__(64) k_ed448_encode(const uint32_t* __restrict__ affine, uint8_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed448_encode_lane(affine + (size_t)i * 28, out + (size_t)i * 57);
}

__global__ void __launch_bounds__(64)
k_ed448_add_pairs(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int subtract, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed448_add_pairs_lane(a + (size_t)i * 28, b + (size_t)i * 28, subtract, out + (size_t)i * 28);
}

// enc = NULL: the base point
__global__ void __launch_bounds__(64)
k_ed448_mul(const uint8_t* __restrict__ enc, const uint32_t* __restrict__ k, int one_scalar, uint8_t* __restrict__ out,
            uint8_t* __restrict__ out_ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* ki = k + (one_scalar ? 0 : (size_t)i * 14);
  if (enc) out_ok[i] = ed448_mul_lane(enc + (size_t)i * 57, ki, out + (size_t)i * 57) ? 1 : 0;
  else ed448_mul_base_lane(ki, out + (size_t)i * 57);
}

__global__ void __launch_bounds__(64)
k_ed448_to_montgomery(const uint8_t* __restrict__ pk, uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t r[14];
  const bool ok = ed448_to_montgomery_lane(pk + (size_t)i * 57, r);
  x448_store(out + (size_t)i * 14, out_ok + i, r, ok);
}

__global__ void __launch_bounds__(64)
k_ed448_verify(const uint8_t* __restrict__ sig, const uint8_t* __restrict__ pk, const uint32_t* __restrict__ k, uint8_t* __restrict__ out_ok,
               int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out_ok[i] = ed448_verify_lane(sig + (size_t)i * 114, pk + (size_t)i * 57, k + (size_t)i * 14) ? 1 : 0;
}

__global__ void __launch_bounds__(64)
k_fe448_check(int op, int variant, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int wa, wb, wo;
  fe448_check_widths(op, wa, wb, wo);
  (void)fe448_check_op(op, variant, a + (size_t)i * wa, b + (size_t)i * wb, out + (size_t)i * wo);
}

#define NCG_ED448_LAUNCH(kernel, n, st, ...)                                                  \
  do {                                                                                        \
    if ((n) <= 0) return hipSuccess;                                                          \
    hipLaunchKernelGGL(kernel, dim3(((unsigned)(n) + 63u) / 64u), dim3(64), 0, st, __VA_ARGS__);          \
    return hipGetLastError();                                                                 \
  } while (0)

hipError_t x448_batch(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_x448, n, st, scalars, u, out, out_ok, n, one_scalar);
}
hipError_t ed448_decode_batch(const uint8_t* enc, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_ed448_decode, n, st, enc, out, out_ok, n);
}
hipError_t ed448_encode_batch(const uint32_t* affine, uint8_t* out, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_ed448_encode, n, st, affine, out, n);
}
hipError_t ed448_add_pairs_batch(const uint32_t* a, const uint32_t* b, int subtract, uint32_t* out, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_ed448_add_pairs, n, st, a, b, subtract, out, n);
}
hipError_t ed448_mul_batch(const uint8_t* enc, const uint32_t* k, int one_scalar, uint8_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_ed448_mul, n, st, enc, k, one_scalar, out, out_ok, n);
}
hipError_t ed448_to_montgomery_batch(const uint8_t* pk, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_ed448_to_montgomery, n, st, pk, out, out_ok, n);
}
hipError_t ed448_verify_batch(const uint8_t* sig, const uint8_t* pk, const uint32_t* k, uint8_t* out_ok, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_ed448_verify, n, st, sig, pk, k, out_ok, n);
}
void fe448_check_row_words(int op, int* wa, int* wb, int* wo) { fe448_check_widths(op, *wa, *wb, *wo); }
hipError_t fe448_check(int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st) {
  NCG_ED448_LAUNCH(k_fe448_check, n, st, op, variant, d_a, d_b, d_out, n);
}

// ---- the CPU twins: the same lane functions, one row after the other
void x448_host(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) x448_row(scalars, u, out, out_ok, i, one_scalar);
}
void ed448_decode_host(const uint8_t* enc, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) out_ok[i] = ed448_decode_lane(enc + (size_t)i * 57, out + (size_t)i * 28) ? 1 : 0;
}
void ed448_encode_host(const uint32_t* affine, uint8_t* out, int n) {
  for (int i = 0; i < n; i++) ed448_encode_lane(affine + (size_t)i * 28, out + (size_t)i * 57);
}
void ed448_add_pairs_host(const uint32_t* a, const uint32_t* b, int subtract, uint32_t* out, int n) {
  for (int i = 0; i < n; i++) ed448_add_pairs_lane(a + (size_t)i * 28, b + (size_t)i * 28, subtract, out + (size_t)i * 28);
}
void ed448_mul_host(const uint8_t* enc, const uint32_t* k, int one_scalar, uint8_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) {
    const uint32_t* ki = k + (one_scalar ? 0 : (size_t)i * 14);
    if (enc) out_ok[i] = ed448_mul_lane(enc + (size_t)i * 57, ki, out + (size_t)i * 57) ? 1 : 0;
    else ed448_mul_base_lane(ki, out + (size_t)i * 57);
  }
}
void ed448_to_montgomery_host(const uint8_t* pk, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t r[14];
    const bool ok = ed448_to_montgomery_lane(pk + (size_t)i * 57, r);
    x448_store(out + (size_t)i * 14, out_ok + i, r, ok);
  }
}
void ed448_verify_host(const uint8_t* sig, const uint8_t* pk, const uint32_t* k, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) out_ok[i] = ed448_verify_lane(sig + (size_t)i * 114, pk + (size_t)i * 57, k + (size_t)i * 14) ? 1 : 0;
}
int fe448_check_host(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out) { return fe448_check_op(op, variant, a, b, out); }

}  // namespace ncg
