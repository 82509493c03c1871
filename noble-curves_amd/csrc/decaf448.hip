// Batch decaf448 (RFC 9496 section 5; _DecafPoint and decaf448_hasher of the reference's src/ed448.ts): one element per lane, the
// lane code of decaf448.hpp on the field and the group law of ed448.hpp.  Everything between the loads of the inputs and the store
// of the result stays in registers.  Every row is made of 56-byte values read as 14 LE words (4-byte aligned): encodings and
// scalars 14 words, affine representatives x || y and uniform bytes 28.
#include "host_api.hpp"
#include "decaf448.hpp"

namespace ncg {

__global__ void __launch_bounds__(64)
k_decaf448_decode(const uint32_t* __restrict__ enc, uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out_ok[i] = decaf_decode_row(enc + (size_t)i * 14, out + (size_t)i * 28) ? 1 : 0;
}

__global__ void __launch_bounds__(64) k_decaf448_encode(const uint32_t* __restrict__ affine, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  decaf_encode_row(affine + (size_t)i * 28, out + (size_t)i * 14);
}

__global__ void __launch_bounds__(64)
k_decaf448_equals(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint8_t* __restrict__ out_eq, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out_eq[i] = decaf_equals_row(a + (size_t)i * 28, b + (size_t)i * 28) ? 1 : 0;
}

__global__ void __launch_bounds__(64) k_decaf448_from_uniform(const uint32_t* __restrict__ uniform, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  decaf_from_uniform_row(uniform + (size_t)i * 28, out + (size_t)i * 14);
}

// enc = NULL: the decaf base point (out_ok is not written then)
__global__ void __launch_bounds__(64)
k_decaf448_mul(const uint32_t* __restrict__ enc, const uint32_t* __restrict__ k, int one_scalar, uint32_t* __restrict__ out,
               uint8_t* __restrict__ out_ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* ki = k + (one_scalar ? 0 : (size_t)i * 14);
  const bool ok = decaf_mul_row(enc ? enc + (size_t)i * 14 : nullptr, ki, out + (size_t)i * 14);
  if (enc) out_ok[i] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(64)
k_decaf448_check(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int wa, wb, wo;
  decaf448_check_widths(op, wa, wb, wo);
  (void)decaf448_check_op(op, a + (size_t)i * wa, b + (size_t)i * wb, out + (size_t)i * wo);
}

#define NCG_DECAF448_LAUNCH(kernel, n, st, ...)                                               \
  do {                                                                                        \
    if ((n) <= 0) return hipSuccess;                                                          \
    hipLaunchKernelGGL(kernel, dim3(((unsigned)(n) + 63u) / 64u), dim3(64), 0, st, __VA_ARGS__);          \
    return hipGetLastError();                                                                 \
  } while (0)

hipError_t decaf448_decode_batch(const uint32_t* enc, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  NCG_DECAF448_LAUNCH(k_decaf448_decode, n, st, enc, out, out_ok, n);
}
hipError_t decaf448_encode_batch(const uint32_t* affine, uint32_t* out, int n, hipStream_t st) {
  NCG_DECAF448_LAUNCH(k_decaf448_encode, n, st, affine, out, n);
}
hipError_t decaf448_equals_batch(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n, hipStream_t st) {
  NCG_DECAF448_LAUNCH(k_decaf448_equals, n, st, a, b, out_eq, n);
}
hipError_t decaf448_from_uniform_batch(const uint32_t* uniform, uint32_t* out, int n, hipStream_t st) {
  NCG_DECAF448_LAUNCH(k_decaf448_from_uniform, n, st, uniform, out, n);
}
hipError_t decaf448_mul_batch(const uint32_t* enc, const uint32_t* k, int one_scalar, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  NCG_DECAF448_LAUNCH(k_decaf448_mul, n, st, enc, k, one_scalar, out, out_ok, n);
}
void decaf448_check_row_words(int op, int* wa, int* wb, int* wo) { decaf448_check_widths(op, *wa, *wb, *wo); }
hipError_t decaf448_check(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st) {
  NCG_DECAF448_LAUNCH(k_decaf448_check, n, st, op, d_a, d_b, d_out, n);
}

// ---- the CPU twins: the same lane functions, one row after the other
void decaf448_decode_host(const uint32_t* enc, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) out_ok[i] = decaf_decode_row(enc + (size_t)i * 14, out + (size_t)i * 28) ? 1 : 0;
}
void decaf448_encode_host(const uint32_t* affine, uint32_t* out, int n) {
  for (int i = 0; i < n; i++) decaf_encode_row(affine + (size_t)i * 28, out + (size_t)i * 14);
}
void decaf448_equals_host(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n) {
  for (int i = 0; i < n; i++) out_eq[i] = decaf_equals_row(a + (size_t)i * 28, b + (size_t)i * 28) ? 1 : 0;
}
void decaf448_from_uniform_host(const uint32_t* uniform, uint32_t* out, int n) {
  for (int i = 0; i < n; i++) decaf_from_uniform_row(uniform + (size_t)i * 28, out + (size_t)i * 14);
}
void decaf448_mul_host(const uint32_t* enc, const uint32_t* k, int one_scalar, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) {
    const uint32_t* ki = k + (one_scalar ? 0 : (size_t)i * 14);
    const bool ok = decaf_mul_row(enc ? enc + (size_t)i * 14 : nullptr, ki, out + (size_t)i * 14);
    if (enc) out_ok[i] = ok ? 1 : 0;
  }
}
int decaf448_check_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) { return decaf448_check_op(op, a, b, out); }

}  // namespace ncg
