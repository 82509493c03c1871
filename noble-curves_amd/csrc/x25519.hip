// Batch X25519 (x25519.scalarMult / getSharedSecret / getPublicKey of src/ed25519.ts:266-292) and ed25519.utils.toMontgomery:
// one item per lane, the lane code of x25519.hpp.  The ladder keeps its whole state in registers (five field elements and the
// temporaries of one step): no table, no LDS, no memory traffic between the loads of the two inputs and the store of the result.
#include "host_api.hpp"
#include "x25519.hpp"

namespace ncg {

constexpr int X25519_MINW = 4;  // waves per SIMD asked of the compiler (DESIGN.md section 8 has the register count)

NCG_DI void x25519_store(uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, const uint32_t (&r)[8], bool ok) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = r[i];
  *out_ok = ok ? 1 : 0;
}

// scalars: 8 words per row, or 8 words in all (one_scalar); u, out: 8 words per row
__global__ void __launch_bounds__(64, X25519_MINW)
k_x25519(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ u, uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok,
         int n, int one_scalar) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t r[8];
  const bool ok = x25519_lane(scalars + (one_scalar ? 0 : (size_t)i * 8), u + (size_t)i * 8, r);
  x25519_store(out + (size_t)i * 8, out_ok + i, r, ok);
}

// getPublicKey through the fixed-base Edwards table: the clamped scalars for k_ed_mul_base ...
__global__ void __launch_bounds__(256) k_x25519_clamp(const uint32_t* __restrict__ scalars, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8];
#pragma unroll
  for (int j = 0; j < 8; j++) k[j] = scalars[(size_t)i * 8 + j];
  x25519_decode_scalar(k);
#pragma unroll
  for (int j = 0; j < 8; j++) out[(size_t)i * 8 + j] = k[j];
}
// ... and u = (Z + Y) / (Z - Y) of its projective results (27 stored words X, Y, Z per item)
__global__ void __launch_bounds__(64, X25519_MINW)
k_x25519_from_proj(const uint32_t* __restrict__ proj, uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, int n) {
  using IO = FieldIO<FEd>;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* p = proj + (size_t)i * (3 * IO::WORDS);
  uint32_t r[8];
  bool ok = x25519_edwards_to_u(IO::load(p + IO::WORDS), IO::load(p + 2 * IO::WORDS), r);
  ok = ok && !x25519_words_small(r, 0u);  // montgomery.ts:340
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = ok ? r[j] : 0u;
  x25519_store(out + (size_t)i * 8, out_ok + i, r, ok);
}

__global__ void __launch_bounds__(64, X25519_MINW)
k_ed25519_to_montgomery(const uint32_t* __restrict__ pk, uint32_t* __restrict__ out, uint8_t* __restrict__ out_ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t r[8];
  const bool ok = ed25519_to_montgomery_lane(pk + (size_t)i * 8, r);
  x25519_store(out + (size_t)i * 8, out_ok + i, r, ok);
}

__global__ void __launch_bounds__(64) k_field_check_x25519(int op, int variant, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                           uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  (void)x25519_check_op(op, variant, a + (size_t)i * 36, b + (size_t)i * 9, out + (size_t)i * 36);
}

hipError_t x25519_batch(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_x25519, dim3((n + 63) / 64), dim3(64), 0, st, scalars, u, out, out_ok, n, one_scalar);
  return hipGetLastError();
}

size_t x25519_base_tmp_words(int n) { return (size_t)n * (3 * FieldIO<FEd>::WORDS + 8); }
hipError_t x25519_base_batch(const uint32_t* table, const uint32_t* scalars, uint32_t* out, uint8_t* out_ok, int n, uint32_t* tmp,
                             hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint32_t* proj = tmp;
  uint32_t* clamped = tmp + (size_t)n * (3 * FieldIO<FEd>::WORDS);
  hipLaunchKernelGGL(k_x25519_clamp, dim3((n + 255) / 256), dim3(256), 0, st, scalars, clamped, n);
  if (hipError_t e = ed25519_mul_base_proj(table, clamped, proj, n, st)) return e;
  hipLaunchKernelGGL(k_x25519_from_proj, dim3((n + 63) / 64), dim3(64), 0, st, proj, out, out_ok, n);
  return hipGetLastError();
}

hipError_t ed25519_to_montgomery_batch(const uint32_t* pk, uint32_t* out, uint8_t* out_ok, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ed25519_to_montgomery, dim3((n + 63) / 64), dim3(64), 0, st, pk, out, out_ok, n);
  return hipGetLastError();
}

hipError_t x25519_field_check(int op, int variant, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_field_check_x25519, dim3((n + 63) / 64), dim3(64), 0, st, op, variant, d_a, d_b, d_out, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same lane functions, one row after the other
void x25519_host(const uint32_t* scalars, const uint32_t* u, int one_scalar, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t r[8];
    const bool ok = x25519_lane(scalars + (one_scalar ? 0 : (size_t)i * 8), u + (size_t)i * 8, r);
    x25519_store(out + (size_t)i * 8, out_ok + i, r, ok);
  }
}
// [k]B by the variable-base Edwards lane (the device walks the fixed-base table: the same point), then the same map
void x25519_base_host(const uint32_t* scalars, uint32_t* out, uint8_t* out_ok, int n) {
  // src/ed25519.ts:57-65 Gx, Gy
  static const uint32_t G[16] = {0x8f25d51au, 0xc9562d60u, 0x9525a7b2u, 0x692cc760u, 0xfdd6dc5cu, 0xc0a4e231u, 0xcd6e53feu, 0x216936d3u,
                                 0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
  for (int i = 0; i < n; i++) {
    uint32_t k[8], pt[16], r[8];
    uint8_t inf;
    for (int j = 0; j < 8; j++) k[j] = scalars[(size_t)i * 8 + j];
    x25519_decode_scalar(k);
    ed25519_mul_var_host(G, k, pt, &inf);
    bool ok = x25519_edwards_to_u(FieldWire<FEd>::load(pt + 8), FEd::one(), r);
    ok = ok && !x25519_words_small(r, 0u);
    for (int j = 0; j < 8; j++) r[j] = ok ? r[j] : 0u;
    x25519_store(out + (size_t)i * 8, out_ok + i, r, ok);
  }
}
void ed25519_to_montgomery_host(const uint32_t* pk, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t r[8];
    const bool ok = ed25519_to_montgomery_lane(pk + (size_t)i * 8, r);
    x25519_store(out + (size_t)i * 8, out_ok + i, r, ok);
  }
}
int x25519_check_host(int op, int variant, const uint32_t* a, const uint32_t* b, uint32_t* out) { return x25519_check_op(op, variant, a, b, out); }

}  // namespace ncg
