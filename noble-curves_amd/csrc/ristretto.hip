// Batch ristretto255 (the _RistrettoPoint and ristretto255_hasher of src/ed25519.ts:443-668): one element per lane, blocks of 64,
// the lane code of ristretto.hpp.  Every kernel is one or two power chains (ed_pow_p58) on values held in registers; the multiplies
// between a decode and an encode are the ed25519 kernels of ed25519.hip, unchanged.
#include "host_api.hpp"
#include "ristretto.hpp"

namespace ncg {

// waves per SIMD asked of the compiler (DESIGN.md section 8 has the register counts): four where the kernel fits 128 registers;
// the projective encoder and the map - two power chains with an extended point live between them - spill at four and run at three
constexpr int RISTRETTO_MINW = 4, RISTRETTO_MINW_WIDE = 3;

NCG_DI void ristretto_store8(uint32_t* __restrict__ out, const uint32_t (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = r[i];
}
NCG_DI void ristretto_load_affine(const uint32_t* __restrict__ p, FEd& x, FEd& y) {
  x = fe9_from_wire<Fe9EdPR>(p);
  y = fe9_from_wire<Fe9EdPR>(p + 8);
}

// One row of the decoder: 8 words in, the 16 words of the ed25519 wire point out.  A rejected row is zero, or the identity (0, 1)
// where the caller multiplies what comes out (identity_on_reject).
NCG_DI bool ristretto_decode_row(const uint32_t* __restrict__ enc, uint32_t* __restrict__ out, bool identity_on_reject) {
  uint32_t w[8], xw[8], yw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = enc[i];
  FEd x, y;
  const bool ok = ristretto_decode_lane(w, x, y);
  fe9_to_wire(xw, x);
  fe9_to_wire(yw, y);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out[i] = ok ? xw[i] : 0u;
    out[8 + i] = ok ? yw[i] : (i == 0 && identity_on_reject ? 1u : 0u);
  }
  return ok;
}
NCG_DI void ristretto_encode_row(const uint32_t* __restrict__ aff, uint32_t* __restrict__ out) {
  FEd x, y;
  ristretto_load_affine(aff, x, y);
  uint32_t r[8];
  ristretto_encode_affine(x, y, r);
  ristretto_store8(out, r);
}
NCG_DI void ristretto_encode_proj_row(const uint32_t* __restrict__ proj, uint32_t* __restrict__ out) {
  using IO = FieldIO<FEd>;
  uint32_t r[8];
  ristretto_encode_proj(IO::load(proj), IO::load(proj + IO::WORDS), IO::load(proj + 2 * IO::WORDS), r);
  ristretto_store8(out, r);
}
NCG_DI bool ristretto_equals_row(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b) {
  FEd x1, y1, x2, y2;
  ristretto_load_affine(a, x1, y1);
  ristretto_load_affine(b, x2, y2);
  return ristretto_equals(x1, y1, x2, y2);
}
// 16 words of uniform bytes in; the encoding out, and the affine representative where out_affine is not null
NCG_DI void ristretto_from_uniform_row(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ out_affine) {
  uint32_t w[16], r[8];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = in[i];
  const EdExt<FEd> p = ristretto_from_uniform(w);
  ristretto_encode_ext(p.X, p.Y, p.Z, p.T, r);
  ristretto_store8(out, r);
  if (out_affine) {
    const FEd zi = f_inv(p.Z);
    fe9_to_wire(out_affine, p.X * zi);
    fe9_to_wire(out_affine + 8, p.Y * zi);
  }
}

__global__ void __launch_bounds__(64, RISTRETTO_MINW)
k_ristretto_decode(const uint32_t* __restrict__ enc, uint32_t* __restrict__ out_affine, uint8_t* __restrict__ out_ok, int n,
                   int identity_on_reject) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out_ok[i] = ristretto_decode_row(enc + (size_t)i * 8, out_affine + (size_t)i * 16, identity_on_reject != 0) ? 1 : 0;
}

__global__ void __launch_bounds__(64, RISTRETTO_MINW)
k_ristretto_encode(const uint32_t* __restrict__ affine, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ristretto_encode_row(affine + (size_t)i * 16, out + (size_t)i * 8);
}

// (X, Y, Z) rows of ed25519_mul_base_proj: 27 stored words per item
__global__ void __launch_bounds__(64, RISTRETTO_MINW_WIDE)
k_ristretto_encode_proj(const uint32_t* __restrict__ proj, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ristretto_encode_proj_row(proj + (size_t)i * (3 * FieldIO<FEd>::WORDS), out + (size_t)i * 8);
}

__global__ void __launch_bounds__(64, RISTRETTO_MINW)
k_ristretto_equals(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint8_t* __restrict__ out_eq, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out_eq[i] = ristretto_equals_row(a + (size_t)i * 16, b + (size_t)i * 16) ? 1 : 0;
}

__global__ void __launch_bounds__(64, RISTRETTO_MINW_WIDE)
k_ristretto_from_uniform(const uint32_t* __restrict__ bytes64, uint32_t* __restrict__ out, uint32_t* __restrict__ out_affine, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ristretto_from_uniform_row(bytes64 + (size_t)i * 16, out + (size_t)i * 8, out_affine ? out_affine + (size_t)i * 16 : nullptr);
}

// one 32-byte scalar copied into every row (NCG_RISTRETTO_ONE_SCALAR): the multiply kernel reads one scalar per item
__global__ void __launch_bounds__(256) k_ristretto_broadcast(const uint32_t* __restrict__ scalar, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int j = 0; j < 8; j++) out[(size_t)i * 8 + j] = scalar[j];
}

__global__ void __launch_bounds__(64) k_field_check_ristretto(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                              uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  (void)ristretto_check_op(op, a + (size_t)i * 36, b + (size_t)i * 9, out + (size_t)i * 36);
}

hipError_t ristretto_decode_batch(const uint32_t* enc, uint32_t* out_affine, uint8_t* out_ok, int identity_on_reject, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ristretto_decode, dim3((n + 63) / 64), dim3(64), 0, st, enc, out_affine, out_ok, n, identity_on_reject);
  return hipGetLastError();
}
hipError_t ristretto_encode_batch(const uint32_t* affine, uint32_t* out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ristretto_encode, dim3((n + 63) / 64), dim3(64), 0, st, affine, out, n);
  return hipGetLastError();
}
hipError_t ristretto_encode_proj_batch(const uint32_t* proj, uint32_t* out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ristretto_encode_proj, dim3((n + 63) / 64), dim3(64), 0, st, proj, out, n);
  return hipGetLastError();
}
hipError_t ristretto_equals_batch(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ristretto_equals, dim3((n + 63) / 64), dim3(64), 0, st, a, b, out_eq, n);
  return hipGetLastError();
}
hipError_t ristretto_from_uniform_batch(const uint32_t* bytes64, uint32_t* out, uint32_t* out_affine, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ristretto_from_uniform, dim3((n + 63) / 64), dim3(64), 0, st, bytes64, out, out_affine, n);
  return hipGetLastError();
}
hipError_t ristretto_broadcast_scalar(const uint32_t* scalar, uint32_t* out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ristretto_broadcast, dim3((n + 255) / 256), dim3(256), 0, st, scalar, out, n);
  return hipGetLastError();
}
size_t ristretto_proj_words(int n) { return (size_t)n * (3 * FieldIO<FEd>::WORDS); }
hipError_t ristretto_field_check(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_field_check_ristretto, dim3((n + 63) / 64), dim3(64), 0, st, op, d_a, d_b, d_out, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same row functions, one row after the other
void ristretto_decode_host(const uint32_t* enc, uint32_t* out_affine, uint8_t* out_ok, int identity_on_reject, int n) {
  for (int i = 0; i < n; i++) out_ok[i] = ristretto_decode_row(enc + (size_t)i * 8, out_affine + (size_t)i * 16, identity_on_reject != 0) ? 1 : 0;
}
void ristretto_encode_host(const uint32_t* affine, uint32_t* out, int n) {
  for (int i = 0; i < n; i++) ristretto_encode_row(affine + (size_t)i * 16, out + (size_t)i * 8);
}
// X Y Z as canonical wire words (24 per row): loaded into the stored form the device rows have, then the same function
void ristretto_encode_proj_host(const uint32_t* proj_wire, uint32_t* out, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t st[27];
    for (int c = 0; c < 3; c++) FieldIO<FEd>::store(st + 9 * c, fe9_from_wire<Fe9EdPR>(proj_wire + (size_t)i * 24 + 8 * c));
    ristretto_encode_proj_row(st, out + (size_t)i * 8);
  }
}
void ristretto_equals_host(const uint32_t* a, const uint32_t* b, uint8_t* out_eq, int n) {
  for (int i = 0; i < n; i++) out_eq[i] = ristretto_equals_row(a + (size_t)i * 16, b + (size_t)i * 16) ? 1 : 0;
}
void ristretto_from_uniform_host(const uint32_t* bytes64, uint32_t* out, uint32_t* out_affine, int n) {
  for (int i = 0; i < n; i++)
    ristretto_from_uniform_row(bytes64 + (size_t)i * 16, out + (size_t)i * 8, out_affine ? out_affine + (size_t)i * 16 : nullptr);
}
// decode, the variable-base Edwards lane, encode: what ncg_ristretto_mul_batch runs as three launches
void ristretto_mul_host(const uint32_t* enc, const uint32_t* scalars, int one_scalar, uint32_t* out, uint8_t* out_ok, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t pt[16], prod[16];
    uint8_t inf;
    out_ok[i] = ristretto_decode_row(enc + (size_t)i * 8, pt, true) ? 1 : 0;
    ed25519_mul_var_host(pt, scalars + (one_scalar ? 0 : (size_t)i * 8), prod, &inf);
    ristretto_encode_row(prod, out + (size_t)i * 8);
  }
}
int ristretto_check_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) { return ristretto_check_op(op, a, b, out); }

}  // namespace ncg
