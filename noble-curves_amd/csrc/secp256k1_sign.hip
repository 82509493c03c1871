// Batch secp256k1 signing (secp256k1_sign.hpp has the lane code and what it computes): secp256k1.getPublicKey / sign (ECDSA with
// RFC 6979 nonces) and schnorr.getPublicKey / sign (BIP-340).  Small kernels, one row per lane, as in ed25519_sign.hip: the hash
// kernels are 32-bit integer code (256-lane blocks; the DRBG works on words, the BIP-340 hashes read their message byte by byte), the
// multiply is the secp256k1 field code plus one inversion (64-lane blocks, so that a wave reads one table row together).
//   k_sha256_msgs (ecdsa.hip)   hash32 = SHA-256(M), the message-taking ECDSA form only
//   k_ecdsa_sign_seed           key and hash -> d, h1, the DRBG's seed and its first candidate k
//   k_secp_sign_mul             x, y of (nonce) G for the nonce in the row
//   k_ecdsa_sign_finish         r, s, recovery id; a refused candidate (about 2^-128 of real inputs) takes the next ones here
//   k_secp_public_key           keys -> 33-, 65- or 32-byte public keys
//   k_secp_key_points           keys -> x, y of d' G (BIP-340 signing needs the parity of y)
//   k_schnorr_sign_nonce        d, t, k' = hash/nonce(t || px || M) mod n
//   k_schnorr_sign_finish       e = hash/challenge(x(R) || px || M) mod n, s = (k + e d) mod n
#include <vector>

#include "host_api.hpp"
#include "secp256k1_sign.hpp"

namespace ncg {

// key_stride / extra_stride in bytes: 32, or 0 when one row serves every message (extra: null when there is none)
__global__ void __launch_bounds__(256) k_ecdsa_sign_seed(uint32_t* __restrict__ ws, const uint8_t* __restrict__ sk,
                                                         int key_stride, const uint8_t* __restrict__ hash, const uint8_t* __restrict__ extra, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ecdsa_sign_seed_lane(ws + (size_t)i * SS_ROW, sk + (size_t)i * key_stride, hash + (size_t)i * 32, extra ? extra + (size_t)i * 32 : nullptr);
}
__global__ void __launch_bounds__(64) k_secp_sign_mul(const uint32_t* __restrict__ table, uint32_t* __restrict__ ws, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  secp_sign_mul_lane(table, ws + (size_t)i * SS_ROW);
}
__global__ void __launch_bounds__(64) k_ecdsa_sign_finish(const uint32_t* __restrict__ table, uint32_t* __restrict__ ws, uint32_t seed_len, uint32_t low_s,
                                                          uint8_t* __restrict__ sig, uint8_t* __restrict__ recid, uint8_t* __restrict__ ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ecdsa_sign_finish_lane(table, ws + (size_t)i * SS_ROW, seed_len, low_s, 0, sig + (size_t)i * 64, recid ? recid + i : nullptr, ok + i);
}
__global__ void __launch_bounds__(64) k_secp_public_key(const uint32_t* __restrict__ table, const uint8_t* __restrict__ sk, int mode,
                                                        uint8_t* __restrict__ out, uint8_t* __restrict__ ok, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  secp_public_key_lane(table, sk + (size_t)i * 32, mode, out + (size_t)i * secp_pk_bytes(mode), ok + i);
}
__global__ void __launch_bounds__(64) k_secp_key_points(const uint32_t* __restrict__ table, const uint8_t* __restrict__ sk, uint32_t* __restrict__ pts,
                                                        int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t d[8], x[8], y[8];
  be32_to_words(d, sk + (size_t)i * 32);
  secp_mul_base_scan(table, d, x, y);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    pts[(size_t)i * 16 + j] = x[j];
    pts[(size_t)i * 16 + 8 + j] = y[j];
  }
}
__global__ void __launch_bounds__(256) k_schnorr_sign_nonce(const uint32_t* __restrict__ table, uint32_t* __restrict__ ws, const uint8_t* __restrict__ sk,
                                                            const uint32_t* __restrict__ pts, int key_stride, const uint8_t* __restrict__ aux,
                                                            const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t lo = off[i];
  schnorr_sign_nonce_lane(table, ws + (size_t)i * SS_ROW, sk + (size_t)i * key_stride, pts + (size_t)i * (key_stride / 2), aux + (size_t)i * 32,
                          msgs + lo, off[i + 1] - lo);
}
__global__ void __launch_bounds__(256) k_schnorr_sign_finish(const uint32_t* __restrict__ table, uint32_t* __restrict__ ws, const uint8_t* __restrict__ msgs,
                                                             const uint64_t* __restrict__ off, uint8_t* __restrict__ sig, uint8_t* __restrict__ ok, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t lo = off[i];
  schnorr_sign_finish_lane(table, ws + (size_t)i * SS_ROW, msgs + lo, off[i + 1] - lo, sig + (size_t)i * 64, ok + i);
}
__global__ void __launch_bounds__(64) k_secp_sign_check(int op, int variant, const uint32_t* __restrict__ table, uint32_t* __restrict__ ws,
                                                        const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int wa, wb, wo;
  secp_sign_check_widths(op, wa, wb, wo);
  (void)secp_sign_check_op(op, variant, table, ws + (size_t)i * SS_ROW, a + (size_t)i * wa, b + (size_t)i * wb, out + (size_t)i * wo);
}

// ---- the table: (2 j + 1) 2^(4 w) G for j < 8, w < 64 as affine points in canonical 29-bit limbs, then the three tag hashes
size_t secp_scan_table_words() { return SECP_SCAN_TABLE_WORDS; }
void secp_build_scan_table(uint32_t* out) {
  using F = FeSecp;
  const int NT = SECP_SCAN_M * SECP_SCAN_T;
  std::vector<Jac<F>> pts(NT);
  Jac<F> bw = jac_from_affine(load_affine_wire<F>(BasePoints::SECP));
  for (int w = 0; w < SECP_SCAN_M; w++) {
    const Jac<F> two = jac_dbl(bw);
    Jac<F> cur = bw;
    for (int j = 0; j < SECP_SCAN_T; j++) {
      if (j > 0) cur = jac_add(cur, two);
      pts[(size_t)w * SECP_SCAN_T + j] = cur;
    }
    for (int d = 0; d < SECP_SCAN_W; d++) bw = jac_dbl(bw);
  }
  for (int t = 0; t < NT; t++) {
    const Affine<F> a = jac_to_affine(pts[t], f_inv(pts[t].Z));
    uint32_t limbs[9];
    fe9_canon_limbs<Fe9SecpPR, 2>(limbs, a.x);
    for (int i = 0; i < 9; i++) out[(size_t)t * SECP_SCAN_EW + i] = limbs[i];
    fe9_canon_limbs<Fe9SecpPR, 2>(limbs, a.y);
    for (int i = 0; i < 9; i++) out[(size_t)t * SECP_SCAN_EW + 9 + i] = limbs[i];
  }
  uint8_t* tail = (uint8_t*)(out + SECP_TAB_TAG_AUX);
  for (int i = 0; i < 32; i++) {
    tail[i] = Bip340AuxTag::H[i];
    tail[32 + i] = Bip340NonceTag::H[i];
    tail[64 + i] = Bip340Tag::H[i];
  }
}

size_t secp_sign_ws_words(int n, int nkeys) { return (size_t)n * SS_ROW + (size_t)nkeys * 16; }

hipError_t secp_public_key_batch(const uint32_t* table, const uint8_t* sk, int mode, uint8_t* out, uint8_t* ok, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_secp_public_key, dim3((n + 63) / 64), dim3(64), 0, st, table, sk, mode, out, ok, n);
  return hipGetLastError();
}
// hash: 32 bytes per row; extra: 32 bytes per row or null; recid may be null; ws: secp_sign_ws_words(n, 0) words
hipError_t ecdsa_sign_batch(const uint32_t* table, const uint8_t* sk, int one_key, const uint8_t* hash, const uint8_t* extra, int low_s, uint8_t* sig,
                            uint8_t* recid, uint8_t* ok, int n, uint32_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ecdsa_sign_seed, dim3((n + 255) / 256), dim3(256), 0, st, ws, sk, one_key ? 0 : 32, hash, extra, n);
  hipLaunchKernelGGL(k_secp_sign_mul, dim3((n + 63) / 64), dim3(64), 0, st, table, ws, n);
  hipLaunchKernelGGL(k_ecdsa_sign_finish, dim3((n + 63) / 64), dim3(64), 0, st, table, ws, extra ? 96u : 64u, low_s ? 1u : 0u, sig, recid, ok, n);
  return hipGetLastError();
}
// ws: secp_sign_ws_words(n, one_key ? 1 : n) words
hipError_t schnorr_sign_batch(const uint32_t* table, const uint8_t* sk, int one_key, const uint8_t* aux, const uint8_t* msgs, const uint64_t* off,
                              uint8_t* sig, uint8_t* ok, int n, uint32_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int nkeys = one_key ? 1 : n;
  uint32_t* pts = ws + (size_t)n * SS_ROW;
  hipLaunchKernelGGL(k_secp_key_points, dim3((nkeys + 63) / 64), dim3(64), 0, st, table, sk, pts, nkeys);
  hipLaunchKernelGGL(k_schnorr_sign_nonce, dim3((n + 255) / 256), dim3(256), 0, st, table, ws, sk, pts, one_key ? 0 : 32, aux, msgs, off, n);
  hipLaunchKernelGGL(k_secp_sign_mul, dim3((n + 63) / 64), dim3(64), 0, st, table, ws, n);
  hipLaunchKernelGGL(k_schnorr_sign_finish, dim3((n + 255) / 256), dim3(256), 0, st, table, ws, msgs, off, sig, ok, n);
  return hipGetLastError();
}
void secp_sign_check_row_words(int op, int* wa, int* wb, int* wo) { secp_sign_check_widths(op, *wa, *wb, *wo); }
// ws: n rows of SS_ROW words
hipError_t secp_sign_check(int op, int variant, const uint32_t* table, uint32_t* ws, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n,
                           hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_secp_sign_check, dim3((n + 63) / 64), dim3(64), 0, st, op, variant, table, ws, d_a, d_b, d_out, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same lane functions, one row after the other
int secp_sign_check_host(int op, int variant, const uint32_t* table, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  uint32_t row[SS_ROW] = {0};
  const int rc = secp_sign_check_op(op, variant, table, row, a, b, out);
  for (int i = 0; i < SS_ROW; i++) ((volatile uint32_t*)row)[i] = 0;
  return rc;
}
void secp_public_key_host(const uint32_t* table, const uint8_t* sk, int mode, uint8_t* out, uint8_t* ok, int n) {
  for (int i = 0; i < n; i++) secp_public_key_lane(table, sk + (size_t)i * 32, mode, out + (size_t)i * secp_pk_bytes(mode), ok + i);
}
// one row; refuse_first: candidates below this index are refused (tests of the retry loop)
void ecdsa_sign_host(const uint32_t* table, const uint8_t* sk, const uint8_t* hash, const uint8_t* extra, int low_s, int refuse_first, uint8_t* sig,
                     uint8_t* recid, uint8_t* ok) {
  uint32_t row[SS_ROW] = {0};
  ecdsa_sign_seed_lane(row, sk, hash, extra);
  secp_sign_mul_lane(table, row);
  ecdsa_sign_finish_lane(table, row, extra ? 96u : 64u, low_s ? 1u : 0u, refuse_first, sig, recid, ok);
  for (int i = 0; i < SS_ROW; i++) ((volatile uint32_t*)row)[i] = 0;
}
void schnorr_sign_host(const uint32_t* table, const uint8_t* sk, const uint8_t* aux, const uint8_t* msg, uint64_t len, uint8_t* sig, uint8_t* ok) {
  uint32_t row[SS_ROW] = {0}, d[8], x[8], y[8], pt[16];
  be32_to_words(d, sk);
  secp_mul_base_scan(table, d, x, y);
  for (int i = 0; i < 8; i++) {
    pt[i] = x[i];
    pt[8 + i] = y[i];
  }
  schnorr_sign_nonce_lane(table, row, sk, pt, aux, msg, len);
  secp_sign_mul_lane(table, row);
  schnorr_sign_finish_lane(table, row, msg, len, sig, ok);
  for (int i = 0; i < SS_ROW; i++) ((volatile uint32_t*)row)[i] = 0;
  for (int i = 0; i < 8; i++) ((volatile uint32_t*)d)[i] = 0;
}

}  // namespace ncg
