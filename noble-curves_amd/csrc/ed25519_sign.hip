// Batch Ed25519 signing (ed25519_sign.hpp has the lane code and what it computes): eddsa.getPublicKey, getExtendedPublicKey and
// sign for ed25519, ed25519ctx and ed25519ph.  Six small kernels instead of one, because the hashes and the multiply want
// different shapes: the SHA-512 kernels are 64-bit integer code with a 16-word schedule (256-lane blocks), the multiply is the
// Edwards field code plus one inversion (64-lane blocks, like the other ed25519 kernels).
//   k_ed_sign_set_dom  dom from the kernel argument into the workspace (one block, only when dom is not empty)
//   k_ed_sign_expand   seeds -> scalar || prefix                      (then the multiply fills in A)
//   k_ed_sign_prehash  PH(M) = SHA-512(M), ed25519ph only
//   k_ed_sign_nonce    r = SHA-512(dom || prefix || M) mod L
//   k_ed_mul_base_scan compress(k B) for secret k: R from r, A from scalar
//   k_ed_sign_finish   k = SHA-512(dom || R || A || M) mod L, S = (r + k scalar) mod L
#include "ed25519_sign.hpp"
#include "host_api.hpp"

namespace ncg {

// dom travels as a kernel argument (it is a host pointer in both forms of the entry point) and is written to the workspace once
struct EdDomArg {
  uint8_t b[ED25519_DOM_MAX + 3];
};
__global__ void __launch_bounds__(320) k_ed_sign_set_dom(EdDomArg dom, uint8_t* __restrict__ out, uint32_t dom_len) {
  if (threadIdx.x < dom_len) out[threadIdx.x] = dom.b[threadIdx.x];
}

// message i: msgs[off[i] .. off[i + 1]), or the 64-byte row i of `msgs` when off is null (the prehashed messages)
struct EdMsgs {
  const uint8_t* msgs;
  const uint64_t* off;
  __device__ const uint8_t* at(int i, uint64_t* len) const {
    if (!off) {
      *len = 64;
      return msgs + (size_t)i * 64;
    }
    const uint64_t lo = off[i];
    *len = off[i + 1] - lo;
    return msgs + lo;
  }
};

__global__ void __launch_bounds__(256) k_ed_sign_expand(const uint8_t* __restrict__ seeds, uint32_t* __restrict__ keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ed25519_expand_lane(seeds + (size_t)i * 32, keys + (size_t)i * ED_KEY_WORDS);
}
__global__ void __launch_bounds__(256) k_ed_sign_prehash(EdMsgs m, uint32_t* __restrict__ ph, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  ed25519_prehash_lane(msg, len, ph + (size_t)i * 16);
}
// key_stride: ED_KEY_WORDS, or 0 when one key row serves every message
__global__ void __launch_bounds__(256) k_ed_sign_nonce(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ keys,
                                                       int key_stride, EdMsgs m, uint32_t* __restrict__ r, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  ed25519_nonce_lane(dom, dom_len, keys + (size_t)i * key_stride, msg, len, r + (size_t)i * 8);
}
// scalars: row i at scalars + i * in_stride words; out: 8 words at out + i * out_stride words
__global__ void __launch_bounds__(64) k_ed_mul_base_scan(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, int in_stride,
                                                         uint32_t* __restrict__ out, int out_stride, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed25519_mul_base_scan_lane(table, scalars + (size_t)i * in_stride, out + (size_t)i * out_stride);
}
__global__ void __launch_bounds__(256) k_ed_sign_finish(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ keys,
                                                        int key_stride, EdMsgs m, const uint32_t* __restrict__ r, uint32_t* __restrict__ sigs,
                                                        uint8_t* __restrict__ ok, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  ed25519_sign_finish_lane(dom, dom_len, keys + (size_t)i * key_stride, msg, len, r + (size_t)i * 8, sigs + (size_t)i * 16, ok + i);
}

size_t ed25519_scan_table_words() { return ED_SCAN_TABLE_WORDS; }
void ed25519_build_scan_table(uint32_t* out) { ed25519_build_window_table(out, ED_SCAN_W, ED_SCAN_M); }

hipError_t ed25519_mul_base_scan_batch(const uint32_t* table, const uint32_t* scalars, int in_stride, uint32_t* out, int out_stride, int n,
                                       hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ed_mul_base_scan, dim3((n + 63) / 64), dim3(64), 0, st, table, scalars, in_stride, out, out_stride, n);
  return hipGetLastError();
}

// seeds -> scalar || prefix in the rows of `keys` (ED_KEY_WORDS words each), and A = scalar B as 8 words at out_a + i * out_stride:
// keys + 16 with stride ED_KEY_WORDS completes the expanded rows, a separate array takes the public keys alone
hipError_t ed25519_expand_batch(const uint32_t* table, const uint8_t* seeds, uint32_t* keys, uint32_t* out_a, int out_stride, int n,
                                hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ed_sign_expand, dim3((n + 255) / 256), dim3(256), 0, st, seeds, keys, n);
  return ed25519_mul_base_scan_batch(table, keys, ED_KEY_WORDS, out_a, out_stride, n, st);
}

// Workspace of one sign call, in words: dom, then n rows of r, then (prehash) n digests, then (seeds) the expanded rows
size_t ed25519_sign_ws_words(int n, int nkeys_to_expand, int prehash) {
  return ED_SIGN_DOM_WORDS + (size_t)n * 8 + (prehash ? (size_t)n * 16 : 0) + (size_t)nkeys_to_expand * ED_KEY_WORDS;
}
hipError_t ed25519_sign_batch(const uint32_t* table, const void* keys, int expanded, int one_key, int prehash, const uint8_t* dom_host,
                              uint32_t dom_len, const uint8_t* msgs, const uint64_t* msg_off, uint32_t* sigs, uint8_t* ok, int n, uint32_t* ws,
                              hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint8_t* d_dom = (uint8_t*)ws;
  uint32_t* d_r = ws + ED_SIGN_DOM_WORDS;
  uint32_t* d_ph = d_r + (size_t)n * 8;
  uint32_t* d_keys = d_ph + (prehash ? (size_t)n * 16 : 0);
  const int nkeys = one_key ? 1 : n;
  if (dom_len) {
    EdDomArg arg;
    for (uint32_t i = 0; i < sizeof arg.b; i++) arg.b[i] = i < dom_len ? dom_host[i] : 0;
    hipLaunchKernelGGL(k_ed_sign_set_dom, dim3(1), dim3(320), 0, st, arg, d_dom, dom_len);
  }
  const uint32_t* krows = (const uint32_t*)keys;
  if (!expanded) {
    if (hipError_t e = ed25519_expand_batch(table, (const uint8_t*)keys, d_keys, d_keys + 16, ED_KEY_WORDS, nkeys, st)) return e;
    krows = d_keys;
  }
  const int kstride = one_key ? 0 : ED_KEY_WORDS;
  const dim3 grid((n + 255) / 256), block(256);
  EdMsgs m{msgs, msg_off};
  if (prehash) {
    hipLaunchKernelGGL(k_ed_sign_prehash, grid, block, 0, st, m, d_ph, n);
    m = EdMsgs{(const uint8_t*)d_ph, nullptr};
  }
  hipLaunchKernelGGL(k_ed_sign_nonce, grid, block, 0, st, d_dom, dom_len, krows, kstride, m, d_r, n);
  if (hipError_t e = ed25519_mul_base_scan_batch(table, d_r, 8, sigs, 16, n, st)) return e;
  hipLaunchKernelGGL(k_ed_sign_finish, grid, block, 0, st, d_dom, dom_len, krows, kstride, m, d_r, sigs, ok, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same lane functions, one row after the other
void ed25519_mul_base_scan_host(const uint32_t* table, const uint32_t* scalars, uint32_t* out, int n) {
  for (int i = 0; i < n; i++) ed25519_mul_base_scan_lane(table, scalars + (size_t)i * 8, out + (size_t)i * 8);
}
void ed25519_expand_host(const uint32_t* table, const uint8_t* seeds, uint32_t* keys, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t* row = keys + (size_t)i * ED_KEY_WORDS;
    ed25519_expand_lane(seeds + (size_t)i * 32, row);
    ed25519_mul_base_scan_lane(table, row, row + 16);
  }
}
// one row; r_in (optional): the nonce scalar to use instead of the derived one
void ed25519_sign_host(const uint32_t* table, const void* key, int expanded, int prehash, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg,
                       uint64_t len, const uint32_t* r_in, uint32_t* sig, uint8_t* ok) {
  uint32_t row[ED_KEY_WORDS], ph[16], r[8];
  if (expanded) {
    for (int i = 0; i < ED_KEY_WORDS; i++) row[i] = ((const uint32_t*)key)[i];
  } else {
    ed25519_expand_host(table, (const uint8_t*)key, row, 1);
  }
  if (prehash) {
    ed25519_prehash_lane(msg, len, ph);
    msg = (const uint8_t*)ph;
    len = 64;
  }
  if (r_in) {
    for (int i = 0; i < 8; i++) r[i] = r_in[i];
  } else {
    ed25519_nonce_lane(dom, dom_len, row, msg, len, r);
  }
  ed25519_mul_base_scan_lane(table, r, sig);
  ed25519_sign_finish_lane(dom, dom_len, row, msg, len, r, sig, ok);
  for (int i = 0; i < ED_KEY_WORDS; i++) ((volatile uint32_t*)row)[i] = 0;
  for (int i = 0; i < 8; i++) ((volatile uint32_t*)r)[i] = 0;
}
void sha512_segments_host(const uint8_t* dom, uint32_t dom_len, const uint8_t* a32, const uint8_t* b32, const uint8_t* msg, uint64_t len,
                          uint8_t* out64) {
  const ShaSeg seg[4] = {{dom, dom_len}, {a32, a32 ? 32u : 0u}, {b32, b32 ? 32u : 0u}, {msg, len}};
  uint64_t h[8];
  sha512_segments<4>(h, seg);
  uint32_t x[16];
  sha512_digest_words(x, h);
  for (int i = 0; i < 64; i++) out64[i] = (uint8_t)(x[i / 4] >> (8 * (i % 4)));
}

}  // namespace ncg
