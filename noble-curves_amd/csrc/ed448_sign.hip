// Batch SHAKE256, Ed448 signing and the challenge of Ed448 verification (ed448_sign.hpp and keccak.hpp have the lane code and what it
// computes): eddsa.getPublicKey, getExtendedPublicKey and sign for ed448 and ed448ph, and k for verify.  The hash kernels are kept
// apart from the kernel that multiplies: ed448_mul fills the register file on its own, a 25-lane Keccak state
// beside it would go to memory.  One row per lane, blocks of one wave like the kernels of ed448.hip.
//   k_ed448_set_dom       dom from the kernel argument into the workspace (one block)
//   k_shake256            SHAKE256(M, out_len) per row, any lengths
//   k_ed448_expand        seeds -> scalar || prefix                       (then the multiply fills in A)
//   k_ed448_prehash       PH(M) = SHAKE256(M, 64), ed448ph only
//   k_ed448_nonce         r = SHAKE256(dom || prefix || M, 114) mod n
//   k_ed448_mul_base_rows encode(k B) for secret k on rows of any stride: R from r, A from scalar
//   k_ed448_sign_finish   k = SHAKE256(dom || R || A || M, 114) mod n, S = (r + k scalar) mod n
//   k_ed448_challenge     k alone, for verification
#include "ed448_sign.hpp"
#include "host_api.hpp"

namespace ncg {

// dom travels as a kernel argument (it is a host pointer in both forms of the entry points) and is written to the workspace once
struct Ed448DomArg {
  uint8_t b[ED448_DOM_WORDS * 4];
};
__global__ void __launch_bounds__(320) k_ed448_set_dom(Ed448DomArg dom, uint8_t* __restrict__ out, uint32_t dom_len) {
  if (threadIdx.x < dom_len) out[threadIdx.x] = dom.b[threadIdx.x];
}

// message i: msgs[off[i] .. off[i + 1]), or the `fixed`-byte row at msgs + i * stride when off is null (prehashed messages, check rows)
struct Ed448Msgs {
  const uint8_t* msgs;
  const uint64_t* off;
  uint32_t fixed, stride;
  NCG_DI const uint8_t* at(int i, uint64_t* len) const {
    if (!off) {
      *len = fixed;
      return msgs + (size_t)i * stride;
    }
    const uint64_t lo = off[i];
    *len = off[i + 1] - lo;
    return msgs + lo;
  }
};

__global__ void __launch_bounds__(64) k_shake256(Ed448Msgs m, uint32_t out_len, uint8_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  const KeccakSeg seg[1] = {{msg, len}};
  uint64_t st[25];
  shake256_absorb<1>(st, seg);
  shake256_squeeze(st, out + (size_t)i * out_len, out_len);
}
__global__ void __launch_bounds__(64) k_ed448_expand(const uint8_t* __restrict__ seeds, uint32_t* __restrict__ keys, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed448_expand_lane(seeds + (size_t)i * 57, keys + (size_t)i * ED448_KEY_WORDS);
}
__global__ void __launch_bounds__(64) k_ed448_prehash(Ed448Msgs m, uint32_t* __restrict__ ph, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  ed448_prehash_lane(msg, len, ph + (size_t)i * 16);
}
// key_stride: ED448_KEY_WORDS, or 0 when one key row serves every message
__global__ void __launch_bounds__(64) k_ed448_nonce(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ keys,
                                                    int key_stride, Ed448Msgs m, uint32_t* __restrict__ r, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  ed448_nonce_lane(dom, dom_len, keys + (size_t)i * key_stride, msg, len, r + (size_t)i * 14);
}
// scalars: 14 words at scalars + i * in_stride words; out: 57 bytes at out + i * out_stride bytes
__global__ void __launch_bounds__(64) k_ed448_mul_base_rows(const uint32_t* __restrict__ scalars, int in_stride, uint8_t* __restrict__ out,
                                                            int out_stride, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed448_mul_base_lane(scalars + (size_t)i * in_stride, out + (size_t)i * out_stride);
}
// r: 14 words at r + i * r_stride words; signatures at sigs + i * sig_stride bytes; ok at ok + i * ok_stride bytes
__global__ void __launch_bounds__(64) k_ed448_sign_finish(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ keys,
                                                          int key_stride, Ed448Msgs m, const uint32_t* __restrict__ r, int r_stride,
                                                          uint8_t* __restrict__ sigs, int sig_stride, uint8_t* __restrict__ ok, int ok_stride, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  ed448_sign_finish_lane(dom, dom_len, keys + (size_t)i * key_stride, msg, len, r + (size_t)i * r_stride, sigs + (size_t)i * sig_stride,
                         ok + (size_t)i * ok_stride);
}
__global__ void __launch_bounds__(64) k_ed448_challenge(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint8_t* __restrict__ sigs,
                                                        const uint8_t* __restrict__ pks, Ed448Msgs m, uint32_t* __restrict__ out_k, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t len;
  const uint8_t* msg = m.at(i, &len);
  uint32_t k[14];
  ed448_challenge_lane(dom, dom_len, sigs + (size_t)i * 114, pks + (size_t)i * 57, msg, len, k);
#pragma unroll
  for (int j = 0; j < 14; j++) out_k[(size_t)i * 14 + j] = k[j];
}
__global__ void __launch_bounds__(64) k_ed448_sign_check(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int wa, wb, wo;
  ed448_sign_check_widths(op, wa, wb, wo);
  (void)ed448_sign_check_op(op, a + (size_t)i * wa, b + (size_t)i * wb, out + (size_t)i * wo);
}

static dim3 ed448_grid(int n) { return dim3(((unsigned)n + 63u) / 64u); }
static void ed448_set_dom(const uint8_t* dom_host, uint32_t dom_len, uint8_t* d_dom, hipStream_t st) {
  if (!dom_len) return;
  Ed448DomArg arg;
  for (uint32_t i = 0; i < sizeof arg.b; i++) arg.b[i] = i < dom_len ? dom_host[i] : 0;
  hipLaunchKernelGGL(k_ed448_set_dom, dim3(1), dim3(320), 0, st, arg, d_dom, dom_len);
}

hipError_t shake256_batch(const uint8_t* msgs, const uint64_t* msg_off, uint32_t out_len, uint8_t* out, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_shake256, ed448_grid(n), dim3(64), 0, st, Ed448Msgs{msgs, msg_off, 0, 0}, out_len, out, n);
  return hipGetLastError();
}
static hipError_t ed448_mul_base_rows(const uint32_t* scalars, int in_stride, uint8_t* out, int out_stride, int n, hipStream_t st) {
  hipLaunchKernelGGL(k_ed448_mul_base_rows, ed448_grid(n), dim3(64), 0, st, scalars, in_stride, out, out_stride, n);
  return hipGetLastError();
}

// seeds -> scalar || prefix in the rows of `keys` (ED448_KEY_WORDS words each), and A = scalar B as 57 bytes at out_a + i * out_stride:
// the rows' own A field completes the expanded rows, a separate array takes the public keys alone
hipError_t ed448_expand_batch(const uint8_t* seeds, uint32_t* keys, uint8_t* out_a, int out_stride, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ed448_expand, ed448_grid(n), dim3(64), 0, st, seeds, keys, n);
  return ed448_mul_base_rows(keys, ED448_KEY_WORDS, out_a, out_stride, n, st);
}

// Workspace of one sign call, in words: dom, then n rows of r, then (prehash) n digests, then (seeds) the expanded rows
size_t ed448_sign_ws_words(int n, int nkeys_to_expand, int prehash) {
  return ED448_DOM_WORDS + (size_t)n * 14 + (prehash ? (size_t)n * 16 : 0) + (size_t)nkeys_to_expand * ED448_KEY_WORDS;
}
hipError_t ed448_sign_batch(const void* keys, int expanded, int one_key, int prehash, const uint8_t* dom_host, uint32_t dom_len,
                            const uint8_t* msgs, const uint64_t* msg_off, uint8_t* sigs, uint8_t* ok, int n, uint32_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint8_t* d_dom = (uint8_t*)ws;
  uint32_t* d_r = ws + ED448_DOM_WORDS;
  uint32_t* d_ph = d_r + (size_t)n * 14;
  uint32_t* d_keys = d_ph + (prehash ? (size_t)n * 16 : 0);
  const int nkeys = one_key ? 1 : n;
  ed448_set_dom(dom_host, dom_len, d_dom, st);
  const uint32_t* krows = (const uint32_t*)keys;
  if (!expanded) {
    if (hipError_t e = ed448_expand_batch((const uint8_t*)keys, d_keys, (uint8_t*)d_keys + ED448_KEY_A_BYTE, ED448_KEY_WORDS * 4, nkeys, st)) return e;
    krows = d_keys;
  }
  const int kstride = one_key ? 0 : ED448_KEY_WORDS;
  const dim3 grid = ed448_grid(n), block(64);
  Ed448Msgs m{msgs, msg_off, 0, 0};
  if (prehash) {
    hipLaunchKernelGGL(k_ed448_prehash, grid, block, 0, st, m, d_ph, n);
    m = Ed448Msgs{(const uint8_t*)d_ph, nullptr, 64, 64};
  }
  hipLaunchKernelGGL(k_ed448_nonce, grid, block, 0, st, d_dom, dom_len, krows, kstride, m, d_r, n);
  if (hipError_t e = ed448_mul_base_rows(d_r, 14, sigs, 114, n, st)) return e;
  hipLaunchKernelGGL(k_ed448_sign_finish, grid, block, 0, st, d_dom, dom_len, krows, kstride, m, d_r, 14, sigs, 114, ok, 1, n);
  return hipGetLastError();
}

// k of verification.  Workspace in words: dom, then (prehash) n digests
size_t ed448_challenge_ws_words(int n, int prehash) { return ED448_DOM_WORDS + (prehash ? (size_t)n * 16 : 0); }
hipError_t ed448_challenge_batch(const uint8_t* sigs, const uint8_t* pks, int prehash, const uint8_t* dom_host, uint32_t dom_len,
                                 const uint8_t* msgs, const uint64_t* msg_off, uint32_t* out_k, int n, uint32_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint8_t* d_dom = (uint8_t*)ws;
  uint32_t* d_ph = ws + ED448_DOM_WORDS;
  ed448_set_dom(dom_host, dom_len, d_dom, st);
  Ed448Msgs m{msgs, msg_off, 0, 0};
  if (prehash) {
    hipLaunchKernelGGL(k_ed448_prehash, ed448_grid(n), dim3(64), 0, st, m, d_ph, n);
    m = Ed448Msgs{(const uint8_t*)d_ph, nullptr, 64, 64};
  }
  hipLaunchKernelGGL(k_ed448_challenge, ed448_grid(n), dim3(64), 0, st, d_dom, dom_len, sigs, pks, m, out_k, n);
  return hipGetLastError();
}

// the pieces on raw words; ws: ED448_DOM_WORDS words (op 3 keeps its dom there)
void ed448_sign_check_row_words(int op, int* wa, int* wb, int* wo) { ed448_sign_check_widths(op, *wa, *wb, *wo); }
size_t ed448_sign_check_ws_words() { return ED448_DOM_WORDS; }
static const uint8_t ED448_PLAIN_DOM[10] = {'S', 'i', 'g', 'E', 'd', '4', '4', '8', 0, 0};
hipError_t ed448_sign_check(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, int n, uint32_t* ws, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (op != 3) {
    hipLaunchKernelGGL(k_ed448_sign_check, ed448_grid(n), dim3(64), 0, st, op, d_a, d_b, d_out, n);
    return hipGetLastError();
  }
  uint8_t* d_dom = (uint8_t*)ws;
  uint8_t* sig = (uint8_t*)d_out;
  ed448_set_dom(ED448_PLAIN_DOM, 10, d_dom, st);
  if (hipError_t e = ed448_mul_base_rows(d_b, 30, sig, 120, n, st)) return e;
  const Ed448Msgs m{(const uint8_t*)(d_b + 14), nullptr, 64, 120};
  hipLaunchKernelGGL(k_ed448_sign_finish, ed448_grid(n), dim3(64), 0, st, d_dom, 10u, d_a, ED448_KEY_WORDS, m, d_b, 30, sig, 120, sig + 116, 120, n);
  return hipGetLastError();
}

// ---- the CPU twins: the same lane functions, one row after the other
int ed448_sign_check_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) { return ed448_sign_check_op(op, a, b, out); }
void ed448_expand_host(const uint8_t* seeds, uint32_t* keys, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t* row = keys + (size_t)i * ED448_KEY_WORDS;
    ed448_expand_lane(seeds + (size_t)i * 57, row);
    ed448_mul_base_lane(row, (uint8_t*)row + ED448_KEY_A_BYTE);
  }
}
// one row; r_in (optional): the nonce scalar to use instead of the derived one
void ed448_sign_host(const void* key, int expanded, int prehash, const uint8_t* dom, uint32_t dom_len, const uint8_t* msg, uint64_t len,
                     const uint32_t* r_in, uint8_t* sig, uint8_t* ok) {
  uint32_t row[ED448_KEY_WORDS], ph[16], r[14];
  if (expanded) {
    for (int i = 0; i < ED448_KEY_WORDS; i++) row[i] = ((const uint32_t*)key)[i];
  } else {
    ed448_expand_host((const uint8_t*)key, row, 1);
  }
  if (prehash) {
    ed448_prehash_lane(msg, len, ph);
    msg = (const uint8_t*)ph;
    len = 64;
  }
  if (r_in) {
    for (int i = 0; i < 14; i++) r[i] = r_in[i];
  } else {
    ed448_nonce_lane(dom, dom_len, row, msg, len, r);
  }
  ed448_mul_base_lane(r, sig);
  ed448_sign_finish_lane(dom, dom_len, row, msg, len, r, sig, ok);
  for (int i = 0; i < ED448_KEY_WORDS; i++) ((volatile uint32_t*)row)[i] = 0;
  for (int i = 0; i < 14; i++) ((volatile uint32_t*)r)[i] = 0;
}
// SHAKE256(dom || a || b || msg, out_len) through the four-segment absorb; a / b may be NULL (segment left out)
void shake256_segments_host(const uint8_t* dom, uint32_t dom_len, const uint8_t* a, uint32_t a_len, const uint8_t* b, uint32_t b_len,
                            const uint8_t* msg, uint64_t len, uint8_t* out, uint32_t out_len) {
  const KeccakSeg seg[4] = {{dom, dom_len}, {a, a ? a_len : 0u}, {b, b ? b_len : 0u}, {msg, len}};
  uint64_t st[25];
  shake256_absorb<4>(st, seg);
  shake256_squeeze(st, out, out_len);
}

}  // namespace ncg
