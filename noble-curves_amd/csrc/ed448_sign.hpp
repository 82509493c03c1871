// Ed448 signing and the challenge of Ed448 verification, one row per lane: the lane functions of ed448_sign.hip and of its CPU twin
// (hosttest.hip).
//
// eddsa.getPublicKey / getExtendedPublicKey / sign of the reference (src/abstract/edwards.ts:866-930, src/ed448.ts:190-246):
//   h = SHAKE256(seed, 114); head = h[0..57) clamped (b[0] &= 252, b[55] |= 128, b[56] = 0); scalar = head mod n;
//   prefix = h[57..114); A = scalar B
//   r = SHAKE256(dom || prefix || M, 114) mod n;  R = r B;  k = SHAKE256(dom || R || A || M, 114) mod n;  S = (r + k scalar) mod n
// with dom = "SigEd448" || phflag || len(ctx) || ctx (never empty) and M replaced by SHAKE256(M, 64) for ed448ph.
//
// The scalar of a key is never 0 mod n: the clamped head lies in [2^447, 2^448) and is a multiple of 4, and the only multiple of n in
// that range, 3 n, is odd.  r = 0 (mod n) is therefore the only row a signing call refuses.
//
// Both multiplications take a SECRET scalar and run ed448_mul (ed448.hpp): double, always add, keep the sum by a select, complete
// formulas.  No branch, address or trip count below depends on a key, a prefix or a nonce; the trip counts of the hashes depend on
// the lengths of dom and of the message, which are public.  This is not a constant-time claim.
#pragma once
#include "ed448.hpp"
#include "keccak.hpp"

namespace ncg {

// an expanded key: scalar (14 LE words, below n) || prefix (57 bytes) || A (57 bytes) || 2 zero bytes
constexpr int ED448_KEY_WORDS = 43, ED448_KEY_PREFIX_BYTE = 56, ED448_KEY_A_BYTE = 113;
constexpr int ED448_DOM_BYTES = 265, ED448_DOM_WORDS = 67;  // NCG_ED448_DOM_MAX, and the words of the workspace that hold it

// SHAKE256(seg..., 114) mod n
template <int NSEG>
NCG_DI void shake256_mod_n(uint32_t (&k)[14], const KeccakSeg (&seg)[NSEG]) {
  uint64_t st[25];
  shake256_absorb<NSEG>(st, seg);
  uint32_t x[29];
  shake256_words<29>(x, st, 114);
  mod_n_912(k, x);
}

// seed -> scalar || prefix of the row; A stays zero until the multiply fills it in (byte stores at ED448_KEY_A_BYTE)
NCG_DI void ed448_expand_lane(const uint8_t* __restrict__ seed57, uint32_t* __restrict__ key_row) {
  const KeccakSeg seg[1] = {{seed57, 57}};
  uint64_t st[25];
  shake256_absorb<1>(st, seg);
  uint32_t x[30], head[29], scalar[14];
  shake256_words<30>(x, st, 114);
#pragma unroll
  for (int i = 0; i < 29; i++) head[i] = i < 14 ? x[i] : 0u;
  head[0] &= 0xfffffffcu;   // byte 0 & 252
  head[13] |= 0x80000000u;  // byte 55 | 128; byte 56 = 0: the head is 56 bytes
  mod_n_912(scalar, head);
#pragma unroll
  for (int i = 0; i < 14; i++) key_row[i] = scalar[i];
  // byte b of the row, 56 <= b < 113, is byte b + 1 of the hash: row word w = hash bytes 4 w + 1 .. 4 w + 4
#pragma unroll
  for (int w = 14; w < 29; w++) key_row[w] = (x[w] >> 8) | (x[w + 1] << 24);
#pragma unroll
  for (int w = 29; w < ED448_KEY_WORDS; w++) key_row[w] = 0;
}

NCG_DI void ed448_prehash_lane(const uint8_t* __restrict__ msg, uint64_t len, uint32_t* __restrict__ out16) {
  const KeccakSeg seg[1] = {{msg, len}};
  uint64_t st[25];
  shake256_absorb<1>(st, seg);
  uint32_t x[16];
  shake256_words<16>(x, st, 64);
#pragma unroll
  for (int i = 0; i < 16; i++) out16[i] = x[i];
}
NCG_DI void ed448_nonce_lane(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ key, const uint8_t* __restrict__ msg,
                             uint64_t len, uint32_t* __restrict__ r_out) {
  const KeccakSeg seg[3] = {{dom, dom_len}, {(const uint8_t*)key + ED448_KEY_PREFIX_BYTE, 57}, {msg, len}};
  uint32_t r[14];
  shake256_mod_n<3>(r, seg);
#pragma unroll
  for (int i = 0; i < 14; i++) r_out[i] = r[i];
}
// k = SHAKE256(dom || R || A || M, 114) mod n; r57 and a57 are packed encodings at any address
NCG_DI void ed448_challenge_lane(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint8_t* r57, const uint8_t* a57,
                                 const uint8_t* __restrict__ msg, uint64_t len, uint32_t (&k)[14]) {
  const KeccakSeg seg[4] = {{dom, dom_len}, {r57, 57}, {a57, 57}, {msg, len}};
  shake256_mod_n<4>(k, seg);
}
// sig: R in bytes 0..56 already; S = (r + k scalar) mod n goes to bytes 57..113 (byte 113 zero).  r == 0 (mod n): 114 zero bytes and
// ok = 0, where the reference's BASE.multiply(r) throws (edwards.ts:920-924).
NCG_DI void ed448_sign_finish_lane(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ key, const uint8_t* __restrict__ msg,
                                   uint64_t len, const uint32_t* __restrict__ r_in, uint8_t* sig, uint8_t* __restrict__ ok) {
  uint32_t k[14], a[14], r[14], s[14], rw[14];
  ed448_challenge_lane(dom, dom_len, sig, (const uint8_t*)key + ED448_KEY_A_BYTE, msg, len, k);
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    a[i] = key[i];
    r[i] = r_in[i];
    any |= r[i];
  }
  ed448_muladd_mod_n(s, r, k, a);
  const uint32_t keep = 0u - (uint32_t)(any != 0);
  const uint32_t rl = ed448_load57(sig, rw);
#pragma unroll
  for (int i = 0; i < 14; i++) {
    rw[i] &= keep;
    s[i] &= keep;
  }
  ed448_store57(sig, rw, rl & keep);
  ed448_store57(sig + 57, s, 0u);
  *ok = (uint8_t)(keep & 1u);
}

// ---- the pieces on raw words (ncg_ed448_sign_check, ht_ed448_sign_op).  Words per row (a, b, out), include/ncg.h has the same
// table:
//   0 keccak_f1600: the 25 lanes as 50 LE words (50, 0, 50)   1 mod_n_912: 29 words, the top one taken below 2^16 (29, 0, 14)
//   2 ed448_muladd_mod_n: a = r || k, b = s, all below n (28, 14, 14)
//   3 a signature with the nonce GIVEN: a = an expanded key row, b = r (14 words, below n) || a 64-byte message,
//     out = R || S (114 bytes), 2 zero bytes, then ok as one word (43, 30, 30); ed448 with an empty context.  Not a lane op: the
//     launcher runs the multiply and the finish kernel.
constexpr int ED448_SIGN_CHECK_OPS = 4;
NCG_DI void ed448_sign_check_widths(int op, int& wa, int& wb, int& wo) {
  const int A[ED448_SIGN_CHECK_OPS] = {50, 29, 28, 43};
  const int B[ED448_SIGN_CHECK_OPS] = {0, 0, 14, 30};
  const int O[ED448_SIGN_CHECK_OPS] = {50, 14, 14, 30};
  const bool known = op >= 0 && op < ED448_SIGN_CHECK_OPS;
  wa = known ? A[op] : 0;
  wb = known ? B[op] : 0;
  wo = known ? O[op] : 0;
}
NCG_DI int ed448_sign_check_op(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  switch (op) {
    case 0: {
      uint64_t st[25];
#pragma unroll
      for (int i = 0; i < 25; i++) st[i] = (uint64_t)a[2 * i] | ((uint64_t)a[2 * i + 1] << 32);
      keccak_f1600(st);
#pragma unroll
      for (int i = 0; i < 25; i++) {
        out[2 * i] = (uint32_t)st[i];
        out[2 * i + 1] = (uint32_t)(st[i] >> 32);
      }
      return 0;
    }
    case 1: {
      uint32_t x[29], k[14];
#pragma unroll
      for (int i = 0; i < 29; i++) x[i] = a[i];
      x[28] &= 0xffffu;
      mod_n_912(k, x);
#pragma unroll
      for (int i = 0; i < 14; i++) out[i] = k[i];
      return 0;
    }
    case 2: {
      uint32_t r[14], k[14], s[14], o[14];
#pragma unroll
      for (int i = 0; i < 14; i++) {
        r[i] = a[i];
        k[i] = a[14 + i];
        s[i] = b[i];
      }
      ed448_muladd_mod_n(o, r, k, s);
#pragma unroll
      for (int i = 0; i < 14; i++) out[i] = o[i];
      return 0;
    }
    default: return -1;
  }
}

}  // namespace ncg
