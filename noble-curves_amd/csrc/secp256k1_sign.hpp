// secp256k1 signing, one row per lane: the lane functions of secp256k1_sign.hip and of its CPU twins (hosttest.hip).
//
// ECDSA with RFC 6979 nonces - secp256k1.sign of the reference (src/abstract/weierstrass.ts:1480-1568, src/utils.ts:755-813):
//   h1 = bits2int_modN(hash);  seed = int2octets(d) || int2octets(h1) [|| extraEntropy];  k = candidate j of the HMAC-SHA256 DRBG
//   R = k G;  r = x(R) mod n;  s = k^-1 (h1 + r d) mod n;  k outside [1, n), r = 0 or s = 0: the next candidate
//   recovery = (y(R) odd) | (x(R) >= n) << 1;  lowS: s > n / 2 becomes n - s and the recovery bit 0 flips
// The reference multiplies k, h1 and d by a random blinding factor b before the inversion (weierstrass.ts:1523-1529); b cancels and
// changes no output bit, so it is NOT reproduced here: k^-1 is fn_inv, a fixed chain over the public exponent n - 2.
// BIP-340 - schnorr.getPublicKey / schnorr.sign (src/secp256k1.ts:147-221):
//   P = d' G;  d = d' for an even y(P), n - d' otherwise;  px = x(P)
//   t = bytes(d) xor tagged("BIP0340/aux", a);  k' = int(tagged("BIP0340/nonce", t || px || m)) mod n;  k' = 0 fails
//   R = k' G;  k = k' for an even y(R), n - k' otherwise;  e = int(tagged("BIP0340/challenge", x(R) || px || m)) mod n
//   sig = x(R) || (k + e d) mod n
//
// Every multiplication here takes a SECRET scalar (a key or a nonce), so it does not index a table by the scalar's digits (k_mul_base
// does): secp_mul_base_scan reads every entry of the current window, at addresses that are the same in every lane, and keeps the one
// whose index matches by masking.  No branch, address or trip count of the multiplication depends on the scalar; the hashes' trip
// counts depend on public lengths.  A refused key, a refused candidate and k' = 0 are reported and do branch.  No constant-time claim.
#pragma once
#include "curves.hpp"
#include "secp_fn.hpp"
#include "sha256.hpp"

namespace ncg {

// ---- SHA-256 over a short list of byte segments read one after the other (the twin of sha512_segments)
struct Sha256Seg {
  const uint8_t* p;
  uint64_t len;
};
template <int NSEG>
NCG_DI void sha256_segments(uint32_t (&h)[8], const Sha256Seg (&seg)[NSEG]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
  uint64_t end[NSEG];  // end[s]: position after the last byte of segment s
  uint64_t total = 0;
#pragma unroll
  for (int s = 0; s < NSEG; s++) end[s] = total += seg[s].len;
  const uint64_t nblocks = (total + 1 + 8 + 63) / 64;  // 0x80, 64-bit length, padding
  for (uint64_t blk = 0; blk < nblocks; blk++) {
    uint32_t w[16];
#pragma unroll 1
    for (int i = 0; i < 16; i++) {
      uint32_t v = 0;
      for (int j = 0; j < 4; j++) {
        const uint64_t pos = blk * 64 + (uint64_t)i * 4 + j;
        uint32_t byte = pos == total ? 0x80u : 0u;
#pragma unroll
        for (int s = 0; s < NSEG; s++) {
          const uint64_t start = end[s] - seg[s].len;
          if (pos >= start && pos < end[s]) byte = seg[s].p[pos - start];
        }
        v = (v << 8) | byte;
      }
      w[i] = v;
    }
    if (blk == nblocks - 1) {  // bit length, big-endian 64-bit
      w[14] = (uint32_t)(total >> 29);
      w[15] = (uint32_t)(total << 3);
    }
    sha256_block(h, w);
  }
}
NCG_DI void sha256_store_be(uint8_t* __restrict__ out, const uint32_t (&h)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    out[4 * j] = (uint8_t)(h[j] >> 24);
    out[4 * j + 1] = (uint8_t)(h[j] >> 16);
    out[4 * j + 2] = (uint8_t)(h[j] >> 8);
    out[4 * j + 3] = (uint8_t)h[j];
  }
}
NCG_DI void words_to_be32(uint8_t* __restrict__ out, const uint32_t (&w)[8]) {  // 8 LE limbs -> 32 big-endian bytes
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; j++) h[j] = w[7 - j];
  sha256_store_be(out, h);
}
// the digest as an integer: 8 LE limbs
NCG_DI void sha256_digest_words(uint32_t (&w)[8], const uint32_t (&h)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = h[7 - j];
}
// v mod n for v < 2^256 < 2n, by select
NCG_DI void fn_reduce_once(uint32_t (&v)[8]) {
  uint32_t n8[8], d8[8];
#pragma unroll
  for (int i = 0; i < 8; i++) n8[i] = ParamsSecpN::P[i];
  const uint32_t ge = 0u - (uint32_t)(mp_sub<8>(d8, v, n8) == 0);
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = (d8[i] & ge) | (v[i] & ~ge);
}
// all ones for k in [1, n)
NCG_DI uint32_t fn_valid_mask(const uint32_t (&k)[8]) {
  uint32_t n8[8], d8[8], any = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    n8[i] = ParamsSecpN::P[i];
    any |= k[i];
  }
  const uint32_t lt = mp_sub<8>(d8, k, n8);   // the borrow: 1 for k < n
  return 0u - (lt & (uint32_t)(any != 0));
}
// mask ? n - k : k  (k in [1, n))
NCG_DI void fn_cneg(uint32_t (&k)[8], uint32_t mask) {
  uint32_t n8[8], d8[8];
#pragma unroll
  for (int i = 0; i < 8; i++) n8[i] = ParamsSecpN::P[i];
  mp_sub<8>(d8, n8, k);
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = (d8[i] & mask) | (k[i] & ~mask);
}

// ---- the workspace row of one signature, in 32-bit words.  It holds the key, the nonce and the DRBG state during a call: the entry
// points clear it on the call's stream before they return.
constexpr int SS_K = 0;        // DRBG K, 8 big-endian words
constexpr int SS_V = 8;        // DRBG V, 8 big-endian words
constexpr int SS_SEED = 16;    // ECDSA: int2octets(d) || int2octets(h1) || extra (96 bytes); BIP-340: t || px || hash/aux(a)
constexpr int SS_NONCE = 40;   // the candidate k (ECDSA) or k' (BIP-340), 8 LE words
constexpr int SS_D = 48;       // d, 8 LE words
constexpr int SS_M = 56;       // h1, 8 LE words
constexpr int SS_PT = 64;      // x || y of (nonce) G, canonical, 8 + 8 LE words
constexpr int SS_FLAGS = 80;   // bit 0: the key is in [1, n); bit 1: a candidate was accepted (ECDSA) / k' != 0 (BIP-340)
constexpr int SS_ROW = 84;

// ---- the constants after the point table: the three BIP-340 tag hashes (32 bytes each), so that every hash segment is a pointer
constexpr int SECP_SCAN_W = 4, SECP_SCAN_M = 64, SECP_SCAN_T = 1 << (SECP_SCAN_W - 1);
constexpr int SECP_SCAN_EW = 2 * 9;  // words per entry: x, y
constexpr int SECP_SCAN_POINT_WORDS = SECP_SCAN_M * SECP_SCAN_T * SECP_SCAN_EW;
constexpr int SECP_TAB_TAG_AUX = SECP_SCAN_POINT_WORDS, SECP_TAB_TAG_NONCE = SECP_TAB_TAG_AUX + 8, SECP_TAB_TAG_CHAL = SECP_TAB_TAG_NONCE + 8;
constexpr int SECP_SCAN_TABLE_WORDS = SECP_TAB_TAG_CHAL + 8;

// ---- HMAC-SHA256 on words.  K: the 32-byte key as 8 big-endian words; msg: the message already cut into nblk padded blocks of 16
// big-endian words whose length field counts the 64 bytes of the ipad block as well.  The four kinds of block - K xor ipad, the
// message, K xor opad, the inner digest - go through ONE loop with one call of the compression function, and the function is not
// inlined: candidate 0 of the DRBG is five of these (22 compressions, 24 with extra entropy), a later candidate three, and that many
// unrolled compressions at every call site would not fit the instruction cache.
__host__ __device__ __noinline__ inline void hmac_sha256_blocks(uint32_t* __restrict__ out8, const uint32_t* __restrict__ K8,
                                                                const uint32_t* __restrict__ msg, int nblk) {
  uint32_t h[8], inner[8], w[16];
#pragma unroll 1
  for (int s = 0; s < nblk + 3; s++) {
    if (s == nblk + 1) {
#pragma unroll
      for (int i = 0; i < 8; i++) inner[i] = h[i];
    }
    if (s == 0 || s == nblk + 1) {
      h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
      h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
      const uint32_t pad = s == 0 ? 0x36363636u : 0x5c5c5c5cu;
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = (i < 8 ? K8[i] : 0u) ^ pad;
    } else if (s <= nblk) {
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = msg[(s - 1) * 16 + i];
    } else {   // the inner digest: 32 bytes after the 64 of the opad block
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = i < 8 ? inner[i] : 0u;
      w[8] = 0x80000000u;
      w[15] = (64 + 32) * 8;
    }
    sha256_block(h, w);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out8[i] = h[i];
}
constexpr int DRBG_MSG_WORDS = 48;   // V || sep || 96 seed bytes, 0x80 and the length: 138 bytes, three blocks
// the blocks of V || sep || seed (SL big-endian words of seed; the separator byte shifts them by one byte); returns their number
template <int SL>
NCG_DI int drbg_update_blocks(uint32_t (&blk)[DRBG_MSG_WORDS], const uint32_t (&V)[8], uint32_t sep, const uint32_t* __restrict__ S) {
  constexpr int LEN = 33 + 4 * SL, NBLK = (LEN + 9 + 63) / 64;
#pragma unroll
  for (int i = 0; i < DRBG_MSG_WORDS; i++) blk[i] = i < 8 ? V[i] : 0u;
  uint32_t carry = sep << 24;
#pragma unroll
  for (int i = 0; i < SL; i++) {
    blk[8 + i] = carry | (S[i] >> 8);
    carry = S[i] << 24;
  }
  blk[8 + SL] = carry | 0x00800000u;
  blk[NBLK * 16 - 1] = (64 + LEN) * 8;
  return NBLK;
}
NCG_DI void drbg_hmac_v(uint32_t (&V)[8], const uint32_t (&K)[8]) {   // V = HMAC(K, V)
  uint32_t blk[16], out[8];
#pragma unroll
  for (int i = 0; i < 16; i++) blk[i] = i < 8 ? V[i] : 0u;
  blk[8] = 0x80000000u;
  blk[15] = (64 + 32) * 8;
  hmac_sha256_blocks(out, K, blk, 1);
#pragma unroll
  for (int i = 0; i < 8; i++) V[i] = out[i];
}

// Candidate j of createHmacDrbg(32, 32, hmac-sha256) (utils.ts:755-813) from the seed at row[SS_SEED] (seed_len = 64, or 96 with extra
// entropy).  j = 0: reset (V = 01.., K = 00..), reseed with the seed, generate.  j > 0, after candidate j - 1 was refused: the empty
// reseed K = HMAC(V || 00), V = HMAC(V), then generate.  The candidates must be asked for in order: K and V wait in the row between
// two calls.  T: the candidate as 8 LE words (bits2int of 32 bytes).
NCG_DI void drbg_next(uint32_t* __restrict__ row, uint32_t seed_len, int j, uint32_t (&T)[8]) {
  uint32_t K[8], V[8], S[24], blk[DRBG_MSG_WORDS], out[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    K[i] = j == 0 ? 0u : row[SS_K + i];
    V[i] = j == 0 ? 0x01010101u : row[SS_V + i];
  }
#pragma unroll
  for (int i = 0; i < 24; i++) S[i] = __builtin_bswap32(row[SS_SEED + i]);   // the seed bytes as big-endian words
  for (uint32_t sep = 0; sep < (j == 0 ? 2u : 1u); sep++) {
    const int nblk = j != 0 ? drbg_update_blocks<0>(blk, V, sep, S) : seed_len == 96 ? drbg_update_blocks<24>(blk, V, sep, S)
                                                                                      : drbg_update_blocks<16>(blk, V, sep, S);
    hmac_sha256_blocks(out, K, blk, nblk);
#pragma unroll
    for (int i = 0; i < 8; i++) K[i] = out[i];
    drbg_hmac_v(V, K);
  }
  drbg_hmac_v(V, K);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    T[i] = V[7 - i];
    row[SS_K + i] = K[i];
    row[SS_V + i] = V[i];
  }
#pragma unroll
  for (int i = 0; i < DRBG_MSG_WORDS; i++) ((volatile uint32_t*)blk)[i] = 0;   // the blocks held the seed: the key and h1
}

// ---- uniform-scan fixed-base multiply.  table[w][j] = (2 j + 1) 2^(4 w) G as affine (x, y) in canonical 29-bit limbs (the Fe9
// storage form), built on the host by secp_build_scan_table: 64 windows of 8 entries of 18 words, 36 864 bytes.
//
// -(P + Q), Q = (x, y) affine: jac_madd_neg_nx (ec_sw.hpp) without its zero test of H.  No exceptional case is reachable from
// secp_mul_base_scan - DESIGN.md section 8 has the argument - so none is tested: the test would branch on a secret.
template <class PR, int B, int BX, int BY>
NCG_DI Jac<Fe9<PR, B>> jac_madd_neg_scan(const Jac<Fe9<PR, B>>& p, const Fe9<PR, BX>& qx, const Fe9<PR, BY>& qy) {
  auto Z1Z1 = f_sqr(p.Z);
  auto Z1Z1Z1 = p.Z * Z1Z1;
  auto H = f_mul_add(qx, Z1Z1, f_neg_lin(p.X));
  auto R = f_mul_add(qy, Z1Z1Z1, f_neg_lin(p.Y));
  auto HH = f_sqr(H);
  auto HHH = H * HH;
  auto V = p.X * HH;
  auto X3 = f_sqr_add(R, f_neg_lin(HHH, V));
  auto W = f_mul_mul(R, X3 - V, p.Y, HHH);
  auto Z3 = p.Z * H;
  return {X3, W, Z3};
}
// mask (all ones) ? -a : a, for an operand of a product or of fe9_to_wire (no literal-zero rule: y is never 0 on this curve)
NCG_DI Fe9<Fe9SecpPR, 2> secp_cneg_mask(const Fe9<Fe9SecpPR, 1>& a, uint32_t mask) {
  Fe9<Fe9SecpPR, 2> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = ((Fe9SecpPR::BIAS[1][i] - a.v[i]) & mask) | (a.v[i] & ~mask);
  return r;
}
// x, y (canonical, 8 LE words each) of k G.  k outside [1, n) is replaced by 1 (the callers refuse such a k themselves).
// An even k is multiplied as n - k, which is odd, and the result negated by mask: the recoding then never needs the "+1, take G
// back out" addition.  The digits are odd and the top one positive, so the accumulator starts as a table entry (no identity), and
// each step is acc = -(acc + (+-entry)): the stored point alternates in sign, which the mask of the entry's y accounts for.
NCG_DI void secp_mul_base_scan(const uint32_t* __restrict__ table, const uint32_t (&k_in)[8], uint32_t (&x_out)[8], uint32_t (&y_out)[8]) {
  using PR = Fe9SecpPR;
  using F1 = Fe9<PR, 1>;
  uint32_t k[8];
  const uint32_t valid = fn_valid_mask(k_in);
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = (k_in[i] & valid) | ((i == 0 ? 1u : 0u) & ~valid);
  const uint32_t even = 0u - (1u & ~k[0]);
  fn_cneg(k, even);
  SignedOddWindows<8, SECP_SCAN_W, SECP_SCAN_M> win;
  win.template init<8>(k);   // k is odd: was_even is false
  Jac<FeSecp> acc;
#pragma unroll 1
  for (int w = SECP_SCAN_M - 1; w >= 0; w--) {
    const int d = win.pop();
    const int sgn = d >> 31;                                          // -1 for a negative digit
    const uint32_t idx = (uint32_t)(((d ^ sgn) - sgn) - 1) >> 1;      // (|d| - 1) / 2
    const uint32_t* __restrict__ row = table + (size_t)w * (SECP_SCAN_T * SECP_SCAN_EW);
    uint32_t e[SECP_SCAN_EW];
#pragma unroll
    for (int i = 0; i < SECP_SCAN_EW; i++) e[i] = 0;
#pragma unroll
    for (int j = 0; j < SECP_SCAN_T; j++) {
      const uint32_t hit = 0u - (uint32_t)(idx == (uint32_t)j);
#pragma unroll
      for (int i = 0; i < SECP_SCAN_EW; i++) {
        const uint32_t v = row[j * SECP_SCAN_EW + i];   // the address is the same in every lane
        e[i] |= v & hit;
      }
    }
    const F1 qx = FieldIO<F1>::load(e), qy = FieldIO<F1>::load(e + 9);
    if (w == SECP_SCAN_M - 1) {   // the top digit is positive: the accumulator starts as its entry
      acc = {qx, qy, FeSecp::one()};
    } else {
      // the stored point is (-1)^(62 - w) times the true partial sum, so the entry goes in with that sign as well
      const uint32_t neg = (uint32_t)sgn ^ (0u - (uint32_t)(w & 1));
      acc = jac_madd_neg_scan(acc, qx, secp_cneg_mask(qy, neg));
    }
  }
  // 63 additions: the stored point is minus the true one; an even k asks for one more negation
  const Fe9<PR, 1> zi = fe9_inv_divsteps<PR, 2, true>(acc.Z);   // Z comes from a secret scalar: the fixed batch count
  const auto zi2 = f_sqr(zi);
  const auto x = acc.X * zi2;
  const F1 y = acc.Y * (zi2 * zi);
  fe9_to_wire(x_out, x);
  fe9_to_wire(y_out, secp_cneg_mask(y, ~even));
}

// ---- ECDSA: k2sig of the reference on words.  k: the candidate; x, y_odd: the affine x and the parity of y of k G; m = h1; d: the
// key; all 8 LE words.  Writes r, s (8 LE words each, zero when refused) and the recovery id; returns 1 when the candidate is accepted.
NCG_DI uint32_t ecdsa_sign_finish(const uint32_t (&k)[8], const uint32_t (&x)[8], uint32_t y_odd, const uint32_t (&m)[8], const uint32_t (&d)[8],
                                  uint32_t low_s, uint32_t (&r)[8], uint32_t (&s)[8], uint32_t* recid) {
  uint32_t n8[8], half[8], d8[8], k1[8];
  const uint32_t kvalid = fn_valid_mask(k);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    n8[i] = ParamsSecpN::P[i];
    half[i] = ParamsSecpN::HALF[i];
    k1[i] = (k[i] & kvalid) | ((i == 0 ? 1u : 0u) & ~kvalid);
  }
  const uint32_t xge = 0u - (uint32_t)(mp_sub<8>(d8, x, n8) == 0);   // x < p < 2n
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = (d8[i] & xge) | (x[i] & ~xge);
  const Fn r2 = Fn::from_const(ParamsSecpN::R2);
  const Fn kinv = fn_inv(fn_from_words(k1) * r2);        // Montgomery form
  const Fn rd = fn_from_words(r) * (fn_from_words(d) * r2);   // plain x Montgomery -> plain
  const Fn sv = (fn_from_words(m) + rd) * kinv;
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = sv.v[i];
  const uint32_t accepted = kvalid & (0u - (uint32_t)(!mp_is_zero<8>(r))) & (0u - (uint32_t)(!mp_is_zero<8>(s)));
  const uint32_t high = (0u - (uint32_t)words_lt(half, s)) & (0u - (low_s & 1u));   // s > n >> 1
  mp_sub<8>(d8, n8, s);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    s[i] = ((d8[i] & high) | (s[i] & ~high)) & accepted;
    r[i] &= accepted;
  }
  *recid = (((y_odd & 1u) | (xge & 2u)) ^ (high & 1u)) & accepted;
  return accepted & 1u;
}

// BIP-340's scalar half: s = (k + e d) mod n with k = k' for an even y(R) and n - k' otherwise
NCG_DI void schnorr_sign_scalar(const uint32_t (&k_)[8], uint32_t y_odd, const uint32_t (&e)[8], const uint32_t (&d)[8], uint32_t (&s)[8]) {
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = k_[i];
  fn_cneg(k, 0u - (y_odd & 1u));
  const Fn r2 = Fn::from_const(ParamsSecpN::R2);
  const Fn ed = fn_from_words(d) * (fn_from_words(e) * r2);
  const Fn sv = fn_from_words(k) + ed;
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = sv.v[i];
}

// ---- lanes of the ECDSA pipeline.  sk, hash, extra: 32 big-endian bytes each (extra may be null)
NCG_DI void ecdsa_sign_seed_lane(uint32_t* __restrict__ row, const uint8_t* __restrict__ sk, const uint8_t* __restrict__ hash,
                                 const uint8_t* __restrict__ extra) {
  uint32_t d[8], m[8], T[8];
  be32_to_words(d, sk);
  be32_to_words(m, hash);
  fn_reduce_once(m);   // bits2int_modN of 32 bytes
  const uint32_t valid = fn_valid_mask(d) & 1u;
  uint8_t* seed = (uint8_t*)(row + SS_SEED);
  for (int i = 0; i < 32; i++) seed[i] = sk[i];   // int2octets(d) is the key itself for d < n
  words_to_be32(seed + 32, m);
  for (int i = 0; i < 32; i++) seed[64 + i] = extra ? extra[i] : 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    row[SS_D + i] = d[i];
    row[SS_M + i] = m[i];
    T[i] = 0;
  }
  if (valid) drbg_next(row, extra ? 96u : 64u, 0, T);
#pragma unroll
  for (int i = 0; i < 8; i++) row[SS_NONCE + i] = T[i];
  row[SS_FLAGS] = valid;
}
NCG_DI void secp_sign_mul_lane(const uint32_t* __restrict__ table, uint32_t* __restrict__ row) {
  uint32_t k[8], x[8], y[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = row[SS_NONCE + i];
  secp_mul_base_scan(table, k, x, y);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    row[SS_PT + i] = x[i];
    row[SS_PT + 8 + i] = y[i];
  }
}
// the candidate in the row through ecdsa_sign_finish; `refuse` (tests): refuse it whatever it is.  Returns 1 when accepted.
NCG_DI uint32_t ecdsa_sign_try_lane(uint32_t* __restrict__ row, uint32_t low_s, uint32_t refuse, uint8_t* __restrict__ sig64, uint8_t* recid_out) {
  uint32_t k[8], x[8], m[8], d[8], r[8], s[8], recid;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    k[i] = row[SS_NONCE + i];
    x[i] = row[SS_PT + i];
    m[i] = row[SS_M + i];
    d[i] = row[SS_D + i];
  }
  uint32_t acc = ecdsa_sign_finish(k, x, row[SS_PT + 8] & 1u, m, d, low_s, r, s, &recid);
  if (refuse) acc = 0;
  if (acc) {
    words_to_be32(sig64, r);
    words_to_be32(sig64 + 32, s);
    if (recid_out) *recid_out = (uint8_t)recid;
  }
  return acc;
}
constexpr int SECP_DRBG_MAX_ITERS = 1000;   // utils.ts:768 _maxDrbgIters
// after the first candidate went through seed, multiply and try: write the row's result, taking further candidates when the first was
// refused (about 2^-128 of real inputs) up to the reference's cap.  refuse_first (tests): candidates below this index are refused.
NCG_DI void ecdsa_sign_finish_lane(const uint32_t* __restrict__ table, uint32_t* __restrict__ row, uint32_t seed_len, uint32_t low_s, int refuse_first,
                                   uint8_t* __restrict__ sig64, uint8_t* recid_out, uint8_t* __restrict__ ok) {
  const uint32_t valid = row[SS_FLAGS] & 1u;
  uint32_t acc = 0;
  if (valid) {
    acc = ecdsa_sign_try_lane(row, low_s, refuse_first > 0, sig64, recid_out);
    for (int j = 1; !acc && j < SECP_DRBG_MAX_ITERS; j++) {
      uint32_t T[8];
      drbg_next(row, seed_len, j, T);
#pragma unroll
      for (int i = 0; i < 8; i++) row[SS_NONCE + i] = T[i];
      secp_sign_mul_lane(table, row);
      acc = ecdsa_sign_try_lane(row, low_s, j < refuse_first, sig64, recid_out);
    }
  }
  if (!acc) {
    for (int i = 0; i < 64; i++) sig64[i] = 0;
    if (recid_out) *recid_out = 0;
  }
  *ok = (uint8_t)acc;
  row[SS_FLAGS] = valid | (acc << 1);
}

// ---- public keys.  mode 0: 33 bytes (02 | y odd) || x; 1: 65 bytes 04 || x || y; 2: 32 bytes x (BIP-340)
constexpr int SECP_PK_COMPRESSED = 0, SECP_PK_UNCOMPRESSED = 1, SECP_PK_XONLY = 2;
NCG_DI int secp_pk_bytes(int mode) { return mode == SECP_PK_UNCOMPRESSED ? 65 : mode == SECP_PK_XONLY ? 32 : 33; }
NCG_DI void secp_public_key_lane(const uint32_t* __restrict__ table, const uint8_t* __restrict__ sk, int mode, uint8_t* __restrict__ out,
                                 uint8_t* __restrict__ ok) {
  uint32_t d[8], x[8], y[8];
  be32_to_words(d, sk);
  const uint32_t valid = fn_valid_mask(d) & 1u;
  secp_mul_base_scan(table, d, x, y);
  const int nb = secp_pk_bytes(mode);
  if (!valid) {
    for (int i = 0; i < nb; i++) out[i] = 0;
  } else if (mode == SECP_PK_XONLY) {
    words_to_be32(out, x);
  } else {
    out[0] = mode == SECP_PK_UNCOMPRESSED ? 4 : (uint8_t)(2u | (y[0] & 1u));
    words_to_be32(out + 1, x);
    if (mode == SECP_PK_UNCOMPRESSED) words_to_be32(out + 33, y);
  }
  *ok = (uint8_t)valid;
}

// ---- lanes of the BIP-340 pipeline.  pt: x || y of d' G (16 LE words, from the multiply); sk, aux: 32 bytes; tags: the table's tail
NCG_DI void schnorr_sign_nonce_lane(const uint32_t* __restrict__ table, uint32_t* __restrict__ row, const uint8_t* __restrict__ sk,
                                    const uint32_t* __restrict__ pt, const uint8_t* __restrict__ aux, const uint8_t* __restrict__ msg, uint64_t len) {
  uint32_t d[8], px[8], h[8], kk[8];
  be32_to_words(d, sk);
  const uint32_t valid = fn_valid_mask(d);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    d[i] &= valid;
    d[0] |= (i == 0 ? 1u : 0u) & ~valid;   // a refused key signs nothing; keep the arithmetic in range
    px[i] = pt[i];
  }
  fn_cneg(d, 0u - (pt[8] & 1u));   // d = n - d' for an odd y(P)
  uint8_t* t = (uint8_t*)(row + SS_SEED);
  uint8_t* pxb = t + 32;
  uint8_t* auxh = t + 64;
  const uint8_t* tag_aux = (const uint8_t*)(table + SECP_TAB_TAG_AUX);
  const uint8_t* tag_nonce = (const uint8_t*)(table + SECP_TAB_TAG_NONCE);
  words_to_be32(pxb, px);
  {
    const Sha256Seg seg[3] = {{tag_aux, 32}, {tag_aux, 32}, {aux, 32}};
    sha256_segments<3>(h, seg);
    sha256_store_be(auxh, h);
  }
  words_to_be32(t, d);
  for (int i = 0; i < 32; i++) t[i] ^= auxh[i];
  {
    const Sha256Seg seg[5] = {{tag_nonce, 32}, {tag_nonce, 32}, {t, 32}, {pxb, 32}, {msg, len}};
    sha256_segments<5>(h, seg);
  }
  sha256_digest_words(kk, h);
  fn_reduce_once(kk);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    row[SS_D + i] = d[i];
    row[SS_NONCE + i] = kk[i];
  }
  row[SS_FLAGS] = (valid & 1u) | ((uint32_t)(!mp_is_zero<8>(kk)) << 1);
}
NCG_DI void schnorr_sign_finish_lane(const uint32_t* __restrict__ table, uint32_t* __restrict__ row, const uint8_t* __restrict__ msg, uint64_t len,
                                     uint8_t* __restrict__ sig64, uint8_t* __restrict__ ok) {
  uint32_t kk[8], d[8], x[8], e[8], s[8], h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    kk[i] = row[SS_NONCE + i];
    d[i] = row[SS_D + i];
    x[i] = row[SS_PT + i];
  }
  const uint32_t good = row[SS_FLAGS] == 3u;
  words_to_be32(sig64, x);
  const uint8_t* tag = (const uint8_t*)(table + SECP_TAB_TAG_CHAL);
  const uint8_t* pxb = (const uint8_t*)(row + SS_SEED) + 32;
  const Sha256Seg seg[5] = {{tag, 32}, {tag, 32}, {sig64, 32}, {pxb, 32}, {msg, len}};
  sha256_segments<5>(h, seg);
  sha256_digest_words(e, h);
  fn_reduce_once(e);
  schnorr_sign_scalar(kk, row[SS_PT + 8] & 1u, e, d, s);
  words_to_be32(sig64 + 32, s);
  if (!good)
    for (int i = 0; i < 64; i++) sig64[i] = 0;
  *ok = (uint8_t)good;
}

// ---- the pieces on raw words (ncg_secp256k1_sign_check, ht_secp_sign_op).  Words per row (a, b, out); include/ncg.h has the same table.
//   0  DRBG candidate j = variant >> 1 (j <= 3) from the seed a (96 bytes as they lie in memory; the last 32 are used when
//      variant & 1): out = the 32 bytes of the candidate                                                     24, 1, 8
//   1  secp_mul_base_scan(a): x || y, canonical LE words                                                       8, 1, 16
//   2  ecdsa_sign_finish: a = k || x(R) || m || d, b = (y(R) odd) | lowS << 1: r || s || recid || accepted    32, 1, 18
//   3  schnorr_sign_scalar: a = k' || e || d, b = y(R) odd: s                                                 24, 1, 8
//   4  the whole ECDSA row with the candidates below `variant >> 1` refused (variant & 1: extra entropy): a = sk || hash || extra as
//      bytes, b = lowS: out = sig64 as bytes || recid || ok                                                    24, 1, 18
constexpr int SECP_SIGN_CHECK_OPS = 5;
NCG_DI void secp_sign_check_widths(int op, int& wa, int& wb, int& wo) {
  wa = wb = wo = 0;
  switch (op) {
    case 0: wa = 24; wb = 1; wo = 8; break;
    case 1: wa = 8; wb = 1; wo = 16; break;
    case 2: wa = 32; wb = 1; wo = 18; break;
    case 3: wa = 24; wb = 1; wo = 8; break;
    case 4: wa = 24; wb = 1; wo = 18; break;
    default: break;
  }
}
// row: SS_ROW words of scratch for ops 0 and 4 (it holds the state of the DRBG afterwards)
NCG_DI int secp_sign_check_op(int op, int variant, const uint32_t* __restrict__ table, uint32_t* __restrict__ row, const uint32_t* __restrict__ a,
                              const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  switch (op) {
    case 0: {
      const int jmax = variant >> 1;
      if (jmax < 0 || jmax > 3) return -1;
      for (int i = 0; i < 24; i++) row[SS_SEED + i] = a[i];
      uint32_t T[8];
      for (int j = 0; j <= jmax; j++) drbg_next(row, (variant & 1) ? 96u : 64u, j, T);
      words_to_be32((uint8_t*)out, T);
      return 0;
    }
    case 1: {
      uint32_t k[8], x[8], y[8];
      for (int i = 0; i < 8; i++) k[i] = a[i];
      secp_mul_base_scan(table, k, x, y);
      for (int i = 0; i < 8; i++) {
        out[i] = x[i];
        out[8 + i] = y[i];
      }
      return 0;
    }
    case 2: {
      uint32_t k[8], x[8], m[8], d[8], r[8], s[8], recid;
      for (int i = 0; i < 8; i++) {
        k[i] = a[i];
        x[i] = a[8 + i];
        m[i] = a[16 + i];
        d[i] = a[24 + i];
      }
      const uint32_t acc = ecdsa_sign_finish(k, x, b[0] & 1u, m, d, (b[0] >> 1) & 1u, r, s, &recid);
      for (int i = 0; i < 8; i++) {
        out[i] = r[i];
        out[8 + i] = s[i];
      }
      out[16] = recid;
      out[17] = acc;
      return 0;
    }
    case 3: {
      uint32_t k[8], e[8], d[8], s[8];
      for (int i = 0; i < 8; i++) {
        k[i] = a[i];
        e[i] = a[8 + i];
        d[i] = a[16 + i];
      }
      schnorr_sign_scalar(k, b[0] & 1u, e, d, s);
      for (int i = 0; i < 8; i++) out[i] = s[i];
      return 0;
    }
    case 4: {
      const int refuse = variant >> 1;
      if (refuse < 0 || refuse > 3) return -1;
      const uint8_t* in = (const uint8_t*)a;
      uint8_t rec = 0, ok = 0;
      ecdsa_sign_seed_lane(row, in, in + 32, (variant & 1) ? in + 64 : nullptr);
      secp_sign_mul_lane(table, row);
      ecdsa_sign_finish_lane(table, row, (variant & 1) ? 96u : 64u, b[0] & 1u, refuse, (uint8_t*)out, &rec, &ok);
      out[16] = rec;
      out[17] = ok;
      return 0;
    }
    default: return -1;
  }
}

}  // namespace ncg
