// Ed25519 signing, one row per lane: the lane functions of ed25519_sign.hip and of its CPU twin (hosttest.hip).
//
// eddsa.getPublicKey / getExtendedPublicKey / sign of the reference (src/abstract/edwards.ts:870-930, src/ed25519.ts:146-223):
//   h = SHA-512(seed); head = h[0..32) clamped; scalar = head mod L; prefix = h[32..64); A = scalar B
//   r = SHA-512(dom || prefix || M) mod L;  R = r B;  k = SHA-512(dom || R || A || M) mod L;  S = (r + k scalar) mod L
// with dom empty for ed25519 and "SigEd25519 no Ed25519 collisions" || phflag || len(ctx) || ctx for ed25519ctx / ed25519ph,
// and M replaced by SHA-512(M) for ed25519ph (edwards.ts:917).
//
// Both fixed-base multiplications take a SECRET scalar, so they do not index a table by their digits (k_ed_mul_base does):
// ed_mul_base_scan reads every entry of the current window, at addresses that are the same for every lane, and keeps the one
// whose index matches by masking.  No branch, address or trip count below depends on a key, a prefix or a nonce; the trip
// counts of the hashes depend on the lengths of dom and of the message, which are public.  This is not a constant-time claim.
#pragma once
#include "ec_te.hpp"
#include "scalar.hpp"
#include "sha512.hpp"

namespace ncg {

// ---- SHA-512 over a short list of byte segments read one after the other (sha512_ram is the case {r32, a32, msg})
struct ShaSeg {
  const uint8_t* p;
  uint64_t len;
};
template <int NSEG>
NCG_DI void sha512_segments(uint64_t (&h)[8], const ShaSeg (&seg)[NSEG]) {
  h[0] = 0x6a09e667f3bcc908ull; h[1] = 0xbb67ae8584caa73bull; h[2] = 0x3c6ef372fe94f82bull; h[3] = 0xa54ff53a5f1d36f1ull;
  h[4] = 0x510e527fade682d1ull; h[5] = 0x9b05688c2b3e6c1full; h[6] = 0x1f83d9abfb41bd6bull; h[7] = 0x5be0cd19137e2179ull;
  uint64_t end[NSEG];  // end[s]: position after the last byte of segment s
  uint64_t total = 0;
#pragma unroll
  for (int s = 0; s < NSEG; s++) end[s] = total += seg[s].len;
  const uint64_t nblocks = (total + 1 + 16 + 127) / 128;  // 0x80, 128-bit length, padding
  for (uint64_t blk = 0; blk < nblocks; blk++) {
    uint64_t w[16];
#pragma unroll 1
    for (int i = 0; i < 16; i++) {
      uint64_t v = 0;
      for (int j = 0; j < 8; j++) {
        const uint64_t pos = blk * 128 + (uint64_t)i * 8 + j;
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
    if (blk == nblocks - 1) {  // bit length, big-endian 128-bit (high half is zero for any real message)
      w[14] = total >> 61;
      w[15] = total << 3;
    }
    sha512_block(h, w);
  }
}
// the digest as 16 LE words (word j = bytes 4j..4j+3 of the byte string)
NCG_DI void sha512_digest_words(uint32_t (&x)[16], const uint64_t (&h)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x[2 * i] = __builtin_bswap32((uint32_t)(h[i] >> 32));
    x[2 * i + 1] = __builtin_bswap32((uint32_t)h[i]);
  }
}

// ---- key expansion: row = scalar (8 LE words) || prefix (8) || A (8, filled in by the multiply that follows)
constexpr int ED_KEY_WORDS = 24;
NCG_DI void ed25519_expand_lane(const uint8_t* __restrict__ seed32, uint32_t* __restrict__ key_row) {
  const ShaSeg seg[1] = {{seed32, 32}};
  uint64_t h[8];
  sha512_segments<1>(h, seg);
  uint32_t x[16], head[16], scalar[8];
  sha512_digest_words(x, h);
#pragma unroll
  for (int i = 0; i < 16; i++) head[i] = i < 8 ? x[i] : 0u;
  head[0] &= ~7u;                                     // byte 0 & 248
  head[7] = (head[7] & 0x7fffffffu) | 0x40000000u;    // byte 31 & 127 | 64
  mod_l_512(scalar, head);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    key_row[i] = scalar[i];
    key_row[8 + i] = x[8 + i];
  }
}

// ---- uniform-scan fixed-base multiply.  table[w][j] = (2 j + 1) 2^(W w) B in affine Niels form (27 stored words), built on
// the host by ed25519_build_window_table.  W = 4: 64 windows of 8 entries, 55 296 bytes.
constexpr int ED_SCAN_W = 4, ED_SCAN_M = 64, ED_SCAN_T = 1 << (ED_SCAN_W - 1);
constexpr int ED_SCAN_EW = 3 * 9;  // words per entry: y+x, y-x, 2dxy
constexpr int ED_SCAN_TABLE_WORDS = ED_SCAN_M * ED_SCAN_T * ED_SCAN_EW;

NCG_DI EdNielsAff<FEd> ed_scan_entry(const uint32_t (&e)[ED_SCAN_EW]) {
  using IO = FieldIO<FEd>;
  return {IO::load(e), IO::load(e + 9), IO::load(e + 18)};
}
NCG_DI FEd ed_select(uint32_t mask /* all ones: a */, const FEd& a, const FEd& b) {
  FEd r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = (a.v[i] & mask) | (b.v[i] & ~mask);
  return r;
}
// ed_madd_niels (ec_te.hpp) with the negation of q chosen by a mask (all ones: add -q) instead of a bool.  ed_madd_niels negates
// through f_cneg, `c ? f_neg(a) : a`, which the compiler turns into a branch on c: fine for a public digit, not for a secret one.
// Here both candidates are computed and combined word by word.  -C is BIAS - C without f_neg's literal-zero rule: it feeds the sums
// D -+ C, never a stored coordinate, so a zero T t2d may become a multiple of p.
NCG_DI EdExt<FEd> ed_madd_niels_masked(const EdExt<FEd>& p, const EdNielsAff<FEd>& q, uint32_t neg) {
  const FEd qa = ed_select(neg, q.yminusx, q.yplusx), qb = ed_select(neg, q.yplusx, q.yminusx);
  auto A = (p.Y - p.X) * qb;
  auto B = (p.Y + p.X) * qa;
  const FEd t = p.T * q.t2d;
  Fe9<Fe9EdPR, 2> C;
#pragma unroll
  for (int i = 0; i < 9; i++) C.v[i] = ((Fe9EdPR::BIAS[1][i] - t.v[i]) & neg) | (t.v[i] & ~neg);
  auto D = f_dbl(p.Z);
  auto E = B - A;
  auto Fq = fe9_norm(D - C);
  auto G = fe9_norm(D + C);
  auto H = B + A;
  return {E * Fq, G * H, Fq * G, E * H};
}
NCG_DI EdExt<FEd> ed_mul_base_scan(const uint32_t* __restrict__ table, const uint32_t (&k)[8]) {
  SignedOddWindows<8, ED_SCAN_W, ED_SCAN_M> win;
  win.template init<8>(k);
  const uint32_t even = 0u - (uint32_t)win.was_even;
  EdExt<FEd> acc = EdExt<FEd>::identity();
#pragma unroll 1
  for (int w = ED_SCAN_M - 1; w >= 0; w--) {
    const int d = win.pop();
    const int sgn = d >> 31;                                          // -1 for a negative digit
    const uint32_t idx = (uint32_t)(((d ^ sgn) - sgn) - 1) >> 1;      // (|d| - 1) / 2
    const uint32_t* __restrict__ row = table + (size_t)w * (ED_SCAN_T * ED_SCAN_EW);
    uint32_t e[ED_SCAN_EW];
#pragma unroll
    for (int i = 0; i < ED_SCAN_EW; i++) e[i] = 0;
#pragma unroll
    for (int j = 0; j < ED_SCAN_T; j++) {
      const uint32_t hit = 0u - (uint32_t)(idx == (uint32_t)j);
#pragma unroll
      for (int i = 0; i < ED_SCAN_EW; i++) {
        const uint32_t v = row[j * ED_SCAN_EW + i];   // the address is the same in every lane
        e[i] |= v & hit;
      }
    }
    acc = ed_madd_niels_masked(acc, ed_scan_entry(e), (uint32_t)sgn);
  }
  {  // an even scalar was bumped by one: B comes back out - always computed, then selected
    uint32_t e[ED_SCAN_EW];
#pragma unroll
    for (int i = 0; i < ED_SCAN_EW; i++) e[i] = table[i];
    const EdExt<FEd> fix = ed_madd_niels_masked(acc, ed_scan_entry(e), ~0u);
    acc = {ed_select(even, fix.X, acc.X), ed_select(even, fix.Y, acc.Y), ed_select(even, fix.Z, acc.Z), ed_select(even, fix.T, acc.T)};
  }
  return acc;
}

// Point.toBytes of a projective point: y, with the parity of x in bit 255 (edwards.ts:611-619); one inversion
NCG_DI void ed_compress_proj(uint32_t (&out)[8], const EdExt<FEd>& p) {
  const FEd zi = fe9_inv_divsteps<Fe9EdPR, 1, true>(p.Z);   // Z comes from a secret scalar: the fixed batch count
  const FEd x = p.X * zi, y = p.Y * zi;
  fe9_to_wire(out, y);
  out[7] |= ed_is_odd(x) ? 0x80000000u : 0u;
}
NCG_DI void ed25519_mul_base_scan_lane(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalar, uint32_t* __restrict__ out) {
  uint32_t k[8], enc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = scalar[i];
  ed_compress_proj(enc, ed_mul_base_scan(table, k));
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = enc[i];
}

// ---- the two hashes of a signature and its scalar half.  dom: dom_len bytes, the same for the whole call; key: an expanded row
NCG_DI void ed25519_prehash_lane(const uint8_t* __restrict__ msg, uint64_t len, uint32_t* __restrict__ out16) {
  const ShaSeg seg[1] = {{msg, len}};
  uint64_t h[8];
  sha512_segments<1>(h, seg);
  uint32_t x[16];
  sha512_digest_words(x, h);
#pragma unroll
  for (int i = 0; i < 16; i++) out16[i] = x[i];
}
NCG_DI void ed25519_nonce_lane(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ key, const uint8_t* __restrict__ msg,
                               uint64_t len, uint32_t* __restrict__ r_out) {
  const ShaSeg seg[3] = {{dom, dom_len}, {(const uint8_t*)(key + 8), 32}, {msg, len}};
  uint64_t h[8];
  sha512_segments<3>(h, seg);
  uint32_t r[8];
  sha512_digest_mod_l(r, h);
#pragma unroll
  for (int i = 0; i < 8; i++) r_out[i] = r[i];
}
// sig: R in words 0..7 already; S = (r + k scalar) mod L goes to words 8..15.  r == 0 (mod L): a zero row and ok = 0, where the
// reference's BASE.multiply(r) throws (edwards.ts:920-924).
NCG_DI void ed25519_sign_finish_lane(const uint8_t* __restrict__ dom, uint32_t dom_len, const uint32_t* __restrict__ key, const uint8_t* __restrict__ msg,
                                     uint64_t len, const uint32_t* __restrict__ r_in, uint32_t* __restrict__ sig, uint8_t* __restrict__ ok) {
  const ShaSeg seg[4] = {{dom, dom_len}, {(const uint8_t*)sig, 32}, {(const uint8_t*)(key + 16), 32}, {msg, len}};
  uint64_t h[8];
  sha512_segments<4>(h, seg);
  uint32_t k[8], a[8], r[16], prod[16], sum[16], s[8];
  sha512_digest_mod_l(k, h);
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = key[i];
#pragma unroll
  for (int i = 0; i < 16; i++) r[i] = i < 8 ? r_in[i] : 0u;
  mp_mul<8, 8>(prod, k, a);   // below 2^506 with r added: k, scalar, r < L < 2^253
  mp_add<16>(sum, prod, r);
  mod_l_512(s, sum);
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) any |= r_in[i];
  const uint32_t keep = 0u - (uint32_t)(any != 0);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    sig[i] &= keep;
    sig[8 + i] = s[i] & keep;
  }
  *ok = (uint8_t)(keep & 1u);
}

}  // namespace ncg
