// ristretto255-SHA512 OPRF (RFC 9497), one row per lane: the lane code of the kernels of oprf.hip and of their CPU twins.
//
// Restates createOPRF of the reference (src/abstract/oprf.ts) with the hooks of ristretto255_oprf (src/ed25519.ts:682):
//   expand_message_xmd        hash-to-curve.ts    xmd_sha512_lane        RFC 9380 section 5.3.1 over SHA-512, at most 256 bytes out
//   hashToGroup / hashToCurve ed25519.ts          ristretto_hash_to_group  xmd(msg, DST, 64) -> two Elligator maps -> their sum
//   hashToScalar              ed25519.ts          ristretto_hash_to_scalar xmd(msg, DST, 64) as a little-endian number mod L
//   blind                     oprf.ts:595-606     oprf_blind_row
//   blindEvaluate / finalize  oprf.ts:624-639     oprf_mul_row, oprf_finalize_row
//   evaluate                  oprf.ts:607-618     oprf_evaluate_row
//   getTranscripts            oprf.ts:502-513     oprf_seed_lane, oprf_composite_row
//
// Every scalar here is a secret (the client's blind, the server's key, the proof nonce), so the multiply does not look anything
// up by its digits: ristretto_mul_secret doubles, always adds, and keeps one of the two by a mask, the shape of ed448_mul and of
// ed_mul_base_scan.  The inversion mod L is the Fermat chain for the PUBLIC exponent L - 2.  No branch, address or trip count
// below depends on a scalar or on the hashed input point; the trip counts of the hashes depend on the lengths of the inputs,
// which are public.  This is not a constant-time claim.
#pragma once
#include "ed25519_sign.hpp"
#include "ristretto.hpp"

namespace ncg {

// ---- SHA-512 over segments that are bytes in memory or up to 16 immediate bytes followed by zeros.  sha512_segments
// (ed25519_sign.hpp) reads every segment through a pointer; the length prefixes, counters and labels of RFC 9497 and the 128 zero
// bytes of b_0 would have to live in per-lane memory for that.  Here they travel in two registers: byte j of an immediate segment
// is byte j of imm0 || imm1 read big-endian, and zero from j = 16 on.
struct OSeg {
  const uint8_t* p;  // null: the immediate
  uint64_t len;
  uint64_t imm0, imm1;
};
NCG_DI OSeg oseg_mem(const uint8_t* p, uint64_t len) { return {p, len, 0, 0}; }
NCG_DI OSeg oseg_zero(uint64_t len) { return {nullptr, len, 0, 0}; }
// the `len` (<= 8) low bytes of v, most significant first: I2OSP(v, len)
NCG_DI OSeg oseg_be(uint64_t v, int len) { return {nullptr, (uint64_t)len, len ? v << (64 - 8 * len) : 0, 0}; }
NCG_DI OSeg oseg_imm(uint64_t imm0, uint64_t imm1, int len) { return {nullptr, (uint64_t)len, imm0, imm1}; }

// PRE: the message starts with the 64 bytes of `pre` (8 big-endian words, a chaining value of the xmd) before the segments
template <int NSEG, bool PRE>
NCG_DI void oprf_sha512(uint64_t (&h)[8], const uint64_t (&pre)[8], const OSeg (&seg)[NSEG]) {
  h[0] = 0x6a09e667f3bcc908ull; h[1] = 0xbb67ae8584caa73bull; h[2] = 0x3c6ef372fe94f82bull; h[3] = 0xa54ff53a5f1d36f1ull;
  h[4] = 0x510e527fade682d1ull; h[5] = 0x9b05688c2b3e6c1full; h[6] = 0x1f83d9abfb41bd6bull; h[7] = 0x5be0cd19137e2179ull;
  uint64_t end[NSEG];  // end[s]: position after the last byte of segment s
  uint64_t total = PRE ? 64 : 0;
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
          if (pos >= start && pos < end[s]) {
            const uint64_t k = pos - start;
            if (seg[s].p) byte = seg[s].p[k];
            else byte = k < 8 ? (uint32_t)(seg[s].imm0 >> (56 - 8 * k)) & 0xffu : (k < 16 ? (uint32_t)(seg[s].imm1 >> (120 - 8 * k)) & 0xffu : 0u);
          }
        }
        v = (v << 8) | byte;
      }
      w[i] = v;
    }
    if (PRE && blk == 0) {
#pragma unroll
      for (int i = 0; i < 8; i++) w[i] = pre[i];
    }
    if (blk == nblocks - 1) {
      w[14] = total >> 61;
      w[15] = total << 3;
    }
    sha512_block(h, w);
  }
}
template <int NSEG>
NCG_DI void oprf_sha512(uint64_t (&h)[8], const OSeg (&seg)[NSEG]) {
  const uint64_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  oprf_sha512<NSEG, false>(h, none, seg);
}
// bytes [0, count) of a digest to memory
NCG_DI void oprf_store_digest(uint8_t* __restrict__ out, const uint64_t (&h)[8], uint32_t count) {
#pragma unroll
  for (int j = 0; j < 64; j++)
    if ((uint32_t)j < count) out[j] = (uint8_t)(h[j / 8] >> (56 - 8 * (j % 8)));
}

// ---- expand_message_xmd (RFC 9380 section 5.3.1).  dstp: DST' = DST || I2OSP(len(DST), 1), dstp_len = len(DST) + 1 in 2..256,
// the same for the whole call.  The message is NSEG segments.  b0 = H(128 zero bytes || msg || I2OSP(out_len, 2) || 0 || DST').
template <int NSEG>
NCG_DI void xmd_sha512_b0(uint64_t (&b0)[8], const OSeg (&msg)[NSEG], const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t out_len) {
  OSeg seg[NSEG + 3];
  seg[0] = oseg_zero(128);
#pragma unroll
  for (int s = 0; s < NSEG; s++) seg[1 + s] = msg[s];
  seg[NSEG + 1] = oseg_be((uint64_t)out_len << 8, 3);
  seg[NSEG + 2] = oseg_mem(dstp, dstp_len);
  oprf_sha512<NSEG + 3>(b0, seg);
}
// b_i = H((b0 ^ b_(i-1)) || I2OSP(i, 1) || DST'), with b_0' = 0 for i = 1
NCG_DI void xmd_sha512_next(uint64_t (&bi)[8], const uint64_t (&b0)[8], const uint64_t (&prev)[8], uint32_t i, const uint8_t* __restrict__ dstp,
                            uint32_t dstp_len) {
  uint64_t pre[8];
#pragma unroll
  for (int j = 0; j < 8; j++) pre[j] = b0[j] ^ prev[j];
  const OSeg seg[2] = {oseg_be(i, 1), oseg_mem(dstp, dstp_len)};
  oprf_sha512<2, true>(bi, pre, seg);
}
// the 64 uniform bytes of the fused rows (ell = 1)
template <int NSEG>
NCG_DI void xmd_sha512_64(uint64_t (&b1)[8], const OSeg (&msg)[NSEG], const uint8_t* __restrict__ dstp, uint32_t dstp_len) {
  uint64_t b0[8];
  const uint64_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  xmd_sha512_b0<NSEG>(b0, msg, dstp, dstp_len, 64);
  xmd_sha512_next(b1, b0, zero, 1, dstp, dstp_len);
}
// out_len in 1..256 bytes to `out`
NCG_DI void xmd_sha512_lane(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t out_len,
                            uint8_t* __restrict__ out) {
  const OSeg m[1] = {oseg_mem(msg, len)};
  uint64_t b0[8], prev[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cur[8];
  xmd_sha512_b0<1>(b0, m, dstp, dstp_len, out_len);
  const uint32_t ell = (out_len + 63) / 64;
#pragma unroll 1
  for (uint32_t i = 1; i <= ell; i++) {
    xmd_sha512_next(cur, b0, prev, i, dstp, dstp_len);
    const uint32_t done = 64 * (i - 1);
    oprf_store_digest(out + done, cur, out_len - done < 64 ? out_len - done : 64);
#pragma unroll
    for (int j = 0; j < 8; j++) prev[j] = cur[j];
  }
}

// ---- scalars mod L as 8 LE words
struct OprfConsts {
  static constexpr uint32_t L[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0, 0, 0, 0x10000000u};
  static constexpr uint32_t L_MINUS_2[8] = {0x5cf5d3ebu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0, 0, 0, 0x10000000u};
};
NCG_DI void sc_load_l(uint32_t (&l)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) l[i] = OprfConsts::L[i];
}
// all ones where 0 < k < L
NCG_DI uint32_t sc_valid_mask(const uint32_t (&k)[8]) {
  uint32_t l[8], d[8], any = 0;
  sc_load_l(l);
  const uint32_t below = mp_sub<8>(d, k, l);  // the borrow: k < L
#pragma unroll
  for (int i = 0; i < 8; i++) any |= k[i];
  return (0u - below) & (0u - (uint32_t)(any != 0));
}
NCG_DI void sc_mul(uint32_t (&r)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t prod[16];
  mp_mul<8, 8>(prod, a, b);
  mod_l_512(r, prod);
}
NCG_DI void sc_add(uint32_t (&r)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {  // a, b < L: the sum is below 2^254
  uint32_t l[8], s[8], d[8];
  sc_load_l(l);
  (void)mp_add<8>(s, a, b);
  const uint32_t keep = 0u - mp_sub<8>(d, s, l);  // borrow: s < L
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = (s[i] & keep) | (d[i] & ~keep);
}
NCG_DI void sc_sub(uint32_t (&r)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t l[8], d[8], s[8];
  sc_load_l(l);
  const uint32_t neg = 0u - mp_sub<8>(d, a, b);
  (void)mp_add<8>(s, d, l);
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = (s[i] & neg) | (d[i] & ~neg);
}
// a^(L - 2): square and multiply over the bits of the constant exponent, 252 squarings and 68 products whatever a is
NCG_DI void sc_inv(uint32_t (&r)[8], const uint32_t (&a)[8]) {
  uint32_t acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = a[i];  // bit 252
#pragma unroll 1
  for (int b = 251; b >= 0; b--) {
    uint32_t t[8];
    sc_mul(t, acc, acc);
    if ((OprfConsts::L_MINUS_2[b >> 5] >> (b & 31)) & 1u) sc_mul(acc, t, a);  // a bit of the constant, the same in every lane
    else {
#pragma unroll
      for (int i = 0; i < 8; i++) acc[i] = t[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = acc[i];
}

// ---- [k] P for a secret k < 2^253: double, always add, keep by mask.  Per bit one ed_dbl (4 products + 4 squarings) and one
// ed_add_niels (8 products): 16 field products, 4048 for the 253 bits, and one product for the Niels form of P.  Everything
// stays in registers; the scalar is shifted left one bit per step so that no limb is indexed by the loop counter.
NCG_DI EdExt<FEd> ristretto_mul_secret(const EdExt<FEd>& P, const uint32_t (&k)[8]) {
  const EdNielsProj<FEd> Q = ed_to_niels(P, EdConsts::d2());
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = k[i];
  mp_shl<8>(s, 3);  // bit 252 to the top
  EdExt<FEd> acc = EdExt<FEd>::identity();
#pragma unroll 1
  for (int b = 0; b < 253; b++) {
    const uint32_t take = 0u - (s[7] >> 31);
    mp_shl<8>(s, 1);
    const EdExt<FEd> dbl = ed_dbl(acc);
    const EdExt<FEd> sum = ed_add_niels(dbl, Q, false);
    acc = {ed_select(take, sum.X, dbl.X), ed_select(take, sum.Y, dbl.Y), ed_select(take, sum.Z, dbl.Z), ed_select(take, sum.T, dbl.T)};
  }
  return acc;
}

// ---- the pieces of a row
constexpr uint8_t OPRF_OK = 0, OPRF_BAD_ENCODING = 1, OPRF_IDENTITY = 2, OPRF_BAD_SCALAR = 3;
constexpr int OPRF_FLAG_ONE_SCALAR = 1, OPRF_FLAG_INVERT = 2;

NCG_DI void oprf_load8(uint32_t (&w)[8], const uint32_t* __restrict__ p) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = p[i];
}
NCG_DI void oprf_store8_masked(uint32_t* __restrict__ out, const uint32_t (&w)[8], uint32_t keep) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = w[i] & keep;
}
// the scalar a row multiplies by: checked, and inverted where asked.  An invalid scalar becomes 1 (the row is dropped anyway).
NCG_DI uint32_t oprf_row_scalar(uint32_t (&k)[8], const uint32_t* __restrict__ scalar, bool invert) {
  uint32_t raw[8];
  oprf_load8(raw, scalar);
  const uint32_t ok = sc_valid_mask(raw);
#pragma unroll
  for (int i = 0; i < 8; i++) raw[i] = (raw[i] & ok) | ((i == 0 ? 1u : 0u) & ~ok);
  if (invert) sc_inv(k, raw);  // a flag of the call
  else {
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = raw[i];
  }
  return ok;
}
NCG_DI EdExt<FEd> ristretto_hash_to_group(const uint8_t* __restrict__ msg, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len) {
  const OSeg m[1] = {oseg_mem(msg, len)};
  uint64_t b1[8];
  xmd_sha512_64<1>(b1, m, dstp, dstp_len);
  uint32_t w[16];
  sha512_digest_words(w, b1);
  return ristretto_from_uniform(w);
}
template <int NSEG>
NCG_DI void ristretto_hash_to_scalar(uint32_t (&k)[8], const OSeg (&msg)[NSEG], const uint8_t* __restrict__ dstp, uint32_t dstp_len) {
  uint64_t b1[8];
  xmd_sha512_64<NSEG>(b1, msg, dstp, dstp_len);
  sha512_digest_mod_l(k, b1);
}
NCG_DI uint32_t oprf_nonzero_mask(const uint32_t (&w)[8]) {
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) any |= w[i];
  return 0u - (uint32_t)(any != 0);
}
// Hash(I2OSP(len(input), 2) || input || [I2OSP(len(info), 2) || info] || I2OSP(32, 2) || element || "Finalize"): hashInput of
// oprf.ts:499.  info is null outside mode 2.  `element` is the 32 bytes at elem (memory the lane wrote itself).
NCG_DI void oprf_finalize_hash(uint64_t (&h)[8], const uint8_t* __restrict__ input, uint64_t len, const uint8_t* __restrict__ info, uint32_t info_len,
                               const uint32_t (&elem)[8]) {
  // the element travels as immediates: two segments of 16 bytes (LE words -> the byte string, big-endian in the immediate)
  uint64_t e[4];
#pragma unroll
  for (int i = 0; i < 4; i++) e[i] = ((uint64_t)__builtin_bswap32(elem[2 * i]) << 32) | __builtin_bswap32(elem[2 * i + 1]);
  const OSeg seg[8] = {oseg_be(len, 2),
                       oseg_mem(input, len),
                       oseg_be(info_len, info ? 2 : 0),
                       oseg_mem(info, info ? info_len : 0),
                       oseg_be(32, 2),
                       oseg_imm(e[0], e[1], 16),
                       oseg_imm(e[2], e[3], 16),
                       oseg_imm(0x46696e616c697a65ull /* "Finalize" */, 0, 8)};
  oprf_sha512<8>(h, seg);
}
NCG_DI void oprf_store_out64(uint8_t* __restrict__ out64, const uint64_t (&h)[8], uint32_t keep) {
#pragma unroll
  for (int j = 0; j < 64; j++) out64[j] = (uint8_t)(h[j / 8] >> (56 - 8 * (j % 8))) & (uint8_t)keep;
}

// ---- the fused rows.  Each returns the row status and writes zero bytes for a rejected row.
// blind: hashToGroup(input, "HashToGroup-" || ctx) times the blind
NCG_DI uint8_t oprf_blind_row(const uint8_t* __restrict__ input, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                              const uint32_t* __restrict__ blind, uint32_t* __restrict__ out) {
  uint32_t k[8], enc[8];
  const uint32_t ok = oprf_row_scalar(k, blind, false);
  const EdExt<FEd> P = ristretto_hash_to_group(input, len, dstp, dstp_len);
  const EdExt<FEd> R = ristretto_mul_secret(P, k);
  ristretto_encode_ext(R.X, R.Y, R.Z, R.T, enc);
  const uint32_t nz = oprf_nonzero_mask(enc);  // 'Input point at infinity'
  oprf_store8_masked(out, enc, ok & nz);
  return ok ? (nz ? OPRF_OK : OPRF_IDENTITY) : OPRF_BAD_SCALAR;
}
// decode -> reject the identity -> [1 /] scalar -> multiply -> encode; the unblinded element stays in `enc`
NCG_DI uint8_t oprf_mul_lane(const uint32_t* __restrict__ element, const uint32_t* __restrict__ scalar, bool invert, uint32_t (&enc)[8]) {
  uint32_t w[8], k[8];
  oprf_load8(w, element);
  FEd x, y;
  const bool dec = ristretto_decode_lane(w, x, y);  // the element came over the wire: public
  const uint32_t nz = oprf_nonzero_mask(w);
  const uint32_t ok = oprf_row_scalar(k, scalar, invert);
  const FEd zero = FEd::zero(), one = FEd::one();
  const uint32_t good = 0u - (uint32_t)dec;
  const EdExt<FEd> P = {ed_select(good, x, zero), ed_select(good, y, one), one, ed_select(good, x * y, zero)};
  const EdExt<FEd> R = ristretto_mul_secret(P, k);
  ristretto_encode_ext(R.X, R.Y, R.Z, R.T, enc);
  const uint32_t keep = good & nz & ok;
#pragma unroll
  for (int i = 0; i < 8; i++) enc[i] &= keep;
  return !nz ? OPRF_IDENTITY : (!dec ? OPRF_BAD_ENCODING : (ok ? OPRF_OK : OPRF_BAD_SCALAR));
}
NCG_DI uint8_t oprf_mul_row(const uint32_t* __restrict__ element, const uint32_t* __restrict__ scalar, bool invert, uint32_t* __restrict__ out) {
  uint32_t enc[8];
  const uint8_t st = oprf_mul_lane(element, scalar, invert, enc);
  oprf_store8_masked(out, enc, ~0u);
  return st;
}
NCG_DI uint8_t oprf_finalize_row(const uint8_t* __restrict__ input, uint64_t len, const uint8_t* __restrict__ info, uint32_t info_len,
                                 const uint32_t* __restrict__ blind, const uint32_t* __restrict__ evaluated, uint8_t* __restrict__ out64) {
  uint32_t enc[8];
  const uint8_t st = oprf_mul_lane(evaluated, blind, true, enc);
  uint64_t h[8];
  oprf_finalize_hash(h, input, len, info, info_len, enc);
  oprf_store_out64(out64, h, st == OPRF_OK ? ~0u : 0u);
  return st;
}
NCG_DI uint8_t oprf_evaluate_row(const uint8_t* __restrict__ input, uint64_t len, const uint8_t* __restrict__ dstp, uint32_t dstp_len,
                                 const uint8_t* __restrict__ info, uint32_t info_len, const uint32_t* __restrict__ scalar, bool invert,
                                 uint8_t* __restrict__ out64) {
  uint32_t k[8], enc[8];
  const uint32_t ok = oprf_row_scalar(k, scalar, invert);
  const EdExt<FEd> P = ristretto_hash_to_group(input, len, dstp, dstp_len);
  const EdExt<FEd> R = ristretto_mul_secret(P, k);
  ristretto_encode_ext(R.X, R.Y, R.Z, R.T, enc);
  const uint32_t nz = oprf_nonzero_mask(enc);
  uint64_t h[8];
  oprf_finalize_hash(h, input, len, info, info_len, enc);
  oprf_store_out64(out64, h, ok & nz);
  return ok ? (nz ? OPRF_OK : OPRF_IDENTITY) : OPRF_BAD_SCALAR;
}
// seed = Hash(I2OSP(32, 2) || B || I2OSP(len(sdst), 2) || sdst), sdst = "Seed-" || ctx
NCG_DI void oprf_seed_lane(const uint8_t* __restrict__ B32, const uint8_t* __restrict__ sdst, uint32_t sdst_len, uint8_t* __restrict__ seed64) {
  const OSeg seg[4] = {oseg_be(32, 2), oseg_mem(B32, 32), oseg_be(sdst_len, 2), oseg_mem(sdst, sdst_len)};
  uint64_t h[8];
  oprf_sha512<4>(h, seg);
  oprf_store_digest(seed64, h, 64);
}
// d_i = hashToScalar(I2OSP(64, 2) || seed || I2OSP(i, 2) || I2OSP(32, 2) || C_i || I2OSP(32, 2) || D_i || "Composite").  C_i and D_i
// are hashed as they were received; a row whose C_i or D_i is the identity or does not decode is reported and gives zero.
NCG_DI uint8_t oprf_composite_row(const uint8_t* __restrict__ seed64, uint32_t i, const uint32_t* __restrict__ C, const uint32_t* __restrict__ D,
                                  const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t* __restrict__ out) {
  uint8_t st = OPRF_OK;
#pragma unroll 1
  for (int which = 1; which >= 0; which--) {  // C's verdict wins
    uint32_t w[8];
    oprf_load8(w, which ? D : C);
    FEd x, y;
    const bool dec = ristretto_decode_lane(w, x, y);
    const bool nz = oprf_nonzero_mask(w) != 0;
    if (!nz) st = OPRF_IDENTITY;
    else if (!dec) st = OPRF_BAD_ENCODING;
  }
  const OSeg seg[7] = {oseg_be(64, 2),
                       oseg_mem(seed64, 64),
                       oseg_be(((uint64_t)i << 16) | 32, 4),
                       oseg_mem((const uint8_t*)C, 32),
                       oseg_be(32, 2),
                       oseg_mem((const uint8_t*)D, 32),
                       oseg_imm(0x436f6d706f736974ull /* "Composit" */, 0x65ull << 56 /* "e" */, 9)};
  uint32_t k[8];
  ristretto_hash_to_scalar<7>(k, seg, dstp, dstp_len);
  oprf_store8_masked(out, k, st == OPRF_OK ? ~0u : 0u);
  return st;
}

// ---- the DLEQ proof (oprf.ts:537-562).  r B for the secret nonce through the masked fixed-base scan of the signers, as an element
NCG_DI void oprf_mul_base_row(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalar, uint32_t* __restrict__ out) {
  uint32_t k[8], enc[8];
  oprf_load8(k, scalar);
  const EdExt<FEd> R = ed_mul_base_scan(table, k);
  ristretto_encode_ext(R.X, R.Y, R.Z, R.T, enc);
  oprf_store8_masked(out, enc, ~0u);
}
// c = hashToScalar(I2OSP(32, 2) || B || .. || M || .. || Z || .. || t2 || .. || t3 || "Challenge"); pts: the five encodings in that order
NCG_DI void oprf_challenge_lane(const uint8_t* __restrict__ pts160, const uint8_t* __restrict__ dstp, uint32_t dstp_len, uint32_t (&c)[8]) {
  const OSeg seg[11] = {oseg_be(32, 2), oseg_mem(pts160, 32),       oseg_be(32, 2), oseg_mem(pts160 + 32, 32),
                        oseg_be(32, 2), oseg_mem(pts160 + 64, 32),  oseg_be(32, 2), oseg_mem(pts160 + 96, 32),
                        oseg_be(32, 2), oseg_mem(pts160 + 128, 32), oseg_imm(0x4368616c6c656e67ull /* "Challeng" */, 0x65ull << 56, 9)};
  ristretto_hash_to_scalar<11>(c, seg, dstp, dstp_len);
}

// ---- the pieces on raw rows (ncg_oprf_check, ht_oprf_check).  a, b, out: 8 words per row unless said otherwise.
//   op 0  a b mod L                                       a, b below L
//   op 1  1 / a mod L                                     0 < a < L
//   op 2  [b] a: a = 16 words, an ed25519 wire point (x, y); b the scalar; out = the ristretto255 encoding of the product
//   op 3  one xmd: a = 32 message bytes, b = DST' (variant = its length, at most 32 bytes), out = 16 words (64 bytes)
//   op 4  a + b mod L          op 5  a - b mod L
constexpr int OPRF_CHECK_OPS = 6;
NCG_DI void oprf_check_row_words(int op, int* wa, int* wb, int* wo) {
  *wa = op == 2 ? 16 : 8;
  *wb = 8;
  *wo = op == 3 ? 16 : 8;
  if (op < 0 || op >= OPRF_CHECK_OPS) *wa = *wb = *wo = 0;
}
NCG_DI int oprf_check_op(int op, int variant, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  uint32_t x[8], y[8], r[8];
  if (op == 3) {
    if (variant < 2 || variant > 32) return -1;
    xmd_sha512_lane((const uint8_t*)a, 32, (const uint8_t*)b, (uint32_t)variant, 64, (uint8_t*)out);
    return 0;
  }
  oprf_load8(y, b);
  if (op == 2) {
    const FEd px = fe9_from_wire<Fe9EdPR>(a), py = fe9_from_wire<Fe9EdPR>(a + 8);
    const EdExt<FEd> P = {px, py, FEd::one(), px * py};
    const EdExt<FEd> R = ristretto_mul_secret(P, y);
    ristretto_encode_ext(R.X, R.Y, R.Z, R.T, r);
  } else {
    oprf_load8(x, a);
    if (op == 0) sc_mul(r, x, y);
    else if (op == 1) sc_inv(r, x);
    else if (op == 4) sc_add(r, x, y);
    else if (op == 5) sc_sub(r, x, y);
    else return -1;
  }
  oprf_store8_masked(out, r, ~0u);
  return 0;
}

}  // namespace ncg
