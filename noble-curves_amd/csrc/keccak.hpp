// Keccak-f[1600], the SHAKE256 sponge and the scalar arithmetic mod the Ed448 group order, one message per lane: the lane code of
// ed448_sign.hip and of its CPU twin (hosttest.hip).  The reference takes shake256 from @noble/hashes (not vendored in the
// repository): this is FIPS 202 restated (rate 136 bytes, suffix 0x1f, last rate byte ^= 0x80); parity is pinned by hashlib in the
// tests.
//
// The 25 lanes of the state live in registers.  Every index into the state below is a compile-time constant: the round body is
// unrolled over x and y with the rotation counts and the pi permutation read from constexpr tables, and the sponge reaches "lane i
// of the block" for a run-time i by a chain of 17 selects, never by an address.  A state array that went to scratch memory would
// show as scratch bytes in the kernels' resource figures: the hash kernels have none.
#pragma once
#include <utility>

#include "fp.hpp"
#include "scalar.hpp"

namespace ncg {

struct KeccakConsts {
  static constexpr uint64_t RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
      0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
      0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
      0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // the rotation of lane x + 5 y
  static constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
};

constexpr int SHAKE256_RATE = 136, SHAKE256_RATE_LANES = 17;

template <int N>
NCG_DI uint64_t keccak_rotl(uint64_t x) {
  if constexpr (N == 0) return x;
  else return (x << N) | (x >> (64 - N));
}

// rho and pi of lane I = x + 5 y, theta's d folded in: b[y][2 x + 3 y] = rotl(a[x][y] ^ d[x]), every index a template constant
template <int I>
NCG_DI void keccak_rho_pi_lane(uint64_t (&b)[25], const uint64_t (&a)[25], const uint64_t (&d)[5]) {
  constexpr int X = I % 5, Y = I / 5;
  b[Y + 5 * ((2 * X + 3 * Y) % 5)] = keccak_rotl<KeccakConsts::RHO[I]>(a[I] ^ d[X]);
}
template <int... I>
NCG_DI void keccak_rho_pi(uint64_t (&b)[25], const uint64_t (&a)[25], const uint64_t (&d)[5], std::integer_sequence<int, I...>) {
  (keccak_rho_pi_lane<I>(b, a, d), ...);
}
NCG_DI void keccak_round(uint64_t (&a)[25], uint64_t rc) {
  uint64_t c[5], d[5], b[25];
#pragma unroll
  for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ keccak_rotl<1>(c[(x + 1) % 5]);
  keccak_rho_pi(b, a, d, std::make_integer_sequence<int, 25>{});
#pragma unroll
  for (int y = 0; y < 5; y++) {
#pragma unroll
    for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
  }
  a[0] ^= rc;
}
// The rounds stay a loop (one round is about 155 64-bit operations; 24 copies would be 30 KiB of code in every hash kernel): the
// only thing the round counter indexes is the table of round constants.
NCG_DI void keccak_f1600(uint64_t (&st)[25]) {
#pragma unroll 1
  for (int r = 0; r < 24; r++) keccak_round(st, KeccakConsts::RC[r]);
}

// st[i] ^= v and st[i] for a run-time i below 17: selects over the rate lanes
NCG_DI void keccak_xor_lane(uint64_t (&st)[25], uint32_t i, uint64_t v) {
#pragma unroll
  for (int j = 0; j < SHAKE256_RATE_LANES; j++) st[j] ^= i == (uint32_t)j ? v : 0ull;
}
NCG_DI uint64_t keccak_get_lane(const uint64_t (&st)[25], uint32_t i) {
  uint64_t v = 0;
#pragma unroll
  for (int j = 0; j < SHAKE256_RATE_LANES; j++) v |= i == (uint32_t)j ? st[j] : 0ull;
  return v;
}

// ---- SHAKE256 over a short list of byte segments read one after the other, at any byte alignment (the manner of sha512_segments).
// On return the state has absorbed every segment and the padding and has been permuted: the first 136 bytes of output are its rate
// lanes.  The trip counts depend on the lengths only.
struct KeccakSeg {
  const uint8_t* p;
  uint64_t len;
};
template <int NSEG>
NCG_DI void shake256_absorb(uint64_t (&st)[25], const KeccakSeg (&seg)[NSEG]) {
#pragma unroll
  for (int i = 0; i < 25; i++) st[i] = 0;
  uint64_t end[NSEG];  // end[s]: position after the last byte of segment s
  uint64_t total = 0;
#pragma unroll
  for (int s = 0; s < NSEG; s++) end[s] = total += seg[s].len;
  const uint64_t nblocks = total / SHAKE256_RATE + 1;  // the suffix always fits: at least one byte of the last block is free
  const uint64_t last = nblocks * SHAKE256_RATE - 1;   // 0x80 goes here; 0x1f | 0x80 = 0x9f where the two meet
  for (uint64_t blk = 0; blk < nblocks; blk++) {
#pragma unroll 1
    for (uint32_t i = 0; i < (uint32_t)SHAKE256_RATE_LANES; i++) {
      uint64_t v = 0;
      for (int j = 7; j >= 0; j--) {
        const uint64_t pos = blk * SHAKE256_RATE + (uint64_t)i * 8 + j;
        uint32_t byte = (pos == total ? 0x1fu : 0u) | (pos == last ? 0x80u : 0u);
#pragma unroll
        for (int s = 0; s < NSEG; s++) {
          const uint64_t start = end[s] - seg[s].len;
          if (pos >= start && pos < end[s]) byte = seg[s].p[pos - start];
        }
        v = (v << 8) | byte;
      }
      keccak_xor_lane(st, i, v);
    }
    keccak_f1600(st);
  }
}
// out_len bytes of output, the permutation again after every 136 of them
NCG_DI void shake256_squeeze(uint64_t (&st)[25], uint8_t* __restrict__ out, uint32_t out_len) {
  uint32_t done = 0;
  while (done < out_len) {
    const uint32_t take = out_len - done < (uint32_t)SHAKE256_RATE ? out_len - done : (uint32_t)SHAKE256_RATE;
#pragma unroll 1
    for (uint32_t i = 0; i * 8 < take; i++) {
      const uint64_t v = keccak_get_lane(st, i);
      for (uint32_t j = 0; j < 8 && i * 8 + j < take; j++) out[done + i * 8 + j] = (uint8_t)(v >> (8 * j));
    }
    done += take;
    if (done < out_len) keccak_f1600(st);
  }
}
// the first 4 NW bytes of output as LE words (one block); the bytes from `bytes` on are cleared
template <int NW>
NCG_DI void shake256_words(uint32_t (&x)[NW], const uint64_t (&st)[25], int bytes) {
  static_assert(NW <= 2 * SHAKE256_RATE_LANES, "one block of output");
#pragma unroll
  for (int i = 0; i < NW; i++) {
    const uint32_t w = (uint32_t)(st[i / 2] >> (32 * (i % 2)));
    const int keep = bytes - 4 * i;  // bytes of this word that belong to the output
    x[i] = keep >= 4 ? w : keep <= 0 ? 0u : w & (0xffffffffu >> (32 - 8 * keep));
  }
}

// ---- arithmetic mod n = 2^446 - C, the order of the Ed448 base point (ed448.ts:55-57); C < 2^224 as 7 LE words
struct Ed448Order {
  static constexpr uint32_t C[7] = {0x54a7bb0du, 0xdc873d6du, 0x723a70aau, 0xde933d8du, 0x5129c96fu, 0x3bb124b6u, 0x8335dc16u};
  static constexpr uint32_t N[14] = {0xab5844f3u, 0x2378c292u, 0x8dc58f55u, 0x216cc272u, 0xaed63690u, 0xc44edb49u, 0x7cca23e9u,
                                     0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x3fffffffu};
};
// One fold by 2^446 = C (mod n): r = (t mod 2^446) + (t >> 446) C, where t >> 446 fits NH words.  The value is unchanged mod n and
// never negative; r has max(NH + 7, 14) words, which the bounds listed at mod_n_912 show to be enough.
template <int NI, int NH>
NCG_DI void ed448_fold(uint32_t (&r)[(NH + 7 > 14 ? NH + 7 : 14)], const uint32_t (&t)[NI]) {
  constexpr int NO = NH + 7 > 14 ? NH + 7 : 14;
  uint32_t hi[NH], c[7], prod[NH + 7];
#pragma unroll
  for (int i = 0; i < 7; i++) c[i] = Ed448Order::C[i];
#pragma unroll
  for (int i = 0; i < NH; i++) hi[i] = (t[13 + i] >> 30) | (14 + i < NI ? t[14 + i] << 2 : 0u);
  mp_mul<NH, 7>(prod, hi, c);
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < NO; i++) {
    const uint32_t lo = i < 13 ? t[i] : i == 13 ? t[13] & 0x3fffffffu : 0u;
    r[i] = __builtin_addc(lo, i < NH + 7 ? prod[i] : 0u, carry, &carry);
  }
}
// k = x mod n for any x below 2^912 (29 LE words, the top one below 2^16), canonical.  Four folds and one subtraction, the same
// instructions for every value:
//   x < 2^912:  hi < 2^466 (15 words)  ->  t < 2^446 + 2^690 < 2^691 (22 words)
//   t < 2^691:  hi < 2^245 (8 words)   ->  u < 2^446 + 2^469 < 2^470 (15 words)
//   u < 2^470:  hi < 2^24  (1 word)    ->  v < 2^446 + 2^248 < 2^447 (14 words)
//   v < 2^447:  hi <= 1                ->  w < 2^446 + 2^224 < 2 n:  w - n where that is not negative
NCG_DI void mod_n_912(uint32_t (&k)[14], const uint32_t (&x)[29]) {
  uint32_t t[22], u[15], v[14], w[14], d[14], n[14];
  ed448_fold<29, 15>(t, x);
  ed448_fold<22, 8>(u, t);
  ed448_fold<15, 1>(v, u);
  ed448_fold<14, 1>(w, v);
#pragma unroll
  for (int i = 0; i < 14; i++) n[i] = Ed448Order::N[i];
  const uint32_t below = mp_sub<14>(d, w, n);  // the borrow: w < n
#pragma unroll
  for (int i = 0; i < 14; i++) k[i] = below ? w[i] : d[i];
}
// (r + k s) mod n for r, k, s below n: k s < 2^892, the sum below 2^893
NCG_DI void ed448_muladd_mod_n(uint32_t (&out)[14], const uint32_t (&r)[14], const uint32_t (&k)[14], const uint32_t (&s)[14]) {
  uint32_t prod[28], x[29];
  mp_mul<14, 14>(prod, k, s);
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 28; i++) x[i] = __builtin_addc(prod[i], i < 14 ? r[i] : 0u, carry, &carry);
  x[28] = carry;
  mod_n_912(out, x);
}

}  // namespace ncg
