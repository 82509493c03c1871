// The scalar field of secp256k1 (arithmetic modulo the group order n) and the byte helpers of the signature code: shared by
// ecdsa.hip (verification, recovery) and secp256k1_sign.hpp (signing).
#pragma once
#include "fp.hpp"
#include "scalar.hpp"

namespace ncg {

// Montgomery constants of the group order n (R = 2^256): python -c "n=0xFFFF...4141; R=1<<256; print(-pow(n,-1,2**32) % 2**32, R % n, R*R % n)"
struct ParamsSecpN {
  static constexpr int N = 8;
  static constexpr uint32_t P[8] = {0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  static constexpr uint32_t INV = 0x5588b13fu;  // -n^-1 mod 2^32
  static constexpr uint32_t R1[8] = {0x2fc9bebfu, 0x402da173u, 0x50b75fc4u, 0x45512319u, 0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u};
  static constexpr uint32_t R2[8] = {0x67d7d140u, 0x896cf214u, 0x0e7cf878u, 0x741496c2u, 0x5bcd07c6u, 0xe697f5e4u, 0x81c69bc5u, 0x9d671cd5u};
  static constexpr bool TOP_SPARE = false;  // n > 2^255: the product keeps its carry word (fp_mul_fips_asm / fp_mul_body)
  static constexpr bool FOLD = false;
  static constexpr uint32_t HALF[8] = {0x681b20a0u, 0xdfe92f46u, 0x57a4501du, 0x5d576e73u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu};  // n >> 1
};
using Fn = Fp<ParamsSecpN>;

NCG_DI Fn fn_from_words(const uint32_t (&w)[8]) {
  Fn r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = w[i];
  return r;
}
// a^(n-2), a != 0 (Montgomery form in and out): 4-bit windows over the exponent, 252 squarings + <= 78 products
NCG_DI Fn fn_inv(const Fn& a) {
  Fn tab[16];
  tab[0] = Fn::one();
  tab[1] = a;
  for (int j = 2; j < 16; j++) tab[j] = tab[j - 1] * a;
  uint32_t e[8];
#pragma unroll
  for (int i = 0; i < 8; i++) e[i] = ParamsSecpN::P[i];
  e[0] -= 2u;  // n - 2 (no borrow: the low limb is 0xd0364141)
  Fn acc = tab[e[7] >> 28];
  for (int w = 62; w >= 0; w--) {
    for (int s = 0; s < 4; s++) acc = fp_sqr<ParamsSecpN>(acc);
    const uint32_t dg = (e[w >> 3] >> ((w & 7) * 4)) & 15u;
    if (dg) acc = acc * tab[dg];
  }
  return acc;
}

NCG_DI void be32_to_words(uint32_t (&w)[8], const uint8_t* __restrict__ p) {  // 32 big-endian bytes -> 8 LE limbs
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = p + 4 * (7 - i);
    w[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
}
NCG_DI bool words_lt(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t d[8];
  return mp_sub<8>(d, a, b) != 0;
}

struct Bip340Tag {  // SHA-256("BIP0340/challenge")
  static constexpr uint8_t H[32] = {0x7b, 0xb5, 0x2d, 0x7a, 0x9f, 0xef, 0x58, 0x32, 0x3e, 0xb1, 0xbf, 0x7a, 0x40, 0x7d, 0xb3, 0x82,
                                    0xd2, 0xf3, 0xf2, 0xd8, 0x1b, 0xb1, 0x22, 0x4f, 0x49, 0xfe, 0x51, 0x8f, 0x6d, 0x48, 0xd3, 0x7c};
};
struct Bip340AuxTag {  // SHA-256("BIP0340/aux")
  static constexpr uint8_t H[32] = {0xf1, 0xef, 0x4e, 0x5e, 0xc0, 0x63, 0xca, 0xda, 0x6d, 0x94, 0xca, 0xfa, 0x9d, 0x98, 0x7e, 0xa0,
                                    0x69, 0x26, 0x58, 0x39, 0xec, 0xc1, 0x1f, 0x97, 0x2d, 0x77, 0xa5, 0x2e, 0xd8, 0xc1, 0xcc, 0x90};
};
struct Bip340NonceTag {  // SHA-256("BIP0340/nonce")
  static constexpr uint8_t H[32] = {0x07, 0x49, 0x77, 0x34, 0xa7, 0x9b, 0xcb, 0x35, 0x5b, 0x9b, 0x8c, 0x7d, 0x03, 0x4f, 0x12, 0x1c,
                                    0xf4, 0x34, 0xd7, 0x3e, 0xf7, 0x2d, 0xda, 0x19, 0x87, 0x00, 0x61, 0xfb, 0x52, 0xbf, 0xeb, 0x2f};
};

}  // namespace ncg
