// Self-check of fr29.hpp (the NTT butterflies' form of bls12-381 Fr, F = Fr29Bls, or bn254 Fr, F = Fr29Bn) on RAW limbs, shared
// by the device (ncg_field_check field 8, selfcheck.hip) and the host twin (hosttest.hip ht_fr29_op / ht_fr29_field_op).
// a, b, r: 9 words, so that the tests check the output limbs as well as the value; b may be null (read as zero).
//   op 0 mont(a, b)   1 a + b   2 a + 3 r - b   3 weak(a)   4 reduce256(a)   5 cond_sub(a)   6 from_words(a[0..8))
//   op 7 to_words(a) (8 words, then 0)   8 one fold (fr29_fold255)
// -1, and nothing written, for any other op.
#pragma once
#include "fr29.hpp"

namespace ncg {

template <class F>
NCG_DI int fr29_check(int op, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  Fr29 x, y, z;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    x.v[i] = a[i];
    y.v[i] = b ? b[i] : 0;
    z.v[i] = 0;
  }
  switch (op) {
    case 0: z = fr29_mont<F>(x, y); break;
    case 1: z = fr29_add(x, y); break;
    case 2: z = fr29_sub<F>(x, y); break;
    case 3: z = fr29_weak(x); break;
    case 4: z = fr29_reduce256<F>(x); break;
    case 5: z = fr29_cond_sub<F>(x); break;
    case 8: z = fr29_fold255<F>(x); break;
    case 6: {
      uint32_t w[8];
#pragma unroll
      for (int i = 0; i < 8; i++) w[i] = a[i];
      z = fr29_from_words(w);
      break;
    }
    case 7: {
      uint32_t w[8];
      fr29_to_words(w, x);
#pragma unroll
      for (int i = 0; i < 8; i++) z.v[i] = w[i];
      break;
    }
    default: return -1;
  }
#pragma unroll
  for (int i = 0; i < 9; i++) r[i] = z.v[i];
  return 0;
}

}  // namespace ncg
