// Field inversion for the plain (non-Montgomery) Fe9 primes by division steps (Bernstein - Yang, "Fast constant-time gcd
// computation and modular inversion", 2019; the half-delta variant with zeta = -(delta + 1/2)).  Included by fe9.hpp.
//
//   divstep(delta, f, g) = (1 - delta, g, (g - f) / 2)          if delta > 0 and g is odd
//                          (1 + delta, f, (g + (g mod 2) f) / 2) otherwise
// started at (f, g) = (p, x).  f stays odd, gcd(f, g) is kept, and g reaches 0 with f = +-1 (x != 0) or f = p (x = 0).  Beside
// (f, g) run (d, e) with d * x = f and e * x = g (mod p), started at (0, 1): at the end d = +-1 / x.
//
// Form: f, g, d, e in 9 SIGNED limbs of 30 bits (limbs 0..7 in [0, 2^30), the sign in limb 8).  One batch is N = 30 steps on the
// low limbs of f and g alone - a step reads one bit of g and the sign of zeta - and yields a 2 x 2 integer matrix t with
//   2^30 (f', g') = t (f, g),   |u| + |v| <= 2^30, |q| + |r| <= 2^30   for t = (u v; q r),
// which is then applied to the full (f, g), exactly divisible by 2^30, and to (d, e) modulo p: a multiple of p, found from
// p^-1 mod 2^30 (PR::PINV30), clears the low limb before the shift, and d, e stay in (-2p, p).  p = 2^k - c in signed limbs has
// three non-zero limbs (PR::P30), so that multiple costs three multiply-adds per row.
//
// The 30 steps run as three groups of 10 with the matrix row PACKED, u + 2^16 v in one register: a step is linear in (u, v), the
// packed word follows it modulo 2^32, and after 10 steps |u|, |v| <= 2^10, so both come back by sign extension.  The three small
// matrices multiply up with 24-bit products.  Per step: 19 plain 32-bit instructions, selects only - every lane does the same
// work.  Per batch: 72 signed 64-bit multiply-adds (v_mad_i64_i32, four to an asm block) and the few of the multiple of p.
//
// End: after each batch, stop when no lane of the wave has g != 0.  Steps taken with g = 0 leave f alone and d congruent (the
// matrix is (2^30 0; 0 1)), so lanes that finish early just wait.  No step bound enters the result: the loop is capped at
// FE9_DS_CAP batches (600 steps; 590 are known to suffice for inputs below 2^256) and a lane that still has g != 0 there
// takes the Fermat chain (f_inv_fermat).
#pragma once

namespace ncg {

constexpr uint32_t FE9_M30 = (1u << 30) - 1u;
constexpr int FE9_DS_CAP = 20;

// true if `c` holds in any active lane of the wave (host twin: one lane)
NCG_DI bool fe9_wave_any(bool c) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_ballot_w64(c) != 0;
#else
  return c;
#endif
}
// keeps the scheduler from interleaving the phases of a batch (the step groups, the matrix on (d, e), the matrix on (f, g)): mixed,
// their temporaries are live together and the calling kernels pay in registers
NCG_DI void fe9_ds_fence() {
#ifdef __HIP_DEVICE_COMPILE__
  __builtin_amdgcn_sched_barrier(0);
#endif
}
// a * b for operands below 2^23 in magnitude
NCG_DI int32_t fe9_mul24(int32_t a, int32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __mul24(a, b);
#else
  return a * b;
#endif
}

struct Fe9DsMat {
  int32_t u, v, q, r;
};

// 10 division steps on the low words f, g (at least 10 valid low bits each); the other bits of f, g stay those of the true values
// shifted along, so three calls in a row consume 30 valid bits
NCG_DI Fe9DsMat fe9_divsteps10(int32_t& zeta, uint32_t& f, uint32_t& g) {
  uint32_t uv = 1u, qr = 1u << 16;  // (u, v) = (1, 0), (q, r) = (0, 1)
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t c1 = (uint32_t)(zeta >> 31);  // all ones: delta > 0
    const uint32_t c2 = 0u - (g & 1u);           // all ones: g odd
    const uint32_t x = (f ^ c1) - c1, y = (uv ^ c1) - c1;  // -f, -(u, v) if delta > 0
    g += x & c2;
    qr += y & c2;
    const uint32_t c3 = c1 & c2;                 // swap
    zeta = (int32_t)(((uint32_t)zeta ^ c3) - 1u);  // -zeta - 2 on a swap, zeta - 1 otherwise
    f += g & c3;
    uv += qr & c3;
    g >>= 1;
    uv <<= 1;
  }
  Fe9DsMat m;
  m.u = (int32_t)(int16_t)(uint16_t)uv;
  m.v = (int32_t)(uv - (uint32_t)m.u) >> 16;
  m.q = (int32_t)(int16_t)(uint16_t)qr;
  m.r = (int32_t)(qr - (uint32_t)m.q) >> 16;
  return m;
}
// b * a (a applied first).  Used twice: 10 steps times 10 steps (|b.u| + |b.v| <= 2^10, |a| <= 2^10 per entry) and 10 steps times 20
// steps (|a| <= 2^20): every operand fits 24 bits, and a row of the product is bounded by (|b.u| + |b.v|) max|a| <= 2^30 - reached
// exactly by the g = 0 matrix (2^30 0; 0 1) - so the int32 sums of the host twin cannot overflow
NCG_DI Fe9DsMat fe9_ds_matmul(const Fe9DsMat& b, const Fe9DsMat& a) {
  Fe9DsMat m;
  m.u = fe9_mul24(b.u, a.u) + fe9_mul24(b.v, a.q);
  m.v = fe9_mul24(b.u, a.v) + fe9_mul24(b.v, a.r);
  m.q = fe9_mul24(b.q, a.u) + fe9_mul24(b.r, a.q);
  m.r = fe9_mul24(b.q, a.v) + fe9_mul24(b.r, a.r);
  return m;
}

// c0 += u x + v y, c1 += q x + r y: one row of a matrix applied to one limb pair, four signed 32 x 32 + 64 multiply-adds as ONE asm
// block (fe9_blk's rule; left to the compiler, the masked limbs - two known zero top bits - turn some of the products into
// unsigned multiplies with sign fix-ups)
NCG_DI void fe9_smac4(int64_t& c0, int64_t& c1, const Fe9DsMat& t, int32_t x, int32_t y) {
#ifdef __HIP_DEVICE_COMPILE__
  asm("v_mad_i64_i32 %0, vcc, %2, %6, %0\n\t"
      "v_mad_i64_i32 %1, vcc, %4, %6, %1\n\t"
      "v_mad_i64_i32 %0, vcc, %3, %7, %0\n\t"
      "v_mad_i64_i32 %1, vcc, %5, %7, %1"
      : "+v"(c0), "+v"(c1)
      : "v"(t.u), "v"(t.v), "v"(t.q), "v"(t.r), "v"(x), "v"(y)
      : "vcc");
#else
  c0 += (int64_t)t.u * x + (int64_t)t.v * y;
  c1 += (int64_t)t.q * x + (int64_t)t.r * y;
#endif
}

// (f, g) <- t (f, g) / 2^30, exact
NCG_DI void fe9_ds_update_fg(int32_t (&f)[9], int32_t (&g)[9], const Fe9DsMat& t) {
  int64_t cf = 0, cg = 0;
  fe9_smac4(cf, cg, t, f[0], g[0]);
  cf >>= 30;  // the low 30 bits are zero
  cg >>= 30;
#pragma unroll
  for (int i = 1; i < 9; i++) {
    fe9_smac4(cf, cg, t, f[i], g[i]);
    f[i - 1] = (int32_t)((uint32_t)cf & FE9_M30);
    g[i - 1] = (int32_t)((uint32_t)cg & FE9_M30);
    cf >>= 30;
    cg >>= 30;
  }
  f[8] = (int32_t)cf;
  g[8] = (int32_t)cg;
}
// (d, e) <- t (d, e) / 2^30 mod p, d and e in (-2p, p) before and after
template <class PR>
NCG_DI void fe9_ds_update_de(int32_t (&d)[9], int32_t (&e)[9], const Fe9DsMat& t) {
  // a negative d or e first gets p added (times its matrix entry): the sums below then lie in (-2^30 p, 2^30 p) up to md p
  const int32_t sd = d[8] >> 31, se = e[8] >> 31;
  int32_t md = (t.u & sd) + (t.v & se), me = (t.q & sd) + (t.r & se);
  int64_t cd = 0, ce = 0;
  fe9_smac4(cd, ce, t, d[0], e[0]);
  // md, me -= the multiple of p that leaves the low limb of t (d, e) + p (md, me) zero
  md -= (int32_t)((PR::PINV30 * (uint32_t)cd + (uint32_t)md) & FE9_M30);
  me -= (int32_t)((PR::PINV30 * (uint32_t)ce + (uint32_t)me) & FE9_M30);
  cd += (int64_t)PR::P30[0] * md;
  ce += (int64_t)PR::P30[0] * me;
  cd >>= 30;
  ce >>= 30;
#pragma unroll
  for (int i = 1; i < 9; i++) {
    fe9_smac4(cd, ce, t, d[i], e[i]);
    if (PR::P30[i] != 0) {
      cd += (int64_t)PR::P30[i] * md;
      ce += (int64_t)PR::P30[i] * me;
    }
    d[i - 1] = (int32_t)((uint32_t)cd & FE9_M30);
    e[i - 1] = (int32_t)((uint32_t)ce & FE9_M30);
    cd >>= 30;
    ce >>= 30;
  }
  d[8] = (int32_t)cd;
  e[8] = (int32_t)ce;
}

// one batch: 30 division steps and their matrix applied to (f, g) and (d, e)
template <class PR>
NCG_DI void fe9_ds_batch(int32_t& zeta, int32_t (&f)[9], int32_t (&g)[9], int32_t (&d)[9], int32_t (&e)[9]) {
  uint32_t f0 = (uint32_t)f[0], g0 = (uint32_t)g[0];
  const Fe9DsMat m1 = fe9_divsteps10(zeta, f0, g0);
  const Fe9DsMat m2 = fe9_divsteps10(zeta, f0, g0);
  const Fe9DsMat m3 = fe9_divsteps10(zeta, f0, g0);
  const Fe9DsMat t = fe9_ds_matmul(m3, fe9_ds_matmul(m2, m1));
  fe9_ds_fence();
  fe9_ds_update_de<PR>(d, e, t);
  fe9_ds_fence();
  fe9_ds_update_fg(f, g, t);
  fe9_ds_fence();
}

// 1 / a (value of modular.ts:159-182 invert; 0 -> 0), the canonical residue in canonical limbs.  FIXED: always FE9_DS_CAP batches, no
// early exit - for a secret input (ed25519_sign.hpp), so that the batch count does not follow the value; steps taken with g = 0 change
// nothing, so the result is the same
template <class PR, int A, bool FIXED = false>
NCG_DI Fe9<PR, 1> fe9_inv_divsteps(const Fe9<PR, A>& a_in) {
  uint32_t c[10];
  {
    uint32_t cc[9];
    fe9_canon_limbs<PR, A>(cc, a_in);
#pragma unroll
    for (int i = 0; i < 9; i++) c[i] = cc[i];
    c[9] = 0;
  }
  int32_t f[9], g[9], d[9], e[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {  // 29-bit limbs -> 30-bit limbs
    const int bit = 30 * i, limb = bit / 29, sh = bit % 29;
    const uint64_t two = ((uint64_t)c[limb + 1] << 29) | c[limb];
    g[i] = (int32_t)((uint32_t)(two >> sh) & FE9_M30);
    f[i] = PR::P30[i];
    d[i] = 0;
    e[i] = 0;
  }
  e[0] = 1;
  int32_t zeta = -1;
  uint32_t gnz = 1;
#pragma unroll 1
  for (int it = 0; it < FE9_DS_CAP; it++) {
    fe9_ds_batch<PR>(zeta, f, g, d, e);
    gnz = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) gnz |= (uint32_t)g[i];
    if constexpr (!FIXED) {
      if (!fe9_wave_any(gnz != 0)) break;
    }
  }
  if (gnz != 0) return f_inv_fermat(a_in);  // the cap's way out (never reached by an input below 2^256)
  // f = +-1 (or p for x = 0): the inverse is d times the sign of f.  2p + (+-d) lies in (0, 4p): carry it into unsigned limbs
  const int32_t s = f[8] >> 31;
  uint32_t w[10];
  int32_t cy = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int32_t t = ((d[i] ^ s) - s) + 2 * PR::P30[i] + cy;
    w[i] = (uint32_t)t & FE9_M30;
    cy = t >> 30;
    if (i == 8) w[i] = (uint32_t)t;  // below 2^18, no sign left
  }
  w[9] = 0;
  Fe9<PR, 1> r;
#pragma unroll
  for (int i = 0; i < 9; i++) {  // 30-bit limbs -> 29-bit limbs
    const int bit = 29 * i, limb = bit / 30, sh = bit % 30;
    const uint64_t two = ((uint64_t)w[limb + 1] << 30) | w[limb];
    r.v[i] = (uint32_t)(two >> sh) & FE9_MASK;
  }
  uint32_t o[9];
  fe9_canon_limbs<PR, 1>(o, r);
  return Fe9<PR, 1>::from_limbs(o);
}

}  // namespace ncg
