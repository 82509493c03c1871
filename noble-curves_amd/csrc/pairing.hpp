// The optimal ate pairing of bls12-381 per lane (pair): input checks, Miller loop, final exponentiation.
// Values of the reference's pairingBatch (src/abstract/bls.ts:575-693) and Fp12finalExponentiate (src/bls12-381.ts:258-276),
// templated on the Fp2 form like fp12.hpp.
#pragma once
#include "fp12.hpp"

namespace ncg {

// why a pair is refused, in the order the reference meets the cases (bls.ts:685-688, weierstrass.ts:748-766)
enum PairingBad : uint32_t {
  PAIRING_OK = 0,
  PAIRING_BAD_ZERO = 1,        // "pairing is not available for ZERO point"
  PAIRING_BAD_G1 = 2,          // g1.assertValidity: coordinate >= p or not on the curve
  PAIRING_BAD_G1_SUBGROUP = 3,  // under the flag: "bad point: not in prime-order subgroup"
  PAIRING_BAD_G2 = 4,
  PAIRING_BAD_G2_SUBGROUP = 5,
};

// NAfDecomposition(|x|) (bls.ts:414-425), most significant digit first: digit of bit b in {-1, 0, 1}, b = 63 .. 0,
// under the marker bit 2^64 the loop starts from
struct AteNaf {
  int8_t d[64];
};
constexpr AteNaf make_ate_naf() {
  AteNaf n{};
  unsigned __int128 a = 0xD201000000010000ull;
  int b = 0;
  for (; a > 1; a >>= 1, b++) {
    if ((a & 1) == 0) n.d[b] = 0;
    else if ((a & 3) == 3) {
      n.d[b] = -1;
      a += 1;
    } else n.d[b] = 1;
  }
  return n;  // b == 64 here
}

// isTorsionFree of the reference for a G1 point (bls12-381.ts:567-577): [x^2] P == phi(P) = (beta x, y), the test of g1_decode_lane
NCG_DI bool pairing_g1_in_subgroup(const Fe29<2>& x, const Fe29<2>& y) {
  using F = FeBls;
  const Jac<F> P{x, y, F::one()};
  const Jac<F> xP = jac_neg(bls_mul_by_x(P));
  const Jac<F> u2P = bls_mul_by_x(xP);
  const Fe29<1> beta = fe29_const(ParamsBls29::G1_BETA);
  const auto zz = f_sqr(u2P.Z);
  return !f_eqz(u2P.Z) && f_eq(u2P.X, x * beta * zz) && f_eq(u2P.Y, y * zz * u2P.Z);
}
// ... and for a G2 point (bls12-381.ts:599-601): -[|x|] P == psi(P), the test of the G2 decoder, in either Fp2 form (pair-uniform)
template <template <int> class F2>
NCG_DI bool pairing_g2_in_subgroup(const F2<64>& x, const F2<64>& y) {
  using F = F2<64>;
  const Jac<F> P{x, y, F::one()};
  const Jac<F> xP = jac_neg(bls_mul_by_x(P));
  const auto psx = F2Form<F2>::konst(ParamsBls29::PSI_X_C0, ParamsBls29::PSI_X_C1);
  const auto psy = F2Form<F2>::konst(ParamsBls29::PSI_Y_C0, ParamsBls29::PSI_Y_C1);
  const auto px = f2_conj(x) * psx, py = f2_conj(y) * psy;
  const auto zz = f_sqr(xP.Z);
  const auto dx = xP.X - px * zz;
  const auto dy = xP.Y - py * zz * xP.Z;
  return !f_eqz(xP.Z) && f_eqz(dx) && f_eqz(dy);
}

template <template <int> class F2>
struct Pairing {
  using T = Tower<F2>;
  using E2 = typename T::E2;
  using E12 = typename T::E12;

  // Fp2.mulByB (bls12-381.ts:252-257): 4 (u + 1) a
  template <int A> static NCG_DI auto mul_by_b(const F2<A>& a) { return f_dbl(f_dbl(f2_mul_nr(a))); }

  // pointDouble (bls.ts:575-592): the line (c0, c1, c2) at R and R <- 2 R
  static NCG_DI void point_double(E2& Rx, E2& Ry, E2& Rz, E2& c0, E2& c1, E2& c2) {
    const Fe29<1> half = fe29_const(ParamsBls29::HALF);
    const auto t0 = f_sqr(Ry), t1 = f_sqr(Rz);
    const auto t2 = mul_by_b(f_x3(t1));
    const auto t3 = f_x3(t2);
    const auto t4 = (f_sqr(Ry + Rz) - t1) - t0;
    c0 = f2_fit<TOWER_B>(t2 - t0);
    c1 = f2_fit<TOWER_B>(f_x3(f_sqr(Rx)));
    c2 = f2_fit<TOWER_B>(f_neg(t4));
    const auto nx = f2_mul_fp(((t0 - t3) * Rx) * Ry, half);
    const auto ny = f_sqr(f2_mul_fp(t0 + t3, half)) - f_x3(f_sqr(t2));
    const auto nz = t0 * t4;
    Rx = f2_fit<TOWER_B>(nx);
    Ry = f2_fit<TOWER_B>(ny);
    Rz = f2_fit<TOWER_B>(nz);
  }
  // pointAdd (bls.ts:593-612): the line through R and Q and R <- R + Q
  static NCG_DI void point_add(E2& Rx, E2& Ry, E2& Rz, const E2& Qx, const E2& Qy, E2& c0, E2& c1, E2& c2) {
    const auto t0 = Ry - Qy * Rz;
    const auto t1 = Rx - Qx * Rz;
    c0 = f2_fit<TOWER_B>(t0 * Qx - t1 * Qy);
    c1 = f2_fit<TOWER_B>(f_neg(t0));
    c2 = f2_fit<TOWER_B>(t1);
    const auto t2 = f_sqr(t1);
    const auto t3 = t2 * t1;
    const auto t4 = t2 * Rx;
    const auto t5 = (t3 - f_dbl(t4)) + f_sqr(t0) * Rz;
    const auto nx = t1 * t5;
    const auto ny = (t4 - t5) * t0 - t3 * Ry;
    const auto nz = Rz * t3;
    Rx = f2_fit<TOWER_B>(nx);
    Ry = f2_fit<TOWER_B>(ny);
    Rz = f2_fit<TOWER_B>(nz);
  }
  // lineFunction of the multiplicative twist (bls.ts:564-566): f <- f * (c0 + c1 Px v + c2 Py v w)
  static NCG_DI void line(E12& f, const E2& c0, const E2& c1, const E2& c2, const Fe29<2>& Px, const Fe29<2>& Py) {
    const E2 o1 = E2(f2_mul_fp(c1, Px)), o4 = E2(f2_mul_fp(c2, Py));
    T::mul014(f, f, c0, o1, o4);
  }
  // millerLoopBatch for one pair (bls.ts:620-666): the loop stays rolled, the addition step is predicated on the constant
  // NAF digit (the same for every lane), the result is conjugated because x is negative
  static NCG_TOWERFN void miller_loop(E12& f, const Fe29<2>& Px, const Fe29<2>& Py, const E2& Qx, const E2& Qy) {
    constexpr AteNaf NAF = make_ate_naf();
    const E2 nQy = E2(f_neg(Qy));
    E2 Rx = Qx, Ry = Qy, Rz = E2::one();
    E2 c0, c1, c2;
    f = E12::one();
    for (int b = 63; b >= 0; b--) {
      if (b != 63) T::sqr(f, f);  // sqr(ONE) skipped at the first step
      point_double(Rx, Ry, Rz, c0, c1, c2);
      line(f, c0, c1, c2, Px, Py);
      const int d = NAF.d[b];
      if (d != 0) {
        point_add(Rx, Ry, Rz, Qx, d < 0 ? nQy : Qy, c0, c1, c2);
        line(f, c0, c1, c2, Px, Py);
      }
    }
    T::conj(f, f);
  }

  // The checks of pairingBatch on one pair of affine wire points (24 + 48 words): both non-zero (bls.ts:685), then
  // assertValidity of each (weierstrass.ts:748-766): coordinates below p, on the curve and - with `subgroup` - torsion-free.  Pair-uniform in the paired form.
  static NCG_DI uint32_t load_checked(const uint32_t* g1, const uint32_t* g2, bool subgroup, Fe29<2>& Px, Fe29<2>& Py, E2& Qx, E2& Qy) {
    uint32_t any1 = 0, any2 = 0;
    bool canon1 = true, canon2 = true;
    for (int k = 0; k < 2; k++) {
      uint32_t w[12];
#pragma unroll
      for (int i = 0; i < 12; i++) {
        w[i] = g1[12 * k + i];
        any1 |= w[i];
      }
      canon1 = canon1 && words12_lt_p(w);
    }
    for (int k = 0; k < 4; k++) {
      uint32_t w[12];
#pragma unroll
      for (int i = 0; i < 12; i++) {
        w[i] = g2[12 * k + i];
        any2 |= w[i];
      }
      canon2 = canon2 && words12_lt_p(w);
    }
    Px = fe29_from_wire(g1);
    Py = fe29_from_wire(g1 + 12);
    Qx = T::load2_wire(g2);
    Qy = T::load2_wire(g2 + 24);
    if (any1 == 0 || any2 == 0) return PAIRING_BAD_ZERO;
    const Fe29<1> four = fe29_const(ParamsBls29::FOUR);
    const bool on1 = f_eqz(f_sqr(Py) - (f_sqr(Px) * Px + four));  // y^2 = x^3 + 4
    if (!canon1 || !on1) return PAIRING_BAD_G1;
    if (subgroup && !pairing_g1_in_subgroup(Px, Py)) return PAIRING_BAD_G1_SUBGROUP;  // g1.assertValidity ends before g2's begins
    const auto b2 = f2_mul_nr(f2_mul_fp(F2<1>::one(), four));      // 4 (u + 1)
    const bool on2 = f_eqz(f_sqr(Qy) - (f_sqr(Qx) * Qx + b2));
    if (!canon2 || !on2) return PAIRING_BAD_G2;
    if (subgroup && !pairing_g2_in_subgroup<F2>(F2<64>(FieldWire<F2<64>>::load(g2)), F2<64>(FieldWire<F2<64>>::load(g2 + 24))))
      return PAIRING_BAD_G2_SUBGROUP;
    return PAIRING_OK;
  }
};

}  // namespace ncg
