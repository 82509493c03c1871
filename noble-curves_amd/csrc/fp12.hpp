// Fp6 = Fp2[v]/(v^3 - (u + 1)) and Fp12 = Fp6[w]/(w^2 - v) over the bls12-381 Fp2 of fe29.hpp, templated on the Fp2
// form: the kernels instantiate the lane-paired Fe29x2P (one tower element per lane PAIR, 6 Fp = 84 registers per lane
// for an Fp12), the host twin the unpaired Fe29x2.  Values of the reference's _Field6 / _Field12 ops
// (src/abstract/tower.ts:563-1092) and of mul014ByLine (src/abstract/bls.ts:476-519).
//
// Bounds: like Fe29<B>, a tower element carries the compile-time bound of its coefficients.  Every formula is written
// with `auto`, so the bound of a result follows from the operators; a value kept across a loop or handed to an
// out-of-line routine has the storage bound TOWER_B and tower_fit() brings a result there - for free when its bound is
// below TOWER_B already (every product, square, inverse and Frobenius map), by conditional subtractions of 2^k p
// otherwise (the cyclotomic square, whose result 3 t - 2 c carries twice the bound of its input c).
#pragma once
#include <type_traits>

#include "bls_lanes.hpp"

namespace ncg {

constexpr int tower_max(int a, int b) { return a > b ? a : b; }
constexpr int TOWER_B = 256;  // Fp12 sqr on inputs below 256 p: largest operand sum 3072 p (bound types end at 4096 p)
#define NCG_TOWERFN __host__ __device__ __noinline__

// ---- conditional subtraction of 2^K p: a value below 2^(K+1) p comes below 2^K p (no product)
template <int K, int A>
NCG_DI Fe29<(1 << K)> fe29_csub(const Fe29<A>& a) {
  static_assert(A <= (2 << K), "fe29_csub: value not below 2^(K+1) p");
  constexpr uint32_t MASK = (1u << 29) - 1u;
  uint32_t s[14];
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 13; i++) {
    int32_t d = (int32_t)a.v[i] - (int32_t)ParamsBls29::PMUL[K][i] + c;
    s[i] = (uint32_t)d & MASK;
    c = d >> 29;
  }
  const int32_t top = (int32_t)a.v[13] - (int32_t)ParamsBls29::PMUL[K][13] + c;
  s[13] = (uint32_t)top;
  Fe29<(1 << K)> r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.v[i] = top < 0 ? a.v[i] : s[i];
  return r;
}
// Fe29<A> -> Fe29<T>: a widening when A <= T, ceil(log2(A / T)) conditional subtractions otherwise (T a power of two)
template <int T, int A>
NCG_DI Fe29<T> fe29_fit(const Fe29<A>& a) {
  static_assert((T & (T - 1)) == 0, "fe29_fit: target bound must be a power of two");
  if constexpr (A <= T) {
    return Fe29<T>(a);
  } else {
    constexpr int K = fe29_pow2ceil_log(A) - 1;  // 2^K < A <= 2^(K+1)
    return fe29_fit<T>(fe29_csub<K>(a));
  }
}
template <int T, int A> NCG_DI Fe29x2<T> f2_fit(const Fe29x2<A>& a) { return {fe29_fit<T>(a.c0), fe29_fit<T>(a.c1)}; }
template <int T, int A> NCG_DI Fe29x2P<T> f2_fit(const Fe29x2P<A>& a) { return Fe29x2P<T>(fe29_fit<T>(a.h)); }

// ---- Fp2 pieces the tower needs, in both forms
// (u + 1) a = (c0 - c1) + (c0 + c1) u   (tower.ts:543-547)
template <int A>
NCG_DI auto f2_mul_nr(const Fe29x2<A>& a) {
  constexpr int R = A + (1 << fe29_pow2ceil_log(A));
  return Fe29x2<R>(Fe29<R>(a.c0 - a.c1), Fe29<R>(a.c0 + a.c1));
}
template <int A>
NCG_DI auto f2_mul_nr(const Fe29x2P<A>& a) {
  constexpr int R = A + (1 << fe29_pow2ceil_log(A));
  // even lane c0 + (-c1), odd lane c1 + c0: the odd lane hands over its half negated, so both lanes ADD what arrives.
  // (Subtracting the swapped half directly, a.h - pair_swap(a.h), came out wrong on gfx950 in the lowest limb of the even lane
  // wherever the difference fed another subtraction - the Fp6 inverse - while the same value was right elsewhere.)
  const bool odd = pair_odd();
  const Fe29<R - A> give = fe29_select(odd, f_neg(a.h), Fe29<R - A>(a.h));
  return Fe29x2P<R>(a.h + pair_swap(give));
}
// c0 - c1 u: Fp2.frobeniusMap with an odd power (tower.ts:556-560)
template <int A>
NCG_DI auto f2_conj(const Fe29x2<A>& a) {
  constexpr int K = 1 << fe29_pow2ceil_log(A);
  return Fe29x2<K>(Fe29<K>(a.c0), f_neg(a.c1));
}
template <int A>
NCG_DI auto f2_conj(const Fe29x2P<A>& a) {
  constexpr int K = 1 << fe29_pow2ceil_log(A);
  return Fe29x2P<K>(fe29_select(pair_odd(), f_neg(a.h), Fe29<K>(a.h)));
}
template <int A, int B> NCG_DI Fe29x2<2> f2_mul_fp(const Fe29x2<A>& a, const Fe29<B>& s) { return {a.c0 * s, a.c1 * s}; }
template <int A, int B> NCG_DI Fe29x2P<2> f2_mul_fp(const Fe29x2P<A>& a, const Fe29<B>& s) { return Fe29x2P<2>(a.h * s); }
template <class T> NCG_DI auto f_x3(const T& a) { return f_dbl(a) + a; }
// constants and the is-it-one test per form
template <template <int> class F2> struct F2Form;
template <> struct F2Form<Fe29x2> {
  static NCG_DI Fe29x2<1> konst(const uint32_t (&c0)[14], const uint32_t (&c1)[14]) { return {fe29_const(c0), fe29_const(c1)}; }
  template <int A> static NCG_DI bool is_one(const Fe29x2<A>& a) { return f_eqz(a.c0 - Fe29<1>::one()) && f_eqz(a.c1); }
};
template <> struct F2Form<Fe29x2P> {
  static NCG_DI Fe29x2P<1> konst(const uint32_t (&c0)[14], const uint32_t (&c1)[14]) { return p2_const(c0, c1); }
  template <int A> static NCG_DI bool is_one(const Fe29x2P<A>& a) { return f_eqz(a - Fe29x2P<1>::one()); }
};

// ---- Fp6
template <template <int> class F2, int B>
struct Fp6T {
  F2<B> c0, c1, c2;
  Fp6T() = default;
  NCG_DI Fp6T(const F2<B>& a, const F2<B>& b, const F2<B>& c) : c0(a), c1(b), c2(c) {}
  template <int B2, class = typename std::enable_if<(B2 < B)>::type>
  NCG_DI Fp6T(const Fp6T<F2, B2>& o) : c0(o.c0), c1(o.c1), c2(o.c2) {}
  static NCG_DI Fp6T zero() { return {F2<B>::zero(), F2<B>::zero(), F2<B>::zero()}; }
  static NCG_DI Fp6T one() { return {F2<B>::one(), F2<B>::zero(), F2<B>::zero()}; }
};
template <template <int> class F2, int A, int B, int C>
NCG_DI Fp6T<F2, tower_max(A, tower_max(B, C))> mk6(const F2<A>& a, const F2<B>& b, const F2<C>& c) {
  constexpr int M = tower_max(A, tower_max(B, C));
  return Fp6T<F2, M>(F2<M>(a), F2<M>(b), F2<M>(c));
}
template <template <int> class F2, int A, int B>
NCG_DI auto f6_add(const Fp6T<F2, A>& a, const Fp6T<F2, B>& b) { return mk6(a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2); }
template <template <int> class F2, int A, int B>
NCG_DI auto f6_sub(const Fp6T<F2, A>& a, const Fp6T<F2, B>& b) { return mk6(a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2); }
template <template <int> class F2, int A>
NCG_DI auto f6_neg(const Fp6T<F2, A>& a) { return mk6(f_neg(a.c0), f_neg(a.c1), f_neg(a.c2)); }
template <template <int> class F2, int A>
NCG_DI auto f6_mul_nr(const Fp6T<F2, A>& a) { return mk6(f2_mul_nr(a.c2), a.c0, a.c1); }  // tower.ts:789-792
template <template <int> class F2, int A, int B>
NCG_DI auto f6_mul(const Fp6T<F2, A>& a, const Fp6T<F2, B>& b) {  // tower.ts:619-646
  const auto t0 = a.c0 * b.c0, t1 = a.c1 * b.c1, t2 = a.c2 * b.c2;
  return mk6(t0 + f2_mul_nr((a.c1 + a.c2) * (b.c1 + b.c2) - (t1 + t2)),
             ((a.c0 + a.c1) * (b.c0 + b.c1) - (t0 + t1)) + f2_mul_nr(t2),
             (t1 + (a.c0 + a.c2) * (b.c0 + b.c2)) - (t0 + t2));
}
template <template <int> class F2, int A>
NCG_DI auto f6_sqr(const Fp6T<F2, A>& a) {  // tower.ts:647-659
  const auto t0 = f_sqr(a.c0), t4 = f_sqr(a.c2);
  const auto t1 = f_dbl(a.c0 * a.c1), t3 = f_dbl(a.c1 * a.c2);
  return mk6(f2_mul_nr(t3) + t0, f2_mul_nr(t4) + t1, (((t1 + f_sqr((a.c0 - a.c1) + a.c2)) + t3) - t0) - t4);
}
template <template <int> class F2, int A, int B>
NCG_DI auto f6_mul_fp2(const Fp6T<F2, A>& a, const F2<B>& s) { return mk6(a.c0 * s, a.c1 * s, a.c2 * s); }  // tower.ts:781-788
template <template <int> class F2, int A>
NCG_DI auto f6_inv(const Fp6T<F2, A>& a) {  // tower.ts:724-734
  const auto t0 = f_sqr(a.c0) - f2_mul_nr(a.c2 * a.c1);
  const auto t1 = f2_mul_nr(f_sqr(a.c2)) - a.c0 * a.c1;
  const auto t2 = f_sqr(a.c1) - a.c0 * a.c2;
  const auto t4 = f_inv(f2_mul_nr(a.c2 * t1 + a.c1 * t2) + a.c0 * t0);
  return mk6(t4 * t0, t4 * t1, t4 * t2);
}
// x -> x^(p^P) for P = 1, 2, 3 (tower.ts:771-780); the coefficients come from tools/gen_consts.py
template <int P, template <int> class F2, int A>
NCG_DI auto f2_frob(const F2<A>& a) {
  if constexpr (P % 2) return f2_conj(a);
  else return a;
}
template <int P, template <int> class F2, int A>
NCG_DI auto f6_frob(const Fp6T<F2, A>& a) {
  static_assert(P >= 1 && P <= 3, "Frobenius power");
  const auto k1 = F2Form<F2>::konst(BlsTower::FROB6_C1[P][0], BlsTower::FROB6_C1[P][1]);
  const auto k2 = F2Form<F2>::konst(BlsTower::FROB6_C2[P][0], BlsTower::FROB6_C2[P][1]);
  return mk6(f2_frob<P>(a.c0), f2_frob<P>(a.c1) * k1, f2_frob<P>(a.c2) * k2);
}

// ---- Fp12
template <template <int> class F2, int B>
struct Fp12T {
  Fp6T<F2, B> c0, c1;
  Fp12T() = default;
  NCG_DI Fp12T(const Fp6T<F2, B>& a, const Fp6T<F2, B>& b) : c0(a), c1(b) {}
  template <int B2, class = typename std::enable_if<(B2 < B)>::type>
  NCG_DI Fp12T(const Fp12T<F2, B2>& o) : c0(o.c0), c1(o.c1) {}
  static NCG_DI Fp12T one() { return {Fp6T<F2, B>::one(), Fp6T<F2, B>::zero()}; }
};
template <template <int> class F2, int A, int B>
NCG_DI Fp12T<F2, tower_max(A, B)> mk12(const Fp6T<F2, A>& a, const Fp6T<F2, B>& b) {
  constexpr int M = tower_max(A, B);
  return Fp12T<F2, M>(Fp6T<F2, M>(a), Fp6T<F2, M>(b));
}
// any bound -> the storage bound
template <template <int> class F2, int A>
NCG_DI Fp6T<F2, TOWER_B> tower_fit(const Fp6T<F2, A>& a) {
  return {f2_fit<TOWER_B>(a.c0), f2_fit<TOWER_B>(a.c1), f2_fit<TOWER_B>(a.c2)};
}
template <template <int> class F2, int A>
NCG_DI Fp12T<F2, TOWER_B> tower_fit(const Fp12T<F2, A>& a) {
  return {tower_fit(a.c0), tower_fit(a.c1)};
}
template <template <int> class F2, int A, int B>
NCG_DI auto f12_add(const Fp12T<F2, A>& a, const Fp12T<F2, B>& b) { return mk12(f6_add(a.c0, b.c0), f6_add(a.c1, b.c1)); }
template <template <int> class F2, int A, int B>
NCG_DI auto f12_sub(const Fp12T<F2, A>& a, const Fp12T<F2, B>& b) { return mk12(f6_sub(a.c0, b.c0), f6_sub(a.c1, b.c1)); }
template <template <int> class F2, int A>
NCG_DI auto f12_neg(const Fp12T<F2, A>& a) { return mk12(f6_neg(a.c0), f6_neg(a.c1)); }
template <template <int> class F2, int A>
NCG_DI auto f12_conj(const Fp12T<F2, A>& a) { return mk12(a.c0, f6_neg(a.c1)); }  // tower.ts:1049-1052
template <template <int> class F2, int A, int B>
NCG_DI auto f12_mul(const Fp12T<F2, A>& a, const Fp12T<F2, B>& b) {  // tower.ts:946-958
  const auto t1 = f6_mul(a.c0, b.c0), t2 = f6_mul(a.c1, b.c1);
  return mk12(f6_add(t1, f6_mul_nr(t2)), f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), f6_add(t1, t2)));
}
template <template <int> class F2, int A>
NCG_DI auto f12_sqr(const Fp12T<F2, A>& a) {  // tower.ts:959-970
  const auto ab = f6_mul(a.c0, a.c1);
  return mk12(f6_sub(f6_sub(f6_mul(f6_add(f6_mul_nr(a.c1), a.c0), f6_add(a.c0, a.c1)), ab), f6_mul_nr(ab)), f6_add(ab, ab));
}
template <template <int> class F2, int A>
NCG_DI auto f12_inv(const Fp12T<F2, A>& a) {  // tower.ts:912-917
  const auto t = f6_inv(f6_sub(f6_sqr(a.c0), f6_mul_nr(f6_sqr(a.c1))));
  return mk12(f6_mul(a.c0, t), f6_neg(f6_mul(a.c1, t)));
}
template <int P, template <int> class F2, int A>
NCG_DI auto f12_frob(const Fp12T<F2, A>& a) {  // tower.ts:1025-1041
  const auto k = F2Form<F2>::konst(BlsTower::FROB12[P][0], BlsTower::FROB12[P][1]);
  return mk12(f6_frob<P>(a.c0), f6_mul_fp2(f6_frob<P>(a.c1), k));
}
// Fp4Square (tower.ts:533-541): first = b^2 (u + 1) + a^2, second = (a + b)^2 - a^2 - b^2
template <template <int> class F2, int A, int B, class FIRST, class SECOND>
NCG_DI void f2_fp4_square(const F2<A>& a, const F2<B>& b, FIRST& first, SECOND& second) {
  const auto a2 = f_sqr(a), b2 = f_sqr(b);
  first = f2_mul_nr(b2) + a2;
  second = (f_sqr(a + b) - a2) - b2;
}
template <template <int> class F2, int A>
NCG_DI auto f12_cyclotomic_sqr(const Fp12T<F2, A>& a) {  // tower.ts:1058-1079
  using T2 = decltype(f_sqr(a.c0.c0));
  using FIRST = decltype(f2_mul_nr(T2()) + T2());
  using SECOND = decltype((T2() - T2()) - T2());
  FIRST t3, t5, t7;
  SECOND t4, t6, t8;
  f2_fp4_square(a.c0.c0, a.c1.c1, t3, t4);
  f2_fp4_square(a.c1.c0, a.c0.c2, t5, t6);
  f2_fp4_square(a.c0.c1, a.c1.c2, t7, t8);
  const auto t9 = f2_mul_nr(t8);
  return mk12(mk6(f_dbl(t3 - a.c0.c0) + t3, f_dbl(t5 - a.c0.c1) + t5, f_dbl(t7 - a.c0.c2) + t7),
              mk6(f_dbl(t9 + a.c1.c0) + t9, f_dbl(t4 + a.c1.c1) + t4, f_dbl(t6 + a.c1.c2) + t6));
}
// f * (o0 + o1 v + o4 v w): the sparse product of a line (bls.ts:476-519 after the scaling by Px, Py)
template <template <int> class F2, int A, int B0, int B1, int B4>
NCG_DI auto f12_mul014(const Fp12T<F2, A>& f, const F2<B0>& o0, const F2<B1>& o1, const F2<B4>& o4) {
  const auto &a0 = f.c0.c0, &a1 = f.c0.c1, &a2 = f.c0.c2, &b0 = f.c1.c0, &b1 = f.c1.c1, &b2 = f.c1.c2;
  // t0 = Fp6.mul01(f0, o0, o1)
  const auto t0_0 = a0 * o0, t0_1 = a1 * o1;
  const auto t0_c0 = f2_mul_nr((a1 + a2) * o1 - t0_1) + t0_0;
  const auto t0_c1 = ((o0 + o1) * (a0 + a1) - t0_0) - t0_1;
  const auto t0_c2 = ((a0 + a2) * o0 - t0_0) + t0_1;
  // t1 = Fp6.mul1(f1, o4)
  const auto t1_c0 = f2_mul_nr(b2 * o4);
  const auto t1_c1 = b0 * o4, t1_c2 = b1 * o4;
  // t2 = Fp6.mul01(f0 + f1, o0, o1 + o4)
  const auto s0 = a0 + b0, s1 = a1 + b1, s2 = a2 + b2;
  const auto o14 = o1 + o4;
  const auto t2_0 = s0 * o0, t2_1 = s1 * o14;
  const auto t2_c0 = f2_mul_nr((s1 + s2) * o14 - t2_1) + t2_0;
  const auto t2_c1 = ((o0 + o14) * (s0 + s1) - t2_0) - t2_1;
  const auto t2_c2 = ((s0 + s2) * o0 - t2_0) + t2_1;
  return mk12(mk6(f2_mul_nr(t1_c2) + t0_c0, t1_c0 + t0_c1, t1_c1 + t0_c2),
              mk6((t2_c0 - t0_c0) - t1_c0, (t2_c1 - t0_c1) - t1_c1, (t2_c2 - t0_c2) - t1_c2));
}
template <template <int> class F2, int A>
NCG_DI bool f12_is_one(const Fp12T<F2, A>& a) {
  const bool z = f_eqz(a.c0.c1) && f_eqz(a.c0.c2) && f_eqz(a.c1.c0) && f_eqz(a.c1.c1) && f_eqz(a.c1.c2);
  return F2Form<F2>::is_one(a.c0.c0) && z;
}

// ---- the same on the storage bound, out of line: what the Miller loop, the final exponentiation and the kernels
// call.  An Fp12 does not fit the argument registers, so these take references (the values live in the caller's frame).
template <template <int> class F2>
struct Tower {
  using E2 = F2<TOWER_B>;
  using E6 = Fp6T<F2, TOWER_B>;
  using E12 = Fp12T<F2, TOWER_B>;
  static NCG_TOWERFN void mul(E12& r, const E12& a, const E12& b) { r = tower_fit(f12_mul(a, b)); }
  static NCG_TOWERFN void sqr(E12& r, const E12& a) { r = tower_fit(f12_sqr(a)); }
  static NCG_TOWERFN void inv(E12& r, const E12& a) { r = tower_fit(f12_inv(a)); }
  static NCG_TOWERFN void cyclotomic_sqr(E12& r, const E12& a) { r = tower_fit(f12_cyclotomic_sqr(a)); }
  static NCG_TOWERFN void mul014(E12& r, const E12& f, const E2& o0, const E2& o1, const E2& o4) { r = tower_fit(f12_mul014(f, o0, o1, o4)); }
  static NCG_TOWERFN void frob1(E12& r, const E12& a) { r = tower_fit(f12_frob<1>(a)); }
  static NCG_TOWERFN void frob2(E12& r, const E12& a) { r = tower_fit(f12_frob<2>(a)); }
  static NCG_TOWERFN void frob3(E12& r, const E12& a) { r = tower_fit(f12_frob<3>(a)); }
  static NCG_DI void conj(E12& r, const E12& a) { r = tower_fit(f12_conj(a)); }

  // a^|x| for a in the cyclotomic subgroup, |x| = 0xd201000000010000: the value of bls12CyclotomicExpX
  // (src/bls12-381.ts:231-242).  The reference squares in Karabina's compressed form and pays one Fp2 inversion per
  // power to decompress; a lane pays ~480 Fp products for that inversion against ~350 saved, so the squarings here
  // are the full cyclotomic ones (tower.ts:1081-1092 _cyclotomicExp): the same element of Fp12, bit for bit.
  static NCG_TOWERFN void cyclotomic_exp_x(E12& r, const E12& a) {
    constexpr uint64_t X = 0xD201000000010000ull;
    E12 z = a;
    for (int bit = 62; bit >= 0; bit--) {
      cyclotomic_sqr(z, z);
      if ((X >> bit) & 1ull) mul(z, z, a);
    }
    r = z;
  }
  static NCG_DI void pow_minus_x(E12& r, const E12& a) {  // x is negative: conjugate (bls12-381.ts:259)
    cyclotomic_exp_x(r, a);
    conj(r, r);
  }
  // Fp12finalExponentiate (src/bls12-381.ts:258-276), step for step
  static NCG_TOWERFN void final_exponentiate(E12& r, const E12& num) {
    E12 t0, t1, t2, t3, t4, t5, t6, t7, a, b;
    inv(a, num);
    conj(b, num);          // frobeniusMap(num, 6)
    mul(t0, b, a);         // num^(q^6) / num
    frob2(a, t0);
    mul(t1, a, t0);
    pow_minus_x(t2, t1);
    cyclotomic_sqr(a, t1);
    conj(a, a);
    mul(t3, a, t2);
    pow_minus_x(t4, t3);
    pow_minus_x(t5, t4);
    pow_minus_x(a, t5);
    cyclotomic_sqr(b, t2);
    mul(t6, a, b);
    pow_minus_x(t7, t6);
    mul(a, t2, t5);
    frob2(a, a);           // (t2 t5)^(q^2)
    mul(b, t4, t1);
    frob3(b, b);           // (t4 t1)^(q^3)
    mul(a, a, b);
    conj(b, t1);
    mul(b, t6, b);
    frob1(b, b);           // (t6 conj(t1))^q
    mul(a, a, b);
    conj(b, t3);
    mul(b, t7, b);
    mul(b, b, t1);         // t7 conj(t3) t1
    mul(r, a, b);
  }

  // wire (12 canonical residues of 12 LE words, tower order c0.c0.c0 .. c1.c2.c1) <-> element
  static NCG_DI E2 load2_wire(const uint32_t* p) { return E2(FieldWire<F2<TOWER_B>>::load(p)); }
  static NCG_DI E12 load_wire(const uint32_t* p) {
    return {E6(load2_wire(p), load2_wire(p + 24), load2_wire(p + 48)), E6(load2_wire(p + 72), load2_wire(p + 96), load2_wire(p + 120))};
  }
  static NCG_DI void store_wire(uint32_t* p, const E12& a) {
    FieldWire<E2>::store(p, a.c0.c0);
    FieldWire<E2>::store(p + 24, a.c0.c1);
    FieldWire<E2>::store(p + 48, a.c0.c2);
    FieldWire<E2>::store(p + 72, a.c1.c0);
    FieldWire<E2>::store(p + 96, a.c1.c1);
    FieldWire<E2>::store(p + 120, a.c1.c2);
  }
  // workspace form: the Montgomery limbs as they are, 6 x 28 words
  static NCG_DI E12 load_ws(const uint32_t* p) {
    using IO = FieldIO<E2>;
    return {E6(IO::load(p), IO::load(p + 28), IO::load(p + 56)), E6(IO::load(p + 84), IO::load(p + 112), IO::load(p + 140))};
  }
  static NCG_DI void store_ws(uint32_t* p, const E12& a) {
    using IO = FieldIO<E2>;
    IO::store(p, a.c0.c0);
    IO::store(p + 28, a.c0.c1);
    IO::store(p + 56, a.c0.c2);
    IO::store(p + 84, a.c1.c0);
    IO::store(p + 112, a.c1.c1);
    IO::store(p + 140, a.c1.c2);
  }
};
constexpr int FP12_WIRE_WORDS = 144, FP12_WS_WORDS = 168;

}  // namespace ncg
