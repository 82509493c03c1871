// X25519 (RFC 7748) on the ed25519 field: the lane code of k_x25519 and of its CPU twin.
//
// Reproduces the values of the reference's montgomery() (src/abstract/montgomery.ts, built at src/ed25519.ts:266-292):
//   scalarMult(scalar, u) = encodeU(montgomeryLadder(decodeU(u), decodeScalar(scalar)))     (montgomery.ts:294-331)
//   decodeScalar = adjustScalarBytes then little-endian                                      (ed25519.ts:93-101)
//   decodeU      = bit 255 cleared, then mod p: 2^255 - 19 .. 2^255 - 1 are accepted          (montgomery.ts:277-287)
//   the five low-order u of the curve and its twist are refused before the ladder, a zero result after it (:303-325)
// One ladder step is montgomery.ts:352-393 (RFC 7748 section 5) on Fe9<Ed25519 p> values with declared limb bounds:
//   A = x2 + z2 (2)   B = x2 - z2 (3)   C = x3 + z3 (2)   D = x3 - z3 (3)
//   AA = A^2          BB = B^2 (B normalised inside f_sqr)
//   DA = D A (3 * 2)  CB = C B (2 * 3)
//   x3' = (DA + CB)^2 (operand bound 2)          z3' = x1 (DA - CB)^2 (the difference, bound 3, normalised inside f_sqr)
//   x2' = AA BB       E = AA - BB (3)            z2' = E (AA + a24 E),  a24 = 121665: fe9_mulk_add, one carry pass
// Every stored value (x1, x2, z2, x3, z3) is a product: limb bound 1.  Per step 5 products + 4 squares + the carry pass of
// AA + a24 E: 5 * 92 + 4 * 56 + 18 = 702 v_mad_u64_u32, two weak normalisations, 36 selects.  (DESIGN.md section 8 has the count
// of the form that fuses DA + CB and DA - CB, and why it is not the one built.)
// Nothing here branches or indexes on a scalar bit: the swap is a per-limb select.
#pragma once
#include "ec_te.hpp"

namespace ncg {

constexpr uint32_t X25519_A24 = 121665u;  // (486662 - 2) / 4 (ed25519.ts:276)

// s + K e for a small constant K (wave-uniform: an SGPR operand), reduced by ONE carry pass: limb i takes s_i + K e_i + carry,
// the carry out of limb 8 (weight 2^261) comes back into limbs 0 and 1 through C0.  Special-form primes with C1 = 0 only.
template <uint32_t K, class PR, int S, int E>
NCG_DI Fe9<PR, 1> fe9_mulk_add(const Fe9<PR, S>& s, const Fe9<PR, E>& e) {
  static_assert(!Fe9IsMont<PR>::value && PR::C1 == 0, "fe9_mulk_add: one-word fold only");
  constexpr uint64_t U = (1ull << 29) + (1ull << 19);
  constexpr uint64_t CMAX = ((uint64_t)K * E * U + (uint64_t)S * U) / (1ull << 29) + 2;  // bound of every carry
  static_assert(CMAX * PR::C0 + (1ull << 29) < (1ull << 32), "fe9_mulk_add: the folded carry overflows 32 bits");
  Fe9<PR, 1> r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    fe9_acc32(c, s.v[i]);
    fe9_mac_k(c, e.v[i], K);
    r.v[i] = (uint32_t)c & FE9_MASK;
    c >>= 29;
  }
  const uint32_t f = r.v[0] + (uint32_t)c * PR::C0;  // below 2^32 (CMAX)
  r.v[0] = f & FE9_MASK;
  r.v[1] += f >> 29;  // below 2^29 + 8 < U
  return r;
}

template <class F>
struct X25519State {  // (x2 : z2) and (x3 : z3), every limb below U
  F x2, z2, x3, z3;
};

template <class F>
NCG_DI void x25519_cswap(uint32_t swap, F& a, F& b) {  // swap = 0 / 1: per-limb selects (v_cndmask), no branch
  const bool s = swap != 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const uint32_t x = a.v[i], y = b.v[i];
    a.v[i] = s ? y : x;
    b.v[i] = s ? x : y;
  }
}

// cswap(swap) then the ladder step of montgomery.ts:352-393
template <class F>
NCG_DI void x25519_step(X25519State<F>& st, const F& x1, uint32_t swap) {
  static_assert(F::BOUND == 1, "the ladder state is stored at bound 1");
  x25519_cswap(swap, st.x2, st.x3);
  x25519_cswap(swap, st.z2, st.z3);
  const auto A = st.x2 + st.z2;
  const auto B = st.x2 - st.z2;
  const auto C = st.x3 + st.z3;
  const auto D = st.x3 - st.z3;
  const F AA = f_sqr(A);
  const F BB = f_sqr(B);
  const F DA = D * A;
  const F CB = C * B;
  st.x3 = f_sqr(DA + CB);
  st.z3 = x1 * f_sqr(DA - CB);
  st.x2 = AA * BB;
  const auto E = AA - BB;
  st.z2 = E * fe9_mulk_add<X25519_A24>(AA, E);
}

// adjustScalarBytes on 8 LE words (ed25519.ts:93-101)
NCG_DI void x25519_decode_scalar(uint32_t (&k)[8]) {
  k[0] &= 0xfffffff8u;
  k[7] = (k[7] & 0x7fffffffu) | 0x40000000u;
}

NCG_DI bool x25519_words_eq(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= a[i] ^ b[i];
  return d == 0;
}
NCG_DI bool x25519_words_small(const uint32_t (&a)[8], uint32_t v) {  // a == v, v one word
  uint32_t d = a[0] ^ v;
#pragma unroll
  for (int i = 1; i < 8; i++) d |= a[i];
  return d == 0;
}

// decodeU + the low-order test: w = the 8 LE words of the encoding; on return w = the canonical residue, u = its field form.
// Returns false for the five low-order values 0, 1, p - 1 and the two points of order 8 (montgomery.ts:303-312).
NCG_DI bool x25519_decode_u(uint32_t (&w)[8], FEd& u) {
  // the two u of order 8 (one on the curve, one on the twist) and p - 1, as LE words
  const uint32_t la[8] = {0x7c7aebe0u, 0xaeb8413bu, 0xfae35616u, 0x6ac49ff1u, 0xeb8d09dau, 0xfdb1329cu, 0x16056286u, 0x00b8495fu};
  const uint32_t lb[8] = {0xbc959c5fu, 0x248c50a3u, 0x55b1d0b1u, 0x5bef839cu, 0xc45c4404u, 0x868e1c58u, 0xdd4e22d8u, 0x57119fd0u};
  const uint32_t pm[8] = {0xffffffecu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu};
  w[7] &= 0x7fffffffu;
  u = fe9_from_wire<Fe9EdPR>(w);  // below 2^255: congruent to the residue
  fe9_to_wire(w, u);              // canonical
  const bool low = x25519_words_small(w, 0u) || x25519_words_small(w, 1u) || x25519_words_eq(w, pm) || x25519_words_eq(w, la) ||
                   x25519_words_eq(w, lb);
  return !low;
}

// montgomeryLadder (montgomery.ts:338-406) without the final division: (x2 : z2) after the 255 steps and the trailing swap.
// The swap bit of step t is bit t of k ^ (k >> 1) (the reference's running `swap ^= k_t`); the 256-bit register is shifted
// left once per step so that the bit is always the top one - no index depends on t or on the scalar.
NCG_DI X25519State<FEd> x25519_ladder(const uint32_t (&k)[8], const FEd& x1) {
  uint32_t kx[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kx[i] = k[i] ^ ((k[i] >> 1) | (i < 7 ? k[i + 1] << 31 : 0u));
  // bit 254 to the top
#pragma unroll
  for (int i = 7; i >= 0; i--) kx[i] = (kx[i] << 1) | (i > 0 ? kx[i - 1] >> 31 : 0u);
  X25519State<FEd> st{FEd::one(), FEd::zero(), x1, FEd::one()};
  for (int t = 254; t >= 0; t--) {
    const uint32_t swap = kx[7] >> 31;
#pragma unroll
    for (int i = 7; i >= 0; i--) kx[i] = (kx[i] << 1) | (i > 0 ? kx[i - 1] >> 31 : 0u);
    x25519_step(st, x1, swap);
  }
  const uint32_t last = k[0] & 1u;
  x25519_cswap(last, st.x2, st.x3);
  x25519_cswap(last, st.z2, st.z3);
  return st;
}

// One scalarMult: raw 32-byte scalar and u as 8 LE words each; out = the 8 LE words of the result, zero where refused.
NCG_DI bool x25519_lane(const uint32_t* __restrict__ scalar, const uint32_t* __restrict__ uenc, uint32_t (&out)[8]) {
  uint32_t k[8], w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    k[i] = scalar[i];
    w[i] = uenc[i];
  }
  x25519_decode_scalar(k);
  FEd x1;
  bool ok = x25519_decode_u(w, x1);
  const X25519State<FEd> st = x25519_ladder(k, x1);
  const FEd r = st.x2 * f_inv(st.z2);
  fe9_to_wire(out, r);
  ok = ok && !x25519_words_small(out, 0u);  // montgomery.ts:321-325
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = ok ? out[i] : 0u;
  return ok;
}

// u = (Z + Y) / (Z - Y) of a projective Edwards point (ed25519.ts:281-290 on [k]B; (1 + y) / (1 - y) with Z = 1).  false where the
// denominator is zero (the reference's Fp.inv(0) throws).
NCG_DI bool x25519_edwards_to_u(const FEd& Y, const FEd& Z, uint32_t (&out)[8]) {
  const auto den = Z - Y;
  const bool ok = !f_eqz(den);
  const FEd r = (Z + Y) * f_inv(den);
  fe9_to_wire(out, r);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = ok ? out[i] : 0u;
  return ok;
}

// ed25519.utils.toMontgomery (ed25519.ts:323-328): Point.fromBytes(pk) strict, then (1 + y) / (1 - y)
NCG_DI bool ed25519_to_montgomery_lane(const uint32_t* __restrict__ pk, uint32_t (&out)[8]) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = pk[i];
  FEd x, y;
  const bool dec = ed_decompress(w, false, x, y);
  const bool ok = x25519_edwards_to_u(y, FEd::one(), out) && dec;
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = ok ? out[i] : 0u;
  return ok;
}

// The pieces on raw words (ncg_field_check field 16, ht_x25519_op).  op 0: a = x2 z2 x3 z3 (36 limbs), b = x1 (9 limbs), one
// x25519_step with swap = variant & 1, out = the 36 limbs.  op 1: a[0..8) = an encoded u; out[0..8) = the canonical residue,
// out[8] = 1 unless it is of low order.  op 2: a[0..8) = raw scalar words; out[0..8) = adjustScalarBytes of them.
NCG_DI int x25519_check_op(int op, int variant, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  if (op == 0) {
    X25519State<FEd> st;
    FEd x1;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      st.x2.v[i] = a[i];
      st.z2.v[i] = a[9 + i];
      st.x3.v[i] = a[18 + i];
      st.z3.v[i] = a[27 + i];
      x1.v[i] = b[i];
    }
    x25519_step(st, x1, (uint32_t)variant & 1u);
#pragma unroll
    for (int i = 0; i < 9; i++) {
      out[i] = st.x2.v[i];
      out[9 + i] = st.z2.v[i];
      out[18 + i] = st.x3.v[i];
      out[27 + i] = st.z3.v[i];
    }
    return 0;
  }
  if (op == 1 || op == 2) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = a[i];
    if (op == 1) {
      FEd u;
      out[8] = x25519_decode_u(w, u) ? 1u : 0u;
    } else {
      x25519_decode_scalar(w);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = w[i];
    return 0;
  }
  return -1;
}

}  // namespace ncg
