// Stand-alone host run of the division-step inversion (noble-curves_amd/csrc/fe9_inv.hpp) on the edge values of both plain
// primes: the CPU twin of the device code, for a sanitizer build (signed shifts and overflow are the typical faults of this kind
// of code).  Each value goes through f_inv at every operand bound the value admits, is compared with the Fermat chain and
// multiplied back to 1.  Exit status 0: every value agreed.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I noble-curves_amd/csrc tools/inv_divsteps_host.hip -o tools/_build/inv_divsteps_host && tools/_build/inv_divsteps_host
#include <cstdio>
#include <vector>

#include "fe9.hpp"

using namespace ncg;

typedef unsigned __int128 u128;
struct U320 {  // little-endian 32-bit words, enough for 7 U 2^232
  uint32_t w[10];
};
static U320 u_zero() {
  U320 r{};
  return r;
}
static U320 u_add(const U320& a, const U320& b) {
  U320 r;
  uint64_t c = 0;
  for (int i = 0; i < 10; i++) {
    c += (uint64_t)a.w[i] + b.w[i];
    r.w[i] = (uint32_t)c;
    c >>= 32;
  }
  return r;
}
static U320 u_sub(const U320& a, const U320& b) {
  U320 r;
  int64_t c = 0;
  for (int i = 0; i < 10; i++) {
    c += (int64_t)a.w[i] - b.w[i];
    r.w[i] = (uint32_t)c;
    c >>= 32;
  }
  return r;
}
static U320 u_pow2(int k) {
  U320 r = u_zero();
  r.w[k / 32] = 1u << (k % 32);
  return r;
}
static U320 u_small(uint32_t v) {
  U320 r = u_zero();
  r.w[0] = v;
  return r;
}
static U320 u_shr1(const U320& a) {
  U320 r;
  for (int i = 0; i < 10; i++) r.w[i] = (a.w[i] >> 1) | (i < 9 ? a.w[i + 1] << 31 : 0);
  return r;
}
template <class PR>
static U320 u_p() {
  U320 r = u_zero();
  for (int i = 0; i < 9; i++) {
    U320 t = u_zero();
    const int bit = 29 * i;
    const uint64_t v = (uint64_t)PR::P[i] << (bit % 32);
    t.w[bit / 32] = (uint32_t)v;
    t.w[bit / 32 + 1] = (uint32_t)(v >> 32);
    r = u_add(r, t);
  }
  return r;
}
// tight 29-bit limbs of a value below 2^261 (limb 8 takes what is left, as the device tests build their operands)
static void limbs29(uint32_t (&l)[9], const U320& a) {
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i;
    const uint64_t two = ((uint64_t)a.w[bit / 32 + 1] << 32) | a.w[bit / 32];
    l[i] = (uint32_t)(two >> (bit % 32)) & (i < 8 ? FE9_MASK : 0xffffffffu);
  }
}

static int g_bad = 0, g_n = 0;

template <class PR, int A>
static void check_limbs(const uint32_t (&l)[9], const char* what) {
  Fe9<PR, A> x;
  for (int i = 0; i < 9; i++) x.v[i] = l[i];
  const Fe9<PR, 1> inv = f_inv(x), fer = f_inv_fermat(x);
  uint32_t wi[8], wf[8], wx[8], wp[8];
  fe9_to_wire(wi, inv);
  fe9_to_wire(wf, fer);
  fe9_to_wire(wx, x);
  fe9_to_wire(wp, inv * x);
  bool zero = true, same = true, one = wp[0] == 1, prod0 = true, lit0 = inv.is_zero();
  for (int i = 0; i < 8; i++) {
    zero = zero && wx[i] == 0;
    same = same && wi[i] == wf[i];
    prod0 = prod0 && wp[i] == 0;
    if (i) one = one && wp[i] == 0;
  }
  g_n++;
  if (!same || (zero ? !(prod0 && lit0) : !one)) {
    g_bad++;
    printf("MISMATCH %s bound %d:", what, A);
    for (int i = 0; i < 9; i++) printf(" %08x", l[i]);
    printf("\n");
  }
}
template <class PR>
static void check_value(const U320& a, const char* what) {
  uint32_t l[9];
  limbs29(l, a);
  check_limbs<PR, 1>(l, what);
  check_limbs<PR, 2>(l, what);
  check_limbs<PR, 7>(l, what);
}

template <class PR>
static void run(const char* name) {
  const U320 p = u_p<PR>(), one = u_small(1);
  check_value<PR>(u_zero(), "0");
  check_value<PR>(one, "1");
  check_value<PR>(u_small(2), "2");
  check_value<PR>(u_sub(p, one), "p-1");
  check_value<PR>(u_sub(p, u_small(2)), "p-2");
  check_value<PR>(u_shr1(u_sub(p, one)), "(p-1)/2");
  check_value<PR>(u_shr1(u_add(p, one)), "(p+1)/2");
  check_value<PR>(p, "p");
  check_value<PR>(u_add(p, p), "2p");
  check_value<PR>(u_sub(u_pow2(256), one), "2^256-1");
  for (int k = 0; k < 256; k++) {
    check_value<PR>(u_pow2(k), "2^k");
    check_value<PR>(u_sub(u_pow2(k), one), "2^k-1");
    if (k < 255) check_value<PR>(u_sub(p, u_pow2(k)), "p-2^k");
  }
  for (uint32_t s = 3; s < 64; s++) {  // small integers and their inverses
    check_value<PR>(u_small(s), "small");
    uint32_t l[9];
    limbs29(l, u_small(s));
    Fe9<PR, 1> x;
    for (int i = 0; i < 9; i++) x.v[i] = l[i];
    const Fe9<PR, 1> inv = f_inv(x);
    check_limbs<PR, 1>(inv.v, "1/small");
  }
  // loose limbs at the top of what each bound type admits, and pseudo-random limbs below it
  const uint32_t U = (1u << 29) + (1u << 19);
  uint64_t st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return st;
  };
  for (int it = 0; it < 3000; it++) {
    uint32_t l1[9], l2[9], l7[9];
    for (int i = 0; i < 9; i++) {
      const bool top = it < 8 ? ((it >> (i % 3)) & 1) : (rnd() % 4 == 0);
      l1[i] = top ? U - 1 : (uint32_t)(rnd() % U);
      l2[i] = top ? 2 * U - 1 : (uint32_t)(rnd() % (2ull * U));
      l7[i] = top ? 7 * U - 1 : (uint32_t)(rnd() % (7ull * U));
    }
    check_limbs<PR, 1>(l1, "loose");
    check_limbs<PR, 2>(l2, "loose");
    check_limbs<PR, 7>(l7, "loose");
  }
  printf("%s: %d inversions checked, %d mismatches so far\n", name, g_n, g_bad);
}

int main() {
  run<Fe9SecpPR>("secp256k1");
  run<Fe9EdPR>("ed25519");
  return g_bad ? 1 : 0;
}
