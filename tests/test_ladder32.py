"""CPU checks of CurveSecpI's 32-window ladder: the split with k1 odd (scalar.hpp secp_glv_make_k1_odd, host twin
ht_glv_split_k1_odd), its signed-odd recoding with M = 32, the ladder model of tests/ladder32.py and the host twin of the ladder
(the k2 fix-up included) against the oracle."""
import hosttest
import ladder32
from helpers import ORACLE_CURVE, SECP_LAMBDA as LAM, points_to_wire, scalars_to_wire, signed_odd_digits, wire_to_affine
from noble_curves_amd._native import SECP256K1
from oracle.curves import SECP256K1_N, Secp256k1, makeRng

N = SECP256K1_N
CURVE_SECP_FUSED = 14   # ht_mul_var: the ladder of CurveSecpI
EDGE = [0, 1, 2, 3, N - 1, N - 2, N - 3, 1 << 128, (1 << 128) - 1, (1 << 128) + 1, (1 << 255), LAM, LAM + 1, LAM - 1, N - LAM,
        (N + 1) // 2, N // 2, (1 << 64), 0xFFFFFFFF, 1 << 32, 15, 16, 17, 255, 256, (1 << 256) - 1]


def test_split_k1_odd():
    """10^5 random scalars, the edge list and scalars at the Babai rounding boundaries: k1 odd, |k1| < 2^128, |k2| + 1 < 2^128,
    k1 + lambda k2 = k (mod n); an odd k1 of the plain split is kept as it is; every parity class of the plain split occurs, and
    the M = 32 signed-odd digits give back |k1| and |k2| + (k2 even)."""
    rng = makeRng(0x32D1)
    ks = EDGE + ladder32.babai_boundary_scalars(rng) + [rng.rndBelow(N) for _ in range(100000)]
    seen, top = set(), [0, 0]
    for i, k in enumerate(ks):
        n1, p1, n2, p2 = hosttest.glv_split(k)
        k1, k2 = ladder32.split_k1_odd(k)
        ladder32.check_split(k, k1, k2)
        seen.add((p1 % 2, p2 % 2))
        if p1 % 2:
            assert (k1, k2) == ((-p1 if n1 else p1), (-p2 if n2 else p2)), hex(k)
        top = [max(top[0], abs(k1)), max(top[1], abs(k2) + 1)]
        if i < 20000:
            for h in (abs(k1), abs(k2) + (k2 % 2 == 0)):
                d = signed_odd_digits(h, ladder32.W, ladder32.M)
                assert sum(x << (4 * j) for j, x in enumerate(d)) == h and all(x % 2 and abs(x) < 16 for x in d), hex(k)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert top[0] < 0.83 * 2 ** 128 and top[1] < 0.9 * 2 ** 128   # the bounds the split's comment derives


def test_ladder32_model():
    """Random scalars meet no exceptional addition before the last window; the search over k = a + b lambda finds exactly
    k = 0 (R = -Q in the last k2 addition: the result is O) and k = +-lambda (R = -Q in the last window, then the fix-up starts
    from R = O).  The fix-up never meets R = +-psi(P): that would need k = -2 s2 lambda with k2 even."""
    rng = makeRng(0x32E0)
    for k in [1, 2, N - 1, LAM, N - LAM, 1 << 128, (1 << 256) - 1] + [rng.rndBelow(N) for _ in range(4000)]:
        assert all(w >= ladder32.M - 1 for w, _, _ in ladder32.ladder_events(k)), hex(k)
    hits = ladder32.ladder_exceptional_scalars()
    last = [(ladder32.M - 1, 1, "neg")]
    assert hits == {0: last, LAM: last + [(ladder32.FIXUP, 1, "inf")], N - LAM: last + [(ladder32.FIXUP, 1, "inf")]}
    for k in (2 * LAM % N, -2 * LAM % N):
        assert ladder32.ladder_events(k) == [], hex(k)


def test_ladder32_host_twin_matches_oracle():
    """The host twin of the ladder on the edge list (2^256 - 1 included), the model's exceptional scalars, +-2 lambda, small scalars, scalars with an
    even and an odd k2, on G, small multiples of G and random points; O as the input point."""
    rng = makeRng(0x32F1)
    G = Secp256k1.BASE
    special = sorted(ladder32.ladder_exceptional_scalars()) + [2 * LAM % N, -2 * LAM % N]
    pts_small = [G, G.multiplyUnsafe(2), G.multiplyUnsafe(3), G.multiplyUnsafe(7)]
    pairs = [(k, p) for k in special for p in pts_small + [G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)]]
    pairs += [(k, G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)) for k in EDGE + list(range(1, 40))]
    pairs += [(k, G.multiplyUnsafe(j)) for j, k in enumerate([rng.rndBelow(N) for _ in range(40)], 1)]
    pairs += [(12345, Secp256k1.ZERO), (LAM, Secp256k1.ZERO)]
    ks, pts = [k for k, _ in pairs], [p for _, p in pairs]
    assert {ladder32.split_k1_odd(k)[1] % 2 for k in ks} == {0, 1}
    out, inf = hosttest.mul_var(CURVE_SECP_FUSED, points_to_wire(SECP256K1, pts), scalars_to_wire(ks))
    zero = ORACLE_CURVE[SECP256K1].ZERO.toAffine()
    for i, (k, p) in enumerate(pairs):
        exp = p.multiplyUnsafe(k % N).toAffine()   # the ladder takes any 256-bit scalar
        assert wire_to_affine(SECP256K1, out[i]) == exp, (i, hex(k))
        assert bool(inf[i]) == (exp == zero), (i, hex(k))
