"""CPU checks of the pair-sum path of the secp256k1 batch multiply (csrc/mulvar_pairsum.hpp) on the host twin of its four
kernels (ht_mul_var_pairsum: prepare, batched inverse over groups of 16, ladder, affine step), against the oracle."""
import numpy as np

import ladder32
import ladder_exceptions as LE
import ladder_pairsum as PS
from helpers import SECP_LAMBDA as LAM, signed_odd_digits, val
from oracle.curves import SECP256K1_N as N, SECP256K1_P as P, Secp256k1

G = Secp256k1.BASE
PLANTED = [0, 1, 2, N - 1, LAM, N - LAM, LAM + 1, LAM - 1]


def test_model_flagging_scalars():
    """The model: random scalars meet no exceptional addition, and the scalars that do are 0 and +-lambda - R = -S_w in the last
    window; +-lambda have an even k2 = +-1 + 1 - 1, whose fix-up then starts from R = O."""
    rng = LE.rng(0x14A0)
    for _ in range(256):
        k = rng.rndBelow(N)
        assert PS.ladder_events(k) == [], hex(k)
    hits = PS.flagging_scalars()
    assert set(hits) == {0, LAM, N - LAM}
    assert hits[0] == [(PS.M - 1, "neg")]
    for k in (LAM, N - LAM):
        assert hits[k] == [(PS.M - 1, "neg"), (PS.FIXUP, "inf")], hits[k]


def test_twin_against_oracle_random():
    """2 000 random pairs: bit-exact against the oracle, no lane flagged"""
    rng = LE.rng(0x14A1)
    pairs = LE.random_pairs(rng, 2000, nbase=16)
    pw, sw = LE.wires(pairs)
    out, inf, flags = PS.mul_var(pw, sw)
    exp, exp_inf = LE.expected(pairs)
    assert np.array_equal(inf, exp_inf) and np.array_equal(out, exp)
    assert not flags.any()


def test_twin_planted_and_flags():
    """k in {0, 1, 2, n - 1, +-lambda, lambda +- 1} on G, 3 G and a random point, P = O, and random pairs with even and odd k2
    around them so that every group of 16 mixes them: the values are the oracle's, and the lanes that go through the complete
    ladder are exactly the ones the model lists (k = 0 and P = O are known beforehand and stay out of it)."""
    rng = LE.rng(0x14A2)
    pts = [G, G.multiplyUnsafe(3), G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)]
    planted = [(k, p) for k in PLANTED for p in pts] + [(k, Secp256k1.ZERO) for k in (0, 1, 12345, LAM)]
    filler = LE.random_pairs(rng, 3 * len(planted))
    pairs = []
    for i, pr in enumerate(planted):          # one planted row in every four
        pairs += [filler[3 * i], pr, filler[3 * i + 1], filler[3 * i + 2]]
    parity = {ladder32.split_k1_odd(k)[1] % 2 for k, _ in pairs[:16]}
    assert parity == {0, 1}
    pw, sw = LE.wires(pairs)
    out, inf, flags = PS.mul_var(pw, sw)
    exp, exp_inf = LE.expected(pairs)
    assert np.array_equal(inf, exp_inf) and np.array_equal(out, exp)
    model = PS.flagging_scalars()
    for i, (k, p) in enumerate(pairs):
        is_o = p.toAffine() == Secp256k1.ZERO.toAffine()
        slow = (k % N) in model and k % N != 0 and not is_o
        assert bool(flags[i] & 2) == slow, (i, hex(k))
        assert bool(flags[i] & 1) == is_o, (i, hex(k))     # the prepare lane flags a degenerate table only


def test_prefixes_and_inverse_of_one_item():
    """pre_w, acc and 1 / acc of one item against big-integer products of H_w = beta x(T[e2]) - x(T[e1]) over the stored table"""
    rng = LE.rng(0x14A3)
    k, pt = rng.rndBelow(N - 1) + 1, G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)
    others = LE.random_pairs(rng, 17)
    pw, sw = LE.wires([(k, pt)] + others)
    _, _, flags, dbg = PS.mul_var(pw, sw, dump=True)
    assert not flags.any()
    fe = lambda off: val(dbg[off:off + PS.FW]) % P                          # noqa: E731
    beta = int(G.multiplyUnsafe(LAM).toAffine()[0]) * pow(int(G.toAffine()[0]), -1, P) % P
    # the table: entry e is (2 e + 1) P at Z = Zg
    zg = fe(PS.ZG_OFF)
    for e in range(PS.TS):
        x, y = pt.multiplyUnsafe(2 * e + 1).toAffine()
        assert fe(e * 2 * PS.FW) == int(x) * zg * zg % P and fe(e * 2 * PS.FW + PS.FW) == int(y) * zg ** 3 % P
    k1, k2 = ladder32.split_k1_odd(k)
    d1, d2 = signed_odd_digits(abs(k1), PS.W, PS.M), signed_odd_digits(abs(k2) + (k2 % 2 == 0), PS.W, PS.M)
    H = {}
    for w in range(1, PS.M):
        e1, e2 = (abs(d1[PS.M - 1 - w]) - 1) >> 1, (abs(d2[PS.M - 1 - w]) - 1) >> 1
        H[w] = (beta * fe(e2 * 2 * PS.FW) - fe(e1 * 2 * PS.FW)) % P
    acc = 1
    for w in range(PS.M - 1, 0, -1):
        assert fe(PS.PRE_OFF + (w - 1) * PS.FW) == acc, w
        acc = acc * H[w] % P
    assert fe(PS.ACC_OFF) == acc
    assert fe(PS.ACC_OFF + PS.FW) * acc % P == 1

