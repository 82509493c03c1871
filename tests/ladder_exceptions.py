"""Inputs shared by test_ladder_exceptions_cpu.py and test_gpu_ladder_exceptions.py: the scalars at which the exception-free
additions of CurveSecpI's ladder (ec_sw.hpp jac_madd_neg_nx / aff_add_neg_nx) flag a lane, and the oracle's products.

Which exceptional additions a scalar can reach.  Every signed-odd digit is odd, so a prefix of the digits of a half is odd and
the running point a P + b lambda P has a, b odd after a window, both multiples of 16 before the next one's first addition and
a odd, b a multiple of 16 before its second.  R = O, R = Q or R = -Q then needs (a, b) to differ from (0, 0) or from the digit
by a NONZERO vector of the lattice {(x, y): x + lambda y = 0 mod n}, whose shortest vectors are near 2^127: out of reach of the
prefixes before the last window.  So no scalar meets an exceptional addition at window 0 or at a middle window, and the search
of ladder32.ladder_exceptional_scalars finds all there is: k = 0 and k = +-lambda (R = -Q in the last k2 addition, and for
+-lambda the fix-up then starts from R = O).  k = n reaches the same addition as k = 0 and is not
`trivial_zero`.  The other positions are covered where they can be: on the formulas themselves (the CPU test)."""
import numpy as np

import ladder32
from helpers import SECP_LAMBDA as LAM, points_to_wire, scalars_to_wire
from noble_curves_amd._native import SECP256K1
from oracle.curves import SECP256K1_N as N, Secp256k1, makeRng

EDGE = [0, 1, 2, N - 1, N - 2, LAM, N - LAM, LAM + 1, LAM - 1, N - LAM + 1, N - LAM - 1]
FLAGGED = [LAM, N - LAM, 0, N]       # the ladder meets an exceptional addition (k = 0: result known beforehand)


def reachable_events():
    """{(window, addition, kind)} over the model's exceptional scalars"""
    return {ev for evs in ladder32.ladder_exceptional_scalars().values() for ev in evs}


def special_pairs(rng):
    """(k, P): the flagged scalars and the edge list on G, small multiples of G and random points; O as the input point"""
    G = Secp256k1.BASE
    pts = [G, G.multiplyUnsafe(2), G.multiplyUnsafe(3), G.multiplyUnsafe(15)]
    pairs = [(k, p) for k in FLAGGED for p in pts[:2] + [G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)]]
    pairs += [(k, pts[i % 4] if i % 2 else G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)) for i, k in enumerate(EDGE)]
    pairs += [(k, Secp256k1.ZERO) for k in (0, 1, 12345, LAM, N - 1)]
    return pairs


def random_pairs(rng, n, nbase=8):
    """n pairs of a random scalar and one of `nbase` random points"""
    base = [Secp256k1.BASE.multiplyUnsafe(rng.rndBelow(N - 1) + 1) for _ in range(nbase)]
    return [(rng.rndBelow(N - 1) + 1, base[i % nbase]) for i in range(n)]


def wires(pairs):
    return points_to_wire(SECP256K1, [p for _, p in pairs]), scalars_to_wire([k for k, _ in pairs])


def expected(pairs):
    """(affine wire rows, infinity flags) of (k mod n) P by the oracle's C restatement; an infinite result is the all-zero row with
    the flag set"""
    from oracle import cport
    pw, _ = wires(pairs)
    return cport.multiply_unsafe("secp256k1", pw, scalars_to_wire([k % N for k, _ in pairs]))


def expected_python(pairs):
    """the same by the Python oracle (slow: for the special pairs)"""
    res = [p.multiplyUnsafe(k % N) for k, p in pairs]
    zero = Secp256k1.ZERO.toAffine()
    inf = np.array([1 if r.toAffine() == zero else 0 for r in res], dtype=np.uint8)
    return points_to_wire(SECP256K1, res), inf


def rng(seed):
    return makeRng(seed)
