"""CPU checks of the exception-free additions of CurveSecpI's ladder (mulvar.hpp mul_var_lane, ec_sw.hpp jac_madd_neg_nx /
aff_add_neg_nx): the premise on the model of tests/ladder32.py, the two formulas and their `degenerate` verdict on the host
twin, and the host twin of the whole ladder (ht_mul_var, curve 14) against the oracle on the scalars that flag a lane."""
import ctypes

import numpy as np

import hosttest
import ladder32
import ladder_exceptions as LE
from helpers import loose, secp_add, secp_from_jac, secp_jac, secp_neg, secp_rand_point
from oracle.curves import SECP256K1_N as N, SECP256K1_P as P, Secp256k1

CURVE_SECP_FUSED = 14   # ht_mul_var: the ladder of CurveSecpI


def test_model_premise():
    """256 random scalars meet no exceptional addition at all (the ladder's start from two table entries is its first window,
    not an event), and the only additions any scalar can reach are R = -Q in the last k2 addition and the fix-up from R = O:
    ladder_exceptions' docstring has the argument for the other windows.  The scalars congruent to 0 and +-lambda reach them
    too."""
    rng = LE.rng(0x10E0)
    for _ in range(256):
        k = rng.rndBelow(N)
        assert ladder32.ladder_events(k) == [], hex(k)
    assert LE.reachable_events() == {(ladder32.M - 1, 1, "neg"), (ladder32.FIXUP, 1, "inf")}
    for k in LE.FLAGGED:
        assert (ladder32.M - 1, 1, "neg") in ladder32.ladder_events(k), hex(k)
    for k in LE.EDGE:
        assert bool(ladder32.ladder_events(k)) == (k in LE.FLAGGED), hex(k)


def _nx(op, pj, qx, qy):
    """ht_jac_neg_nx: op 0 jac_madd_neg_nx(P, qx, qy), op 1 aff_add_neg_nx((P.X, P.Y), (beta qx, qy)) -> (27 limbs, verdict)"""
    fn = hosttest.lib().ht_jac_neg_nx
    fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    out = np.zeros(28, dtype=np.uint32)
    a, bx, by = (np.ascontiguousarray(np.array(v, dtype=np.uint32)) for v in (pj, qx, qy))
    assert fn(op, a.ctypes.data, bx.ctypes.data, by.ctypes.data, out.ctypes.data) == 0
    return [int(x) for x in out[:27]], bool(out[27])


def test_additions_without_exceptions():
    """Both formulas give -(P + Q) at the loosest limbs of their operand bounds with the verdict clear, and set it for P = Q
    and P = -Q - the "dbl" and "neg" kinds at any window, window 0 included, which no scalar can stage in the whole ladder."""
    rng = LE.rng(0x10E1)
    g = Secp256k1.BASE.toAffine()
    beta = int(Secp256k1.BASE.multiplyUnsafe(LE.LAM).toAffine()[0]) * pow(int(g[0]), -1, P) % P
    psi = lambda q: (beta * q[0] % P, q[1])                         # noqa: E731
    for i in range(24):
        p1, q = secp_rand_point(rng), secp_rand_point(rng)
        z = rng.rndBelow(P - 1) + 1
        got, flag = _nx(0, secp_jac(p1, z), loose(q[0], 2, P), loose(q[1], 3, P))
        assert not flag and secp_from_jac(got) == secp_neg(secp_add(p1, q))
        got, flag = _nx(1, secp_jac(p1, 1), loose(q[0], 2, P), loose(q[1], 3, P))
        assert not flag and secp_from_jac(got) == secp_neg(secp_add(p1, psi(q)))
        for y in (q[1], P - q[1]):                                   # R = Q, R = -Q
            assert _nx(0, secp_jac(q, z), loose(q[0], 2, P), loose(y, 3, P))[1]
            assert _nx(1, secp_jac(psi(q), 1), loose(q[0], 2, P), loose(y, 3, P))[1]


def test_host_twin_on_flagged_lanes():
    """The host twin against the oracle on k in {0, 1, 2, n - 1, n - 2, +-lambda, +-lambda +- 1} and the scalars congruent to 0
    and +-lambda (flagged in the last window; +-lambda then run the fix-up from R = O), on G, small multiples of G and random
    points, on P = O, and on 256 random pairs."""
    rng = LE.rng(0x10E2)
    special = LE.special_pairs(rng)
    pairs = special + LE.random_pairs(rng, 256)
    pw, sw = LE.wires(pairs)
    out, inf = hosttest.mul_var(CURVE_SECP_FUSED, pw, sw)
    exp, exp_inf = LE.expected(pairs)
    assert np.array_equal(inf, exp_inf) and np.array_equal(out, exp)
    py, py_inf = LE.expected_python(special)
    assert np.array_equal(exp[:len(special)], py) and np.array_equal(exp_inf[:len(special)], py_inf)
    assert exp_inf[:len(special)].any() and not exp_inf[len(special):].any()
