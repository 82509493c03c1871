"""CPU execution of the fused Fe9 expressions (fe9.hpp f_mul_mul / f_mul_sqr / f_mul_add / f_sqr_add / f_half), the negated
ladder formulas built on them (ec_sw.hpp jac_dbl_neg / jac_madd_neg), the odd GLV halves (scalar.hpp secp_glv_make_odd) and
the ladder that uses all three (CurveSecpI) against big-integer arithmetic and the oracle."""
import pytest

import hosttest
from helpers import (ORACLE_CURVE, SECP_LAMBDA as LAM, U, ladder_events, ladder_exceptional_scalars, loose, points_to_wire,
                     scalars_to_wire, secp_add, secp_from_jac, secp_jac, secp_neg, secp_rand_point, signed_odd_digits, val,
                     wire_to_affine)
from noble_curves_amd._native import SECP256K1
from oracle.curves import ED25519_P, SECP256K1_N, SECP256K1_P, Secp256k1, makeRng

CURVE_SECP_FUSED = 14   # ht_mul_var: the ladder of CurveSecpI


def fused(fid, op, variant, a, b, c, d):
    return hosttest.fe9_fused(fid, op, variant, a, b, c, d)


# (op, variants A B C D): op 0 a*b + c*d, 1 a*b + c^2, 2 a*b + c, 3 a^2 + c, 4 a / 2
CASES = [(0, (1111, 1322, 3211, 2311, 1123, 3121)), (1, (1111, 1322, 3211, 2311, 3121)), (2, (1111, 1327, 7171, 1771, 2171)),
         (3, (1111, 1327, 2171)), (4, (1111, 1771))]


@pytest.mark.parametrize("fid,p", [(0, SECP256K1_P), (1, ED25519_P)])
def test_fused_expressions_at_their_bounds(fid, p):
    """Every fused entry point on random limbs and on the loosest limbs each bound admits: the value mod p, and output limbs
    below U (below 2U for the halving)."""
    rng = makeRng(0xF5ED + fid)

    def operand(B, kind):
        if kind == 0:
            return [B * U - 1] * 9
        if kind == 1:
            return loose(rng.rndBelow(p), B, p)
        if kind == 2:
            return [0] * 8 + [B * U - 1]
        return [rng.rndBelow(B * U) for _ in range(9)]

    for op, variants in CASES:
        for variant in variants:
            A, B, C, D = (variant // 1000, variant // 100 % 10, variant // 10 % 10, variant % 10)
            for kind in range(16):
                a, b = operand(A, kind % 4), operand(B, (kind // 4) % 4)
                c, d = operand(C, (kind + 1) % 4), operand(D, (kind // 2) % 4)
                va, vb, vc, vd = val(a), val(b), val(c), val(d)
                r = fused(fid, op, variant, a, b, c, d)
                exp = {0: va * vb + vc * vd, 1: va * vb + vc * vc, 2: va * vb + vc, 3: va * va + vc,
                       4: va * pow(2, -1, p)}[op]
                assert val(r) % p == exp % p, (op, variant, kind)
                assert max(r) < (2 * U if op == 4 else U), (op, variant, kind)


# ---- the negated Jacobian formulas, secp256k1 (a = 0, b = 7)
P = SECP256K1_P


def jac_neg(op, pj, qx=None, qy=None):
    r = hosttest.jac_neg(op, pj, qx, qy)
    assert max(r) < 2 * U
    return r


def test_negated_doubling_and_mixed_addition():
    """jac_dbl_neg = -(2P) and jac_madd_neg = -(P + Q) at the loosest limbs of their operand bounds (P at 2, qx at 2, qy at 3),
    including P = Q, P = -Q, P = infinity and Q = infinity."""
    rng = makeRng(0x5E9)
    for i in range(24):
        p1 = secp_rand_point(rng)
        z = rng.rndBelow(P - 1) + 1
        assert secp_from_jac(jac_neg(0, secp_jac(p1, z))) == secp_neg(secp_add(p1, p1))
        q = secp_rand_point(rng) if i % 4 else p1
        assert secp_from_jac(jac_neg(1, secp_jac(p1, z), loose(q[0], 2, P), loose(q[1], 3, P))) == secp_neg(secp_add(p1, q))
    p1 = secp_rand_point(rng)
    z = rng.rndBelow(P - 1) + 1
    # P = Q (doubling through the exceptional branch), P = -Q (infinity)
    assert secp_from_jac(jac_neg(1, secp_jac(p1, z), loose(p1[0], 2, P), loose(p1[1], 3, P))) == secp_neg(secp_add(p1, p1))
    assert secp_from_jac(jac_neg(1, secp_jac(p1, z), loose(p1[0], 2, P), loose(P - p1[1], 3, P))) is None
    # P = infinity: -Q;  Q = infinity (literal (0, 0)): -P;  doubling infinity stays infinity
    assert secp_from_jac(jac_neg(1, secp_jac(None, 1), loose(p1[0], 2, P), loose(p1[1], 3, P))) == secp_neg(p1)
    assert secp_from_jac(jac_neg(1, secp_jac(p1, z), [0] * 9, [0] * 9)) == secp_neg(p1)
    assert secp_from_jac(jac_neg(0, secp_jac(None, 1))) is None


# ---- odd GLV halves
glv_split_odd = hosttest.glv_split_odd


def test_glv_odd_halves():
    """Both halves odd, k = k1 + lambda k2 (mod n), |ki| < 2^130; edge scalars and every parity case of the plain split."""
    n = SECP256K1_N
    rng = makeRng(0x0DD)
    ks = [0, 1, 2, 3, n - 1, n - 2, n // 2, LAM, n - LAM, 1 << 128, (1 << 256) - 1]
    ks += [rng.rndBelow(n) for _ in range(4000)]
    seen = set()
    for k in ks:
        _, k1, _, k2 = hosttest.glv_split(k)
        seen.add((k1 % 2, k2 % 2))
        s1, s2 = glv_split_odd(k)
        assert s1 % 2 == 1 and s2 % 2 == 1, hex(k)
        assert (s1 + LAM * s2 - k) % n == 0, hex(k)
        assert abs(s1) < (1 << 130) and abs(s2) < (1 << 130), hex(k)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- the ladder model (helpers.ladder_events): which scalars make CurveSecpI's ladder meet R = O, R = Q or R = -Q
def test_ladder_model():
    """The signed-odd recoding gives back |k1|, |k2|; random scalars meet no exceptional addition before the last window (the
    first addition, from R = O, is the ladder's start and not counted); the search over k = a + b lambda finds exactly k = 0
    (R = -Q in the last addition: the result is O) and k = -26 lambda (R = Q in the last addition: jac_madd_neg doubles)."""
    n = SECP256K1_N
    rng = makeRng(0x1ADE)
    ks = [1, 2, n - 1, LAM, n - LAM, 1 << 128, (1 << 256) - 1] + [rng.rndBelow(n) for _ in range(4000)]
    for k in ks:
        for h in glv_split_odd(k):
            d = signed_odd_digits(abs(h))
            assert sum(x << (4 * i) for i, x in enumerate(d)) == abs(h) and all(x % 2 and abs(x) < 16 for x in d)
        assert all(w == 32 for w, _, _ in ladder_events(k, glv_split_odd)), hex(k)
    assert ladder_events((-26 * LAM) % n, glv_split_odd) == [(32, 1, "dbl")]
    assert ladder_events(0, glv_split_odd) == [(32, 1, "neg")]
    assert ladder_exceptional_scalars(glv_split_odd) == {0: [(32, 1, "neg")], (-26 * LAM) % n: [(32, 1, "dbl")]}


# ---- the fused-formula ladder on the CPU
def test_fused_ladder_matches_oracle():
    n = SECP256K1_N
    rng = makeRng(0xF1AD)
    ks = [0, 1, 2, 3, 4, 5, n - 1, n - 2, n - 3, 1 << 128, (1 << 128) - 1, (1 << 128) + 1, LAM, LAM + 1, n - LAM, 15, 16, 17,
          (1 << 255), n // 2]
    ks += sorted(ladder_exceptional_scalars(glv_split_odd))   # the scalars of the model's exceptional additions (0, -26 lambda)
    ks += [rng.rndBelow(n) for _ in range(60)]
    pts = [Secp256k1.BASE.multiplyUnsafe(rng.rndBelow(n - 1) + 1) for _ in ks]
    pts[3] = Secp256k1.ZERO
    pts[7] = Secp256k1.BASE
    out, inf = hosttest.mul_var(CURVE_SECP_FUSED, points_to_wire(SECP256K1, pts), scalars_to_wire(ks))
    Pt = ORACLE_CURVE[SECP256K1]
    for i, (p, k) in enumerate(zip(pts, ks)):
        exp = p.multiplyUnsafe(k).toAffine()
        assert wire_to_affine(SECP256K1, out[i]) == exp, (i, hex(k))
        assert bool(inf[i]) == (exp == Pt.ZERO.toAffine())
