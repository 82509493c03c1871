"""CPU execution of the fused Fe9 expressions (fe9.hpp f_mul_mul / f_mul_sqr / f_mul_add / f_sqr_add / f_half), the negated
ladder formulas built on them (ec_sw.hpp jac_dbl_neg / jac_madd_neg), the odd GLV halves (scalar.hpp secp_glv_make_odd) and
the ladder that uses all three (CurveSecpI) against big-integer arithmetic and the oracle."""
import ctypes

import numpy as np
import pytest

import hosttest
from helpers import ORACLE_CURVE, points_to_wire, scalars_to_wire, wire_to_affine
from noble_curves_amd._native import SECP256K1
from oracle.curves import ED25519_P, SECP256K1_N, SECP256K1_P, Secp256k1, makeRng

U = (1 << 29) + (1 << 19)
MASK = (1 << 29) - 1
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
CURVE_SECP_FUSED = 14   # ht_mul_var: the ladder of CurveSecpI


def _lib():
    lib = hosttest.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.ht_fe9_fused.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    lib.ht_jac_neg.argtypes = [i32, vp, vp, vp, vp]
    lib.ht_glv_split_odd.argtypes = [vp, vp]
    return lib


def _arr(limbs):
    return np.ascontiguousarray(np.array(limbs, dtype=np.uint32))


def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def loose(v, B, p):
    """limbs below B*U, each as high as possible, with value = v (mod p): (B*U - 1) in every limb minus the canonical limbs of
    the difference"""
    top = [B * U - 1] * 9
    delta = (val(top) - v) % p
    return [t - ((delta >> (29 * i)) & MASK) for i, t in enumerate(top)]


def fused(fid, op, variant, a, b, c, d):
    out = np.zeros(9, dtype=np.uint32)
    arrs = [_arr(x) for x in (a, b, c, d)]
    assert _lib().ht_fe9_fused(fid, op, variant, *[x.ctypes.data for x in arrs], out.ctypes.data) == 0
    return [int(x) for x in out]


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


def _aff_add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def _neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


def _rand_point(rng):
    q = Secp256k1.BASE.multiplyUnsafe(rng.rndBelow(SECP256K1_N - 1) + 1).toAffine()
    return int(q[0]), int(q[1])


def _jac(pt, z, B=2):
    """Jacobian limbs (loose, bound B) of affine pt at Z = z; None = infinity (1, 1, 0) with a literal zero Z"""
    if pt is None:
        return [1] + [0] * 8 + [1] + [0] * 8 + [0] * 9
    x, y = pt
    return loose(x * z * z % P, B, P) + loose(y * z ** 3 % P, B, P) + loose(z, B, P)


def _from_jac(l):
    X, Y, Z = val(l[:9]) % P, val(l[9:18]) % P, val(l[18:])
    if Z % P == 0:
        assert Z == 0, "infinity must come back as a literal zero Z"
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi ** 3 % P


def jac_neg(op, pj, qx=None, qy=None):
    out = np.zeros(27, dtype=np.uint32)
    a = _arr(pj)
    bx = _arr(qx if qx is not None else [0] * 9)
    by = _arr(qy if qy is not None else [0] * 9)
    assert _lib().ht_jac_neg(op, a.ctypes.data, bx.ctypes.data, by.ctypes.data, out.ctypes.data) == 0
    r = [int(x) for x in out]
    assert max(r) < 2 * U
    return r


def test_negated_doubling_and_mixed_addition():
    """jac_dbl_neg = -(2P) and jac_madd_neg = -(P + Q) at the loosest limbs of their operand bounds (P at 2, qx at 2, qy at 3),
    including P = Q, P = -Q, P = infinity and Q = infinity."""
    rng = makeRng(0x5E9)
    for i in range(24):
        p1 = _rand_point(rng)
        z = rng.rndBelow(P - 1) + 1
        assert _from_jac(jac_neg(0, _jac(p1, z))) == _neg(_aff_add(p1, p1))
        q = _rand_point(rng) if i % 4 else p1
        assert _from_jac(jac_neg(1, _jac(p1, z), loose(q[0], 2, P), loose(q[1], 3, P))) == _neg(_aff_add(p1, q))
    p1 = _rand_point(rng)
    z = rng.rndBelow(P - 1) + 1
    # P = Q (doubling through the exceptional branch), P = -Q (infinity)
    assert _from_jac(jac_neg(1, _jac(p1, z), loose(p1[0], 2, P), loose(p1[1], 3, P))) == _neg(_aff_add(p1, p1))
    assert _from_jac(jac_neg(1, _jac(p1, z), loose(p1[0], 2, P), loose(P - p1[1], 3, P))) is None
    # P = infinity: -Q;  Q = infinity (literal (0, 0)): -P;  doubling infinity stays infinity
    assert _from_jac(jac_neg(1, _jac(None, 1), loose(p1[0], 2, P), loose(p1[1], 3, P))) == _neg(p1)
    assert _from_jac(jac_neg(1, _jac(p1, z), [0] * 9, [0] * 9)) == _neg(p1)
    assert _from_jac(jac_neg(0, _jac(None, 1))) is None


# ---- odd GLV halves
def glv_split_odd(k):
    out = np.zeros(12, dtype=np.uint32)
    kk = np.frombuffer(int(k % (1 << 256)).to_bytes(32, "little"), dtype=np.uint32).copy()
    assert _lib().ht_glv_split_odd(kk.ctypes.data, out.ctypes.data) == 0
    k1 = sum(int(out[i]) << (32 * i) for i in range(5))
    k2 = sum(int(out[5 + i]) << (32 * i) for i in range(5))
    return (-k1 if out[10] else k1), (-k2 if out[11] else k2)


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


# ---- the fused-formula ladder on the CPU
def test_fused_ladder_matches_oracle():
    n = SECP256K1_N
    rng = makeRng(0xF1AD)
    ks = [0, 1, 2, 3, 4, 5, n - 1, n - 2, n - 3, 1 << 128, (1 << 128) - 1, (1 << 128) + 1, LAM, LAM + 1, n - LAM, 15, 16, 17,
          (1 << 255), n // 2]
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
