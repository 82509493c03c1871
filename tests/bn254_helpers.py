"""bn254 G1 (src/bn254.ts, alt_bn128 / EIP-196) for the tests: the curve built from the generic oracle, the wire helpers, and
the operand cases of the radix-2^29 Montgomery field form (fe9m.hpp) shared by the host twin and ncg_field_check field 9."""
import ctypes

import numpy as np

from oracle.curves import makeRng
from oracle.field import Field
from oracle.weierstrass import weierstrass

BN254_P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
BN254_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BN254_CURVE = dict(p=BN254_P, n=BN254_R, h=1, a=0, b=3, Gx=1, Gy=2)
Bn254 = weierstrass(BN254_CURVE, Field(BN254_P), Field(BN254_R), name="bn254_G1")
BN254_G1 = 5

M29 = (1 << 29) - 1
MONT_R = 1 << 261
RINV = pow(MONT_R, -1, BN254_P)


def to_wire(pts):
    """oracle Points -> uint8 [n, 64] (x || y, 32-byte LE each; ZERO -> zeros)."""
    out = np.zeros((len(pts), 64), dtype=np.uint8)
    for i, p in enumerate(pts):
        x, y = p.toAffine()
        out[i] = np.frombuffer(int(x).to_bytes(32, "little") + int(y).to_bytes(32, "little"), dtype=np.uint8)
    return out


def from_wire(row):
    b = bytes(np.asarray(row, dtype=np.uint8))
    return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")


def scalars_wire(ks):
    return np.array([np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint8) for k in ks], dtype=np.uint8).reshape(-1, 32)


def rand_point(rng):
    return Bn254.BASE.multiplyUnsafe(rng.rndBelow(BN254_R - 1) + 1)


# ---- the field form -------------------------------------------------------------------------------------------------
def val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def spread(v, A, rng, loosest=False):
    """v (below 2 A p) as 9 limbs below A 2^29, the low limbs as loose as the value lets them be."""
    out = []
    for _ in range(8):
        low = v & M29
        kmax = min(A - 1, v >> 29)
        k = kmax if loosest else rng.rndBelow(kmax + 1)
        out.append(low + (k << 29))
        v = (v - out[-1]) >> 29
    out.append(v)
    assert all(x < (A << 29) for x in out)
    return out


def elem(rng, A, i):
    """the i-th operand of bound A: the extremes first, then random values below 2 A p"""
    top = 2 * A * BN254_P
    special = [top - 1, 0, BN254_P - 1, BN254_P, 1, top - BN254_P, (1 << 254) - 1 if A > 1 else BN254_P + 7]
    v = special[i] if i < len(special) else rng.rndBelow(top)
    return spread(v, A, rng, loosest=i % 2 == 0)


def in_bound(limbs, B):
    return all(x < (B << 29) for x in limbs) and val(limbs) < 2 * B * BN254_P


VARIANTS = (11, 12, 22, 23, 32, 17, 71, 33, 77)
OPS = range(9)


def fe9m_cases(rows=24):
    """{(op, variant): (a rows, b rows, check)}: ncg_field_check field 9 / ht_fe9m_op numbering (include/ncg.h)."""
    p = BN254_P
    rng = makeRng(0xB254)
    cases = {}
    for variant in VARIANTS:
        A, B = divmod(variant, 10)
        a_rows = [elem(rng, A, i) for i in range(rows)]
        b_rows = [elem(rng, B, (i * 5 + 3) % rows) for i in range(rows)]
        for op in OPS:
            ra, rb = a_rows, b_rows
            if op == 8:  # canonical residues as 8 LE words
                vs = [0, 1, p - 1, p - 2] + [rng.rndBelow(p) for _ in range(rows - 4)]
                ra = [[(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)] + [0] for v in vs]
            cases[(op, variant)] = (ra, rb, _checker(op, A, B))
    return cases


def _checker(op, A, B):
    p = BN254_P

    def check(a, b, out):
        va, vb, vo = val(a), val(b), val(out)
        if op == 0:
            assert vo % p == va * vb * RINV % p and in_bound(out, 1) and all(x <= M29 for x in out[:8])
        elif op == 1:
            assert vo % p == va * va * RINV % p and in_bound(out, 1) and all(x <= M29 for x in out[:8])
        elif op == 2:
            if A + B <= 7:
                assert list(out) == [x + y for x, y in zip(a, b)]
            else:
                assert vo == 0
        elif op == 3:
            if A + B + 1 <= 7:
                assert vo % p == (va - vb) % p and in_bound(out, A + B + 1)
            else:
                assert vo == 0
        elif op == 4:
            if A + 1 <= 7:
                assert vo % p == (-va) % p and in_bound(out, A + 1) and (vo != 0 or va % p == 0)
                if va == 0:
                    assert vo == 0                      # the literal zero of the identity stays zero
            else:
                assert vo == 0
        elif op == 5:
            exp = MONT_R * MONT_R * pow(va, -1, p) % p if va % p else 0
            assert vo % p == exp and in_bound(out, 1)
        elif op == 6:
            assert vo % p == va % p and vo < 2 * p and all(x <= M29 for x in out[:8])
        elif op == 7:
            assert sum(int(x) << (32 * j) for j, x in enumerate(out[:8])) == va * RINV % p and out[8] == 0
        elif op == 8:
            x = sum(int(w) << (32 * j) for j, w in enumerate(a[:8]))
            assert vo % p == x * MONT_R % p and in_bound(out, 1)
    return check


def ht_fe9m_op(op, variant, a, b):
    """the host twin (hosttest.hip ht_fe9m_op): (out limbs, overflow count)"""
    import hosttest
    lib = hosttest.lib()
    lib.ht_fe9m_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    x = np.array(a, dtype=np.uint32)
    y = np.array(b, dtype=np.uint32)
    r = np.zeros(9, dtype=np.uint32)
    ovf = lib.ht_fe9m_op(op, variant, x.ctypes.data, y.ctypes.data, r.ctypes.data)
    return [int(v) for v in r], ovf
