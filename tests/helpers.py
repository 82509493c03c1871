"""Shared helpers for parity tests: wire-format marshalling between oracle points and the
C-ABI byte layout (include/ncg.h); the NTT sweep's size bound; raw Fe9 limbs and secp256k1 affine / Jacobian references for the
fused-ladder tests; a model of the secp256k1 ladder's exceptional events."""
import json
import os

import numpy as np

from bn254_helpers import Bn254
from noble_curves_amd._native import (BLS12_381_G1, BLS12_381_G2, BN254_G1, ED25519, FIELD_BYTES, POINT_BYTES, SECP256K1,
                                      ints_to_le, le_to_ints)
from oracle.curves import SECP256K1_N, SECP256K1_P, BlsG1, BlsG2, Ed25519, Secp256k1

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ORACLE_CURVE = {SECP256K1: Secp256k1, BLS12_381_G1: BlsG1, BLS12_381_G2: BlsG2, ED25519: Ed25519, BN254_G1: Bn254}
# the largest transform test_gpu_ntt.py's sweep runs: every NTT pass shape (ntt.hip ntt_schedule) occurs at or below it,
# which test_host_logic.py's test_ntt_sweep_reaches_every_pass_shape checks against the planner
NTT_SWEEP_MAX_LOG2N = 24


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def affine_to_wire(curve, aff):
    """oracle affine tuple -> bytes (x||y little-endian; Fp2 as c0||c1)."""
    fb = FIELD_BYTES[curve]
    x, y = aff
    if curve == BLS12_381_G2:
        parts = [x[0], x[1], y[0], y[1]]
    else:
        parts = [x, y]
    return b"".join(int(p).to_bytes(fb, "little") for p in parts)


def points_to_wire(curve, pts):
    """list of oracle Points -> uint8 [n, POINT_BYTES] (infinity -> all zero)."""
    pb = POINT_BYTES[curve]
    out = np.zeros((len(pts), pb), dtype=np.uint8)
    for i, p in enumerate(pts):
        out[i] = np.frombuffer(affine_to_wire(curve, p.toAffine()), dtype=np.uint8)
    return out


def wire_to_affine(curve, row):
    fb = FIELD_BYTES[curve]
    vals = le_to_ints(np.asarray(row, dtype=np.uint8).reshape(-1, fb), fb)
    if curve == BLS12_381_G2:
        return ((vals[0], vals[1]), (vals[2], vals[3]))
    return (vals[0], vals[1])


def scalars_to_wire(scalars):
    return ints_to_le(scalars, 32)


# ---- raw Fe9 limbs (fe9.hpp: radix 2^29, nine limbs; every limb of a value at bound B is below B * U)
U = (1 << 29) + (1 << 19)
MASK29 = (1 << 29) - 1
SECP_LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72


def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def limbs(v):
    """canonical limbs of 0 <= v < 2^261"""
    return [(v >> (29 * i)) & MASK29 for i in range(8)] + [v >> 232]


def loose(v, B, p):
    """limbs below B*U, each as high as possible, with value = v (mod p): (B*U - 1) in every limb minus the canonical limbs of
    the difference"""
    top = [B * U - 1] * 9
    delta = (val(top) - v) % p
    return [t - ((delta >> (29 * i)) & MASK29) for i, t in enumerate(top)]


# ---- secp256k1 (a = 0, b = 7) in affine coordinates, None = infinity, and Jacobian raw limbs
def secp_add(p1, p2):
    P = SECP256K1_P
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


def secp_neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % SECP256K1_P)


def secp_rand_point(rng):
    q = Secp256k1.BASE.multiplyUnsafe(rng.rndBelow(SECP256K1_N - 1) + 1).toAffine()
    return int(q[0]), int(q[1])


def secp_jac(pt, z, B=2):
    """Jacobian limbs (loose, bound B) of affine pt at Z = z; None = infinity (1, 1, 0) with a literal zero Z"""
    P = SECP256K1_P
    if pt is None:
        return [1] + [0] * 8 + [1] + [0] * 8 + [0] * 9
    x, y = pt
    return loose(x * z * z % P, B, P) + loose(y * z ** 3 % P, B, P) + loose(z, B, P)


def secp_from_jac(l):
    P = SECP256K1_P
    X, Y, Z = val(l[:9]) % P, val(l[9:18]) % P, val(l[18:])
    if Z % P == 0:
        assert Z == 0, "infinity must come back as a literal zero Z"
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi ** 3 % P


# ---- the secp256k1 ladder (mulvar.hpp mul_var_lane for CurveSecpI, k_mul_var_gtab<CurveSecpI, 4, 3, 16>) as a walk of
# coefficients: the running point is r P (r mod n), every window multiplies r by 2^W and adds d1 s1 and d2 s2 lambda, the
# signed-odd digits (scalar.hpp SignedOddWindows) of the odd halves |k1|, |k2| with their signs s1, s2.  A mixed addition
# R + Q is exceptional when R = O (after the ladder's first addition), R = Q (jac_madd_neg doubles) or R = -Q (the sum is O).
LADDER_W, LADDER_M = 4, 33


def signed_odd_digits(k, W=LADDER_W, M=LADDER_M):
    """the M odd digits of odd 0 < k < 2^(W M) - 1, least significant first: k = sum d_i 2^(W i), |d_i| < 2^W"""
    assert k % 2 == 1 and k + 1 < (1 << (W * M))
    t = k | (1 << (W * M))
    return [2 * ((t >> (W * i + 1)) & ((1 << W) - 1)) - ((1 << W) - 1) for i in range(M)]


def ladder_events(k, split):
    """[(window, addition, kind)] of the exceptional additions for scalar k; window 0 is the most significant, addition 0 / 1
    the k1 / k2 stream, kind "inf" (R = O), "dbl" (R = Q) or "neg" (R = -Q).  split(k) -> (k1, k2), the signed odd halves."""
    n = SECP256K1_N
    k1, k2 = split(k)
    d1, d2 = signed_odd_digits(abs(k1)), signed_odd_digits(abs(k2))
    g1, g2 = (-1 if k1 < 0 else 1), (-1 if k2 < 0 else 1)
    r, ev = 0, []
    for w in range(LADDER_M):
        i = LADDER_M - 1 - w
        r = (r << LADDER_W) % n
        for e, q in ((0, g1 * d1[i] % n), (1, g2 * d2[i] * SECP_LAMBDA % n)):
            if r == 0 and (w, e) != (0, 0):
                ev.append((w, e, "inf"))
            elif r == q:
                ev.append((w, e, "dbl"))
            elif (r + q) % n == 0:
                ev.append((w, e, "neg"))
            r = (r + q) % n
    assert r == k % n
    return ev


def ladder_exceptional_scalars(split, bound=33):
    """{k: events} over k = a + b lambda (mod n), |a|, |b| <= bound, for the scalars whose ladder meets an exceptional addition.
    The running point before an addition of the last window is k - q1 - q2 or k - q2 (q1 = d1 s1, q2 = d2 s2 lambda, |d| < 16),
    so an event there needs k = a + b lambda with |a|, |b| <= 30.  An event in an earlier window would need a prefix of the
    halves (below 2^126) to differ from a digit by a nonzero lattice vector (those of the split's basis have a coordinate
    above 2^127); test_fe9_fused.py::test_ladder_model checks on random scalars that none occurs."""
    n = SECP256K1_N
    hits = {}
    for a in range(-bound, bound + 1):
        for b in range(-bound, bound + 1):
            k = (a + b * SECP_LAMBDA) % n
            ev = ladder_events(k, split)
            if ev:
                hits[k] = ev
    return hits
