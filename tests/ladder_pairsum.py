"""The walk of the pair-sum ladder of the secp256k1 batch multiply (csrc/mulvar_pairsum.hpp): ladder32's split and digits, but
every window adds ONE point, the affine sum S_w = d1 s1 P + d2 s2 lambda P of its two table entries, so the state between the
two additions of a window does not exist.  Shared by test_pairsum_cpu.py and test_gpu_pairsum.py.

Which scalars flag a lane.  S_w itself is exceptional only when d1 s1 = +-d2 s2 lambda (mod n) with |d| < 16 - a lattice vector
far shorter than the shortest (near 2^127) - so never on a point of the group.  R + S_w is exceptional when the prefix (a, b) of
the halves, a and b multiples of 16 after the doublings, differs from -+(d1 s1, d2 s2) by a lattice vector: the zero vector is
out (a digit is odd), a non-zero one is out of reach of the prefixes before the last window.  In the last window R = k - S_w
(k2 odd) or k + s2 lambda - S_w (k2 even, recoded as |k2| + 1), and the fix-up for an even k2 adds -s2 lambda to R: the search
below over k = a + b lambda with small a, b finds all there is."""
import ctypes

import numpy as np

import hosttest
import ladder32
from helpers import SECP_LAMBDA, signed_odd_digits
from oracle.curves import SECP256K1_N

W, M, FIXUP = ladder32.W, ladder32.M, ladder32.FIXUP


def pair_sums(k, split=ladder32.split_k1_odd):
    """([S_0 .. S_31] as coefficients of P mod n, most significant window first; the fix-up's coefficient or None)"""
    n = SECP256K1_N
    k1, k2 = split(k)
    e2 = k2 % 2 == 0
    d1, d2 = signed_odd_digits(abs(k1), W, M), signed_odd_digits(abs(k2) + e2, W, M)
    g1, g2 = (-1 if k1 < 0 else 1), (-1 if k2 < 0 else 1)
    return ([(g1 * d1[M - 1 - w] + g2 * d2[M - 1 - w] * SECP_LAMBDA) % n for w in range(M)],
            (-g2 * SECP_LAMBDA % n) if e2 else None)


def ladder_events(k, split=ladder32.split_k1_odd):
    """[(window, kind)] of the exceptional additions for scalar k: kinds "inf" (R = O), "dbl" (R = S), "neg" (R = -S), and "sum"
    for a pair sum that is itself exceptional (S_w = O or a doubling); window FIXUP is the addition after the last window."""
    n = SECP256K1_N
    sums, fix = pair_sums(k, split)
    ev = []
    r = sums[0]
    if r == 0:
        ev.append((0, "sum"))
    for w in range(1, M):
        r = (r << W) % n
        q = sums[w]
        if q == 0:
            ev.append((w, "sum"))
        if r == 0:
            ev.append((w, "inf"))
        elif r == q:
            ev.append((w, "dbl"))
        elif (r + q) % n == 0:
            ev.append((w, "neg"))
        r = (r + q) % n
    if fix is not None:
        if r == 0:
            ev.append((FIXUP, "inf"))
        elif r == fix:
            ev.append((FIXUP, "dbl"))
        elif (r + fix) % n == 0:
            ev.append((FIXUP, "neg"))
        r = (r + fix) % n
    assert r == k % n
    return ev


def flagging_scalars(bound=34):
    """{k: events} over k = a + b lambda (mod n), |a|, |b| <= bound: every scalar whose lane is flagged on a point of the group"""
    hits = {}
    for a in range(-bound, bound + 1):
        for b in range(-bound, bound + 1):
            k = (a + b * SECP_LAMBDA) % SECP256K1_N
            ev = ladder_events(k)
            if ev:
                hits[k] = ev
    return hits


def min_n():
    """PAIRSUM_MIN_N: the item count from which mul_var_batch takes the pair-sum path on the device"""
    return int(hosttest.lib().ht_pairsum_min_n())


# layout of the twin's dump of item 0 (PairSumCfg<CurveSecpI, 4>): the table, the lane's column (pre_1 .. pre_31, Zg), acc, 1 / acc
FW, TS = 9, 8
PRE_OFF = TS * 2 * FW
ZG_OFF = PRE_OFF + (M - 1) * FW
ACC_OFF = ZG_OFF + FW


def mul_var(pts, scalars, dump=False):
    """the host twin of the four kernels -> (affine wire rows, infinity flags, lane flags[, dump words of item 0]);
    lane flags: bit 0 the prepare lane's flag, bit 1 the lane went through the complete ladder"""
    lib = hosttest.lib()
    vp = ctypes.c_void_p
    lib.ht_mul_var_pairsum.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int]
    pts = np.ascontiguousarray(pts, dtype=np.uint8)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint8)
    n = pts.shape[0]
    out, inf, flags = np.zeros_like(pts), np.zeros((n,), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
    dbg = np.zeros((lib.ht_pairsum_dbg_words(),), dtype=np.uint32)
    assert lib.ht_mul_var_pairsum(pts.ctypes.data, scalars.ctypes.data, out.ctypes.data, inf.ctypes.data, flags.ctypes.data,
                                  dbg.ctypes.data if dump else None, n) == 0
    return (out, inf, flags, dbg) if dump else (out, inf, flags)
