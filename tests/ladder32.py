"""The split and the walk of CurveSecpI's ladder since it runs 32 windows per half (mulvar.hpp mul_var_lane with
scalar.hpp secp_glv_make_k1_odd): k1 odd, k2 of either parity; an even k2 is recoded as |k2| + 1 and psi(P) taken back out by
one mixed addition after the last window.  Shared by test_ladder32.py (CPU) and test_gpu_ladder32.py."""
import ctypes
import os
import re

import numpy as np

import hosttest
from helpers import SECP_LAMBDA, signed_odd_digits
from oracle.curves import SECP256K1_N

W, M = 4, 32            # MulVarCfg<CurveSecpI, 4>: KBITS 128
FIXUP = M               # window index of ladder_events' fix-up addition (after the last window)


def split_k1_odd_words(k):
    """secp_glv_split + secp_glv_make_k1_odd of k (host twin ht_glv_split_k1_odd): the 12 words k1[5] k2[5] k1neg k2neg"""
    lib = hosttest.lib()
    fn = lib.ht_glv_split_k1_odd
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    out = np.zeros(12, dtype=np.uint32)
    kk = np.frombuffer(int(k % (1 << 256)).to_bytes(32, "little"), dtype=np.uint32).copy()
    assert fn(kk.ctypes.data, out.ctypes.data) == 0
    return [int(x) for x in out]


def split_k1_odd(k):
    """the signed halves (k1, k2) of k: k1 odd"""
    return hosttest.split_words_to_ints(split_k1_odd_words(k))


def ladder_events(k, split=split_k1_odd):
    """[(window, addition, kind)] of the exceptional mixed additions for scalar k, as helpers.ladder_events, plus the fix-up:
    window FIXUP, addition 1, when k2 is even.  Kinds "inf" (R = O), "dbl" (R = Q), "neg" (R = -Q)."""
    n = SECP256K1_N
    k1, k2 = split(k)
    e2 = k2 % 2 == 0
    d1, d2 = signed_odd_digits(abs(k1), W, M), signed_odd_digits(abs(k2) + e2, W, M)
    g1, g2 = (-1 if k1 < 0 else 1), (-1 if k2 < 0 else 1)
    adds = []
    for w in range(M):
        i = M - 1 - w
        adds.append((w, 0, g1 * d1[i] % n))
        adds.append((w, 1, g2 * d2[i] * SECP_LAMBDA % n))
    if e2:
        adds.append((FIXUP, 1, -g2 * SECP_LAMBDA % n))
    r, ev = 0, []
    for w, e, q in adds:
        if e == 0 and w > 0:      # W doublings in front of each window's first addition; none before the fix-up
            r = (r << W) % n
        if r == 0 and (w, e) != (0, 0):
            ev.append((w, e, "inf"))
        elif r == q:
            ev.append((w, e, "dbl"))
        elif (r + q) % n == 0:
            ev.append((w, e, "neg"))
        r = (r + q) % n
    assert r == k % n
    return ev


def ladder_exceptional_scalars(split=split_k1_odd, bound=34):
    """{k: events} over k = a + b lambda (mod n), |a|, |b| <= bound, for the scalars whose ladder meets an exceptional addition.
    Before an addition of the last window or the fix-up the running point is k minus at most d1 s1 + d2 s2 lambda + s2 lambda
    (|d| < 16), so an event there needs |a| <= 30 and |b| <= 32; earlier windows would need a prefix of the halves to differ from a
    digit by a nonzero lattice vector, which random scalars check (test_ladder32.py)."""
    n = SECP256K1_N
    hits = {}
    for a in range(-bound, bound + 1):
        for b in range(-bound, bound + 1):
            k = (a + b * SECP_LAMBDA) % n
            ev = ladder_events(k, split)
            if ev:
                hits[k] = ev
    return hits


def _glv_const(name):
    """SecpGlv::<name> (consts_gen.hpp) as an integer"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "noble-curves_amd", "csrc",
                            "consts_gen.hpp")).read()
    body = src[src.index("struct SecpGlv {"):]
    words = re.search(r"\b%s\[\d+\] = \{([^}]*)\}" % name, body).group(1)
    return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words.split(",")))


def babai_boundary_scalars(rng, per_constant=64):
    """k < n with k g / 2^384 within 2^-20 of a half-integer, for g = g1 and g = g2 of secp_glv_split (where its rounding
    flips): both neighbours of (t + 1/2) 2^384 / g for t = 0, the largest t and random t"""
    n = SECP256K1_N
    ks = []
    for g in (_glv_const("G1"), _glv_const("G2")):
        tmax = (n - 1) * g >> 384
        for j in range(per_constant):
            t = 0 if j == 0 else tmax if j == 1 else rng.rndBelow(tmax)
            k0 = ((2 * t + 1) << 383) // g
            for k in (k0, k0 + 1):
                if k < n:
                    assert abs((k * g) % (1 << 384) - (1 << 383)) < 1 << (384 - 20)
                    ks.append(k)
    return ks


def check_split(k, k1, k2):
    """the contract of secp_glv_make_k1_odd for one scalar"""
    assert k1 % 2 == 1, hex(k)
    assert (k1 + SECP_LAMBDA * k2 - k) % SECP256K1_N == 0, hex(k)
    assert abs(k1) < (1 << 128) and abs(k2) + 1 < (1 << 128), hex(k)
