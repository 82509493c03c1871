"""GPU parity of what the fused secp256k1 ladder (CurveSecpI) runs: the fused Fe9 expressions (fe9.hpp, the generated
v_mad_u64_u32 column blocks of fe9_asm_gen.hpp), the negated formulas jac_dbl_neg / jac_madd_neg with their exceptional
branch (ec_sw.hpp), the odd GLV halves (scalar.hpp secp_glv_make_odd) and the ladder itself.  The pieces go through
ncg_field_check fields 5 / 6 / 7 on raw limbs; every expected value comes from Python big integers or the oracle, and the raw
output limbs are compared with the host twin's (tests/hosttest.py) as well."""
import os
import re

import numpy as np
import pytest

import hosttest
from helpers import (LADDER_M, ORACLE_CURVE, SECP_LAMBDA as LAM, U, ladder_events, ladder_exceptional_scalars, limbs, loose,
                     points_to_wire, scalars_to_wire, secp_add, secp_from_jac, secp_jac, secp_neg, secp_rand_point, val,
                     wire_to_affine)
from noble_curves_amd import get_engine
from noble_curves_amd._native import SECP256K1
from oracle.curves import ED25519_P, SECP256K1_N, SECP256K1_P, Secp256k1, makeRng

pytestmark = pytest.mark.gpu

N = SECP256K1_N
P = SECP256K1_P
FIELD_FUSED = {SECP256K1_P: 5, ED25519_P: 6}     # ncg_field_check field ids; hosttest.fe9_fused: 0 / 1
FIELD_LADDER = 7
# (op, variants A B C D) of hosttest.hip ht_fe9_fused_t: op 0 a*b + c*d, 1 a*b + c^2, 2 a*b + c, 3 a^2 + c, 4 a / 2
CASES = [(0, (1111, 1322, 3211, 2311, 1123, 3121)), (1, (1111, 1322, 3211, 2311, 3121)), (2, (1111, 1327, 7171, 1771, 2171)),
         (3, (1111, 1327, 2171)), (4, (1111, 1771))]
ITEMS = 2048 + 40         # every wave mixes operand kinds, and the last one is partial


def _exceptional_lanes(n):
    """lanes 0, 31, 32, 63 of every full wave and three lanes of the final partial wave (n % 64 != 0)"""
    assert n % 64
    full = n - n % 64
    return sorted({w + o for w in range(0, full, 64) for o in (0, 31, 32, 63)} | {full, full + (n % 64) // 2, n - 1})


# ---- fused expressions, both primes, every (op, variant)
@pytest.mark.parametrize("p", [SECP256K1_P, ED25519_P], ids=["secp256k1", "ed25519"])
def test_fused_expressions_on_device(p):
    """All 16 operand-kind combinations of the CPU test (all limbs at the bound, loosest form of a random value, top limb only,
    random limbs) and the special values 0, 1, p - 1, (p - 1) / 2, p, 2p (canonical and loosest limbs), mixed in every wave:
    the value mod p, output limbs below U (2U for the halving), and the raw limbs equal to the host twin's."""
    eng = get_engine()
    fid = FIELD_FUSED[p]
    rng = makeRng(0xF5ED6 + fid)
    specials = [0, 1, p - 1, (p - 1) // 2, p, 2 * p]

    def operand(B, kind):
        if kind == 0:
            return [B * U - 1] * 9
        if kind == 1:
            return loose(rng.rndBelow(p), B, p)
        if kind == 2:
            return [0] * 8 + [B * U - 1]
        if kind == 3:
            return [rng.rndBelow(B * U) for _ in range(9)]
        s = specials[rng.rndBelow(len(specials))]
        return limbs(s) if kind == 4 else loose(s, B, p)

    inv2 = pow(2, -1, p)
    for op, variants in CASES:
        for variant in variants:
            A, B, C, D = (variant // 1000, variant // 100 % 10, variant // 10 % 10, variant % 10)
            ops = []
            for i in range(ITEMS):
                kind = i % 16 if i % 3 == 0 else rng.rndBelow(16)
                ka, kb, kc, kd = kind % 4, (kind // 4) % 4, (kind + 1) % 4, (kind // 2) % 4
                if i % 5 == 1:      # special values
                    ka, kb, kc, kd = (4 + rng.rndBelow(2) for _ in range(4))
                ops.append((operand(A, ka), operand(B, kb), operand(C, kc), operand(D, kd)))
            ac = np.array([a + c for a, _, c, _ in ops], dtype=np.uint32)
            bd = np.array([b + d for _, b, _, d in ops], dtype=np.uint32)
            out = eng.field_check(fid, op, variant, ac, bd)
            for i, (a, b, c, d) in enumerate(ops):
                r = [int(x) for x in out[i]]
                va, vb, vc, vd = val(a), val(b), val(c), val(d)
                exp = {0: va * vb + vc * vd, 1: va * vb + vc * vc, 2: va * vb + vc, 3: va * va + vc, 4: va * inv2}[op]
                assert val(r) % p == exp % p, (op, variant, i)
                assert max(r) < (2 * U if op == 4 else U), (op, variant, i, r)
                assert r == hosttest.fe9_fused(fid - 5, op, variant, a, b, c, d), (op, variant, i)


# ---- the negated formulas: generic items with the exceptional ones at lanes 0, 31, 32, 63 and in a final partial wave
def _walk(rng, n):
    """n distinct affine points: P, P + S, P + 2S, ..."""
    pt, step = secp_rand_point(rng), secp_rand_point(rng)
    out = []
    for _ in range(n):
        out.append(pt)
        pt = secp_add(pt, step)
    return out


def _coords(pt, z, i):
    """P in Jacobian limbs at bound 2: the loosest limbs for two items in three, canonical limbs for the third"""
    if i % 3 == 2 and pt is not None:
        return limbs(pt[0] * z * z % P) + limbs(pt[1] * z ** 3 % P) + limbs(z)
    return secp_jac(pt, z)


def _affine_q(q, i):
    """Q = (x, y) at bounds 2 / 3, loosest or canonical; None = the literal (0, 0)"""
    if q is None:
        return [0] * 9, [0] * 9
    if i % 3 == 2:
        return limbs(q[0]), limbs(q[1])
    return loose(q[0], 2, P), loose(q[1], 3, P)


@pytest.mark.parametrize("op", [0, 1], ids=["jac_dbl_neg", "jac_madd_neg"])
def test_negated_formulas_on_device(op):
    """jac_dbl_neg = -(2P) and jac_madd_neg = -(P + Q) against affine big-integer arithmetic at random Z, with the exceptional
    cases P = Q, P = -Q, P = O, Q = (0, 0) and doubling O in waves whose other lanes take the generic path; output limbs below
    2U, O back with a literal zero Z, raw limbs equal to the host twin's."""
    eng = get_engine()
    rng = makeRng(0xD8E6 + op)
    n = 64 * 15 + 40
    pts, qs = _walk(rng, n), _walk(rng, n)
    exc = _exceptional_lanes(n)
    cases = ["inf"] if op == 0 else ["P=Q", "P=-Q", "P=O", "Q=O"]
    kinds = {lane: cases[j % len(cases)] for j, lane in enumerate(exc)}
    A, Bw, exp = [], [], []
    for i in range(n):
        p1, q, kind = pts[i], qs[i], kinds.get(i)
        if kind == "inf" or kind == "P=O":
            p1 = None
        elif kind == "P=Q":
            q = p1
        elif kind == "P=-Q":
            q = secp_neg(p1)
        elif kind == "Q=O":
            q = None
        z = rng.rndBelow(P - 1) + 1
        qx, qy = _affine_q(q, i)
        A.append(_coords(p1, z, i))
        Bw.append(qx + qy)
        exp.append(secp_neg(secp_add(p1, p1) if op == 0 else secp_add(p1, q)))
    out = eng.field_check(FIELD_LADDER, op, 0, np.array(A, dtype=np.uint32), np.array(Bw, dtype=np.uint32))
    assert sum(e is None for e in exp) >= len(exc) // len(cases)   # the exceptional results are there
    for i in range(n):
        r = [int(x) for x in out[i]]
        assert max(r) < 2 * U, (i, kinds.get(i))
        assert secp_from_jac(r) == exp[i], (i, kinds.get(i))
        assert r == hosttest.jac_neg(op, A[i], Bw[i][:9], Bw[i][9:]), (i, kinds.get(i))


# ---- the odd GLV split on the device
def _glv_const(name):
    """SecpGlv::<name> (consts_gen.hpp) as an integer"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "noble-curves_amd", "csrc",
                            "consts_gen.hpp")).read()
    body = src[src.index("struct SecpGlv {"):]
    words = re.search(r"\b%s\[\d+\] = \{([^}]*)\}" % name, body).group(1)
    return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words.split(",")))


def _babai_boundary_scalars(rng, per_constant=64):
    """k < n with k g / 2^384 within 2^-20 of a half-integer, for g = g1 and g = g2 of secp_glv_split (round(k g / 2^384) is
    where the split's rounding flips): both neighbours of (t + 1/2) 2^384 / g for t = 0 and random t"""
    ks = []
    for g in (_glv_const("G1"), _glv_const("G2")):
        tmax = (N - 1) * g >> 384
        for j in range(per_constant):
            t = 0 if j == 0 else tmax if j == 1 else rng.rndBelow(tmax)
            k0 = ((2 * t + 1) << 383) // g
            for k in (k0, k0 + 1):
                if k < N:
                    assert abs((k * g) % (1 << 384) - (1 << 383)) < 1 << (384 - 20)
                    ks.append(k)
    return ks


def test_glv_odd_split_on_device():
    """secp_glv_split + secp_glv_make_odd on 2^16 random scalars, the CPU test's edge scalars and scalars at the Babai rounding
    boundaries: both halves odd, k = k1 + lambda k2 (mod n), |ki| < 2^130, the words equal to the host twin's, and all four
    parity classes of the plain split among the inputs."""
    eng = get_engine()
    rng = makeRng(0x0DD6)
    ks = [0, 1, 2, 3, N - 1, N - 2, N // 2, LAM, N - LAM, 1 << 128, (1 << 256) - 1]
    ks += _babai_boundary_scalars(rng)
    ks += [rng.rndBelow(N) for _ in range(1 << 16)]
    A = np.zeros((len(ks), 27), dtype=np.uint32)
    A[:, :8] = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint32).reshape(-1, 8)
    out = eng.field_check(FIELD_LADDER, 2, 0, A, np.zeros((len(ks), 18), dtype=np.uint32))
    seen = set()
    for i, k in enumerate(ks):
        w = [int(x) for x in out[i, :12]]
        assert w == hosttest.glv_split_odd_words(k), hex(k)
        k1, k2 = hosttest.split_words_to_ints(w)
        assert k1 % 2 == 1 and k2 % 2 == 1, hex(k)
        assert (k1 + LAM * k2 - k) % N == 0, hex(k)
        assert abs(k1) < (1 << 130) and abs(k2) < (1 << 130), hex(k)
        _, p1, _, p2 = hosttest.glv_split(k)
        seen.add((p1 % 2, p2 % 2))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- the ladder through the public batch multiplies
EDGE = [0, 1, 2, 3, N - 1, N - 2, N - 3, 1 << 128, (1 << 128) - 1, (1 << 128) + 1, (1 << 255), LAM, LAM + 1, LAM - 1, N - LAM,
        (N + 1) // 2, N // 2, (1 << 64), 0xFFFFFFFF, 1 << 32, 15, 16, 17, 255, 256]   # test_gpu_mulvar.py's edge list


def test_fused_ladder_exceptional_scalars_on_device():
    """mul_var_batch (the fused ladder k_mul_var_gtab<CurveSecpI, 4, 3, 16>) and mul_base_batch on the scalars whose ladder
    meets an exceptional addition by the model (helpers.ladder_events: k = 0 ends in R = -Q, k = -26 lambda in R = Q) with
    G, small multiples of G and random points, and the edge list, all at lanes 0, 31, 32, 63 and in a final partial wave
    among random items; results and infinity flags against the oracle."""
    eng = get_engine()
    rng = makeRng(0x1ADD6)
    model = ladder_exceptional_scalars(hosttest.glv_split_odd)
    kinds = {kd for ev in model.values() for _, _, kd in ev}
    assert (-26 * LAM) % N in model and 0 in model and kinds == {"dbl", "neg"}
    assert all(w == LADDER_M - 1 for ev in model.values() for w, _, _ in ev)
    G = Secp256k1.BASE
    special = [(k, p) for k in sorted(model) for p in [G, G.multiplyUnsafe(2), G.multiplyUnsafe(3), G.multiplyUnsafe(7)] +
               [G.multiplyUnsafe(rng.rndBelow(N - 1) + 1) for _ in range(3)]]
    special += [(k, G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)) for k in EDGE]
    special += [(12345, Secp256k1.ZERO), ((-26 * LAM) % N, Secp256k1.ZERO)]
    n = 64 * 10 + 21
    lanes = _exceptional_lanes(n)
    assert len(lanes) >= len(special)
    walk = _walk(rng, n)
    ks = [rng.rndBelow(N) for _ in range(n)]
    pts = [Secp256k1.fromAffine(xy) for xy in walk]
    for lane, (k, p) in zip(lanes, special):
        ks[lane], pts[lane] = k, p
    assert any(ladder_events(k, hosttest.glv_split_odd) == [(LADDER_M - 1, 1, "dbl")] for k in ks)
    zero = ORACLE_CURVE[SECP256K1].ZERO.toAffine()
    out, inf = eng.mul_var_batch(SECP256K1, points_to_wire(SECP256K1, pts), scalars_to_wire(ks))
    for i, (p, k) in enumerate(zip(pts, ks)):
        exp = p.multiplyUnsafe(k).toAffine()
        assert wire_to_affine(SECP256K1, out[i]) == exp, (i, hex(k))
        assert bool(inf[i]) == (exp == zero), (i, hex(k))
    outb, infb = eng.mul_base_batch(SECP256K1, scalars_to_wire(ks))
    for i, k in enumerate(ks):
        exp = G.multiplyUnsafe(k).toAffine()
        assert wire_to_affine(SECP256K1, outb[i]) == exp, (i, hex(k))
        assert bool(infb[i]) == (exp == zero), (i, hex(k))
