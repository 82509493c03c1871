"""GPU checks of CurveSecpI's 32-window ladder (k_mul_var_gtab<CurveSecpI, 4, 3, true>): the split with k1 odd on the device
(ncg_field_check field 7, op 3) word for word against its host twin, and mul_var_batch against the oracle on the edge list, the
scalars whose ladder meets an exceptional addition (tests/ladder32.py, the k2 fix-up starting from R = O among them), small
multiples of G and scalars of both k2 parities, at lanes 0 / 31 / 32 / 63 of full waves and in a final partial wave."""
import numpy as np
import pytest

import ladder32
from helpers import (ORACLE_CURVE, SECP_LAMBDA as LAM, points_to_wire, scalars_to_wire, secp_add, secp_rand_point,
                     wire_to_affine)
from noble_curves_amd import get_engine
from noble_curves_amd._native import SECP256K1
from oracle.curves import SECP256K1_N, Secp256k1, makeRng

pytestmark = pytest.mark.gpu

N = SECP256K1_N
FIELD_LADDER = 7        # ncg_field_check: secp256k1 ladder pieces; op 3 = secp_glv_split + secp_glv_make_k1_odd
EDGE = [0, 1, 2, 3, N - 1, N - 2, N - 3, 1 << 128, (1 << 128) - 1, (1 << 128) + 1, (1 << 255), LAM, LAM + 1, LAM - 1, N - LAM,
        (N + 1) // 2, N // 2, (1 << 64), 0xFFFFFFFF, 1 << 32, 15, 16, 17, 255, 256]


def test_split_k1_odd_on_device():
    """2^16 random scalars, the edge list and the Babai boundary scalars: the device's words equal the host twin's, and the
    split's contract (k1 odd, |k1| < 2^128, |k2| + 1 < 2^128, k1 + lambda k2 = k mod n) holds."""
    eng = get_engine()
    rng = makeRng(0x32D6)
    ks = EDGE + [(1 << 256) - 1] + ladder32.babai_boundary_scalars(rng) + [rng.rndBelow(N) for _ in range(1 << 16)]
    A = np.zeros((len(ks), 27), dtype=np.uint32)
    A[:, :8] = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint32).reshape(-1, 8)
    out = eng.field_check(FIELD_LADDER, 3, 0, A, np.zeros((len(ks), 18), dtype=np.uint32))
    parities = set()
    for i, k in enumerate(ks):
        w = [int(x) for x in out[i, :12]]
        assert w == ladder32.split_k1_odd_words(k), hex(k)
        k1, k2 = ladder32.split_k1_odd(k)
        ladder32.check_split(k, k1, k2)
        parities.add(k2 % 2)
    assert parities == {0, 1}


def _exceptional_lanes(n):
    """lanes 0, 31, 32, 63 of every full wave and three lanes of the final partial wave (n % 64 != 0)"""
    assert n % 64
    full = n - n % 64
    return sorted({w + o for w in range(0, full, 64) for o in (0, 31, 32, 63)} | {full, full + (n % 64) // 2, n - 1})


def test_ladder32_batch_on_device():
    """mul_var_batch on the model's exceptional scalars (0: R = -Q in the last window; +-lambda: the same, then the k2 fix-up
    from R = O), +-2 lambda, the edge list and k = 1..24, with G, small multiples of G and random points, placed at the lanes of
    _exceptional_lanes among random items; results and infinity flags against the oracle."""
    eng = get_engine()
    rng = makeRng(0x32B6)
    model = ladder32.ladder_exceptional_scalars()
    assert sorted(model) == sorted([0, LAM, N - LAM])
    assert any(ev[-1] == (ladder32.FIXUP, 1, "inf") for ev in model.values())
    G = Secp256k1.BASE
    small = [G, G.multiplyUnsafe(2), G.multiplyUnsafe(3), G.multiplyUnsafe(7)]
    special = [(k, p) for k in sorted(model) + [2 * LAM % N, -2 * LAM % N]
               for p in small + [G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)]]
    special += [(k, G.multiplyUnsafe(rng.rndBelow(N - 1) + 1)) for k in EDGE]
    special += [(k, G.multiplyUnsafe(k + 4)) for k in range(1, 25)]
    special += [(12345, Secp256k1.ZERO), (LAM, Secp256k1.ZERO)]
    n = 64 * 20 + 37
    lanes = _exceptional_lanes(n)
    assert len(lanes) >= len(special)
    pt, step = secp_rand_point(rng), secp_rand_point(rng)
    walk = []
    for _ in range(n):
        walk.append(pt)
        pt = secp_add(pt, step)
    ks = [rng.rndBelow(N) for _ in range(n)]
    pts = [Secp256k1.fromAffine(xy) for xy in walk]
    for lane, (k, p) in zip(lanes, special):
        ks[lane], pts[lane] = k, p
    assert {ladder32.split_k1_odd(k)[1] % 2 for k in ks} == {0, 1}
    zero = ORACLE_CURVE[SECP256K1].ZERO.toAffine()
    out, inf = eng.mul_var_batch(SECP256K1, points_to_wire(SECP256K1, pts), scalars_to_wire(ks))
    for i, (p, k) in enumerate(zip(pts, ks)):
        exp = p.multiplyUnsafe(k).toAffine()
        assert wire_to_affine(SECP256K1, out[i]) == exp, (i, hex(k))
        assert bool(inf[i]) == (exp == zero), (i, hex(k))
