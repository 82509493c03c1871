"""bn254 G1 without a GPU: the C ABI sizes, the Montgomery field form on the host twin (fe9m.hpp at every bound its types
admit, no 64-bit column overflow), the batch-multiply ladder, the MSM host finish and the shard combine against the oracle."""
import ctypes
import os

import numpy as np
import pytest

import hosttest
from bn254_helpers import (BN254_G1, BN254_P, BN254_R, Bn254, OPS, VARIANTS, fe9m_cases, from_wire, ht_fe9m_op, rand_point,
                           scalars_wire, to_wire)
from oracle.curves import makeRng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _abi():
    so = os.path.join(ROOT, "noble-curves_amd", "libncg.so")
    if not os.path.exists(so):
        pytest.skip("libncg.so not built")
    return ctypes.CDLL(so)


def test_point_and_field_bytes():
    lib = _abi()
    assert lib.ncg_point_bytes(5) == 64 and lib.ncg_field_bytes(5) == 32
    assert lib.ncg_point_bytes(4) == 0


def test_python_mirror_sizes():
    from noble_curves_amd._native import BN254_G1 as ID, FIELD_BYTES, POINT_BYTES
    from noble_curves_amd.curve import bn254_G1_Point
    assert ID == 5 and POINT_BYTES[5] == 64 and FIELD_BYTES[5] == 32
    assert bn254_G1_Point.BASE.toAffine() == (1, 2)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("op", OPS)
def test_fe9m_host_twin_at_the_bounds(op, variant):
    """Every op of the bn254 form at operands up to the bound of its type (values just below 2 B p with the low limbs as loose
    as the value allows, 0, p - 1, p, random) against Python integers; the twin counts column overflows (must be none)."""
    rows_a, rows_b, check = fe9m_cases()[(op, variant)]
    for a, b in zip(rows_a, rows_b):
        out, ovf = ht_fe9m_op(op, variant, a, b)
        assert ovf == 0, (op, variant, a, b)
        check(a, b, out)


def test_fe9m_worst_column_budget():
    """limbs 0..7 at B 2^29 - 1 whatever the value, limb 8 at the most a value below 2 B p leaves it (fe9m.hpp's column
    budget): no column overflows"""
    def top(B):
        return [(B << 29) - 1] * 8 + [(2 * B * BN254_P) >> 232]
    for variant, a, b in ((17, top(1), top(7)), (71, top(7), top(1)), (11, top(1), top(1))):
        _, ovf = ht_fe9m_op(0, variant, a, b)
        assert ovf == 0, variant
    _, ovf = ht_fe9m_op(1, 22, top(2), [0] * 9)
    assert ovf == 0


def test_host_ladder_against_oracle():
    rng = makeRng(0x254A)
    ks = [0, 1, 2, 3, 15, 16, 17, BN254_R - 1, BN254_R - 2, BN254_R // 2] + [rng.rndBelow(BN254_R) for _ in range(20)]
    pts = [rand_point(rng) for _ in ks]
    pts[3] = Bn254.ZERO
    out, inf = hosttest.mul_var(BN254_G1, to_wire(pts), scalars_wire(ks))
    for i, (p, k) in enumerate(zip(pts, ks)):
        exp = p.multiplyUnsafe(k)
        assert from_wire(out[i]) == exp.toAffine(), i
        assert bool(inf[i]) == exp.is0()


def test_host_shard_combine_against_oracle():
    """hosttest's sharded MSM twin (the real slot format, partial sums and host finish) for curve 5"""
    rng = makeRng(0x254B)
    n = 40
    pts = [rand_point(rng) for _ in range(n)]
    pts[5] = Bn254.ZERO
    ks = [rng.rndBelow(BN254_R) for _ in range(n)]
    ks[7], ks[8] = 0, BN254_R - 1
    exp = Bn254.ZERO
    for p, k in zip(pts, ks):
        exp = exp.add(p.multiplyUnsafe(k))
    pw, sw = to_wire(pts), scalars_wire(ks)
    nparts = 3
    bounds = [0, 13, 27, n]
    slots = []
    for r in range(nparts):
        lo, hi = bounds[r], bounds[r + 1]
        p_r = np.ascontiguousarray(pw[lo:hi])
        s_r = np.ascontiguousarray(sw[lo:hi])
        slots.append(hosttest.msm_shard_local(BN254_G1, hi - lo, n, p_r.ctypes.data, s_r.ctypes.data))
    out, inf = hosttest.msm_shard_combine(BN254_G1, n, np.array(slots), 64)
    assert from_wire(out) == exp.toAffine() and bool(inf) == exp.is0()


def test_golden_vectors_against_oracle():
    """tests/golden/bn254_g1_eip196.json (EIP-196 ECADD / ECMUL vectors of the reference) against the bn254 oracle"""
    from helpers import load_golden
    g = load_golden("bn254_g1_eip196.json")
    assert len(g["add"]) >= 40 and len(g["mul"]) >= 100
    P = lambda xy: Bn254.ZERO if xy == [0, 0] else Bn254.fromAffine(tuple(xy))
    for v in g["add"]:
        a, b = [[int(t, 16) for t in v[k]] for k in ("a", "b")]
        assert P(a).add(P(b)).toAffine() == tuple(int(t, 16) for t in v["out"])
    for v in g["mul"]:
        a = [int(t, 16) for t in v["p"]]
        assert P(a).multiplyUnsafe(int(v["k"], 16) % BN254_R).toAffine() == tuple(int(t, 16) for t in v["out"])
