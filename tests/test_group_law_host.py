"""The group law the MSM runs on its buckets, on the CPU through the host twin (hosttest.hip ht_group_op = group_check.hpp, the
code of ncg_field_check fields 10-14) on the rows of group_law_cases.py: MsmGroup<C>::madd / add / dbl for every group on stored
words at the edges of the storage bounds, against the oracle's point classes; f_eqz of the bls12-381 forms at the bounds the
group law instantiates (ht_fe29_eqz).  The four-lane form of msm_coop.hpp exists on the device only: its rows go through the
single-lane twin of the same group here (op 8 as op 2, op 11 as op 3), which proves the case builder and its expected values
before a GPU sees them.  Field 13 runs the UNPAIRED Fp2 form on the host (the lane-paired products are device code)."""
import ctypes

import numpy as np
import pytest

import group_law_cases as G
import hosttest


def _lib():
    lib = hosttest.lib()
    lib.ht_group_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ht_fe29_eqz.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def _group_op(lib, fid, op, a, b):
    x, y = np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)
    out = np.full(len(a), 0xA5A5A5A5, dtype=np.uint32)
    assert lib.ht_group_op(fid, op, x.ctypes.data, y.ctypes.data, out.ctypes.data) == 0
    return [int(w) for w in out]


@pytest.mark.parametrize("fid", G.FIELDS)
@pytest.mark.parametrize("op", G.SINGLE_OPS)
def test_group_op_host(fid, op):
    lib = _lib()
    c = G.cases(fid, op)
    assert len(c.a) == G.ROWS
    for i, (a, b) in enumerate(zip(c.a, c.b)):
        c.check(a, b, _group_op(lib, fid, op, a, b), what="field %d op %d row %d (%s)" % (fid, op, i, c.kinds[i]))


@pytest.mark.parametrize("fid", G.COOP_FIELDS)
@pytest.mark.parametrize("op", [8, 11])
def test_coop_rows_through_the_single_lane_twin(fid, op):
    lib = _lib()
    c = G.coop_cases(fid, op)
    assert c.op == G.COOP_AS_SINGLE[op]
    for i, (a, b) in enumerate(zip(c.a, c.b)):
        c.check(a, b, _group_op(lib, fid, c.op, a, b), what="field %d op %d row %d (%s)" % (fid, op, i, c.kinds[i]))


def test_unknown_group_op_is_refused():
    lib = _lib()
    z = np.zeros(112, dtype=np.uint32)
    for fid, op in ((9, 0), (15, 0), (12, 4), (12, 8), (12, -1)):
        assert lib.ht_group_op(fid, op, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -1


def test_case_counters():
    """every kind in every 16-row window; every multiple of p the operands can put under the zero tests of the bls12-381 forms"""
    got = G.check_counters()
    assert got["P66"] >= set(range(1, 65))


def test_storage_bounds_come_from_the_sources():
    b = G.storage_bounds()
    assert {k: b[k] for k in ("CurveSecp", "CurveEd", "CurveG1", "CurveG2P", "CurveBn254")} == {
        "CurveSecp": ("Fe9", 2), "CurveEd": ("Fe9", 1), "CurveG1": ("Fe29", 64), "CurveG2P": ("Fe29x2P", 64), "CurveBn254": ("Fe9", 2)}


@pytest.mark.parametrize("A", G.EQZ_BOUNDS)
def test_fe29_eqz_host(A):
    lib = _lib()
    rows = G.eqz_rows(A)
    assert sum(G.eqz_expected(A, r) for r in rows) >= A           # every j p, j < A, says yes
    for i, r in enumerate(rows):
        x = np.array(r, dtype=np.uint32)
        assert lib.ht_fe29_eqz(0, A, x.ctypes.data) == G.eqz_expected(A, r), (A, i, r)


@pytest.mark.parametrize("A", G.EQZ_BOUNDS)
def test_fe29_eqz_pair_host(A):
    """the two halves through the unpaired Fe29x2<A> (pair_swap is device code)"""
    lib = _lib()
    rows = G.eqz_rows_paired(A)
    assert sum(G.eqz_expected_paired(A, r) for r in rows) >= A
    for i, r in enumerate(rows):
        x = np.array(r, dtype=np.uint32)
        assert lib.ht_fe29_eqz(1, A, x.ctypes.data) == G.eqz_expected_paired(A, r), (A, i, r)


def test_fe29_eqz_unknown_bound():
    x = np.zeros(28, dtype=np.uint32)
    assert _lib().ht_fe29_eqz(0, 5, x.ctypes.data) == -1 and _lib().ht_fe29_eqz(1, 5, x.ctypes.data) == -1
