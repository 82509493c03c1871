"""The group law of the MSM buckets ON THE DEVICE, below the MSM: ncg_field_check fields 10-14 run MsmGroup<C>::madd / add / dbl
(ec_sw.hpp xyzz_*, ec_te.hpp ed_*) and the four-lane CoopXyzz<C>::add / dbl / copy of msm_coop.hpp - which has no host twin - on
stored words; op 7 of fields 3 / 4 runs f_eqz of Fe29 / the lane-paired Fp2 at the bounds under the group law's branches.  Rows,
expected values (the oracle's point classes) and assertions: group_law_cases.py, proved on the CPU by test_group_law_host.py.
Every launch holds 167 rows with the row kinds interleaved, so one wave runs the four steps in one group, returns early in its
neighbour and goes to the complete routine in a third; the last block of every launch is partial."""
import numpy as np
import pytest

import group_law_cases as G
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu

GROUP_OPS = [(f, op) for f in G.FIELDS for op in G.SINGLE_OPS] + [(f, op) for f in G.COOP_FIELDS for op in (8, 9, 10, 11, 12)]


def _run(fid, op, c):
    a, b = np.array(c.a, dtype=np.uint32), np.array(c.b, dtype=np.uint32)
    out = get_engine().field_check(fid, op, 0, a, b)
    assert out.shape == a.shape
    return out


@pytest.mark.parametrize("fid,op", GROUP_OPS)
def test_group_op_on_device(fid, op):
    c = G.cases(fid, op) if op in G.SINGLE_OPS else G.coop_cases(fid, op)
    out = _run(fid, op, c)
    for i, (a, b) in enumerate(zip(c.a, c.b)):
        c.check(a, b, out[i], what="field %d op %d row %d (%s)" % (fid, op, i, c.kinds[i]))


@pytest.mark.parametrize("fid", G.COOP_FIELDS)
def test_coop_aliasing_and_copy(fid):
    """out aliasing a (op 9) or b (op 10) gives the group element of op 8 row by row; the in-place doubling (12) that of op 11; the
    copy (13) returns its input words; the fields without a four-lane form leave out zero"""
    c = G.coop_cases(fid, 8)
    o8, o9, o10 = (_run(fid, op, c) for op in (8, 9, 10))
    for i in range(G.ROWS):
        e = c.element(o8[i])
        assert c.element(o9[i]) == e and c.element(o10[i]) == e, (fid, i, c.kinds[i])
    d = G.coop_cases(fid, 11)
    o11, o12 = _run(fid, 11, d), _run(fid, 12, d)
    for i in range(G.ROWS):
        assert d.element(o12[i]) == d.element(o11[i]), (fid, i, d.kinds[i])
    assert _run(fid, 13, c).tolist() == c.a
    other = G.cases(10, 2)
    for op in G.COOP_OPS:
        assert not _run(10, op, other).any(), op


@pytest.mark.parametrize("paired,A", [(p, A) for p in (0, 1) for A in G.EQZ_BOUNDS])
def test_fe29_eqz_on_device(paired, A):
    rows = G.eqz_rows_paired(A) if paired else G.eqz_rows(A)
    width = 56 if paired else 28                                  # the row widths of fields 4 / 3; c and b are ignored
    a = np.zeros((len(rows), width), dtype=np.uint32)
    a[:, :len(rows[0])] = np.array(rows, dtype=np.uint32)
    a[:, len(rows[0]):] = 0x1FFFFFFF                              # the ignored element c: anything
    out = get_engine().field_check(4 if paired else 3, 7, A, a, np.zeros_like(a))
    exp = [G.eqz_expected_paired(A, r) if paired else G.eqz_expected(A, r) for r in rows]
    assert sum(exp) >= A
    got = [int(x) for x in out[:, 0]]
    bad = [i for i in range(len(rows)) if got[i] != exp[i]]
    assert not bad, (paired, A, bad[:8], [rows[i] for i in bad[:2]])
    assert not out[:, 1:].any()
    if A == 4:                                                    # a bound the group law does not instantiate leaves out zero
        assert not get_engine().field_check(4 if paired else 3, 7, 5, a[:70], np.zeros_like(a[:70])).any()
