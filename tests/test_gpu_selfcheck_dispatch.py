"""The dispatch and launch geometry of ncg_field_check (csrc/selfcheck.hip), below the family tests: every registered field takes
a full wave and a partial one, an op no family defines leaves out zero, the four-lane copy of fields 12 / 13 returns its rows at
a partial group block, and an unassigned field is refused before anything is written."""
import numpy as np
import pytest

from noble_curves_amd import get_engine
from noble_curves_amd._native import FIELD_CHECK_WORDS

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED = 0, -4
# a variant the family instantiates, so that the op reaches the family's own switch (fields that ignore it: 0)
VARIANTS = {0: [11], 1: [11], 5: [1111], 6: [1111], 8: [0, 1], 9: [11]}


def _rows(seed, n, words):
    return np.random.default_rng(seed).integers(0, 1 << 28, (n, words), dtype=np.uint32)


@pytest.mark.parametrize("field", sorted(FIELD_CHECK_WORDS))
def test_undefined_op_leaves_out_zero(field):
    wa, wb, wo = FIELD_CHECK_WORDS[field]
    a, b = _rows(0x5E1F + field, 70, wa), _rows(0xC4EC + field, 70, wb)
    for variant in VARIANTS.get(field, [0]):
        out = get_engine().field_check(field, 63, variant, a, b)
        assert out.shape == (70, wo) and not out.any(), (field, variant)


@pytest.mark.parametrize("field", [12, 13])
def test_four_lane_copy_at_a_partial_block(field):
    wa, wb, wo = FIELD_CHECK_WORDS[field]
    a, b = _rows(0xC0B1 + field, 17, wa), _rows(0xC0B2 + field, 17, wb)
    assert np.array_equal(get_engine().field_check(field, 13, 0, a, b), a)


@pytest.mark.parametrize("field", [15, 18, -1])
def test_unassigned_field_is_refused(field):
    eng = get_engine()
    a, b = _rows(1, 70, 112), _rows(2, 70, 112)
    out = np.full((70, 112), 0xA5A5A5A5, np.uint32)
    assert eng.lib.ncg_field_check(eng.h, field, 63, 0, 70, a.ctypes.data, b.ctypes.data, out.ctypes.data) == UNSUPPORTED
    assert (out == 0xA5A5A5A5).all()
