"""The field table of ncg_field_check (csrc/selfcheck.hpp) as the host twin shows it (ht_field_check_shape) against the Python
mirror _native.FIELD_CHECK_WORDS: the same fields are registered, with the same words per row of a, b and out."""
import ctypes

import numpy as np

import hosttest
from noble_curves_amd._native import FIELD_CHECK_WORDS


def _shape(field):
    fn = hosttest.lib().ht_field_check_shape
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p]
    out = np.full(3, -7, dtype=np.int32)
    rc = fn(field, out.ctypes.data)
    return rc, tuple(int(x) for x in out)


def test_field_table_agrees_with_python_mirror():
    for field in range(-1, 19):
        rc, words = _shape(field)
        if field in FIELD_CHECK_WORDS:
            assert rc == 0 and words == FIELD_CHECK_WORDS[field], field
        else:
            assert rc == -1 and words == (-7, -7, -7), field     # refused, out untouched


def test_unassigned_fields_are_refused_on_both_sides():
    assert sorted(FIELD_CHECK_WORDS) == [f for f in range(18) if f != 15]
    for field in (-1, 15, 18):
        assert field not in FIELD_CHECK_WORDS and _shape(field)[0] == -1
