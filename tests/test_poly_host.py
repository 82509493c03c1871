"""poly() without a GPU: the fixture of the reference's own answers (tests/golden/poly_kat.json) against the plain-Python
restatement (poly_helpers) and against the host twin of csrc/poly.hip (the per-element and per-run functions of the kernels
executed on the CPU), the argument handling of the mirror (noble_curves_amd.fft.poly), which raises before the engine is
touched, and the NULL-context answers of the C ABI."""
import ctypes

import numpy as np
import pytest

from noble_curves_amd import fft as G
from noble_curves_amd._native import load_library

import poly_helpers as P
from poly_helpers import FIELDS, ORDERS

NCG_ERR_INVALID_ARG = -1


@pytest.mark.parametrize("field", FIELDS)
def test_restatement_reproduces_every_fixture_entry(field):
    fd = P.kat()["fields"][field]
    r = fd["order"]
    assert r == ORDERS[field] and P.kat()["generator"] == 7
    assert len(fd["cases"]) > 250
    seen = set()
    for c in fd["cases"]:
        assert P.restate(r, c) == c["out"], {k: v for k, v in c.items() if k != "out"}
        seen.add(c["op"])
    assert seen >= {"add", "sub", "dot", "mul", "scale", "convolve", "shift", "eval", "monomial_basis", "monomial_eval", "lagrange_basis",
                    "lagrange_eval", "vanishing", "degree", "extend", "roots", "omega"}
    lengths = {len(c["a"]) for c in fd["cases"] if c["op"] == "mul"}
    assert lengths == {1, 2, 3, 4, 5, 8, 16}


def test_fixture_holds_the_trial_vectors():
    """the three answers quoted when the fixture was planned, on both fields"""
    for field in FIELDS:
        r = ORDERS[field]
        got = {(c["op"], tuple(c["a"])): c["out"] for c in P.cases(field, "mul", "convolve", "vanishing")}
        assert got[("mul", (1, 2, 3, r - 1))] == [13, 33, 6, r - 2]
        assert got[("convolve", (1, 2, 3))] == [4, 13, 22, 15]
        assert got[("vanishing", (1, 2, 3))] == [r - 6, 11, r - 6, 1]


@pytest.mark.parametrize("field", FIELDS)
def test_host_twin_pointwise_scale_shift(field):
    ops = {"add": P.POLY_ADD, "sub": P.POLY_SUB, "dot": P.POLY_DOT}
    n = 0
    for c in P.cases(field, "add", "sub", "dot"):
        assert P.ht_pointwise(field, ops[c["op"]], c["a"], c["b"]) == c["out"], c["op"]
        n += 1
    for c in P.cases(field, "scale", "shift"):
        for T in (0, 1, 3):     # the device's thread count, one thread stepping through every index, a stride that does not divide n
            assert P.ht_scale(field, c["a"], c["x"], c["op"] == "shift", T) == c["out"], (c["op"], T)
        n += 1
    for c in P.cases(field, "monomial_basis"):
        assert P.ht_scale(field, [1] * c["n"], c["x"], True, 2) == c["out"]
    assert n > 60


@pytest.mark.parametrize("field", FIELDS)
def test_host_twin_sums_and_horner(field):
    r = ORDERS[field]
    for c in P.cases(field, "eval"):
        for T in (0, 1, 3):
            assert P.ht_eval(field, c["a"], c["b"], T) == c["out"]
    by_a = {}
    for c in P.cases(field, "monomial_eval"):
        by_a.setdefault(tuple(c["a"]), []).append(c)
        for T in (0, 1, 3, 5):
            assert P.ht_eval_monomial(field, c["a"], [c["x"]], T) == [c["out"]], (len(c["a"]), T)
    for a, cs in by_a.items():                 # the four points of a vector in one pass, and padded to all eight
        xs = [c["x"] for c in cs]
        assert P.ht_eval_monomial(field, list(a), xs, 3) == [c["out"] for c in cs]
        assert P.ht_eval_monomial(field, list(a), (xs * 2)[:8], 2) == ([c["out"] for c in cs] * 2)[:8]
    # operands at their maxima: every product is (r - 1)^2, and a run longer than one step of every thread
    top = [r - 1] * 700
    assert P.ht_eval(field, top, top, 64) == 700 % r
    assert P.ht_eval_monomial(field, top, [1, r - 1, 0], 64) == [(-700) % r, 0, r - 1]
    a = P.rand_vec(r, 517, "horner")
    xs = [P.rand_vec(r, 9, "x")[4], r - 1, 2]
    assert P.ht_eval_monomial(field, a, xs, 0) == [P.horner(r, a, x) for x in xs]
    assert P.ht_eval_monomial(field, a, xs, 40) == [P.horner(r, a, x) for x in xs]
    assert P.ht_eval(field, [], [], 0) == 0 and P.ht_eval_monomial(field, [], [5], 0) == [0]


@pytest.mark.parametrize("field", FIELDS)
def test_host_twin_start_power(field):
    r = ORDERS[field]
    s = P.rand_vec(r, 9, "pow")[4]
    for base in (s, 0, 1, r - 1):
        for start in (0, 1, 2, 255, 256, 257, 2 ** 20 + 3):
            assert P.ht_pow(field, base, start) == pow(base, start, r), (base, start)


@pytest.mark.parametrize("field", FIELDS)
def test_host_twin_lagrange_basis(field):
    r = ORDERS[field]
    for c in P.cases(field, "lagrange_basis"):
        bits = c["n"].bit_length() - 1
        for T in (0, 1) + ((2,) if c["n"] <= 2 * P.ht().ht_poly_lag_run() else ()):
            got, root = P.ht_lagrange(field, bits, c["x"], c["brp"], T)
            assert got == c["out"], (c["n"], c["brp"], T)
            table = P.roots(r, bits, c["brp"])
            assert root == (table.index(c["x"]) if c["x"] in table else 0xFFFFFFFF)
    # one thread's run of 16 denominators with the zero first, last and in the middle (natural order: the run is the table)
    assert P.ht().ht_poly_lag_run() == 16
    w = P.roots(r, 4)
    for k in (0, 15, 7, 8):
        got, root = P.ht_lagrange(field, 4, w[k], False, 1)
        assert root == k and got == [1 if i == k else 0 for i in range(16)]
    # several runs per launch, bit-reversed and natural, against the restatement; the basis sums to 1
    x = P.rand_vec(r, 9, "lag")[4]
    for bits, T in ((6, 4), (7, 8), (5, 0)):
        for brp in (False, True):
            got, root = P.ht_lagrange(field, bits, x, brp, T)
            assert got == P.lagrange_basis(r, x, 1 << bits, brp) and root == 0xFFFFFFFF and sum(got) % r == 1


# ---------------------------------------------------------------- the mirror's argument handling
def _polys():
    out = []
    for fr in (G.bls12_381_Fr, G.bn254_Fr):
        roots = G.rootsOfUnity(fr, 7)
        out.append((fr, roots, G.poly(fr, roots)))
    return out


def test_mirror_messages_are_the_references():
    E = P.kat()["errors"]
    for fr, roots, p in _polys():
        with pytest.raises(ValueError) as e:
            p.add([1, 2], [1])
        assert str(e.value) == E["mismatched"]
        fixed = G.poly(fr, roots, None, None, 4)
        with pytest.raises(ValueError) as e:
            fixed.add([1], [1])
        assert str(e.value) == E["fixed_length"]
        with pytest.raises(ValueError) as e:
            fixed.shift([1, 2], 3)
        assert str(e.value) == E["fixed_length_shift"]
        with pytest.raises(ValueError) as e:
            p.lagrange.basis(2, 3)
        assert str(e.value) == E["lagrange_basis_length"]
        with pytest.raises(ValueError) as e:
            p.lagrange.eval([1, 2, 3], 2)
        assert str(e.value) == E["lagrange_eval_length"]
        with pytest.raises(TypeError) as e:
            p.add(5, [1])
        assert str(e.value) == E["not_poly_bigint"]
        with pytest.raises(TypeError) as e:
            p.add("x", [1])
        assert str(e.value) == E["not_poly_string"]
        with pytest.raises(TypeError) as e:
            p.add([1], 5)
        assert str(e.value) == E["not_poly_b"]
        with pytest.raises(TypeError) as e:
            p.shift(7, 3)
        assert str(e.value) == E["not_poly_shift"]
        with_fft = G.poly(fr, roots, None, G.FFT(roots, fr))
        with pytest.raises(ValueError) as e:
            with_fft.mul([1, 2, 3], [1, 2, 3])
        assert str(e.value) == E["fft_length"]
        for call in (lambda: p.add([fr.ORDER], [0]), lambda: p.dot([0, 1], [1, -1]), lambda: p.mul([1, 2], fr.ORDER),
                     lambda: p.shift([1, 2], fr.ORDER + 1), lambda: p.monomial.eval([1, True], 2), lambda: p.eval([1], [fr.ORDER]),
                     lambda: p.lagrange.basis(fr.ORDER, 4), lambda: p.convolve([1, 2], [fr.ORDER])):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == E["out_of_range"]


def test_mirror_host_side_operations():
    """create / degree / extend / clone / vanishing never leave the host"""
    for field, (fr, roots, p) in zip(FIELDS, _polys()):
        assert p.roots is roots and p.length is None and p.create(3) == [0, 0, 0] and p.create(2, 7) == [7, 7]
        for c in P.cases(field, "degree"):
            assert p.degree(c["a"]) == c["out"]
        for c in P.cases(field, "extend"):
            assert p.extend(c["a"], c["n"]) == c["out"]
        for c in P.cases(field, "vanishing"):
            assert p.vanishing(c["a"]) == c["out"]
        a = P.cases(field, "degree")[-1]["a"]
        b = p.clone(a)
        assert b == a and b is not a
        raw = P.to_wire(a)
        assert p.degree(raw) == P.degree(a) and np.array_equal(p.clone(raw), raw)
        assert p.add([], []) == [] and p.mul([], []) == [] and p.shift([], 3) == []


def test_library_loads_and_refuses_a_null_context():
    lib = load_library()
    buf = (ctypes.c_uint8 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "ncg_poly_pointwise": (None, 0, 0, 1, b, b, b),
        "ncg_poly_pointwise_dev": (None, 0, 0, 1, b, b, b, None),
        "ncg_poly_scale": (None, 0, 1, b, b, 0, b),
        "ncg_poly_scale_dev": (None, 0, 1, b, b, 0, b, None),
        "ncg_poly_eval": (None, 0, 1, b, b, b),
        "ncg_poly_eval_dev": (None, 0, 1, b, b, b, None),
        "ncg_poly_eval_monomial": (None, 0, 1, b, 1, b, b),
        "ncg_poly_eval_monomial_dev": (None, 0, 1, b, 1, b, b, None),
        "ncg_poly_lagrange_basis": (None, 0, 0, b, b, 0, b),
        "ncg_poly_lagrange_basis_dev": (None, 0, 0, b, b, 0, b, None),
        "ncg_poly_mul": (None, 0, 0, b, 1, b, 1, b, b),
        "ncg_poly_mul_dev": (None, 0, 0, b, 1, b, 1, b, b, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == NCG_ERR_INVALID_ARG, name
        assert b"ctx is NULL" in lib.ncg_last_error(None)
