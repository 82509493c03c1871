"""GPU tests of the polynomial layer (csrc/poly.hip) over both scalar fields: the C ABI (`ncg_poly_*`, host and _dev forms), the
Engine methods and the mirror noble_curves_amd.fft.poly, against the reference's own answers (tests/golden/poly_kat.json) and,
beyond the fixture's sizes, the plain-Python restatement of poly_helpers and the reference's test properties
(test/fft.test.ts:430-660)."""
import ctypes
import random

import numpy as np
import pytest
import torch

from noble_curves_amd import fft as G
from noble_curves_amd import get_engine
from noble_curves_amd._native import Engine, NativeError

import poly_helpers as P
from poly_helpers import FIELD_IDS, FIELDS, ORDERS, from_wire, to_wire

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -4
FR = {"bls12_381": G.bls12_381_Fr, "bn254": G.bn254_Fr}
ENTRY_POINTS = ("pointwise", "scale", "eval", "eval_monomial", "lagrange_basis", "mul")


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t.ctypes.data)


def _cuda(arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def _small(*values):
    return to_wire(list(values))


def _mirror(field, **kw):
    fr = FR[field]
    return G.poly(fr, G.rootsOfUnity(fr, 7), **kw)


class _Side:
    """the _dev forms on a side stream"""

    def __init__(self):
        self.eng = get_engine()
        self.stream = torch.cuda.Stream()

    @property
    def s(self):
        """the stream's handle, once the tensors made on torch's own stream are complete"""
        torch.cuda.synchronize()
        return self.stream.cuda_stream

    def done(self, t):
        self.stream.synchronize()
        return t.cpu().numpy()


def _raw_calls(L, h, fid, om, a, b, x, out, dev, stream=None, n=4, log2n=2, m=1, op=0, na=4, nb=4, only=None):
    """the entry points (all, or the one named `only`) once with the given field id; returns the statuses by name.  a, b, out:
    buffers of the calling form"""
    tail = (stream,) if dev else ()
    sfx = "_dev" if dev else ""
    calls = {
        "pointwise": lambda: getattr(L, "ncg_poly_pointwise" + sfx)(h, fid, op, n, _vp(a), _vp(b), _vp(out), *tail),
        "scale": lambda: getattr(L, "ncg_poly_scale" + sfx)(h, fid, n, _vp(a), _vp(x), 1, _vp(out), *tail),
        "eval": lambda: getattr(L, "ncg_poly_eval" + sfx)(h, fid, n, _vp(a), _vp(b), _vp(out), *tail),
        "eval_monomial": lambda: getattr(L, "ncg_poly_eval_monomial" + sfx)(h, fid, n, _vp(a), m, _vp(x), _vp(out), *tail),
        "lagrange_basis": lambda: getattr(L, "ncg_poly_lagrange_basis" + sfx)(h, fid, log2n, _vp(om), _vp(x), 0, _vp(out), *tail),
        "mul": lambda: getattr(L, "ncg_poly_mul" + sfx)(h, fid, log2n, _vp(om), na, _vp(a), nb, _vp(b), _vp(out), *tail),
    }
    return {k: f() for k, f in calls.items() if only in (None, k)}


@pytest.mark.parametrize("field", FIELDS)
def test_abi_fixture_vectors_host_and_dev(field):
    """each entry point, host form and _dev form on a side stream, on the fixture's vectors of every length"""
    r, fid = ORDERS[field], FIELD_IDS[field]
    side = _Side()
    eng = side.eng
    ops = {"add": P.POLY_ADD, "sub": P.POLY_SUB, "dot": P.POLY_DOT}
    count = 0
    for c in P.cases(field, "add", "sub", "dot", "scale", "shift", "eval", "monomial_eval", "lagrange_basis", "mul", "convolve"):
        op, exp = c["op"], c["out"]
        a = to_wire(c["a"]) if "a" in c else None
        b = to_wire(c["b"]) if "b" in c else None
        da, db = (_cuda(a) if a is not None else None), (_cuda(b) if b is not None else None)
        if op in ops:
            host = eng.poly_pointwise(ops[op], a, b, field=fid)
            out = torch.full_like(da, 0xFF)
            eng.poly_pointwise_dev(ops[op], len(exp), da.data_ptr(), db.data_ptr(), out.data_ptr(), side.s, field=fid)
        elif op in ("scale", "shift"):
            host = eng.poly_scale(a, c["x"], powers=op == "shift", field=fid)
            out = torch.full_like(da, 0xFF)
            eng.poly_scale_dev(len(exp), da.data_ptr(), c["x"], op == "shift", out.data_ptr(), side.s, field=fid)
        elif op == "eval":
            host, exp = to_wire([eng.poly_eval(a, b, field=fid)]), [exp]
            out = torch.full((1, 32), 0xFF, dtype=torch.uint8, device="cuda")
            eng.poly_eval_dev(len(c["a"]), da.data_ptr(), db.data_ptr(), out.data_ptr(), side.s, field=fid)
        elif op == "monomial_eval":
            host, exp = to_wire(eng.poly_eval_monomial(a, [c["x"]], field=fid)), [exp]
            out = torch.full((1, 32), 0xFF, dtype=torch.uint8, device="cuda")
            eng.poly_eval_monomial_dev(len(c["a"]), da.data_ptr(), [c["x"]], out.data_ptr(), side.s, field=fid)
        elif op == "lagrange_basis":
            bits = c["n"].bit_length() - 1
            host = eng.poly_lagrange_basis(bits, P.omega(r, bits), c["x"], brp=c["brp"], field=fid)
            out = torch.full((c["n"], 32), 0xFF, dtype=torch.uint8, device="cuda")
            eng.poly_lagrange_basis_dev(bits, P.omega(r, bits), c["x"], c["brp"], out.data_ptr(), side.s, field=fid)
        else:   # mul (power-of-two lengths here; the others go through the mirror) and convolve
            if op == "mul" and len(c["a"]) & (len(c["a"]) - 1):
                continue
            bits = len(exp).bit_length() - 1
            host = eng.poly_mul(bits, P.omega(r, bits), a, b, field=fid)
            out = torch.full((len(exp), 32), 0xFF, dtype=torch.uint8, device="cuda")
            eng.poly_mul_dev(bits, P.omega(r, bits), len(c["a"]), da.data_ptr(), len(c["b"]), db.data_ptr(), out.data_ptr(), side.s, field=fid)
        got = side.done(out)
        what = {k: v for k, v in c.items() if k not in ("a", "b", "out")}
        assert from_wire(host) == exp, ("host form", what)
        assert np.array_equal(got, host), ("_dev form differs from the host form", what)
        count += 1
    assert count > 150


def test_abi_refusals_and_messages():
    side = _Side()
    eng = side.eng
    L, h = eng.lib, eng.h

    def err():
        return (L.ncg_last_error(h) or b"").decode()
    r = ORDERS["bls12_381"]
    om, x = _small(P.omega(r, 2)), _small(5)
    a, b, out = to_wire([1, 2, 3, 4]), to_wire([5, 6, 7, 8]), np.zeros((8, 32), dtype=np.uint8)
    da, db, dout = _cuda(a), _cuda(b), _cuda(out)
    assert set(_raw_calls(L, h, 0, om, a, b, x, out, False).values()) == {OK}, err()
    assert set(_raw_calls(L, h, 0, om, da, db, x, dout, True, side.s).values()) == {OK}, err()
    side.stream.synchronize()
    for fid in (1, 2, 3, 4, 6, 7, -1):
        for dev, bufs in ((False, (a, b, x, out)), (True, (da, db, x, dout))):
            for name in ENTRY_POINTS:
                assert _raw_calls(L, h, fid, om, *bufs, dev, side.s, only=name) == {name: UNSUPPORTED}, (fid, dev, name)
                assert err().endswith("poly: unsupported field %d" % fid)
    for dev, bufs in ((False, (a, b, x, out)), (True, (da, db, x, dout))):
        for bad_op in (3, -1):
            assert _raw_calls(L, h, 0, om, *bufs, dev, side.s, op=bad_op, only="pointwise") == {"pointwise": INVALID_ARG}
            assert "unknown op" in err()
        for bad_m in (0, 9):
            assert _raw_calls(L, h, 0, om, *bufs, dev, side.s, m=bad_m, only="eval_monomial") == {"eval_monomial": INVALID_ARG}
            assert "out of range 1..8" in err()
        for na, nb in ((5, 1), (1, 5)):
            assert _raw_calls(L, h, 0, om, *bufs, dev, side.s, na=na, nb=nb, only="mul") == {"mul": INVALID_ARG}
            assert "do not fit" in err()
        for bad_bits in (-1, 29):
            for name in ("lagrange_basis", "mul"):
                assert _raw_calls(L, h, 0, om, *bufs, dev, side.s, log2n=bad_bits, na=0, nb=0, only=name) == {name: INVALID_ARG}
                assert "log2n %d out of range 0..28" % bad_bits in err()
    # a misaligned device pointer is refused, not dereferenced
    off = ctypes.c_void_p(da.data_ptr() + 8)
    assert L.ncg_poly_pointwise_dev(h, 0, 0, 3, off, _vp(db), _vp(dout), side.s) == INVALID_ARG
    assert "16-byte aligned" in err()
    assert L.ncg_poly_scale_dev(h, 0, 3, _vp(da), _vp(x), 0, off, side.s) == INVALID_ARG
    assert L.ncg_poly_eval_dev(h, 0, 3, _vp(da), off, _vp(dout), side.s) == INVALID_ARG
    assert L.ncg_poly_eval_monomial_dev(h, 0, 3, off, 1, _vp(x), _vp(dout), side.s) == INVALID_ARG
    assert L.ncg_poly_lagrange_basis_dev(h, 0, 2, _vp(om), _vp(x), 0, off, side.s) == INVALID_ARG
    assert L.ncg_poly_mul_dev(h, 0, 2, _vp(om), 3, off, 4, _vp(db), _vp(dout), side.s) == INVALID_ARG
    # a root of the other field is refused with the NTT's message
    om_bn = _small(P.omega(ORDERS["bn254"], 2))
    assert L.ncg_poly_mul(h, 0, 2, _vp(om_bn), 4, _vp(a), 4, _vp(b), _vp(out)) == INVALID_ARG
    assert "not a primitive 2^2-th root" in err()
    assert L.ncg_poly_lagrange_basis(h, 5, 2, _vp(om), _vp(x), 0, _vp(out)) == INVALID_ARG
    assert "not a primitive 2^2-th root" in err()
    # n = 0: the vector operations touch nothing, the evaluations write zero and need their output
    assert L.ncg_poly_pointwise(h, 0, 0, 0, None, None, None) == OK and L.ncg_poly_pointwise_dev(h, 5, 2, 0, None, None, None, None) == OK
    assert L.ncg_poly_scale(h, 0, 0, None, None, 1, None) == OK and L.ncg_poly_scale_dev(h, 5, 0, None, None, 0, None, None) == OK
    out[:] = 0xAB
    assert L.ncg_poly_eval(h, 0, 0, None, None, _vp(out)) == OK and not out[0].any() and (out[1] == 0xAB).all()
    out[:] = 0xAB
    assert L.ncg_poly_eval_monomial(h, 5, 0, None, 3, _vp(x), _vp(out)) == OK and not out[:3].any() and (out[3] == 0xAB).all()
    dout.fill_(0xAB)
    assert L.ncg_poly_eval_dev(h, 5, 0, None, None, _vp(dout), side.s) == OK
    assert L.ncg_poly_eval_monomial_dev(h, 0, 0, None, 2, _vp(x), ctypes.c_void_p(dout.data_ptr() + 64), side.s) == OK
    got = side.done(dout)
    assert not got[0].any() and (got[1] == 0xAB).all() and not got[2:4].any() and (got[4] == 0xAB).all()
    assert L.ncg_poly_eval(h, 0, 0, None, None, None) == INVALID_ARG and L.ncg_poly_eval_monomial_dev(h, 0, 0, None, 1, None, None, None) == INVALID_ARG
    assert L.ncg_poly_eval_monomial(h, 0, 0, None, 0, None, _vp(out)) == INVALID_ARG      # m is checked before the empty input


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000, 4097, 2 ** 18 + 3])
@pytest.mark.parametrize("field", FIELDS)
def test_pointwise_and_scale(field, n):
    """vector width, wave, block and grid-stride edges; in place over either operand; host form == _dev form"""
    r, fid = ORDERS[field], FIELD_IDS[field]
    side = _Side()
    eng = side.eng
    if n <= 4097:
        av, bv = P.rand_vec(r, n, "pa"), P.rand_vec(r, n, "pb")[::-1]
        a, b = to_wire(av), to_wire(bv)
    else:
        a, b = P.rand_wire(r, n, "pa"), P.rand_wire(r, n, "pb")[::-1].copy()
        av, bv = from_wire(a), from_wire(b)
    sc = P.rand_vec(r, 9, "scalar")[4]
    want = {P.POLY_ADD: P.add(r, av, bv), P.POLY_SUB: P.sub(r, av, bv), P.POLY_DOT: P.dot(r, av, bv)}
    da, db = _cuda(a), _cuda(b)
    for op, exp in want.items():
        host = eng.poly_pointwise(op, a, b, field=fid)
        assert from_wire(host) == exp, (op, n)
        out = torch.full_like(da, 0xFF)
        eng.poly_pointwise_dev(op, n, da.data_ptr(), db.data_ptr(), out.data_ptr(), side.s, field=fid)
        assert np.array_equal(side.done(out), host), (op, n)
        for alias in (0, 1):                    # out aliasing a, then b
            xa, xb = da.clone(), db.clone()
            torch.cuda.synchronize()
            eng.poly_pointwise_dev(op, n, xa.data_ptr(), xb.data_ptr(), (xa, xb)[alias].data_ptr(), side.s, field=fid)
            assert np.array_equal(side.done((xa, xb)[alias]), host), (op, n, alias)
            assert torch.equal((xb, xa)[alias], (db, da)[alias])
    host = eng.poly_scale(a, sc, field=fid)
    assert from_wire(host) == P.scale(r, av, sc)
    xa = da.clone()
    torch.cuda.synchronize()
    eng.poly_scale_dev(n, xa.data_ptr(), sc, False, xa.data_ptr(), side.s, field=fid)
    assert np.array_equal(side.done(xa), host)
    # all r - 1: 2 (r - 1) = r - 2, 0, (r - 1)^2 = 1, (r - 1) s = -s
    top = np.tile(to_wire([r - 1]), (n, 1))
    for op, v in ((P.POLY_ADD, r - 2), (P.POLY_SUB, 0), (P.POLY_DOT, 1)):
        assert np.array_equal(eng.poly_pointwise(op, top, top, field=fid), np.tile(to_wire([v]), (n, 1)))
    assert np.array_equal(eng.poly_scale(top, r - 1, field=fid), np.tile(to_wire([1]), (n, 1)))
    assert np.array_equal(eng.poly_scale(top, sc, field=fid), np.tile(to_wire([(r - sc) % r]), (n, 1)))


@pytest.mark.parametrize("n", [1, 2, 257, 2 ** 14 + 5])
@pytest.mark.parametrize("field", FIELDS)
def test_shift(field, n):
    r, fid = ORDERS[field], FIELD_IDS[field]
    side = _Side()
    eng = side.eng
    av = P.rand_vec(r, n, "shift")
    a = to_wire(av)
    da = _cuda(a)
    for f in (0, 1, r - 1, P.rand_vec(r, 9, "factor")[4]):
        pw, exp = 1, []
        for v in av:                             # the reference's loop (fft.ts:844-848), 0^0 = 1
            exp.append(v * pw % r)
            pw = pw * f % r
        host = eng.poly_scale(a, f, powers=True, field=fid)
        assert from_wire(host) == exp, (n, f)
        xa = da.clone()
        torch.cuda.synchronize()
        eng.poly_scale_dev(n, xa.data_ptr(), f, True, xa.data_ptr(), side.s, field=fid)     # in place
        assert np.array_equal(side.done(xa), host)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 ** 17 + 1])
@pytest.mark.parametrize("field", FIELDS)
def test_dot_sum_and_monomial_eval(field, n):
    """a block's span is 256 elements for the dot-sum (more than one block from 257) and 2048 for the Horner runs (a second
    step of every thread from 2049); 2^17 + 1 leaves the second launch of the dot-sum 513 partials for its 256 threads"""
    r, fid = ORDERS[field], FIELD_IDS[field]
    side = _Side()
    eng = side.eng
    if n <= 4096:
        av, bv = P.rand_vec(r, n, "da"), P.rand_vec(r, n, "db")[::-1]
        a, b = to_wire(av), to_wire(bv)
    else:
        a, b = P.rand_wire(r, n, "da"), P.rand_wire(r, n, "db")[::-1].copy()
        av, bv = from_wire(a), from_wire(b)
    assert eng.poly_eval(a, b, field=fid) == P.dot_sum(r, av, bv)
    top = np.tile(to_wire([r - 1]), (n, 1))
    assert eng.poly_eval(top, top, field=fid) == n % r
    rng = random.Random("xs-%s-%d" % (field, n))
    xs = [1, r - 1, 0] + [rng.randrange(r) for _ in range(5)]
    exp = [sum(av) % r, sum(v if i % 2 == 0 else -v for i, v in enumerate(av)) % r, av[0]] + [P.horner(r, av, x) for x in xs[3:]]
    got8 = eng.poly_eval_monomial(a, xs, field=fid)
    assert got8 == exp
    assert eng.poly_eval_monomial(a, xs[:3], field=fid) == exp[:3]
    singles = [eng.poly_eval_monomial(a, [x], field=fid)[0] for x in xs]
    assert singles == got8
    # the _dev forms write exactly their outputs
    da, db = _cuda(a), _cuda(b)
    out = torch.full((10, 32), 0xEE, dtype=torch.uint8, device="cuda")
    eng.poly_eval_dev(n, da.data_ptr(), db.data_ptr(), out.data_ptr(), side.s, field=fid)
    eng.poly_eval_monomial_dev(n, da.data_ptr(), xs, out.data_ptr() + 32, side.s, field=fid)
    got = side.done(out)
    assert from_wire(got[:9]) == [P.dot_sum(r, av, bv)] + exp and (got[9] == 0xEE).all()


@pytest.mark.parametrize("field", FIELDS)
def test_monomial_eval_more_partials_than_threads(field):
    """2^19 + 2049 coefficients: 257 blocks, one partial more than the second launch's block holds threads; closed forms"""
    r, fid = ORDERS[field], FIELD_IDS[field]
    n = 2 ** 19 + 2049
    top = np.tile(to_wire([r - 1]), (n, 1))
    top[0] = to_wire([5])[0]
    got = get_engine().poly_eval_monomial(top, [1, r - 1, 0, 2], field=fid)
    geo = (pow(2, n, r) - 1 - 1) % r            # sum_{i >= 1} 2^i = 2^n - 2
    assert got == [(5 - (n - 1)) % r, (5 + 1) % r if (n - 1) % 2 else 5, 5, (5 - geo) % r]


@pytest.mark.parametrize("field", FIELDS)
def test_mirror_replays_the_fixture(field):
    """every device-side entry of the fixture through the mirror's names, lists in and out, with and without an fft"""
    fr = FR[field]
    roots = G.rootsOfUnity(fr, 7)
    p0, p1 = G.poly(fr, roots), G.poly(fr, roots, None, G.FFT(roots, fr))
    for c in P.kat()["fields"][field]["cases"]:
        op = c["op"]
        for p in (p0, p1) if c["fft"] else (p0,):
            if op in ("add", "sub", "dot", "mul", "convolve", "eval"):
                got = getattr(p, op)(c["a"], c["b"])
            elif op == "scale":
                got = p.mul(c["a"], c["x"])
            elif op == "shift":
                got = p.shift(c["a"], c["x"])
            elif op == "monomial_basis":
                got = p.monomial.basis(c["x"], c["n"])
            elif op == "monomial_eval":
                got = p.monomial.eval(c["a"], c["x"])
            elif op == "lagrange_basis":
                got = p.lagrange.basis(c["x"], c["n"], c["brp"])
            elif op == "lagrange_eval":
                got = p.lagrange.eval(c["a"], c["x"], c["brp"])
            else:
                continue
            assert got == c["out"], {k: v for k, v in c.items() if k != "out"}
    # arrays in, arrays out
    c = P.cases(field, "dot")[-2]
    got = p0.dot(to_wire(c["a"]), to_wire(c["b"]))
    assert isinstance(got, np.ndarray) and from_wire(got) == c["out"]
    # the reference's P.eval(a, P.monomial.basis(x, n)) == P.monomial.eval(a, x)
    a = P.rand_vec(fr.ORDER, 777, "basis")
    x = P.rand_vec(fr.ORDER, 9, "bx")[4]
    assert p0.eval(a, p0.monomial.basis(x, len(a))) == p0.monomial.eval(a, x) == P.horner(fr.ORDER, a, x)


@pytest.mark.parametrize("log2n", [0, 1, 6, 10, 13])
@pytest.mark.parametrize("field", FIELDS)
def test_lagrange_basis(field, log2n):
    r, fid = ORDERS[field], FIELD_IDS[field]
    fr = FR[field]
    n = 1 << log2n
    eng = get_engine()
    om = P.omega(r, log2n)
    p = _mirror(field)
    fft = G.FFT(p.roots, fr)
    a = P.rand_vec(r, n, "lag-a")
    coeffs = fft.inverse(a)                      # the polynomial whose values on the roots are a
    x = P.rand_vec(r, 9, "lag-x")[4]
    for brp in (False, True):
        table = P.roots(r, log2n, brp)
        for xx in (x, 0):
            if log2n == 0 and xx == 1:
                continue
            basis = from_wire(eng.poly_lagrange_basis(log2n, om, xx, brp=brp, field=fid))
            assert sum(basis) % r == 1
            if log2n <= 10:
                assert basis == P.lagrange_basis(r, xx, n, brp), (log2n, brp, xx)
            vals = G.bitReversalPermutation(a) if brp and log2n else a
            # 'lagrange interpolation' (test/fft.test.ts:650-653): sum a_i L_i(x) == monomial.eval(inverse(a), x)
            assert P.dot_sum(r, vals, basis) == P.horner(r, coeffs, xx)
            assert p.lagrange.eval(vals, xx, brp) == P.horner(r, coeffs, xx)
        for k in sorted({0, n // 2, n - 1}):     # x a root: the exact delta, then a dense basis again (the index word is cleared)
            delta = eng.poly_lagrange_basis(log2n, om, table[k], brp=brp, field=fid)
            exp = np.zeros((n, 32), dtype=np.uint8)
            exp[k, 0] = 1
            assert np.array_equal(delta, exp), (log2n, brp, k)
            assert p.lagrange.eval(a, table[k], brp) == a[k]
            if log2n:
                dense = from_wire(eng.poly_lagrange_basis(log2n, om, x, brp=brp, field=fid))
                assert all(dense) and sum(dense) % r == 1
    # the _dev form on a side stream, no host synchronisation in between: root, non-root, root
    side = _Side()
    outs = [torch.full((n, 32), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(3)]
    table = P.roots(r, log2n)
    stream = side.s
    for o, xx in zip(outs, (table[n - 1], x, table[n // 2])):
        eng.poly_lagrange_basis_dev(log2n, om, xx, False, o.data_ptr(), stream, field=fid)
    side.stream.synchronize()
    for o, xx in zip(outs, (table[n - 1], x, table[n // 2])):
        assert np.array_equal(o.cpu().numpy(), eng.poly_lagrange_basis(log2n, om, xx, field=fid))


def _check_product(r, a, b, got, n, wraps):
    if n <= 2 ** 11 and (len(a) <= 2 ** 10 or not wraps):
        assert got == P.cyclic(r, a, b, n)
        return
    rng = random.Random("prod-%d" % n)
    for _ in range(3):                           # eval(ab, x) == eval(a, x) eval(b, x) (x^n = 1 makes the wrap exact at roots only,
        x = rng.randrange(r)                     # so a wrapped product is compared at roots of unity of order n)
        if wraps:
            x = pow(P.omega(r, n.bit_length() - 1), rng.randrange(n), r)
        assert P.horner(r, got, x) == P.horner(r, a, x) * P.horner(r, b, x) % r


@pytest.mark.parametrize("log2n", [0, 1, 5, 10, 11, 14])
@pytest.mark.parametrize("field", FIELDS)
def test_mul_and_convolve(field, log2n):
    """one-pass and two-pass transforms; full-length cyclic products, short operands zero-extended on the device, out over a"""
    r, fid = ORDERS[field], FIELD_IDS[field]
    n = 1 << log2n
    side = _Side()
    eng = side.eng
    om = P.omega(r, log2n)
    a, b = P.rand_vec(r, n, "mul-a"), P.rand_vec(r, n, "mul-b")[::-1]
    shapes = [(n, n), (min(3, n), min(2, n)), (1, n), (max(n // 2, 1), max(n // 2, 1)), (min(n // 2 + 1, n), max(n // 2, 1)), (0, min(5, n))]
    for na, nb in shapes:
        aa, bb = a[:na], b[:nb]
        A, B = to_wire(aa).reshape(-1, 32), to_wire(bb).reshape(-1, 32)
        host = eng.poly_mul(log2n, om, A, B, field=fid)
        got = from_wire(host)
        if na == 0:
            assert got == [0] * n
        else:
            _check_product(r, aa, bb, got, n, wraps=na + nb - 1 > n)
        da, db = _cuda(np.concatenate([A, np.zeros((n - na, 32), dtype=np.uint8)])), _cuda(B if nb else np.zeros((1, 32), dtype=np.uint8))
        keep_b = db.clone()
        torch.cuda.synchronize()
        eng.poly_mul_dev(log2n, om, na, da.data_ptr(), nb, db.data_ptr(), da.data_ptr(), side.s, field=fid)    # out over a
        assert np.array_equal(side.done(da), host), (log2n, na, nb)
        assert torch.equal(db, keep_b)


@pytest.mark.parametrize("field", FIELDS)
def test_mirror_products(field):
    """the quadratic product of lengths that are no power of two, and the reference's convolve distributivity"""
    r = ORDERS[field]
    p = _mirror(field)
    for L in (3, 5):
        a, b = P.rand_vec(r, L, "q-a"), P.rand_vec(r, L, "q-b")[::-1]
        assert p.mul(a, b) == P.cyclic(r, a, b, L)
    L = 1000
    a, b = P.rand_vec(r, L, "q-a"), P.rand_vec(r, L, "q-b")[::-1]
    got = p.mul(a, b)
    assert len(got) == L
    assert got == P.cyclic(r, a, b, L)              # the quadratic form itself, which holds the evaluation property
    full = p.convolve(a, b)                         # ... that the linear product shows at three random points
    assert len(full) == 2048 and got == [(full[k] + full[k + L]) % r for k in range(L)]
    rng = random.Random("mirror-1000")
    for _ in range(3):
        x = rng.randrange(r)
        assert P.horner(r, full, x) == P.horner(r, a, x) * P.horner(r, b, x) % r
    # a * (b + c) == a * b + a * c
    a, b, c = P.rand_vec(r, 37, "d-a"), P.rand_vec(r, 50, "d-b"), P.rand_vec(r, 50, "d-c")
    assert p.convolve(a, p.add(b, c)) == p.add(p.convolve(a, b), p.convolve(a, c))
    assert p.convolve([1, 2, 3], [4, 5]) == [4, 13, 22, 15]


@pytest.mark.parametrize("field", FIELDS)
def test_chained_on_the_device(field):
    """the pipeline the layer exists for, on one side stream with no host copy in between: two resident polynomials through
    ncg_ntt_dev, ncg_poly_pointwise_dev (dot), the inverse ncg_ntt_dev and ncg_poly_eval_monomial_dev == the host forms"""
    r, fid = ORDERS[field], FIELD_IDS[field]
    bits, h = 12, 1 << 11
    n = 1 << bits
    side = _Side()
    eng = side.eng
    om = P.omega(r, bits)
    a, b = P.rand_vec(r, h, "ch-a"), P.rand_vec(r, h, "ch-b")[::-1]
    A, B = to_wire(a + [0] * h), to_wire(b + [0] * h)
    xs = [P.rand_vec(r, 9, "ch-x")[4], 1, r - 1]
    da, db = _cuda(A), _cuda(B)
    out = torch.full((3, 32), 0xFF, dtype=torch.uint8, device="cuda")
    s = side.s
    eng.ntt_dev(bits, 1, om, da.data_ptr(), da.data_ptr(), s, brp_output=True, field=fid)
    eng.ntt_dev(bits, 1, om, db.data_ptr(), db.data_ptr(), s, brp_output=True, field=fid)
    eng.poly_pointwise_dev(P.POLY_DOT, n, da.data_ptr(), db.data_ptr(), da.data_ptr(), s, field=fid)
    eng.ntt_dev(bits, 1, om, da.data_ptr(), da.data_ptr(), s, inverse=True, brp_input=True, field=fid)
    eng.poly_eval_monomial_dev(n, da.data_ptr(), xs, out.data_ptr(), s, field=fid)
    side.stream.synchronize()
    prod = eng.poly_mul(bits, om, to_wire(a), to_wire(b), field=fid)
    assert np.array_equal(da.cpu().numpy(), prod)
    assert from_wire(out.cpu().numpy()) == eng.poly_eval_monomial(prod, xs, field=fid) == \
        [P.horner(r, a, x) * P.horner(r, b, x) % r for x in xs]


def test_fields_alternating_on_one_fresh_context():
    """bls12-381 and bn254 calls interleaved at one size on a fresh Engine: the workspace and the twiddle tables of one field
    are not disturbed by the other"""
    eng = Engine(0)
    try:
        bits, n = 9, 512
        data = {}
        for field in FIELDS:
            r = ORDERS[field]
            a, b = P.rand_vec(r, n, "alt-a"), P.rand_vec(r, n, "alt-b")[::-1]
            x = P.rand_vec(r, 9, "alt-x")[4]
            data[field] = (a, b, x, P.cyclic(r, a, b, n), P.lagrange_basis(r, x, n), P.dot_sum(r, a, b), P.horner(r, a, x))
        for _ in range(2):
            for field in FIELDS + FIELDS[::-1]:
                r, fid = ORDERS[field], FIELD_IDS[field]
                a, b, x, prod, basis, ds, hv = data[field]
                om = P.omega(r, bits)
                assert from_wire(eng.poly_mul(bits, om, to_wire(a), to_wire(b), field=fid)) == prod
                assert from_wire(eng.poly_lagrange_basis(bits, om, x, field=fid)) == basis
                assert eng.poly_eval(to_wire(a), to_wire(b), field=fid) == ds
                assert eng.poly_eval_monomial(to_wire(a), [x], field=fid) == [hv]
                assert from_wire(eng.poly_pointwise(P.POLY_DOT, to_wire(a), to_wire(b), field=fid)) == P.dot(r, a, b)
        with pytest.raises(NativeError, match="not a primitive 2\\^9-th root"):
            eng.poly_mul(bits, P.omega(ORDERS["bn254"], bits), to_wire(data["bls12_381"][0]), to_wire(data["bls12_381"][1]), field=0)
    finally:
        eng.close()
