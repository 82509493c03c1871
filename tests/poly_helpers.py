"""Shared by the poly tests: the fixture tests/golden/poly_kat.json (the reference's own answers), a plain-Python restatement of
poly() (src/abstract/fft.ts:583-926) on integers - the oracle for the sizes the fixture does not reach - seeded input builders and
the ctypes side of the ht_poly_* host twin (csrc/hosttest.hip)."""
import ctypes
import json
import os
import random
import zlib

import numpy as np

import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
ORDERS = {
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    "bn254": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
}
FIELD_IDS = {"bls12_381": 0, "bn254": 5}
FIELDS = ("bls12_381", "bn254")
POLY_ADD, POLY_SUB, POLY_DOT = 0, 1, 2
_kat = None


def kat():
    """{"errors": {...}, "fields": {name: {"order": int, "cases": [case]}}}: vectors resolved, numbers as ints"""
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "poly_kat.json")) as f:
            raw = json.load(f)
        vecs = [[int(x) for x in v] for v in raw["vectors"]]
        fields = {}
        for name, fd in raw["fields"].items():
            cases = []
            for c in fd["cases"]:
                c = dict(c)
                for k in ("a", "b"):
                    if k in c:
                        c[k] = vecs[c[k]]
                if "x" in c:
                    c["x"] = int(c["x"])
                o = c["out"]
                c["out"] = vecs[o["v"]] if isinstance(o, dict) else (int(o) if isinstance(o, str) else o)
                cases.append(c)
            fields[name] = {"order": int(fd["order"]), "cases": cases}
        _kat = {"errors": raw["errors"], "fields": fields, "generator": int(raw["generator"])}
    return _kat


def cases(field, *ops):
    return [c for c in kat()["fields"][field]["cases"] if c["op"] in ops]


# ---------------------------------------------------------------- the formulas on integers
def omega(r, bits, generator=7):
    """roots.omega(bits): G^((r - 1) / 2^bits) (fft.ts:238-241)"""
    assert (r - 1) % (1 << bits) == 0
    return pow(generator, (r - 1) >> bits, r)


def rev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def roots(r, bits, brp=False):
    w = omega(r, bits)
    t = [pow(w, k, r) for k in range(1 << bits)]
    return [t[rev(i, bits)] for i in range(1 << bits)] if brp else t


def add(r, a, b):
    return [(x + y) % r for x, y in zip(a, b)]


def sub(r, a, b):
    return [(x - y) % r for x, y in zip(a, b)]


def dot(r, a, b):
    return [x * y % r for x, y in zip(a, b)]


def scale(r, a, s):
    return [x * s % r for x in a]


def shift(r, a, s):
    return [x * pow(s, i, r) % r for i, x in enumerate(a)]


def dot_sum(r, a, b):
    return sum(x * y for x, y in zip(a, b)) % r


def horner(r, a, x):
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % r
    return acc


def monomial_basis(r, x, n):
    return [pow(x, i, r) for i in range(n)]


def cyclic(r, a, b, n):
    """the product of a and b mod x^n - 1 (fft.ts:816-824 for equal lengths)"""
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[(i + j) % n] = (out[(i + j) % n] + x * y) % r
    return out


def next_pow2(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def convolve(r, a, b):
    return cyclic(r, a, b, next_pow2(len(a) + len(b) - 1))


def lagrange_basis(r, x, n, brp=False):
    bits = n.bit_length() - 1
    w = roots(r, bits, brp)
    if x in w:
        return [1 if v == x else 0 for v in w]
    c = (pow(x, n, r) - 1) * pow(n, -1, r) % r
    return [c * wi % r * pow(x - wi, -1, r) % r for wi in w]


def lagrange_eval(r, a, x, brp=False):
    return dot_sum(r, a, lagrange_basis(r, x, len(a), brp))


def vanishing(r, rs):
    out = [1] + [0] * len(rs)
    for root in rs:
        neg = -root % r
        for j in range(len(rs), 0, -1):
            out[j] = (out[j] * neg + out[j - 1]) % r
        out[0] = out[0] * neg % r
    return out


def degree(a):
    for i in range(len(a) - 1, -1, -1):
        if a[i]:
            return i
    return -1


def extend(a, n):
    return (list(a) + [0] * n)[:n]


def restate(r, c):
    """the answer of the restatement for one fixture case"""
    op = c["op"]
    if op == "add":
        return add(r, c["a"], c["b"])
    if op == "sub":
        return sub(r, c["a"], c["b"])
    if op == "dot":
        return dot(r, c["a"], c["b"])
    if op == "mul":
        return cyclic(r, c["a"], c["b"], len(c["a"]))
    if op == "scale":
        return scale(r, c["a"], c["x"])
    if op == "convolve":
        return convolve(r, c["a"], c["b"])
    if op == "shift":
        return shift(r, c["a"], c["x"])
    if op == "eval":
        return dot_sum(r, c["a"], c["b"])
    if op == "monomial_basis":
        return monomial_basis(r, c["x"], c["n"])
    if op == "monomial_eval":
        return horner(r, c["a"], c["x"])
    if op == "lagrange_basis":
        return lagrange_basis(r, c["x"], c["n"], c["brp"])
    if op == "lagrange_eval":
        return lagrange_eval(r, c["a"], c["x"], c["brp"])
    if op == "vanishing":
        return vanishing(r, c["a"])
    if op == "degree":
        return degree(c["a"])
    if op == "extend":
        return extend(c["a"], c["n"])
    if op == "roots":
        return roots(r, c["n"], c["brp"])
    if op == "omega":
        return omega(r, c["n"])
    raise AssertionError(op)


# ---------------------------------------------------------------- inputs
def rand_vec(r, n, seed):
    """n seeded values with 0, 1 and r - 1 planted at both ends (as far as n allows)"""
    rng = random.Random("poly-%s-%d" % (seed, n))
    v = [rng.randrange(r) for _ in range(n)]
    for i, s in enumerate((0, 1, r - 1)):
        if 2 * (i + 1) <= n:
            v[i] = s
            v[n - 1 - i] = s
    return v


def rand_wire(r, n, seed):
    """a large seeded vector as uint8 [n, 32] without a Python loop: 31 random bytes per element (values below 2^248 < r) with
    0, 1 and r - 1 planted at both ends"""
    rs = np.random.RandomState(zlib.crc32(("poly-%s-%d" % (seed, n)).encode()))
    out = np.zeros((n, 32), dtype=np.uint8)
    out[:, :31] = rs.randint(0, 256, size=(n, 31), dtype=np.uint8)
    for i, s in enumerate((0, 1, r - 1)):
        if 2 * (i + 1) <= n:
            out[i] = out[n - 1 - i] = np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8)
    return out


def to_wire(values):
    out = np.empty((len(values), 32), dtype=np.uint8)
    for i, v in enumerate(values):
        out[i] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
    return out


def from_wire(arr):
    flat = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") for row in flat]


# ---------------------------------------------------------------- host twin
_ht = None


def ht():
    global _ht
    if _ht is None:
        lib = hosttest.lib()
        vp, i32, sz, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint64
        lib.ht_poly_pointwise.argtypes = [i32, i32, sz, vp, vp, vp]
        lib.ht_poly_scale.argtypes = [i32, sz, vp, vp, i32, sz, vp]
        lib.ht_poly_eval.argtypes = [i32, sz, vp, vp, sz, vp]
        lib.ht_poly_eval_monomial.argtypes = [i32, sz, vp, i32, vp, sz, vp]
        lib.ht_poly_pow.argtypes = [i32, vp, u64, vp]
        lib.ht_poly_lagrange.argtypes = [i32, i32, vp, vp, i32, sz, vp, vp]
        lib.ht_poly_lag_run.argtypes = []
        _ht = lib
    return _ht


def _aligned(n_rows):
    """uint8 [n_rows, 32] at a 16-byte aligned address (the element loads are 16-byte accesses)"""
    raw = np.zeros(n_rows * 32 + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n_rows * 32].reshape(n_rows, 32)


def _in(values):
    a = _aligned(max(len(values), 1))
    if len(values):
        a[:len(values)] = to_wire(values)
    return a


def ht_pointwise(field, op, a, b):
    A, B, O = _in(a), _in(b), _aligned(max(len(a), 1))
    assert ht().ht_poly_pointwise(FIELD_IDS[field], op, len(a), A.ctypes.data, B.ctypes.data, O.ctypes.data) == 0
    return from_wire(O[:len(a)])


def ht_scale(field, a, s, powers, T=0):
    A, S, O = _in(a), _in([s]), _aligned(max(len(a), 1))
    assert ht().ht_poly_scale(FIELD_IDS[field], len(a), A.ctypes.data, S.ctypes.data, 1 if powers else 0, T, O.ctypes.data) == 0
    return from_wire(O[:len(a)])


def ht_eval(field, a, basis, T=0):
    A, B, O = _in(a), _in(basis), _aligned(1)
    assert ht().ht_poly_eval(FIELD_IDS[field], len(a), A.ctypes.data, B.ctypes.data, T, O.ctypes.data) == 0
    return from_wire(O)[0]


def ht_eval_monomial(field, a, xs, T=0):
    A, X, O = _in(a), _in(xs), _aligned(8)
    assert ht().ht_poly_eval_monomial(FIELD_IDS[field], len(a), A.ctypes.data, len(xs), X.ctypes.data, T, O.ctypes.data) == 0
    return from_wire(O)[:len(xs)]


def ht_pow(field, s, start):
    S, O = _in([s]), _aligned(1)
    assert ht().ht_poly_pow(FIELD_IDS[field], S.ctypes.data, start, O.ctypes.data) == 0
    return from_wire(O)[0]


def ht_lagrange(field, log2n, x, brp=False, T=0):
    """(basis, root index word): the word is 0xFFFFFFFF unless x is one of the roots"""
    r = ORDERS[field]
    W, X, O = _in([omega(r, log2n)]), _in([x]), _aligned(1 << log2n)
    root = np.zeros(1, dtype=np.uint32)
    assert ht().ht_poly_lagrange(FIELD_IDS[field], log2n, W.ctypes.data, X.ctypes.data, 1 if brp else 0, T, O.ctypes.data,
                                 root.ctypes.data) == 0
    return from_wire(O), int(root[0])
