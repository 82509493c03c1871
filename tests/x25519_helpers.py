"""Shared by the X25519 tests: the fixture tests/golden/x25519_kat.json (the reference's own answers), a plain-Python restatement
of the ladder of src/abstract/montgomery.ts:352-393 with clamp and decode - the oracle for random batches - the rows of the ladder
pieces (ncg_field_check field 16 / ht_x25519_op) and the ctypes side of the ht_x25519* host twins (csrc/hosttest.hip)."""
import ctypes
import json
import os
import random

import numpy as np

import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
P = 2**255 - 19
A24 = 121665
U = (1 << 29) + (1 << 19)          # fe9.hpp: a bound-B element has limbs below B * U
FIELD_X25519 = 16                   # ncg_field_check: the ladder pieces (15 is unassigned)
LOW_ORDER = (0, 1, P - 1, 325606250916557431795983626356110631294008115727848805560023387167927233504,
             39382357235489614581723060781553021112529911719440698176882885853963445705823)
INVALID = "invalid private or public key received"
_kat = None


def kat():
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "x25519_kat.json")) as f:
            _kat = json.load(f)
    return _kat


# ---------------------------------------------------------------- the reference's formulas on integers
def clamp(scalar):
    b = bytearray(scalar)
    b[0] &= 248
    b[31] = (b[31] & 127) | 64
    return int.from_bytes(b, "little")


def decode_u(u):
    return (int.from_bytes(u, "little") & ((1 << 255) - 1)) % P


def step(x1, x2, z2, x3, z3, swap):
    """cswap(swap) then one round of montgomery.ts:366-386"""
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    a, b, c, d = x2 + z2, x2 - z2, x3 + z3, x3 - z3
    aa, bb = a * a % P, b * b % P
    e, da, cb = aa - bb, d * a % P, c * b % P
    return aa * bb % P, e * (aa + A24 * e) % P, (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P


def ladder(u, k):
    x2, z2, x3, z3 = 1, 0, u, 1
    kx = k ^ (k >> 1)
    for t in range(254, -1, -1):
        x2, z2, x3, z3 = step(u, x2, z2, x3, z3, (kx >> t) & 1)
    if k & 1:
        x2, z2 = x3, z3
    return x2 * pow(z2, P - 2, P) % P


def scalar_mult(scalar, u):
    """x25519.scalarMult: 32 bytes, or None where the reference throws"""
    pu = decode_u(u)
    if pu in LOW_ORDER:
        return None
    r = ladder(pu, clamp(scalar))
    return None if r == 0 else r.to_bytes(32, "little")


def rand_rows(n, seed):
    rng = random.Random("x25519-%s-%d" % (seed, n))
    return np.frombuffer(bytes(rng.getrandbits(8) for _ in range(n * 32)), np.uint8).reshape(n, 32).copy()


def expect(scalars, us):
    """(out uint8 [n, 32], ok uint8 [n]) of the restatement; one scalar row is used for every u"""
    n = len(us)
    out, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        r = scalar_mult(bytes(scalars[i if len(scalars) == n else 0]), bytes(us[i]))
        if r is not None:
            out[i], ok[i] = np.frombuffer(r, np.uint8), 1
    return out, ok


def hex_rows(items):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in items), np.uint8).reshape(len(items), 32).copy()


def kat_expected(rows):
    """(out, ok) of fixture rows ({"out": hex or None})"""
    out, ok = np.zeros((len(rows), 32), np.uint8), np.zeros(len(rows), np.uint8)
    for i, c in enumerate(rows):
        if c["out"] is not None:
            out[i], ok[i] = np.frombuffer(bytes.fromhex(c["out"]), np.uint8), 1
    return out, ok


# ---------------------------------------------------------------- the ladder pieces on raw limbs
def limbs_value(limbs):
    return sum(int(v) << (29 * i) for i, v in enumerate(limbs))


def step_rows():
    """a [n, 36] = x2 z2 x3 z3 and b [n, 9] = x1 as raw limbs at the bound the ladder stores them at (1): every limb at the top
    of the bound (U - 1), every limb 0, each element in turn at the top with the others random, and 256 seeded random rows"""
    rng = random.Random("x25519-step")
    top, rows = U - 1, []
    rows.append(([top] * 36, [top] * 9))
    rows.append(([0] * 36, [0] * 9))
    for e in range(5):
        v = [rng.randrange(U) for _ in range(45)]
        v[9 * e:9 * e + 9] = [top] * 9
        rows.append((v[:36], v[36:]))
    for _ in range(256):
        v = [rng.randrange(U) for _ in range(45)]
        rows.append((v[:36], v[36:]))
    return np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.uint32)


def check_step(a, b, out, swap):
    """out [n, 36] against the restatement: the four values mod p, and every output limb below the declared bound (1 * U)"""
    assert int(out.max()) < U, "an output limb of x25519_step at or above its declared bound"
    for i in range(a.shape[0]):
        x2, z2, x3, z3 = (limbs_value(a[i, 9 * j:9 * j + 9]) for j in range(4))
        want = step(limbs_value(b[i]), x2, z2, x3, z3, swap)
        got = tuple(limbs_value(out[i, 9 * j:9 * j + 9]) % P for j in range(4))
        assert got == tuple(w % P for w in want), (i, swap)


def edge_u_rows():
    """encoded u of the fixture's edge rows (the low-order set in all its encodings, the non-canonical values) and 32 random ones"""
    us = [c["u"] for c in kat()["scalar_mult"] if not c["name"].startswith("random")]
    return np.concatenate([hex_rows(us), rand_rows(32, "edge-u")])


def edge_scalar_rows():
    return np.concatenate([hex_rows(["00" * 32, "ff" * 32, "07" + "00" * 30 + "80", "f8" + "ff" * 30 + "7f"]), rand_rows(32, "edge-k")])


def words36(rows8):
    """[n, 32] bytes -> the a operand of ops 1 / 2: the 8 LE words in front of 28 zero words"""
    a = np.zeros((rows8.shape[0], 36), np.uint32)
    a[:, :8] = np.ascontiguousarray(rows8).view("<u4").reshape(-1, 8)
    return a


def check_decode_u(rows8, out):
    for i in range(rows8.shape[0]):
        v = decode_u(bytes(rows8[i]))
        assert out[i, :8].astype("<u4").tobytes() == v.to_bytes(32, "little"), i
        assert int(out[i, 8]) == (0 if v in LOW_ORDER else 1), i


def check_decode_scalar(rows8, out):
    for i in range(rows8.shape[0]):
        assert out[i, :8].astype("<u4").tobytes() == clamp(bytes(rows8[i])).to_bytes(32, "little"), i


# ---------------------------------------------------------------- host twin
_ht = None


def ht():
    global _ht
    if _ht is None:
        lib = hosttest.lib()
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        lib.ht_x25519.argtypes = [vp, vp, i32, vp, vp, i32]
        lib.ht_x25519_base.argtypes = [vp, vp, vp, i32]
        lib.ht_ed25519_to_montgomery.argtypes = [vp, vp, vp, i32]
        lib.ht_x25519_op.argtypes = [i32, i32, vp, vp, vp]
        _ht = lib
    return _ht


def _rows32(a):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)


def ht_x25519(scalars, us, flags=0):
    s, u = _rows32(scalars), _rows32(us)
    n = u.shape[0]
    out, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert ht().ht_x25519(s.ctypes.data, u.ctypes.data, flags, out.ctypes.data, ok.ctypes.data, n) == 0
    return out, ok


def ht_x25519_base(scalars):
    s = _rows32(scalars)
    n = s.shape[0]
    out, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert ht().ht_x25519_base(s.ctypes.data, out.ctypes.data, ok.ctypes.data, n) == 0
    return out, ok


def ht_to_montgomery(pks):
    k = _rows32(pks)
    n = k.shape[0]
    out, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert ht().ht_ed25519_to_montgomery(k.ctypes.data, out.ctypes.data, ok.ctypes.data, n) == 0
    return out, ok


def ht_op(op, variant, a, b):
    """rows of ht_x25519_op: a [n, 36], b [n, 9] -> [n, 36] uint32"""
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    out = np.zeros((a.shape[0], 36), np.uint32)
    for i in range(a.shape[0]):
        assert ht().ht_x25519_op(op, variant, a[i].ctypes.data, b[i].ctypes.data, out[i].ctypes.data) == 0
    return out
