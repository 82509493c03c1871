"""Shared by the ristretto255 tests: the fixture tests/golden/ristretto255_kat.json (the reference's own answers), a plain-Python
restatement of fromBytes / toBytes / equals / the Elligator map / deriveToCurve of src/ed25519.ts:443-668 on integers - the oracle
for random batches, itself checked against the fixture - the edge rows, and the ctypes side of the ht_ristretto* host twins
(csrc/hosttest.hip).  Group arithmetic on representatives is plain affine Edwards addition here."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np

import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, -1, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
U = (1 << 29) + (1 << 19)          # fe9.hpp: a bound-1 element has limbs below U
FIELD_RISTRETTO = 17                # ncg_field_check: the ristretto255 pieces
ENC1, ENC2 = "invalid ristretto255 encoding 1", "invalid ristretto255 encoding 2"
DEFAULT_DST = b"ristretto255_XMD:SHA-512_R255MAP_RO_"
BASE = (15112221349535400772501151409588531511454012693041857206046113283949847762202,
        46316835694926478169428394003475163141307993866256225615783033603165251855960)
_kat = None


SEEDED = 256                        # seeded rows per family; the fixture stores their ANSWERS, the inputs are rebuilt here
SEEDED_AFFINE = 32                  # ... and the reference's representative (x || y) of the first 32 seeded rows that decode


def seeded_bytes(tag, i, n):
    """n bytes of row i of the family `tag`: SHA-512 in counter mode over a fixed label"""
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(b"ristretto255-kat/%s/%d/%d" % (tag.encode(), i, c)).digest()
        c += 1
    return out[:n]


def seeded_derive_in(i):
    return seeded_bytes("derive", i, 64)


def seeded_msg(i):
    return seeded_bytes("msg", i, 37 * i % 200)


def seeded_dst(i):
    return b"custom-DST-%d" % (i % 7)


def seeded_encoding(i, derive_out):
    """odd rows: a valid encoding (a hashed point); even rows: random, canonical and even, so that 'encoding 2' decides"""
    if i % 2:
        return bytes.fromhex(derive_out[i // 2])
    return (int.from_bytes(seeded_bytes("decode", i, 32), "little") % P & ~1).to_bytes(32, "little")


def kat():
    """the fixture with its seeded families expanded: decode = the listed rows + 256 seeded ones, derive = the 18 vectors of the RFC
    + 256 seeded + the listed edge rows, hash = the listed rows + 256 seeded messages under the default and 256 under a custom DST
    + the row with an oversize DST"""
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "ristretto255_kat.json")) as f:
            k = json.load(f)
        sd = k["seeded"]
        cut = lambda h, w: [h[j:j + w] for j in range(0, len(h), w)]  # noqa: E731
        dout, hdef, hcus = (cut("".join(sd[key]), 64) for key in ("derive_out", "hash_default_out", "hash_custom_out"))
        affine = iter(cut("".join(sd["decode_affine"]), 128) + [None] * SEEDED)
        assert len(dout) == len(hdef) == len(hcus) == len(sd["decode_verdict"]) == SEEDED
        msg = {"0": None, "1": ENC1, "2": ENC2}
        for i, v in enumerate(sd["decode_verdict"]):
            enc = seeded_encoding(i, dout).hex()
            k["decode"].append({"name": "random %d" % i, "enc": enc, "affine": next(affine) if v == "0" else None,
                                "bytes": enc if v == "0" else None, "error": msg[v]})
        rows = [{"in": seeded_derive_in(i).hex(), "out": o} for i, o in enumerate(dout)]
        k["derive"] = k["derive"][:18] + rows + k["derive"][18:]
        k["hash"] = k["hash"][:-1] + [{"msg": seeded_msg(i).hex(), "dst": None, "out": o} for i, o in enumerate(hdef)] + \
            [{"msg": seeded_msg(i).hex(), "dst": seeded_dst(i).hex(), "out": o} for i, o in enumerate(hcus)] + k["hash"][-1:]
        _kat = k
    return _kat


def kat_affine(c):
    """the wire point a decoder must give for a fixture row: the reference's representative where the fixture carries it, the
    restatement's (itself pinned by those rows) for the other rows that decode, zero for a rejected row"""
    if c["error"] is not None:
        return "00" * 64
    return c["affine"] or wire([decode(bytes.fromhex(c["enc"]))])[0].tobytes().hex()


# ---------------------------------------------------------------- the reference's formulas on integers
def is_odd(v):
    return v % P & 1


def uv_ratio(u, v):
    """uvRatio (src/ed25519.ts:107-125): (isValid, non-negative value)"""
    v3 = v * v * v % P
    v7 = v3 * v3 * v % P
    x = u * v3 * pow(u * v7, (P - 5) // 8, P) % P
    vx2 = v * x * x % P
    root2 = x * SQRT_M1 % P
    use1, use2, no = vx2 == u % P, vx2 == -u % P, vx2 == -u * SQRT_M1 % P
    if use2 or no:
        x = root2
    if is_odd(x):
        x = -x % P
    return use1 or use2, x


def _sqrt_even(v):
    ok, x = uv_ratio(v, 1)
    assert ok
    return x


SQRT_AD_MINUS_ONE = P - _sqrt_even(-D - 1)
INVSQRT_A_MINUS_D = pow(_sqrt_even(-1 - D), P - 2, P)
ONE_MINUS_D_SQ = (1 - D * D) % P
D_MINUS_ONE_SQ = (D - 1) ** 2 % P


def decode(enc):
    """fromBytes (:510-533): the affine representative (x, y), or the message of the error"""
    s = int.from_bytes(enc, "little")
    if s >= P or s & 1:
        return ENC1
    s2 = s * s % P
    u1, u2 = (1 - s2) % P, (1 + s2) % P
    v = (-D * u1 * u1 - u2 * u2) % P
    ok, inv = uv_ratio(1, v * u2 * u2 % P)
    dx = inv * u2 % P
    dy = inv * dx * v % P
    x = 2 * s * dx % P
    if is_odd(x):
        x = -x % P
    y = u1 * dy % P
    if not ok or is_odd(x * y) or y == 0:
        return ENC2
    return x, y


def encode_ext(X, Y, Z, T):
    """toBytes (:548-572) of an extended point"""
    u1 = (Z + Y) * (Z - Y) % P
    u2 = X * Y % P
    _, inv = uv_ratio(1, u1 * u2 * u2 % P)
    d1, d2 = inv * u1 % P, inv * u2 % P
    zinv = d1 * d2 * T % P
    if is_odd(T * zinv):
        X, Y, dd = Y * SQRT_M1 % P, X * SQRT_M1 % P, d1 * INVSQRT_A_MINUS_D % P
    else:
        dd = d2
    if is_odd(X * zinv):
        Y = -Y % P
    s = (Z - Y) * dd % P
    if is_odd(s):
        s = -s % P
    return s.to_bytes(32, "little")


def rotates(x, y):
    """whether toBytes takes its rotation branch for the affine point"""
    u1, u2 = (1 + y) * (1 - y) % P, x * y % P
    _, inv = uv_ratio(1, u1 * u2 * u2 % P)
    return bool(is_odd(x * y * inv * u1 * inv * u2 * x * y % P))


def encode(pt):
    x, y = pt
    return encode_ext(x, y, 1, x * y % P)


def equals(a, b):
    return a[0] * b[1] % P == a[1] * b[0] % P or a[1] * b[1] % P == a[0] * b[0] % P


def elligator(r0):
    """calcElligatorRistrettoMap (:443-461): the extended point and whether Ns / D was a square"""
    r = SQRT_M1 * r0 * r0 % P
    ns = (r + 1) * ONE_MINUS_D_SQ % P
    c = -1
    d = (c - D * r) * (r + D) % P
    sq, s = uv_ratio(ns, d)
    s_ = s * r0 % P
    if not is_odd(s_):
        s_ = -s_ % P
    if not sq:
        s, c = s_, r
    nt = (c * (r - 1) * D_MINUS_ONE_SQ - d) % P
    s2 = s * s % P
    w0, w1, w2, w3 = 2 * s * d % P, nt * SQRT_AD_MINUS_ONE % P, (1 - s2) % P, (1 + s2) % P
    return (w0 * w3 % P, w2 * w1 % P, w1 * w3 % P, w0 * w2 % P), sq


def ext_add(p, q):
    """the unified addition add-2008-hwcd-3 with a = -1 on extended points"""
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    A, B = (Y1 - X1) * (Y2 - X2) % P, (Y1 + X1) * (Y2 + X2) % P
    C, Dd = T1 * 2 * D * T2 % P, 2 * Z1 * Z2 % P
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return E * F % P, G * H % P, F * G % P, E * H % P


def to_affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def add(a, b):
    return to_affine(ext_add((a[0], a[1], 1, a[0] * a[1] % P), (b[0], b[1], 1, b[0] * b[1] % P)))


def mul(pt, k):
    acc, q = (0, 1, 1, 0), (pt[0], pt[1], 1, pt[0] * pt[1] % P)
    while k:
        if k & 1:
            acc = ext_add(acc, q)
        q = ext_add(q, q)
        k >>= 1
    return to_affine(acc)


def half255(b):
    return (int.from_bytes(b, "little") & ((1 << 255) - 1)) % P


def derive(b64):
    """deriveToCurve (:658-666): the extended representative R1 + R2"""
    return ext_add(elligator(half255(b64[:32]))[0], elligator(half255(b64[32:]))[0])


def derive_bytes(b64):
    return encode_ext(*derive(b64))


def expand_message_xmd(msg, dst, n=64):
    """RFC 9380 5.3.1 over SHA-512"""
    H = hashlib.sha512
    dstp = dst + bytes([len(dst)])
    b0 = H(bytes(128) + msg + n.to_bytes(2, "big") + b"\0" + dstp).digest()
    out = [H(b0 + b"\x01" + dstp).digest()]
    while 64 * len(out) < n:
        out.append(H(bytes(x ^ y for x, y in zip(b0, out[-1])) + bytes([len(out) + 1]) + dstp).digest())
    return b"".join(out)[:n]


def hash_to_curve_bytes(msg, dst=DEFAULT_DST):
    return derive_bytes(expand_message_xmd(msg, dst))


# the points of order 1, 2 and 4 (x = +-sqrt(-1), y = 0)
TORSION4 = [(0, 1), (0, P - 1), (SQRT_M1, 0), (P - SQRT_M1, 0)]


def order8_point():
    """a point of order 8: y = (u - 1) / (u + 1) of a Montgomery u of order 8, x a root of (y^2 - 1) / (d y^2 + 1)"""
    for u in (325606250916557431795983626356110631294008115727848805560023387167927233504,
              39382357235489614581723060781553021112529911719440698176882885853963445705823):
        y = (u - 1) * pow(u + 1, P - 2, P) % P
        ok, x = uv_ratio((y * y - 1) % P, (D * y * y + 1) % P)
        if ok and mul((x, y), 2) in TORSION4[2:]:
            return x, y
    raise AssertionError("no point of order 8 found")


# ---------------------------------------------------------------- rows
def rand_bytes(n, width, seed):
    rng = random.Random("ristretto-%s-%d" % (seed, n))
    return np.frombuffer(bytes(rng.getrandbits(8) for _ in range(n * width)), np.uint8).reshape(n, width).copy()


def hex_rows(items, width=32):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in items), np.uint8).reshape(len(items), width).copy()


def wire(pts):
    """affine pairs -> ed25519 wire points uint8 [n, 64]"""
    return np.frombuffer(b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for x, y in pts), np.uint8).reshape(len(pts), 64).copy()


def unwire(row):
    b = bytes(row)
    return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")


def expect_decode(rows):
    """(wire points [n, 64], ok [n]) of the restatement; a rejected row is zero"""
    out, ok = np.zeros((len(rows), 64), np.uint8), np.zeros(len(rows), np.uint8)
    for i, r in enumerate(rows):
        d = decode(bytes(r))
        if not isinstance(d, str):
            out[i], ok[i] = wire([d])[0], 1
    return out, ok


_multiples = None


def base_multiples(n=64):
    """[1..n] B as affine pairs (computed once)"""
    global _multiples
    if _multiples is None or len(_multiples) < n:
        pts, cur = [], BASE
        for _ in range(n):
            pts.append(cur)
            cur = add(cur, BASE)
        _multiples = pts
    return _multiples[:n]


_mixed = {}


def mixed_encodings(n, seed="mixed"):
    """n seeded rows, about half of them valid encodings (of k B, k random) and the rest random bytes (valid with probability 1/8
    when even and canonical), with the expected decoder output - cached per (n, seed)"""
    if (n, seed) not in _mixed:
        rng = random.Random("ristretto-%s" % seed)
        raw = rand_bytes(n, 32, seed)
        base = base_multiples(64)
        for i in range(n):
            if rng.random() < 0.5:
                raw[i] = np.frombuffer(encode(base[rng.randrange(64)]), np.uint8)
        _mixed[(n, seed)] = (raw, expect_decode(raw))
    return _mixed[(n, seed)]


def edge_encodings():
    """(name, 32 bytes, expected: 'ok' / ENC1 / ENC2) - the smallest inputs at which the decoder can go wrong"""
    i_even = SQRT_M1 if SQRT_M1 % 2 == 0 else P - SQRT_M1
    rows = [("identity", 0, "ok"), ("s = even sqrt(-1): u2 = 0", i_even, ENC2), ("s = odd sqrt(-1)", P - i_even, ENC1),
            ("s = p - 1: y = 0", P - 1, ENC2), ("s = p", P, ENC1), ("s = p + 1", P + 1, ENC1), ("s = 2^255 - 1", 2**255 - 1, ENC1),
            ("bit 255 on the identity", 1 << 255, ENC1), ("bit 255 on the basepoint", int.from_bytes(encode(BASE), "little") | 1 << 255, ENC1),
            ("s = 1", 1, ENC1), ("s = 2^256 - 1", 2**256 - 1, ENC1), ("basepoint", int.from_bytes(encode(BASE), "little"), "ok")]
    return [(n, v.to_bytes(32, "little"), w) for n, v, w in rows]


def edge_uniform():
    """(name, 64 bytes) rows of from_uniform: zero halves, equal halves (a doubling), bit 255, p - 1, 2^255 - 1"""
    le = lambda v: v.to_bytes(32, "little")  # noqa: E731
    h = bytes(rand_bytes(1, 32, "uniform-half")[0])
    hm = bytes(h[:31]) + bytes([h[31] & 0x7F])
    return [("both halves zero", bytes(64)), ("equal halves", hm + hm), ("first half with bit 255", hm[:31] + bytes([hm[31] | 0x80]) + le(5)),
            ("first half without bit 255", hm + le(5)), ("halves p - 1 and 2^255 - 1", le(P - 1) + le(2**255 - 1)),
            ("halves 2^255 - 1 and p - 1", le(2**255 - 1) + le(P - 1)), ("halves p and 0", le(P) + bytes(32)), ("halves 1 and 2^256 - 1", le(1) + le(2**256 - 1))]


def limbs(v):
    return [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]


def limbs_value(a):
    return sum(int(v) << (29 * i) for i, v in enumerate(a))


def op_rows(op):
    """a [n, 36], b [n, 9] raw limbs for ncg_field_check field 17: every limb at the top of the declared bound (U - 1), every limb
    zero, 256 seeded random rows.  For op 1 the random rows are extended points of the curve at a random projective scale (raw
    limbs of values below 2^255), so that their encodings have a known answer; the first two rows are arbitrary limbs."""
    rng = random.Random("ristretto-op-%d" % op)
    rows = [([U - 1] * 36, [U - 1] * 9), ([0] * 36, [0] * 9)]
    base = base_multiples(64)
    for j in range(256):
        if op == 1:
            x, y = base[j % 64]
            if j >= 64:
                x, y = add((x, y), TORSION4[1 + j % 3])
            z = rng.randrange(1, P)
            a = limbs(x * z % P) + limbs(y * z % P) + limbs(z) + limbs(x * y * z % P)
            rows.append((a, [0] * 9))
        else:
            rows.append(([rng.randrange(U) for _ in range(36)], [rng.randrange(U) for _ in range(9)]))
    return np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.uint32)


def check_op(op, a, b, out):
    """out [n, 36] of field 17 against the restatement (values mod p; output limbs below the declared bound)"""
    assert int(out.max()) < (1 << 32)
    for i in range(a.shape[0]):
        v = [limbs_value(a[i, 9 * j:9 * j + 9]) for j in range(4)]
        if op == 0:
            assert int(out[i, :9].max()) < U
            ok, x = uv_ratio(v[0] % P, limbs_value(b[i]) % P)
            assert limbs_value(out[i, :9]) % P == x and int(out[i, 9]) == int(ok), i
            assert not out[i, 10:].any()
        elif op == 1:
            if i >= 2:                                   # rows 0, 1 are not points: device against twin only
                assert out[i, :8].astype("<u4").tobytes() == encode_ext(*[x % P for x in v]), i
            assert not out[i, 8:].any()
        else:
            assert int(out[i].max()) < U
            want, _ = elligator(v[0] % P)
            got = tuple(limbs_value(out[i, 9 * j:9 * j + 9]) % P for j in range(4))
            assert got == want, i


# ---------------------------------------------------------------- host twin
_ht = None


def ht():
    global _ht
    if _ht is None:
        lib = hosttest.lib()
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        lib.ht_ristretto_decode.argtypes = [vp, vp, vp, i32]
        lib.ht_ristretto_encode.argtypes = [vp, vp, i32]
        lib.ht_ristretto_encode_proj.argtypes = [vp, vp, i32]
        lib.ht_ristretto_equals.argtypes = [vp, vp, vp, i32]
        lib.ht_ristretto_from_uniform.argtypes = [vp, vp, vp, i32]
        lib.ht_ristretto_mul.argtypes = [vp, vp, i32, vp, vp, i32]
        lib.ht_ristretto_op.argtypes = [i32, vp, vp, vp]
        lib.ht_ristretto_consts.argtypes = [vp]
        _ht = lib
    return _ht


def _rows(a, width):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, width)


def ht_decode(enc):
    e = _rows(enc, 32)
    n = e.shape[0]
    out, ok = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8)
    assert ht().ht_ristretto_decode(e.ctypes.data, out.ctypes.data, ok.ctypes.data, n) == 0
    return out, ok


def ht_encode(pts):
    p = _rows(pts, 64)
    out = np.zeros((p.shape[0], 32), np.uint8)
    assert ht().ht_ristretto_encode(p.ctypes.data, out.ctypes.data, p.shape[0]) == 0
    return out


def ht_encode_proj(xyz):
    p = _rows(xyz, 96)
    out = np.zeros((p.shape[0], 32), np.uint8)
    assert ht().ht_ristretto_encode_proj(p.ctypes.data, out.ctypes.data, p.shape[0]) == 0
    return out


def ht_equals(a, b):
    a, b = _rows(a, 64), _rows(b, 64)
    out = np.zeros(a.shape[0], np.uint8)
    assert ht().ht_ristretto_equals(a.ctypes.data, b.ctypes.data, out.ctypes.data, a.shape[0]) == 0
    return out


def ht_from_uniform(b64, affine=False):
    b = _rows(b64, 64)
    n = b.shape[0]
    out, aff = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    assert ht().ht_ristretto_from_uniform(b.ctypes.data, out.ctypes.data, aff.ctypes.data if affine else None, n) == 0
    return (out, aff) if affine else out


def ht_mul(enc, scalars, flags=0):
    e, s = _rows(enc, 32), _rows(scalars, 32)
    n = e.shape[0]
    out, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert ht().ht_ristretto_mul(e.ctypes.data, s.ctypes.data, flags, out.ctypes.data, ok.ctypes.data, n) == 0
    return out, ok


def ht_op(op, a, b):
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    out = np.zeros((a.shape[0], 36), np.uint32)
    for i in range(a.shape[0]):
        assert ht().ht_ristretto_op(op, a[i].ctypes.data, b[i].ctypes.data, out[i].ctypes.data) == 0
    return out


def ht_consts():
    out = np.zeros(32, np.uint32)
    assert ht().ht_ristretto_consts(out.ctypes.data) == 0
    return [int.from_bytes(out[8 * i:8 * i + 8].astype("<u4").tobytes(), "little") for i in range(4)]


def scalars_le(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), np.uint8).reshape(len(ks), 32).copy()
