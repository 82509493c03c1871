"""Shared by the RFC 9380 tests of edwards448 and decaf448: the fixture tests/golden/h2c448_kat.json (the reference's own answers), the
inputs of its rows - the listed ones by name, the seeded ones from a counter hash, so that the file stores answers only - an
independent restatement in plain Python (expand_message_xof on hashlib.shake_256, hash_to_field, big-integer models of
map_to_curve_elligator2_curve448 / _edwards448, the cofactor clearing and, through decaf448_helpers, the decaf448 map), and the ctypes
side of the ht_h2c448_* host twins (csrc/hosttest.hip)."""
import ctypes
import hashlib
import json
import os

import numpy as np

import decaf448_helpers as dh
import ed448_helpers as eh
import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
P, N = eh.P, eh.N
J = 156326
L = 84                                         # ceil((448 + 224) / 8) = ceil((446 + 224) / 8)
RO, NU = b"edwards448_XOF:SHAKE256_ELL2_RO_", b"edwards448_XOF:SHAKE256_ELL2_NU_"
QUUX = b"QUUX-V01-CS02-with-"
SCALAR_DST = b"HashToScalar-"
DECAF_DST = dh.DEFAULT_DST
SEEDED = 128
_kat = None


def kat():
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "h2c448_kat.json")) as f:
            _kat = json.load(f)
    return _kat


def seeded_bytes(tag, i, n):
    """n bytes of row i of the family `tag`: SHA-512 in counter mode over a fixed label (the generator and the tests share it)"""
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(b"h2c448-kat/%s/%d/%d" % (tag.encode(), i, c)).digest()
        c += 1
    return out[:n]


# ---------------------------------------------------------------- the listed rows
MESSAGES = [("empty", b""), ("abc", b"abc"), ("abcdef", b"abcdef0123456789"), ("q133", b"q" * 133), ("a512", b"a" * 512)]


def boundary_lengths(dst=RO):
    """message lengths for which len(msg) + 2 + len(DST) + 1 is 135, 136 and 137 mod 136: at 135 the suffix 0x1f and the final 0x80
    meet in one byte, at 136 the padding takes a block of its own"""
    fixed = 2 + len(dst) + 1
    return [(r - fixed) % 136 + 136 for r in (135, 0, 1)]


def listed_rows():
    """(name, msg, dst, count) of the hashToCurve / encodeToCurve rows"""
    rows = []
    for name, msg in MESSAGES:
        rows += [("%s/rfc/ro" % name, msg, QUUX + RO, 2), ("%s/rfc/nu" % name, msg, QUUX + NU, 1),
                 ("%s/default/ro" % name, msg, RO, 2), ("%s/default/nu" % name, msg, NU, 1)]
    rows += [("dst300", b"abc", b"x" * 300, 2), ("dst1", b"abc", b"D", 2), ("dst255", b"abc", b"y" * 255, 1)]
    rows += [("boundary%d" % r, seeded_bytes("boundary", k, n), RO, 2) for k, (r, n) in enumerate(zip((135, 136, 137), boundary_lengths()))]
    rows += [("long1000", seeded_bytes("long", 0, 1000), RO, 2)]
    return rows


def scalar_rows():
    """(name, msg, dst or None for the default) of hashToScalar, for ed448_hasher and decaf448_hasher alike"""
    return [(name, msg, None) for name, msg in MESSAGES] + [("abc/custom", b"abc", QUUX + RO), ("abc/dst300", b"abc", b"z" * 300)]


def decaf_rows():
    """(name, msg, dst) of decaf448_hasher.hashToCurve"""
    rows = [(name, msg, DECAF_DST) for name, msg in MESSAGES] + [("fill5", b"\x05" * 10, DECAF_DST)]
    return rows + [("abc/custom", b"abc", QUUX + DECAF_DST), ("abc/dst300", b"abc", b"w" * 300), ("abc/dst255", b"abc", b"v" * 255)]


def xof_rows():
    """(name, msg, dst, out_len) of expand_message_xof"""
    rows = [("len%d" % n, b"abc", RO, n) for n in (1, 135, 136, 137, 272, 273)]
    rows += [("boundary%d" % r, seeded_bytes("boundary", k, n), RO, 84) for k, (r, n) in enumerate(zip((135, 136, 137), boundary_lengths()))]
    rows += [("empty", b"", RO, 168), ("long1000", seeded_bytes("long", 0, 1000), RO, 112), ("dst1", b"abc", b"D", 64),
             ("dst255", b"abc", b"y" * 255, 64)]
    return rows


def edge_us():
    return [0, 1, P - 1, P, P + 1, 2**448 - 1]


def pair_rows():
    """(u0, u1) of the count = 2 map: (u, p - u) maps both to the same point (the map depends on u^2 and the sign of y on nothing
    else), so the sum is a doubling; then two generic pairs"""
    us = [5, int.from_bytes(seeded_bytes("pair", 0, 56), "big") % P]
    return [(u, P - u) for u in us] + [(u, u) for u in us] + [(us[0], us[1]), (1, 2)]


SEEDED_SUITES = ("ro", "nu", "decaf")          # hashToCurve, encodeToCurve, decaf448 hashToCurve: 128 seeded rows each
SEEDED_BATCH = 16
SEEDED_PAIRS = 32


def seeded_dst(suite, b):
    """the DST of batch b of a suite's seeded rows: its own bytes and its own length (1..255)"""
    return seeded_bytes("dst-" + suite, b, 1 + (37 * b + 11 * SEEDED_SUITES.index(suite)) % 255)


def seeded_row(suite, i):
    """(msg, dst) of row i < 128 of a suite's seeded family.  The rows come in 8 batches of 16, each batch with its own DST, so
    that a call (one DST) takes 16 rows; the message lengths run from 0 to 210"""
    return seeded_bytes("msg-" + suite, i, (13 * i + 5 * SEEDED_SUITES.index(suite)) % 211), seeded_dst(suite, i // SEEDED_BATCH)


def seeded_pairs():
    """32 seeded (u0, u1) of the count = 2 map, any values below 2^448"""
    return [(int.from_bytes(seeded_bytes("u0", i, 56), "big"), int.from_bytes(seeded_bytes("u1", i, 56), "big")) for i in range(SEEDED_PAIRS)]


def seeded_us():
    """128 seeded u below 2^448 for the single map"""
    return [int.from_bytes(seeded_bytes("u", i, 56), "big") for i in range(SEEDED)]


def _xy(h):
    return int(h[:112], 16), int(h[112:], 16)


def seeded_answers(suite):
    """the fixture's answers of a suite's 128 seeded rows: (x, y) for "ro" and "nu", the 56-byte encodings for decaf"""
    rows = kat()["seeded_" + suite]
    assert len(rows) == SEEDED
    return [bytes.fromhex(h) if suite == "decaf" else _xy(h) for h in rows]


def seeded_pair_answers():
    return [_xy(h) for h in kat()["seeded_pairs"]]


# ---------------------------------------------------------------- hashing in plain Python
def effective_dst(dst, k=224):
    """what the device is given: an oversize DST compressed first (hash-to-curve.ts:263-266)"""
    return hashlib.shake_256(b"H2C-OVERSIZE-DST-" + dst).digest((2 * k + 7) // 8) if len(dst) > 255 else dst


def xof(msg, dst, out_len, k=224):
    """expand_message_xof (RFC 9380 section 5.3.2) with hashlib"""
    dst = effective_dst(dst, k)
    return hashlib.shake_256(msg + out_len.to_bytes(2, "big") + dst + bytes([len(dst)])).digest(out_len)


def hash_to_field(msg, dst, count, modulus=P):
    prb = xof(msg, dst, L * count)
    return [int.from_bytes(prb[L * j:L * j + L], "big") % modulus for j in range(count)]


def hash_to_scalar(msg, dst=SCALAR_DST):
    return hash_to_field(msg, dst, 1, N)[0]


# ---------------------------------------------------------------- big-integer models of the maps
def map_curve448(u):
    """map_to_curve_elligator2_curve448 (RFC 9380 appendix G.2.3 with the reference's signs): (xn, xd, y), the point (xn / xd, y)"""
    u %= P
    tv1 = u * u % P
    e1 = tv1 == 1
    if e1:
        tv1 = 0
    xd = (1 - tv1) % P
    x1n = -J % P
    tv2 = xd * xd % P
    gxd = tv2 * xd % P
    gx1 = ((tv1 * x1n % P * x1n + tv2) * x1n) % P
    tv2 = gx1 * gxd % P
    tv3 = gxd * gxd * tv2 % P
    y1 = pow(tv3, (P - 3) // 4, P) * tv2 % P
    x2n = x1n * (-tv1) % P
    y2 = 0 if e1 else y1 * u % P
    e2 = y1 * y1 * gxd % P == gx1
    xn, y = (x1n, y1) if e2 else (x2n, y2)
    if e2 != (y & 1 == 1):
        y = -y % P
    return xn, xd, y


def map_edwards448(u):
    """map_to_curve_elligator2_edwards448 (appendix G.2.4) with yd = 1: (xEn, xEd, yEn, yEd, took_exception)"""
    xn, xd, yn = map_curve448(u)
    xn2, xd2, yn2 = xn * xn % P, xd * xd % P, yn * yn % P
    xd4 = xd2 * xd2 % P
    xEn = (xn2 - xd2) * xd2 * yn * 4 % P
    tv2 = (xn2 - 2 * xd2) * xn2 % P
    tv3 = 4 * yn2 % P
    xEd = ((tv3 + 1) * xd4 + tv2) % P
    tv2 = tv2 * xn % P
    tv4 = xn * xd4 % P
    yEn = ((tv3 - 1) * tv4 - tv2) % P
    tv1 = -2 * (xn2 + xd2) * xd2 * xd * yn2 % P
    yEd = (tv2 + tv1 + tv4) % P
    if xEd * yEd % P == 0:
        return 0, 1, 1, 1, True
    return xEn, xEd, yEn, yEd, False


def map_edwards448_proj(u):
    """the projective point the lane forms: (xEn yEd : yEn xEd : xEd yEd)"""
    xEn, xEd, yEn, yEd, _ = map_edwards448(u)
    return xEn * yEd % P, yEn * xEd % P, xEd * yEd % P


def map_affine(u):
    xEn, xEd, yEn, yEd, _ = map_edwards448(u)
    return xEn * pow(xEd, P - 2, P) % P, yEn * pow(yEd, P - 2, P) % P


def map_to_curve(us):
    """the hasher tail: the sum of the images of the one or two elements, times the cofactor 4: affine (x, y)"""
    q = map_affine(us[0])
    for u in us[1:]:
        q = eh.pt_add(q, map_affine(u))
    q = eh.pt_add(q, q)
    return eh.pt_add(q, q)


def hash_to_curve(msg, dst, count):
    return map_to_curve(hash_to_field(msg, dst, count))


def decaf_hash_to_group(msg, dst=DECAF_DST):
    return dh.hash_to_curve(msg, dst)


def decaf_hash_to_scalar(msg, dst=SCALAR_DST):
    return dh.hash_to_scalar(msg, dst)


def _sqrt(v):
    v %= P
    r = pow(v, (P + 1) // 4, P)
    return r if r * r % P == v else None


def exception_us():
    """the u whose image has xEd yEd = 0, found with big integers: {name: u}.  Candidates: u = 0, 1, p - 1 (tv1 = 0, so x2 = 0), and
    the roots of the u^2 that put x1 = -J / (1 - u^2) or x2 = -x1 - J on x = 1 or x = -1, where the denominators of the map to
    Edwards form could vanish; a candidate counts only where the model really takes the exceptional branch."""
    cands = {"u0": 0, "u1": 1, "um1": P - 1}
    inv = lambda v: pow(v % P, P - 2, P)  # noqa: E731
    squares = {"x1=1": 1 + J, "x1=-1": 1 - J, "x2=1": inv(1 + J), "x2=-1": inv(1 - J)}
    for name, sq in squares.items():
        r = _sqrt(sq)
        if r is not None:
            cands[name + "+"], cands[name + "-"] = r, (P - r) % P
    return {name: u for name, u in cands.items() if map_edwards448(u)[4]}


# ---------------------------------------------------------------- the host twins (csrc/hosttest.hip ht_h2c448_*)
def _lib():
    lib = hosttest.lib()
    vp, i32, u32, u64, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p
    lib.ht_h2c448_xof.argtypes = [cp, u64, cp, u32, u32, vp]
    lib.ht_h2c448_hash_to_field.argtypes = [cp, u64, cp, u32, i32, vp]
    lib.ht_h2c448_hash_to_scalar.argtypes = [cp, u64, cp, u32, vp]
    lib.ht_h2c448_map.argtypes = [cp, i32, vp]
    lib.ht_h2c448_hash.argtypes = [cp, u64, cp, u32, i32, vp]
    lib.ht_h2c448_decaf_hash_to_group.argtypes = [cp, u64, cp, u32, vp]
    lib.ht_h2c448_decaf_hash_to_scalar.argtypes = [cp, u64, cp, u32, vp]
    lib.ht_h2c448_check.argtypes = [i32, vp, vp]
    return lib


def _ints(out, k):
    b = np.ascontiguousarray(out).tobytes()
    return [int.from_bytes(b[56 * j:56 * j + 56], "little") for j in range(k)]


def ht_xof(msg, dst, out_len):
    out = np.zeros(max(out_len, 1), dtype=np.uint8)
    rc = _lib().ht_h2c448_xof(msg, len(msg), dst, len(dst), out_len, out.ctypes.data)
    return rc, out.tobytes()[:out_len]


def ht_hash_to_field(msg, dst, count):
    out = np.zeros(14 * count, dtype=np.uint32)
    assert _lib().ht_h2c448_hash_to_field(msg, len(msg), dst, len(dst), count, out.ctypes.data) == 0
    return _ints(out, count)


def ht_hash_to_scalar(msg, dst):
    out = np.zeros(14, dtype=np.uint32)
    assert _lib().ht_h2c448_hash_to_scalar(msg, len(msg), dst, len(dst), out.ctypes.data) == 0
    return _ints(out, 1)[0]


def ht_map(us):
    """us: one or two integers below 2^448 -> (x, y)"""
    out = np.zeros(28, dtype=np.uint32)
    raw = b"".join(int(u).to_bytes(56, "little") for u in us)
    assert _lib().ht_h2c448_map(raw, len(us), out.ctypes.data) == 0
    return tuple(_ints(out, 2))


def ht_hash(msg, dst, count):
    out = np.zeros(28, dtype=np.uint32)
    assert _lib().ht_h2c448_hash(msg, len(msg), dst, len(dst), count, out.ctypes.data) == 0
    return tuple(_ints(out, 2))


def ht_decaf_hash_to_group(msg, dst):
    out = np.zeros(14, dtype=np.uint32)
    assert _lib().ht_h2c448_decaf_hash_to_group(msg, len(msg), dst, len(dst), out.ctypes.data) == 0
    return out.tobytes()


def ht_decaf_hash_to_scalar(msg, dst):
    out = np.zeros(14, dtype=np.uint32)
    assert _lib().ht_h2c448_decaf_hash_to_scalar(msg, len(msg), dst, len(dst), out.ctypes.data) == 0
    return _ints(out, 1)[0]


# ---------------------------------------------------------------- ncg_h2c448_check / ht_h2c448_check: rows of 42 words
CHECK_OPS = 5
CHECK_IN_WORDS = (21, 21, 16, 14, 14)
CHECK_OUT_ELEMS = (1, 1, 1, 3, 3)


def check_row(op, value):
    raw = int(value).to_bytes(4 * CHECK_IN_WORDS[op], "little")
    return np.frombuffer(raw + bytes(168 - len(raw)), dtype=np.uint32).copy()


def check_inputs(op):
    """the integers each op is asked about"""
    if op in (0, 1):
        top = 2**672 - 1
        vals = [0, 1, P - 1, P, P + 1, N - 1, N, N + 1, 2**448 - 1, 2**448, 2**448 + 2**224, top, top - 1, (P << 224) - 1, P << 224,
                2**671, 2**224 - 1, 2**224, (2**224 - 1) << 448]
        return vals + [int.from_bytes(seeded_bytes("check%d" % op, i, L), "big") for i in range(24)]
    if op == 2:
        vals = [0, 1, N - 1, N, N + 1, 2**512 - 1, 2**446, 2**446 - 1, N << 66]
        return vals + [int.from_bytes(seeded_bytes("check2", i, 64), "little") for i in range(24)]
    return edge_us() + list(exception_us().values()) + seeded_us()[:24]


def check_expected(op, v):
    """the integers of the output elements"""
    if op == 0:
        return [v % P]
    if op in (1, 2):
        return [v % N]
    return list(map_curve448(v)) if op == 3 else list(map_edwards448_proj(v))


def check_rows(op):
    vals = check_inputs(op)
    return vals, np.stack([check_row(op, v) for v in vals])


def check_out_ints(op, out_row):
    return _ints(np.ascontiguousarray(out_row, dtype=np.uint32)[:14 * CHECK_OUT_ELEMS[op]], CHECK_OUT_ELEMS[op])


def ht_check(op, row):
    """-> (rc, the 42 output words)"""
    out = np.zeros(42, dtype=np.uint32)
    rc = _lib().ht_h2c448_check(op, np.ascontiguousarray(row, dtype=np.uint32).ctypes.data, out.ctypes.data)
    return rc, out


def cycle(rows, n):
    rows = np.ascontiguousarray(rows)
    return np.ascontiguousarray(rows[np.arange(n) % rows.shape[0]])
