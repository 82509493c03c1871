"""Shared by the decaf448 tests: the fixture tests/golden/decaf448_kat.json (the reference's own answers), a plain-Python
restatement on integers of the reference's _DecafPoint and decaf448_hasher (src/ed448.ts:462-701: SQRT_RATIO_M1, decode, encode,
equals, the Elligator map, deriveToCurve, expand_message_xof) - the oracle for cycled rows, itself pinned by the fixture in
test_decaf448_host.py - the raw-limb rows of ncg_decaf448_check / ht_decaf448_op, and the ctypes side of the ht_decaf448* host
twins (csrc/hosttest.hip)."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np

import ed448_helpers as eh
import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
P, N, D, U = eh.P, eh.N, eh.D, eh.U
ONE_MINUS_D, ONE_MINUS_TWO_D = 39082, 78163
SQRT_MINUS_D = pow(39081, (P + 1) // 4, P)
SQRT_MINUS_D = SQRT_MINUS_D if SQRT_MINUS_D % 2 == 0 else P - SQRT_MINUS_D       # the even root (pinned by the fixture)
INVSQRT_MINUS_D = pow(SQRT_MINUS_D, P - 2, P)
BASE = eh.pt_add(eh.BASE, eh.BASE)                                               # twice the Ed448 base
ENC1, ENC2 = "invalid decaf448 encoding 1", "invalid decaf448 encoding 2"
RANGE = "invalid field element: outside of range 0..ORDER"
DEFAULT_DST = b"decaf448_XOF:SHAKE256_D448MAP_RO_"
TORSION = eh.TORSION
_kat = None


def kat():
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "decaf448_kat.json")) as f:
            _kat = json.load(f)
    return _kat


# ---------------------------------------------------------------- the restatement on integers
def uv_ratio(u, v):
    """ed448.ts:135-153: (isValid, value)"""
    u2v = u * u * v % P
    u3v = u2v * u % P
    x = u3v * pow(u3v * u2v * v % P, (P - 3) // 4, P) % P
    return x * x * v % P == u % P, x


def sqrt_ratio_m1(u, v):
    """ed448.ts:462-465: the even one of +-value"""
    ok, x = uv_ratio(u, v)
    return ok, (P - x) % P if x & 1 else x


def _abs(v):
    v %= P
    return P - v if v & 1 else v


def decode(enc):
    """fromBytes (ed448.ts:569-595): (x, y), or the message of the error the reference throws"""
    s = int.from_bytes(enc, "little")
    if s >= P:
        return RANGE
    if s & 1:
        return ENC1
    s2 = s * s % P
    u1 = (1 + s2) % P
    u1sq = u1 * u1 % P
    u2 = (u1sq - 4 * D * s2) % P
    ok, inv = sqrt_ratio_m1(1, u2 * u1sq % P)
    u3 = _abs(2 * s * inv * u1 * SQRT_MINUS_D)
    x = u3 * inv * u2 * INVSQRT_MINUS_D % P
    y = (1 - s2) * inv * u1 % P
    return (x, y) if ok else ENC2


def encode_ext(X, Y, Z, T):
    """toBytes (ed448.ts:610-621) of an extended point"""
    u1 = (X + T) * (X - T) % P
    _, inv = sqrt_ratio_m1(1, u1 * ONE_MINUS_D * X * X % P)
    ratio = _abs(inv * u1 * SQRT_MINUS_D)
    u2 = (INVSQRT_MINUS_D * ratio * Z - T) % P
    return _abs(ONE_MINUS_D * inv * X * u2).to_bytes(56, "little")


def encode(p):
    return encode_ext(p[0], p[1], 1, p[0] * p[1] % P)


def equals(p, q):
    return (p[0] * q[1] - p[1] * q[0]) % P == 0


def elligator(r0):
    """calcElligatorDecafMap (ed448.ts:474-510): (X, Y, Z, T)"""
    r = -r0 * r0 % P
    u0 = D * (r - 1) % P
    u1 = (u0 + 1) * (u0 - r) % P
    sq, v = sqrt_ratio_m1(ONE_MINUS_TWO_D, (r + 1) * u1 % P)
    vp = v if sq else r0 * v % P
    sgn = 1 if sq else P - 1
    s = vp * (r + 1) % P
    s_abs = _abs(s)
    s2 = s * s % P
    w0, w1, w2 = 2 * s_abs % P, (s2 + 1) % P, (s2 - 1) % P
    w3 = (vp * s * (r - 1) * ONE_MINUS_TWO_D + sgn) % P
    return w0 * w3 % P, w2 * w1 % P, w1 * w3 % P, w0 * w2 % P


def derive(uniform):
    """deriveToCurve (ed448.ts:689-700): the affine sum of the two mapped points"""
    pts = []
    for half in (uniform[:56], uniform[56:]):
        X, Y, Z, _ = elligator(int.from_bytes(half, "little") % P)
        zi = pow(Z, P - 2, P)
        pts.append((X * zi % P, Y * zi % P))
    return eh.pt_add(*pts)


def expand_message_xof(msg, dst, length, k):
    if len(dst) > 255:
        dst = hashlib.shake_256(b"H2C-OVERSIZE-DST-" + dst).digest((2 * k + 7) // 8)
    return hashlib.shake_256(msg + length.to_bytes(2, "big") + dst + bytes([len(dst)])).digest(length)


def hash_to_curve(msg, dst=DEFAULT_DST):
    return encode(derive(expand_message_xof(msg, dst, 112, 224)))


def hash_to_scalar(msg, dst=b"HashToScalar-"):
    return int.from_bytes(expand_message_xof(msg, dst, 64, 256), "little") % N


def mul_enc(enc, k):
    """fromBytes(enc).multiplyUnsafe(k).toBytes(): 56 bytes, or None where the encoding is refused"""
    p = decode(enc)
    return None if isinstance(p, str) else encode(eh.pt_mul(p, k))


# ---------------------------------------------------------------- rows (built once by the callers, cycled to n)
rows, cycle, le56, affine_rows = eh.rows, eh.cycle, eh.le56, eh.affine_rows
EDGE_SCALARS = (0, 1, 2, N - 1, N, N + 1, 2**448 - 1)


def hexint(h):
    return int(h, 16)


def multiples():
    """(k, encoding, (x, y)) of the fixture's multiples of BASE"""
    return [(hexint(c["k"]), bytes.fromhex(c["enc"]), (hexint(c["x"]), hexint(c["y"]))) for c in kat()["multiples"]]


def decode_rows():
    """enc [m, 56], the representatives [m, 112] (zero where refused), ok [m]: the fixture's rows with the reference's verdicts"""
    k = kat()["decode"]
    enc = rows([bytes.fromhex(c["enc"]) for c in k], 56)
    aff = rows([bytes(112) if c["error"] else le56(hexint(c["x"])) + le56(hexint(c["y"])) for c in k], 112)
    return enc, aff, np.array([0 if c["error"] else 1 for c in k], np.uint8)


def encode_rows():
    """affine points [m, 112] -> encodings [m, 56]: the fixture's coset rows, the multiples, and their torsion translates (the one by
    (0, -1) keeps the bytes; those by the points of order 4 are answered by the restatement, which the fixture's coset rows pin)"""
    k = kat()
    pts = [(hexint(c["x"]), hexint(c["y"])) for c in k["encode_affine"]]
    want = [bytes.fromhex(c["enc"]) for c in k["encode_affine"]]
    for _, enc, p in multiples():
        pts.append(p)
        want.append(enc)
    for _, enc, p in multiples()[16:20]:
        pts.append(eh.pt_add(p, TORSION[1]))
        want.append(enc)
        for t in TORSION[2:]:
            pts.append(eh.pt_add(p, t))
            want.append(encode(pts[-1]))
    return affine_rows(pts), rows(want, 56)


def equals_rows():
    k = kat()["equals"]
    a = affine_rows([(hexint(c["x1"]), hexint(c["y1"])) for c in k])
    b = affine_rows([(hexint(c["x2"]), hexint(c["y2"])) for c in k])
    return a, b, np.array([1 if c["equal"] else 0 for c in k], np.uint8)


def derive_rows(extra=24):
    """uniform [m, 112] -> encodings [m, 56]: the fixture's rows, then seeded rows answered by the restatement"""
    k = kat()["derive"]
    uni = [bytes.fromhex(c["uniform"]) for c in k]
    want = [bytes.fromhex(c["enc"]) for c in k]
    more = eh.rand_rows(extra, "decaf-derive", 112)
    for r in more:
        uni.append(bytes(r))
        want.append(encode(derive(bytes(r))))
    return rows(uni, 112), rows(want, 56)


def mul_rows():
    """enc [m, 56], k [m, 56], want [m, 56], ok [m]: the fixture's rows, every edge scalar against a few elements (answered by the
    restatement), and refused encodings among them"""
    enc, ks, want = [], [], []
    for c in kat()["mul"]:
        k = hexint(c["k"])
        if c["multiplyUnsafe"]["error"] is None:
            enc.append(bytes.fromhex(c["enc"]))
            ks.append(k)
            want.append(bytes.fromhex(c["multiplyUnsafe"]["out"]))
    m = multiples()
    rng = random.Random("decaf-mul-rows")
    for _, e, _p in (m[0], m[1], m[5], m[17], m[20]):
        for k in EDGE_SCALARS + (rng.getrandbits(448),):
            enc.append(e)
            ks.append(k)
            want.append(mul_enc(e, k))
    for bad in (le56(P), le56(1), bytes.fromhex(kat()["decode"][16 + 14]["enc"])):     # not canonical, odd, a non-square ratio
        enc.append(bad)
        ks.append(5)
        want.append(None)
    ok = np.array([0 if w is None else 1 for w in want], np.uint8)
    return rows(enc, 56), rows([le56(k) for k in ks], 56), rows([w or bytes(56) for w in want], 56), ok


# ---------------------------------------------------------------- the pieces on raw limbs (ncg_decaf448_check / ht_decaf448_op)
DECAF448_OPS = {0: (16, 16, 17), 1: (64, 0, 14), 2: (16, 0, 64)}      # op -> words of (a, b, out); every input element at bound 1


def _limbs(v):
    return eh.value_limbs(v % P)


def _loose(v, rng):
    """the limbs of v mod p, with a unit of limb i + 1 moved down into limb i (as 2^28) where that stays below bound 1: the same
    integer in limbs that are not all below 2^28"""
    limbs = _limbs(v)
    for i in range(15):
        if limbs[i] < (1 << 10) and limbs[i + 1] > 0 and rng.randrange(2):
            limbs[i] += 1 << 28
            limbs[i + 1] -= 1
    return limbs


def check_rows(op, nrandom=40):
    """a [n, wa], b [n, max(wb, 1)]: every limb at the top of bound 1, every limb 0, canonical edge values, and seeded rows.
    op 0: u / v square, non-square, u = 0, v = 0, both 0.  op 1: points of the curve in every projective scale, the small-order
    points, and arbitrary limbs.  op 2: r0 = 0, 1, p - 1 and random values."""
    rng = random.Random("decaf448-op-%d" % op)
    top = [U - 1] * 16
    rnd = lambda: [rng.randrange(U) for _ in range(16)]  # noqa: E731
    a, b = [], []
    if op == 0:
        pairs = [(top, top), ([0] * 16, [0] * 16), (_limbs(1), [0] * 16), ([0] * 16, _limbs(1)), (top, _limbs(1)), (_limbs(1), top)]
        for _ in range(nrandom // 2):
            v, x = rng.randrange(1, P), rng.randrange(1, P)
            pairs.append((_loose(x * x * v, rng), _loose(v, rng)))                 # u / v = x^2: a square
            pairs.append((_loose(x * x * v * (P - 1), rng), _loose(v, rng)))       # -1 is a non-square (p = 3 mod 4)
        pairs += [(rnd(), rnd()) for _ in range(nrandom)]
        a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    elif op == 1:
        a = [top * 4, [0] * 64]
        pts = TORSION + [BASE, eh.BASE] + [m[2] for m in multiples()[2:12]]
        for x, y in pts:
            for z in (1, P - 1, rng.randrange(1, P)):
                a.append(_loose(x * z, rng) + _loose(y * z, rng) + _loose(z, rng) + _loose(x * y * z, rng))
        a += [rnd() + rnd() + rnd() + rnd() for _ in range(nrandom)]
    else:
        a = [top, [0] * 16, _limbs(1), _limbs(P - 1), _limbs(2), eh.value_limbs(P), eh.value_limbs(P + 1)]
        a += [rnd() for _ in range(nrandom)]
    a = np.array(a, np.uint32)
    b = np.array(b, np.uint32) if op == 0 else np.zeros((len(a), 1), np.uint32)
    return a, b


def check_decaf448(op, a, b, out):
    """out against the restatement: values mod p, flags and words bit for bit, every output limb below bound 1"""
    assert out.shape[1] == DECAF448_OPS[op][2]
    el = lambda row, j: eh.limbs_value(row[16 * j:16 * j + 16]) % P  # noqa: E731
    for i in range(a.shape[0]):
        if op == 0:
            ok, x = sqrt_ratio_m1(el(a[i], 0), el(b[i], 0))
            assert int(out[i, :16].max()) < U and el(out[i], 0) == x and int(out[i, 16]) == int(ok), (op, i)
        elif op == 1:
            want = encode_ext(*(el(a[i], j) for j in range(4)))
            assert out[i].astype("<u4").tobytes() == want, (op, i)
        else:
            assert int(out[i].max()) < U
            assert tuple(el(out[i], j) for j in range(4)) == elligator(el(a[i], 0)), (op, i)


# ---------------------------------------------------------------- host twins
_ht = None


def ht():
    global _ht
    if _ht is None:
        lib = hosttest.lib()
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        lib.ht_decaf448_decode.argtypes = [vp, vp, vp, i32]
        lib.ht_decaf448_encode.argtypes = [vp, vp, i32]
        lib.ht_decaf448_encode_proj.argtypes = [vp, vp, i32]
        lib.ht_decaf448_equals.argtypes = [vp, vp, vp, i32]
        lib.ht_decaf448_from_uniform.argtypes = [vp, vp, i32]
        lib.ht_decaf448_mul.argtypes = [vp, vp, i32, vp, vp, i32]
        lib.ht_decaf448_op.argtypes = [i32, vp, vp, vp]
        lib.ht_decaf448_widths.argtypes = [i32, vp, vp, vp]
        lib.ht_decaf448_widths.restype = None
        lib.ht_decaf448_consts.argtypes = [vp]
        lib.ht_decaf448_consts.restype = None
        _ht = lib
    return _ht


def _u8(a, width):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, width)


class TwinEngine(eh.TwinEngine):
    """the decaf448 methods of noble_curves_amd._native.Engine on the CPU twins (and the Ed448 ones of ed448_helpers)"""

    def decaf448_decode_batch(self, enc):
        e = _u8(enc, 56)
        n = e.shape[0]
        out, ok = np.zeros((n, 112), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_decaf448_decode(e.ctypes.data, out.ctypes.data, ok.ctypes.data, n) == 0
        return out, ok.astype(bool)

    def decaf448_encode_batch(self, affine):
        a = _u8(affine, 112)
        out = np.zeros((a.shape[0], 56), np.uint8)
        assert ht().ht_decaf448_encode(a.ctypes.data, out.ctypes.data, a.shape[0]) == 0
        return out

    def decaf448_equals_batch(self, a, b):
        a, b = _u8(a, 112), _u8(b, 112)
        out = np.zeros(a.shape[0], np.uint8)
        assert ht().ht_decaf448_equals(a.ctypes.data, b.ctypes.data, out.ctypes.data, a.shape[0]) == 0
        return out.astype(bool)

    def decaf448_from_uniform_batch(self, bytes112):
        u = _u8(bytes112, 112)
        out = np.zeros((u.shape[0], 56), np.uint8)
        assert ht().ht_decaf448_from_uniform(u.ctypes.data, out.ctypes.data, u.shape[0]) == 0
        return out

    def decaf448_mul_batch(self, enc, ks, one_scalar=False):
        e, k = _u8(enc, 56), _u8(ks, 56)
        n = e.shape[0]
        out, ok = np.zeros((n, 56), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_decaf448_mul(e.ctypes.data, k.ctypes.data, 1 if one_scalar else 0, out.ctypes.data, ok.ctypes.data, n) == 0
        return out, ok.astype(bool)

    def decaf448_mul_base_batch(self, ks):
        k = _u8(ks, 56)
        n = k.shape[0]
        out, ok = np.zeros((n, 56), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_decaf448_mul(None, k.ctypes.data, 0, out.ctypes.data, ok.ctypes.data, n) == 0
        return out


def ht_encode_proj(xyz):
    """X Y Z [n, 168] -> encodings [n, 56]"""
    x = _u8(xyz, 168)
    out = np.zeros((x.shape[0], 56), np.uint8)
    assert ht().ht_decaf448_encode_proj(x.ctypes.data, out.ctypes.data, x.shape[0]) == 0
    return out


def ht_consts():
    out = np.zeros(6 * 56, np.uint8)
    ht().ht_decaf448_consts(out.ctypes.data)
    return [int.from_bytes(out[56 * i:56 * i + 56].tobytes(), "little") for i in range(6)]


def ht_op(op, a, b):
    """rows of ht_decaf448_op -> [n, wo] uint32"""
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    out = np.zeros((a.shape[0], DECAF448_OPS[op][2]), np.uint32)
    for i in range(a.shape[0]):
        assert ht().ht_decaf448_op(op, a[i].ctypes.data, b[i].ctypes.data, out[i].ctypes.data) == 0
    return out
