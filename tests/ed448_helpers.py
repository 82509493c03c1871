"""Shared by the X448 / Ed448 tests: the fixtures tests/golden/ed448_kat.json (the reference's own answers) and
ed448_wycheproof_old.json, a plain-Python restatement on integers of the reference's src/ed448.ts over montgomery.ts / edwards.ts
(ladder, clamp, decode, encode, the Edwards group law, dom4 / challenge, sign for generating rows) - the oracle for random batches,
itself pinned by the fixture - the raw-limb rows of ncg_fe448_check / ht_fe448_op, and the ctypes side of the ht_x448 / ht_ed448*
host twins (csrc/hosttest.hip)."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np

import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
P = 2**448 - 2**224 - 1
N = 2**446 - 13818066809895115352007386748515426880336692474882178609894547503885
D = P - 39081
A24 = 39081
GX = 0x4f1970c66bed0ded221d15a622bf36da9e146570470f1767ea6de324a3d3a46412ae1af72ab66511433b80e18b00938e2626a82bc70cc05e
GY = 0x693f46716eb6bc248876203756c9c7624bea73736ca3984087789c1e05a0c2d73ad3ff1ce67c39c4fdbd132c4ed7c8ad9808795bf230fa14
BASE = (GX, GY)
IDENTITY = (0, 1)
TORSION = [(0, 1), (0, P - 1), (1, 0), (P - 1, 0)]      # orders 1, 2, 4, 4
U = (1 << 28) + (1 << 10)                              # fe448.hpp: a bound-B element has limbs below B * U
LOW_ORDER = (0, 1, P - 1)
INVALID = "invalid private or public key received"
_kat = None


def kat():
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "ed448_kat.json")) as f:
            _kat = json.load(f)
        # the 256 seeded random rows: the fixture keeps the reference's answers, the inputs are rebuilt as make_ed448_kat.py built them
        rng = random.Random("ed448-kat-random")
        for i, out in enumerate(_kat.pop("scalar_mult_random_out")):
            sc, u = (bytes(rng.randrange(256) for _ in range(56)).hex() for _ in range(2))
            _kat["scalar_mult"].append({"name": "random %d" % i, "scalar": sc, "u": u, "out": out, "error": None})
    return _kat


def wycheproof():
    with open(os.path.join(HERE, "golden", "ed448_wycheproof_old.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- X448 on integers
def clamp(scalar):
    b = bytearray(scalar)
    b[0] &= 252
    b[55] |= 128
    return int.from_bytes(b[:56], "little")


def decode_u(u):
    return int.from_bytes(u, "little") % P


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
    for t in range(447, -1, -1):
        x2, z2, x3, z3 = step(u, x2, z2, x3, z3, (kx >> t) & 1)
    if k & 1:
        x2, z2 = x3, z3
    return x2 * pow(z2, P - 2, P) % P


def scalar_mult(scalar, u):
    """x448.scalarMult: 56 bytes, or None where the reference throws"""
    pu = decode_u(u)
    if pu in LOW_ORDER:
        return None
    r = ladder(pu, clamp(scalar))
    return None if r == 0 else r.to_bytes(56, "little")


# ---------------------------------------------------------------- Ed448 on integers (affine, the complete a = 1 law)
def pt_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + t, P - 2, P) % P, (y1 * y2 - x1 * x2) * pow(1 - t, P - 2, P) % P)


def pt_neg(p):
    return ((P - p[0]) % P, p[1])


def pt_mul(p, k):
    """the exact integer multiple, any k >= 0 (projective inside: one inversion)"""
    r, q = (0, 1, 1), (p[0], p[1], 1)
    while k:
        if k & 1:
            r = _proj_add(r, q)
        q = _proj_dbl(q)
        k >>= 1
    zi = pow(r[2], P - 2, P)
    return (r[0] * zi % P, r[1] * zi % P)


def on_curve(p):
    x, y = p
    return (x * x + y * y - 1 - D * x * x * y * y) % P == 0


def pt_encode(p):
    return (p[1] | ((p[0] & 1) << 455)).to_bytes(57, "little")


def pt_decode(enc):
    """Point.fromBytes strict: (x, y), or the message of the error the reference throws"""
    last = enc[56]
    y = int.from_bytes(enc[:56] + bytes([last & 0x7f]), "little")
    if y >= P:
        return "point.y"
    u, v = (y * y - 1) % P, (D * y * y - 1) % P
    u2v = u * u * v % P
    u3v = u2v * u % P
    x = u3v * pow(u3v * u2v * v % P, (P - 3) // 4, P) % P
    if x * x * v % P != u:
        return "bad point: invalid y coordinate"
    if x == 0 and last & 0x80:
        return "bad point: x=0 and x_0=1"
    if (x & 1) != (last >> 7):
        x = (P - x) % P
    return (x, y)


def is_small_order(p):
    return pt_mul(p, 4) == IDENTITY


def dom4(data, ctx=b"", ph=False):
    if len(ctx) > 255:
        raise ValueError("context must be smaller than 255, got: %d" % len(ctx))
    return b"SigEd448" + bytes([1 if ph else 0, len(ctx)]) + ctx + data


def shake114(data):
    return hashlib.shake_256(data).digest(114)


def prehash(msg):
    return hashlib.shake_256(msg).digest(64)


def challenge(r, a, msg, ctx=b"", ph=False):
    """the UNREDUCED challenge as an integer (114 bytes little-endian)"""
    return int.from_bytes(shake114(dom4(r + a + (prehash(msg) if ph else msg), ctx, ph)), "little")


def secret_scalar(seed):
    h = shake114(seed)
    return clamp(h[:56] + b"\0"), h[57:]


def public_key(seed):
    return pt_encode(pt_mul(BASE, secret_scalar(seed)[0] % N))


def to_montgomery_secret(seed):
    """ed448.utils.toMontgomerySecret: the clamped head of the key expansion, 56 bytes"""
    return secret_scalar(seed)[0].to_bytes(56, "little")


def sign(msg, seed, ctx=b"", ph=False):
    s, prefix = secret_scalar(seed)
    a = pt_encode(pt_mul(BASE, s % N))
    m = prehash(msg) if ph else msg
    r = int.from_bytes(shake114(dom4(prefix + m, ctx, ph)), "little") % N
    rb = pt_encode(pt_mul(BASE, r))
    k = challenge(rb, a, msg, ctx, ph) % N
    return rb + ((r + k * s) % N).to_bytes(57, "little")


def verify_k(sig, pk, k, cofactored=True):
    """eddsa.verify strict with the challenge given (any integer)"""
    a, r = pt_decode(pk), pt_decode(sig[:57])
    s = int.from_bytes(sig[57:], "little")
    if isinstance(a, str) or isinstance(r, str) or s >= N:
        return False
    if is_small_order(a):
        return False
    q = pt_add(pt_add(pt_mul(BASE, s), pt_neg(pt_mul(a, k))), pt_neg(r))
    return (pt_mul(q, 4) if cofactored else q) == IDENTITY


def verify(sig, msg, pk, ctx=b"", ph=False):
    return verify_k(sig, pk, challenge(sig[:57], pk, msg, ctx, ph) % N)


def to_montgomery(pk):
    p = pt_decode(pk)
    if isinstance(p, str) or p[0] == 0:
        return None
    return (p[1] * p[1] * pow(p[0] * p[0], P - 2, P) % P).to_bytes(56, "little")


# ---------------------------------------------------------------- rows
def rand_rows(n, seed, width=56):
    rng = random.Random("ed448-%s-%d" % (seed, n))
    return np.frombuffer(bytes(rng.getrandbits(8) for _ in range(n * width)), np.uint8).reshape(n, width).copy()


def rows(items, width):
    """list of bytes -> uint8 [n, width]"""
    return np.frombuffer(b"".join(bytes(b) for b in items), np.uint8).reshape(len(items), width).copy()


def hex_rows(items, width=56):
    return rows([bytes.fromhex(h) for h in items], width)


def le56(v):
    return int(v).to_bytes(56, "little")


def cycle(a, n):
    """the rows of a repeated to n rows"""
    return np.ascontiguousarray(np.resize(a, (n,) + a.shape[1:]))


def expect_x448(scalars, us):
    n = len(us)
    out, ok = np.zeros((n, 56), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        r = scalar_mult(bytes(scalars[i if len(scalars) == n else 0]), bytes(us[i]))
        if r is not None:
            out[i], ok[i] = np.frombuffer(r, np.uint8), 1
    return out, ok


def kat_expected(items, width=56):
    out, ok = np.zeros((len(items), width), np.uint8), np.zeros(len(items), np.uint8)
    for i, c in enumerate(items):
        if c["out"] is not None:
            out[i], ok[i] = np.frombuffer(bytes.fromhex(c["out"]), np.uint8), 1
    return out, ok


def affine_rows(pts):
    return rows([le56(x) + le56(y) for x, y in pts], 112)


def edge_points():
    """the identity, the torsion points, the base point and a few multiples"""
    return TORSION + [BASE, pt_neg(BASE), pt_mul(BASE, 2), pt_mul(BASE, N - 1), pt_add(BASE, TORSION[2]), pt_add(pt_mul(BASE, 7), TORSION[1])]


EDGE_SCALARS = (0, 1, 2, N - 1, N, N + 1, 2**448 - 1)


def decode_edge_rows():
    """encodings the decoder must refuse or accept at the edges, with the restatement's verdict"""
    y_off = next(y for y in range(2, 100) if isinstance(pt_decode(y.to_bytes(57, "little")), str))
    enc = [(P).to_bytes(57, "little"), (P + 1).to_bytes(57, "little"), (2**448 - 1).to_bytes(57, "little")]
    g = pt_encode(BASE)
    enc += [g[:56] + bytes([g[56] | b]) for b in (0x01, 0x40)] + [g[:56] + b"\x81"]
    enc += [(1 | 1 << 455).to_bytes(57, "little"), ((P - 1) | 1 << 455).to_bytes(57, "little"), y_off.to_bytes(57, "little")]
    enc += [pt_encode(p) for p in edge_points()]
    return enc


# ---------------------------------------------------------------- verification rows
_sigs = None


def signatures(count=40):
    """(sig, msg, pk, ctx, ph) made by the restatement: seeded keys, messages of several lengths, with and without context / prehash"""
    global _sigs
    if _sigs is None:
        rng = random.Random("ed448-sigs")
        _sigs = []
        for i in range(count):
            seed = bytes(rng.getrandbits(8) for _ in range(57))
            msg = bytes(rng.getrandbits(8) for _ in range(i % 7 * 5))
            ctx = b"" if i % 3 else b"ctx-%d" % i
            ph = i % 5 == 4
            _sigs.append((sign(msg, seed, ctx, ph), msg, public_key(seed), ctx, ph))
    return _sigs


def flip(b, byte, bit=0):
    return b[:byte] + bytes([b[byte] ^ (1 << bit)]) + b[byte + 1:]


_vrows = None


def verify_rows():
    """(sig114, pk57, k integer, want) rows covering the accept / reject rules; want comes from the restatement, and the rows that
    must discriminate the cofactored equation are asserted to do so here.  Computed once."""
    global _vrows
    if _vrows is None:
        _vrows = _verify_rows()
    return _vrows


def _verify_rows():
    out = []
    for sig, msg, pk, ctx, ph in signatures():
        out.append((sig, pk, challenge(sig[:57], pk, msg, ctx, ph) % N, True))
    sig, msg, pk, ctx, ph = signatures()[1]
    k = challenge(sig[:57], pk, msg, ctx, ph)
    s0 = int.from_bytes(sig[57:], "little")
    out.append((sig, pk, k % N + N, True))                             # k >= n unreduced, up to the top of the 448 bits
    out.append((sig, pk, k % N + 3 * N, True))
    for bad in (flip(sig, 3), flip(sig, 60), flip(sig, 112, 7)):       # R, s, s byte 55
        out.append((bad, pk, k % N, False))
    out.append((sig, flip(pk, 5), k % N, False))
    out.append((sig, pk, challenge(sig[:57], pk, msg + b"!", ctx, ph) % N, False))
    out.append((sig[:57] + N.to_bytes(57, "little"), pk, k % N, False))                 # s = n
    out.append((sig[:57] + (s0 + N).to_bytes(57, "little"), pk, k % N, False))          # s = s0 + n
    out.append((sig[:113] + b"\x01", pk, k % N, False))                                 # byte 56 of s
    # small-order A with R = [s]B: the equation holds, the row is refused
    for t in TORSION:
        out.append((pt_encode(pt_mul(BASE, 5)) + (5).to_bytes(57, "little"), pt_encode(t), 4, False))
    # R' = R + T with s computed for R': accepted by the cofactored equation only
    seed = b"\x42" * 57
    a, prefix = secret_scalar(seed)
    apk = public_key(seed)
    for t in TORSION[1:]:
        r = 0x1234567 + len(out)
        rb = pt_encode(pt_add(pt_mul(BASE, r), t))
        kk = challenge(rb, apk, b"torsion") % N
        row = rb + ((r + kk * a) % N).to_bytes(57, "little")
        assert verify_k(row, apk, kk) and not verify_k(row, apk, kk, cofactored=False)
        out.append((row, apk, kk, True))
    # k = 0: [s]B = R
    out.append((pt_encode(pt_mul(BASE, 77)) + (77).to_bytes(57, "little"), apk, 0, True))
    out.append((pt_encode(pt_mul(BASE, 77)) + (78).to_bytes(57, "little"), apk, 0, False))
    # non-canonical A and R: only y below 2^224 + 1 has a second encoding y + p in 448 bits; y = p stands for y = 0 (an order-4
    # point) and must be refused as R and as A
    nc = (P).to_bytes(57, "little")
    out.append((nc + (0).to_bytes(57, "little"), apk, 0, False))
    out.append((sig, nc, k % N, False))
    for row in out:
        assert verify_k(row[0], row[1], row[2]) == row[3], "the restatement disagrees with the intended verdict"
    return out


def verify_arrays(n):
    """the rows cycled to n: sig [n, 114], pk [n, 57], k [n, 56], want [n]"""
    r = verify_rows()
    sig, pk = rows([x[0] for x in r], 114), rows([x[1] for x in r], 57)
    k, want = rows([le56(x[2]) for x in r], 56), np.array([x[3] for x in r], np.uint8)
    return cycle(sig, n), cycle(pk, n), cycle(k, n), cycle(want, n)


# ---------------------------------------------------------------- the pieces on raw limbs (ncg_fe448_check / ht_fe448_op)
# op -> (words of a, b, out, input bound of a, of b)
FE448_OPS = {0: (16, 16, 16, 3, 2), 1: (16, 0, 16, 2, 0), 2: (16, 16, 48, 1, 1), 3: (16, 16, 16, 3, 2), 4: (16, 0, 14, 8, 0),
             5: (14, 0, 16, 0, 0), 6: (16, 0, 16, 1, 0), 7: (16, 0, 16, 1, 0), 8: (64, 16, 64, 1, 1), 9: (48, 48, 48, 1, 1),
             10: (48, 0, 48, 1, 0)}


def limbs_value(limbs):
    return sum(int(v) << (28 * i) for i, v in enumerate(limbs))


def value_limbs(v):
    return [(v >> (28 * i)) & ((1 << 28) - 1) for i in range(16)]


def fe448_rows(op, nrandom=256):
    """a [n, wa], b [n, max(wb, 1)]: every limb at the top of the declared bound, every limb 0, each element in turn at the top
    with the others random, the edge values (store and load), and seeded random rows"""
    wa, wb, _, ba, bb = FE448_OPS[op]
    rng = random.Random("fe448-op-%d" % op)
    if op == 5:                                                   # words of any 448-bit value
        vals = [0, 1, P - 1, P, P + 1, 2**224, 2**448 - 1] + [rng.getrandbits(448) for _ in range(nrandom)]
        a = np.array([[(v >> (32 * i)) & 0xffffffff for i in range(14)] for v in vals], np.uint32)
        return a, np.zeros((len(vals), 1), np.uint32)
    ta, tb = ba * U - 1, bb * U - 1
    ea, eb = wa // 16, wb // 16
    out = [([ta] * wa, [tb] * wb), ([0] * wa, [0] * wb)]
    for e in range(ea + eb):
        ra, rb = [rng.randrange(ta + 1) for _ in range(wa)], [rng.randrange(tb + 1) for _ in range(wb)]
        if e < ea:
            ra[16 * e:16 * e + 16] = [ta] * 16
        else:
            rb[16 * (e - ea):16 * (e - ea) + 16] = [tb] * 16
        out.append((ra, rb))
    if op == 4:
        for v in (0, 1, P - 1, P, P + 1, 2**224, 2**448 - 1):
            out.append((value_limbs(v), []))
    for _ in range(nrandom):
        out.append(([rng.randrange(ta + 1) for _ in range(wa)], [rng.randrange(tb + 1) for _ in range(wb)]))
    a = np.array([r[0] for r in out], np.uint32)
    b = np.array([r[1] for r in out], np.uint32) if wb else np.zeros((len(out), 1), np.uint32)
    return a, b


def _els(row, count):
    return [limbs_value(row[16 * j:16 * j + 16]) for j in range(count)]


def _proj_add(p, q):
    """add-2007-bl on integers, for projective operands that are not points (the raw-limb rows are random values)"""
    (x1, y1, z1), (x2, y2, z2) = p, q
    a = z1 * z2
    b, c, d = a * a, x1 * x2, y1 * y2
    e = D * c * d
    f, g = b - e, b + e
    return a * f * ((x1 + y1) * (x2 + y2) - c - d) % P, a * g * (d - c) % P, f * g % P


def _proj_dbl(p):
    x, y, z = p
    b, c, d = (x + y) ** 2, x * x, y * y
    f = c + d
    j = f - 2 * z * z
    return (b - c - d) * j % P, f * (c - d) % P, f * j % P


def check_fe448(op, variant, a, b, out):
    """out against the restatement: the values mod p, and every output limb below its declared bound"""
    wo = FE448_OPS[op][2]
    assert out.shape[1] == wo
    if op == 4:
        for i in range(a.shape[0]):
            want = limbs_value(a[i]) % P
            assert out[i].astype("<u4").tobytes() == want.to_bytes(56, "little"), (op, i)
        return
    bounds = {2: [2, 3, 1]}.get(op, [1] * (wo // 16))
    for j, bd in enumerate(bounds):
        assert int(out[:, 16 * j:16 * j + 16].max()) < bd * U, "op %d: an output limb at or above its declared bound" % op
    for i in range(a.shape[0]):
        got = tuple(v % P for v in _els(out[i], wo // 16))
        if op == 5:
            v = sum(int(w) << (32 * k) for k, w in enumerate(a[i]))
            assert limbs_value(out[i]) == v, (op, i)               # the load is exact, not merely congruent
            continue
        x = _els(a[i], a.shape[1] // 16)
        y = _els(b[i], b.shape[1] // 16)
        if op == 0:
            want = (x[0] * y[0] % P,)
        elif op == 1:
            want = (x[0] * x[0] % P,)
        elif op == 2:
            want = ((x[0] + y[0]) % P, (x[0] - y[0]) % P, -x[0] % P)
        elif op == 3:
            want = ((x[0] + A24 * y[0]) % P,)
        elif op == 6:
            want = (pow(x[0], (P - 3) // 4, P),)
        elif op == 7:
            want = (pow(x[0], P - 2, P),)
        elif op == 8:
            want = step(y[0], x[0], x[1], x[2], x[3], variant & 1)
        elif op == 9:
            want = _proj_add(tuple(x), tuple(y))
        else:
            want = _proj_dbl(tuple(x))
        assert got == tuple(w % P for w in want), (op, variant, i)


# ---------------------------------------------------------------- host twins
_ht = None


def ht():
    global _ht
    if _ht is None:
        lib = hosttest.lib()
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        lib.ht_x448.argtypes = [vp, vp, i32, vp, vp, i32]
        lib.ht_ed448_decode.argtypes = [vp, vp, vp, i32]
        lib.ht_ed448_encode.argtypes = [vp, vp, i32]
        lib.ht_ed448_add_pairs.argtypes = [vp, vp, i32, vp, i32]
        lib.ht_ed448_mul.argtypes = [vp, vp, i32, vp, vp, i32]
        lib.ht_ed448_to_montgomery.argtypes = [vp, vp, vp, i32]
        lib.ht_ed448_verify.argtypes = [vp, vp, vp, vp, i32]
        lib.ht_fe448_op.argtypes = [i32, i32, vp, vp, vp]
        lib.ht_fe448_widths.argtypes = [i32, vp, vp, vp]
        lib.ht_fe448_widths.restype = None
        _ht = lib
    return _ht


def _u8(a, width):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, width)


class TwinEngine:
    """the Ed448 / X448 methods of noble_curves_amd._native.Engine on the CPU twins"""

    def x448_batch(self, scalars, us, one_scalar=False):
        s, u = _u8(scalars, 56), _u8(us, 56)
        n = u.shape[0]
        out, ok = np.zeros((n, 56), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_x448(s.ctypes.data, u.ctypes.data, 1 if one_scalar else 0, out.ctypes.data, ok.ctypes.data, n) == 0
        return out, ok.astype(bool)

    def x448_base_batch(self, scalars):
        s = _u8(scalars, 56)
        n = s.shape[0]
        out, ok = np.zeros((n, 56), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_x448(s.ctypes.data, None, 0, out.ctypes.data, ok.ctypes.data, n) == 0
        return out, ok.astype(bool)

    def ed448_decode_batch(self, enc):
        e = _u8(enc, 57)
        n = e.shape[0]
        out, ok = np.zeros((n, 112), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_ed448_decode(e.ctypes.data, out.ctypes.data, ok.ctypes.data, n) == 0
        return out, ok.astype(bool)

    def ed448_encode_batch(self, affine):
        a = _u8(affine, 112)
        out = np.zeros((a.shape[0], 57), np.uint8)
        assert ht().ht_ed448_encode(a.ctypes.data, out.ctypes.data, a.shape[0]) == 0
        return out

    def ed448_add_pairs_batch(self, a, b, subtract=False):
        a, b = _u8(a, 112), _u8(b, 112)
        out = np.zeros((a.shape[0], 112), np.uint8)
        assert ht().ht_ed448_add_pairs(a.ctypes.data, b.ctypes.data, 1 if subtract else 0, out.ctypes.data, a.shape[0]) == 0
        return out

    def ed448_mul_batch(self, enc, ks, one_scalar=False):
        e, k = _u8(enc, 57), _u8(ks, 56)
        n = e.shape[0]
        out, ok = np.zeros((n, 57), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_ed448_mul(e.ctypes.data, k.ctypes.data, 1 if one_scalar else 0, out.ctypes.data, ok.ctypes.data, n) == 0
        return out, ok.astype(bool)

    def ed448_mul_base_batch(self, ks):
        k = _u8(ks, 56)
        n = k.shape[0]
        out, ok = np.zeros((n, 57), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_ed448_mul(None, k.ctypes.data, 0, out.ctypes.data, ok.ctypes.data, n) == 0
        return out

    def ed448_to_montgomery_batch(self, pks):
        p = _u8(pks, 57)
        n = p.shape[0]
        out, ok = np.zeros((n, 56), np.uint8), np.zeros(n, np.uint8)
        assert ht().ht_ed448_to_montgomery(p.ctypes.data, out.ctypes.data, ok.ctypes.data, n) == 0
        return out, ok.astype(bool)

    def ed448_verify_batch(self, sigs, pks, ks):
        s, p, k = _u8(sigs, 114), _u8(pks, 57), _u8(ks, 56)
        n = s.shape[0]
        ok = np.zeros(n, np.uint8)
        assert ht().ht_ed448_verify(s.ctypes.data, p.ctypes.data, k.ctypes.data, ok.ctypes.data, n) == 0
        return ok.astype(bool)


def ht_op(op, variant, a, b):
    """rows of ht_fe448_op -> [n, wo] uint32"""
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    out = np.zeros((a.shape[0], FE448_OPS[op][2]), np.uint32)
    for i in range(a.shape[0]):
        assert ht().ht_fe448_op(op, variant, a[i].ctypes.data, b[i].ctypes.data, out[i].ctypes.data) == 0
    return out
