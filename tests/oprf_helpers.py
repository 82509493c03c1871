"""Shared by the OPRF tests: the fixture tests/golden/ristretto255_oprf_kat.json (the reference's own answers), a plain-Python
OPRF / VOPRF / POPRF of RFC 9497 for ristretto255-SHA512 on the integers of ristretto_helpers (decode, encode, mul,
expand_message_xmd) - the oracle for seeded rows, itself checked against the fixture and the RFC's vectors - and the ctypes side of
the ht_oprf_* host twins (csrc/hosttest.hip)."""
import ctypes
import hashlib
import json
import os

import numpy as np

import hosttest
import ristretto_helpers as rh

HERE = os.path.dirname(os.path.abspath(__file__))
L = rh.L
NAME = b"ristretto255-SHA512"
OK, BAD_ENCODING, IDENTITY, BAD_SCALAR = 0, 1, 2, 3
ONE_SCALAR, INVERT = 1, 2
_kat = None


def kat():
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "ristretto255_oprf_kat.json")) as f:
            _kat = json.load(f)
    return _kat


def seeded_bytes(tag, i, n):
    """n bytes of row i of the family `tag`: SHA-512 in counter mode over a fixed label (the generator and the tests share it)"""
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(b"ristretto255-oprf-kat/%s/%d/%d" % (tag.encode(), i, c)).digest()
        c += 1
    return out[:n]


INPUT_LENGTHS = (0, 1, 67, 68, 84, 200, 1000)
XMD_OUT_LENS = (1, 32, 64, 65, 128, 256)


def seeded_inputs():
    return [b"\x00", b"\x5a" * 17] + [seeded_bytes("input", n, n) for n in INPUT_LENGTHS]


def seeded_scalar_msg(i):
    return seeded_bytes("h2s", i, 29 * i % 150)


def seeded_xmd_row(i):
    """(msg, dst, out_len) of the i-th xmd row"""
    return seeded_bytes("xmd", i, 41 * i % 300), b"xmd-DST-%d" % (i % 5) + b"y" * (i % 40), XMD_OUT_LENS[i % len(XMD_OUT_LENS)]


# ---------------------------------------------------------------- the protocol on integers
def ctx_of(mode):
    return b"OPRFV1-" + bytes([mode]) + b"-" + NAME


def i2osp(v, n):
    return int(v).to_bytes(n, "big")


def encode_args(*args):
    """encode() of oprf.ts:476: a number is I2OSP(., 2), a str its ASCII bytes, bytes are length-prefixed"""
    out = b""
    for a in args:
        if isinstance(a, int):
            out += i2osp(a, 2)
        elif isinstance(a, str):
            out += a.encode()
        else:
            out += i2osp(len(a), 2) + bytes(a)
    return out


def le32(v):
    return int(v).to_bytes(32, "little")


def hash_to_scalar(msg, dst):
    return int.from_bytes(rh.expand_message_xmd(msg, dst, 64), "little") % L


def hash_to_scalar_ctx(msg, mode):
    return hash_to_scalar(msg, b"HashToScalar-" + ctx_of(mode))


def hash_to_group(msg, mode):
    """the affine representative of hashToGroup(msg, ctx)"""
    return rh.to_affine(rh.derive(rh.expand_message_xmd(msg, b"HashToGroup-" + ctx_of(mode), 64)))


def random_scalar(rng48):
    """mapHashToField on the 48 bytes an rng gave, little-endian: in 1..L-1"""
    assert len(rng48) == 48
    return int.from_bytes(rng48, "little") % (L - 1) + 1


def wire_point(b):
    """(status, affine point) of a received element"""
    if bytes(b) == bytes(32):
        return IDENTITY, None
    d = rh.decode(bytes(b))
    return (BAD_ENCODING, None) if isinstance(d, str) else (OK, d)


def scalar_of(b):
    k = int.from_bytes(bytes(b), "little")
    return k if 0 < k < L else None


def derive_key_pair(mode, seed, info):
    dst = b"DeriveKeyPair" + ctx_of(mode)
    for counter in range(256):
        sk = hash_to_scalar(seed + encode_args(info) + bytes([counter]), dst)
        if sk:
            return le32(sk), rh.encode(rh.mul(rh.BASE, sk))
    raise AssertionError("Cannot derive key")


def blind(mode, inp, blind_int):
    return rh.encode(rh.mul(hash_to_group(inp, mode), blind_int))


def mul_row(element, scalar, invert=False):
    """(status, 32 bytes) of one row of the multiply: the element is looked at first, then the scalar"""
    st, pt = wire_point(element)
    if st:
        return st, bytes(32)
    k = scalar_of(scalar)
    if k is None:
        return BAD_SCALAR, bytes(32)
    return OK, rh.encode(rh.mul(pt, pow(k, -1, L) if invert else k))


def finalize_hash(inp, element, info=None):
    parts = [inp] + ([info] if info is not None else []) + [element, "Finalize"]
    return hashlib.sha512(encode_args(*parts)).digest()


def finalize(mode, inp, blind_b, evaluated, info=None):
    st, un = mul_row(evaluated, blind_b, True)
    return (st, bytes(64)) if st else (OK, finalize_hash(inp, un, info if mode == 2 else None))


def evaluate(mode, inp, scalar, invert=False, info=None):
    k = scalar_of(scalar)
    if k is None:
        return BAD_SCALAR, bytes(64)
    un = rh.encode(rh.mul(hash_to_group(inp, mode), pow(k, -1, L) if invert else k))
    return OK, finalize_hash(inp, un, info if mode == 2 else None)


def poprf_m(info):
    return hash_to_scalar_ctx(encode_args("Info", info), 2)


def composite_scalars(mode, B, C, D):
    c = ctx_of(mode)
    seed = hashlib.sha512(encode_args(B, b"Seed-" + c)).digest()
    return [hash_to_scalar_ctx(encode_args(seed, i, Ci, Di, "Composite"), mode) for i, (Ci, Di) in enumerate(zip(C, D))]


def msm(encs, ks):
    acc = (0, 1, 1, 0)
    for e, k in zip(encs, ks):
        pt = rh.mul(rh.decode(bytes(e)), k)
        acc = rh.ext_add(acc, (pt[0], pt[1], 1, pt[0] * pt[1] % rh.P))
    return rh.to_affine(acc)


def challenge(mode, B, M, Z, t2, t3):
    return hash_to_scalar_ctx(encode_args(B, M, Z, t2, t3, "Challenge"), mode)


def generate_proof(mode, k, B, C, D, r):
    M = msm(C, composite_scalars(mode, B, C, D))
    Z, t2, t3 = rh.mul(M, k), rh.mul(rh.BASE, r), rh.mul(M, r)
    c = challenge(mode, B, *[rh.encode(p) for p in (M, Z, t2, t3)])
    return le32(c) + le32((r - c * k) % L)


def verify_proof(mode, B, C, D, proof):
    d = composite_scalars(mode, B, C, D)
    M, Z = msm(C, d), msm(D, d)
    c, s = int.from_bytes(proof[:32], "little"), int.from_bytes(proof[32:], "little")
    if c >= L or s >= L:
        return False
    Me, Ze = rh.encode(M), rh.encode(Z)
    t2 = msm([rh.encode(rh.BASE), B], [s, c])
    t3 = msm([Me, Ze], [s, c])
    return challenge(mode, B, Me, Ze, rh.encode(t2), rh.encode(t3)) == c


# ---------------------------------------------------------------- rows for the multiply and the scalar tests
def edge_scalars():
    rng = np.random.RandomState(9497)
    seeded = [int.from_bytes(rng.bytes(32), "little") % (L - 1) + 1 for _ in range(64)]
    return [1, 2, 3, L - 1, 2**252, 2**252 - 1, int("55" * 31, 16) | 1 << 250, int("aa" * 31, 16)] + seeded


def blob(msgs):
    """(bytes, uint64 offsets [n + 1]) of a list of messages"""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return b"".join(msgs), off


# ---------------------------------------------------------------- host twins
_ht = None


def ht():
    global _ht
    if _ht is None:
        lib = hosttest.lib()
        vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
        lib.ht_oprf_xmd.argtypes = [vp, u64, vp, u32, u32, vp]
        lib.ht_oprf_hash_to_group.argtypes = [vp, u64, vp, u32, vp, vp]
        lib.ht_oprf_hash_to_scalar.argtypes = [vp, u64, vp, u32, vp]
        lib.ht_oprf_blind.argtypes = [i32, vp, u64, vp, vp]
        lib.ht_oprf_mul.argtypes = [vp, vp, i32, vp]
        lib.ht_oprf_finalize.argtypes = [i32, vp, u64, vp, u32, vp, vp, vp]
        lib.ht_oprf_evaluate.argtypes = [i32, vp, u64, vp, u32, vp, i32, vp]
        lib.ht_oprf_composite.argtypes = [i32, vp, vp, vp, vp, vp, i32]
        lib.ht_oprf_challenge.argtypes = [i32, vp, vp]
        lib.ht_oprf_proof.argtypes = [i32, vp, vp, vp, vp, vp]
        lib.ht_oprf_check.argtypes = [i32, i32, vp, vp, vp]
        _ht = lib
    return _ht


def _buf(b, pad=4):
    """bytes -> a 4-byte aligned uint8 array (never empty, so that .ctypes.data is a real address)"""
    a = np.zeros(max(len(b), 1) + pad, np.uint8)
    a[:len(b)] = np.frombuffer(bytes(b), np.uint8)
    return a


def ht_xmd(msg, dst, out_len):
    m, d, out = _buf(msg), _buf(dst), np.zeros(out_len, np.uint8)
    assert ht().ht_oprf_xmd(m.ctypes.data, len(msg), d.ctypes.data, len(dst), out_len, out.ctypes.data) == 0
    return out.tobytes()


def ht_hash_to_group(msg, dst, affine=False):
    m, d, out, aff = _buf(msg), _buf(dst), np.zeros(32, np.uint8), np.zeros(64, np.uint8)
    assert ht().ht_oprf_hash_to_group(m.ctypes.data, len(msg), d.ctypes.data, len(dst), out.ctypes.data, aff.ctypes.data if affine else None) == 0
    return (out.tobytes(), aff.tobytes()) if affine else out.tobytes()


def ht_hash_to_scalar(msg, dst):
    m, d, out = _buf(msg), _buf(dst), np.zeros(32, np.uint8)
    assert ht().ht_oprf_hash_to_scalar(m.ctypes.data, len(msg), d.ctypes.data, len(dst), out.ctypes.data) == 0
    return out.tobytes()


def ht_blind(mode, inp, blind32):
    m, b, out = _buf(inp), _buf(blind32), np.zeros(32, np.uint8)
    st = ht().ht_oprf_blind(mode, m.ctypes.data, len(inp), b.ctypes.data, out.ctypes.data)
    return st, out.tobytes()


def ht_mul(element, scalar, flags=0):
    e, k, out = _buf(element), _buf(scalar), np.zeros(32, np.uint8)
    st = ht().ht_oprf_mul(e.ctypes.data, k.ctypes.data, flags, out.ctypes.data)
    return st, out.tobytes()


def ht_finalize(mode, inp, blind32, evaluated, info=None):
    m, b, e, out = _buf(inp), _buf(blind32), _buf(evaluated), np.zeros(64, np.uint8)
    i = _buf(info or b"")
    st = ht().ht_oprf_finalize(mode, m.ctypes.data, len(inp), i.ctypes.data if info is not None else None, len(info or b""), b.ctypes.data,
                               e.ctypes.data, out.ctypes.data)
    return st, out.tobytes()


def ht_evaluate(mode, inp, scalar, flags=0, info=None):
    m, k, out = _buf(inp), _buf(scalar), np.zeros(64, np.uint8)
    i = _buf(info or b"")
    st = ht().ht_oprf_evaluate(mode, m.ctypes.data, len(inp), i.ctypes.data if info is not None else None, len(info or b""), k.ctypes.data, flags,
                               out.ctypes.data)
    return st, out.tobytes()


def ht_composite(mode, B, C, D):
    n = len(C)
    b, c, d = _buf(B), _buf(b"".join(C)), _buf(b"".join(D))
    out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert ht().ht_oprf_composite(mode, b.ctypes.data, c.ctypes.data, d.ctypes.data, out.ctypes.data, st.ctypes.data, n) == 0
    return [bytes(r) for r in out], list(st)


def ht_challenge(mode, five):
    p, out = _buf(b"".join(five)), np.zeros(32, np.uint8)
    assert ht().ht_oprf_challenge(mode, p.ctypes.data, out.ctypes.data) == 0
    return out.tobytes()


def ht_proof(mode, k32, B, M, r32):
    k, b, m, r, out = _buf(k32), _buf(B), _buf(M), _buf(r32), np.zeros(64, np.uint8)
    rc = ht().ht_oprf_proof(mode, k.ctypes.data, b.ctypes.data, m.ctypes.data, r.ctypes.data, out.ctypes.data)
    return rc, out.tobytes()


CHECK_WORDS = {0: (8, 8, 8), 1: (8, 8, 8), 2: (16, 8, 8), 3: (8, 8, 16), 4: (8, 8, 8), 5: (8, 8, 8)}


def ht_check(op, variant, a, b):
    """a [n, 4 wa] and b [n, 32] uint8 rows -> out [n, 4 wo] uint8"""
    wa, wb, wo = CHECK_WORDS[op]
    a, b = np.ascontiguousarray(a, np.uint8).reshape(-1, 4 * wa), np.ascontiguousarray(b, np.uint8).reshape(-1, 4 * wb)
    out = np.zeros((a.shape[0], 4 * wo), np.uint8)
    for i in range(a.shape[0]):
        assert ht().ht_oprf_check(op, variant, a[i].ctypes.data, b[i].ctypes.data, out[i].ctypes.data) == 0
    return out
