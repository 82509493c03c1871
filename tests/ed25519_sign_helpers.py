"""Shared by the Ed25519 signing tests: a plain-Python signer (hashlib + the oracle's curve) that restates RFC 8032 5.1.5 / 5.1.6 with
the dom2 prefix of ed25519ctx / ed25519ph, the message lengths on both sides of every SHA-512 block edge, the fixture
(tests/golden/ed25519_sign_kat.json, written by make_ed25519_sign_kat.py from the reference's own answers) and the bindings of the
CPU twins of csrc/ed25519_sign.hip."""
import ctypes
import functools
import hashlib
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = 2**252 + 27742317777372353535851937790883648493
DOM_PREFIX = b"SigEd25519 no Ed25519 collisions"
EXPANDED, ONE_KEY, PREHASH = 1, 2, 4
DOM_MAX = 289


# ---- message lengths.  A SHA-512 input of `total` bytes takes one block more from total % 128 == 112 on (0x80 and the 16 length
# bytes no longer fit), so the edges are total = 111 | 112 (mod 128).  The nonce hash sees dom || prefix (32) || M, the challenge
# hash dom || R || A (64) || M.
def edge_lengths(dom_len, longest=300):
    out = set()
    for fixed in (dom_len + 32, dom_len + 64):
        for total in range(111, fixed + longest + 1, 128):
            out |= {n for n in (total - fixed, total + 1 - fixed) if 0 <= n <= longest}
    return sorted(out)


def dom2(context, prehash):
    """ed25519_domain (src/ed25519.ts:148-160); plain ed25519 has no prefix at all (context None, prehash False)"""
    if context is None and not prehash:
        return b""
    context = context or b""
    assert len(context) <= 255
    return DOM_PREFIX + bytes([1 if prehash else 0, len(context)]) + context


# ---- the signer
@functools.lru_cache(maxsize=None)
def expand(seed):
    """scalar (int), prefix, public key of a 32-byte seed"""
    from oracle.curves import Ed25519
    h = hashlib.sha512(seed).digest()
    head = bytearray(h[:32])
    head[0] &= 248
    head[31] = (head[31] & 127) | 64
    scalar = int.from_bytes(head, "little") % L
    return scalar, h[32:], Ed25519.BASE.multiply(scalar).toBytes()


def expanded_row(seed):
    scalar, prefix, pk = expand(seed)
    return scalar.to_bytes(32, "little") + prefix + pk


def sign(msg, seed, context=None, prehash=False, r=None):
    """R || S, or None where r = 0 (mod L) (the reference's BASE.multiply(0) throws)"""
    from oracle.curves import Ed25519
    scalar, prefix, pk = expand(bytes(seed))
    dom = dom2(context, prehash)
    m = hashlib.sha512(msg).digest() if prehash else bytes(msg)
    if r is None:
        r = int.from_bytes(hashlib.sha512(dom + prefix + m).digest(), "little") % L
    if r % L == 0:
        return None
    R = Ed25519.BASE.multiply(r).toBytes()
    k = int.from_bytes(hashlib.sha512(dom + R + pk + m).digest(), "little") % L
    return R + ((r + k * scalar) % L).to_bytes(32, "little")


# ---- fixtures
@functools.lru_cache(maxsize=None)
def kat():
    with open(os.path.join(HERE, "golden", "ed25519_sign_kat.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def vectors():
    """the 160 sk / pk / msg / sig rows of the reference's ed25519 vectors"""
    with open(os.path.join(HERE, "golden", "ed25519_vectors.json")) as f:
        rows = json.load(f)
    rows = rows["vectors"] if isinstance(rows, dict) else rows
    return [{k: bytes.fromhex(v) for k, v in r.items() if k in ("sk", "pk", "msg", "sig")} for r in rows]


def kat_context(row):
    return None if row["context"] is None else bytes.fromhex(row["context"])


def rand_bytes(n, seed):
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))


def blob(msgs):
    """messages back to back (uint8) and their n + 1 offsets (uint64)"""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    data = np.frombuffer(b"".join(msgs), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8)
    return data, off


def rows(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width).copy()


# ---- the CPU twins (csrc/hosttest.hip)
@functools.lru_cache(maxsize=None)
def ht():
    import hosttest
    lib = hosttest.lib()
    vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    lib.ht_ed25519_expand.argtypes = [vp, vp, i32]
    lib.ht_ed25519_sign.argtypes = [vp, i32, vp, u32, vp, u64, vp, vp]
    lib.ht_ed25519_sign_with_r.argtypes = [vp, i32, vp, u32, vp, u64, vp, vp, vp]
    lib.ht_ed_mul_base_scan.argtypes = [vp, vp, i32]
    lib.ht_sha512_segments.argtypes = [vp, u32, vp, vp, vp, u64, vp]
    return lib


def _buf(b):
    """an aligned uint8 array holding b (at least one byte, so that its address is valid)"""
    a = np.zeros(max(len(b), 1) + 3 & ~3, np.uint8)
    a[:len(b)] = np.frombuffer(bytes(b), np.uint8)
    return a


def ht_expand(seeds):
    s = rows(seeds, 32)
    out = np.zeros((len(seeds), 96), np.uint8)
    assert ht().ht_ed25519_expand(s.ctypes.data, out.ctypes.data, len(seeds)) == 0
    return [out[i].tobytes() for i in range(len(seeds))]


def ht_sign(key, msg, flags=0, dom=b"", r=None):
    """(64 signature bytes, ok) of one row; r: the nonce scalar to use instead of the derived one"""
    k, m, d = _buf(key), _buf(msg), _buf(dom)
    sig, ok = np.full(64, 0xAA, np.uint8), np.full(1, 7, np.uint8)
    if r is None:
        rc = ht().ht_ed25519_sign(k.ctypes.data, flags, d.ctypes.data, len(dom), m.ctypes.data, len(msg), sig.ctypes.data, ok.ctypes.data)
    else:
        rr = _buf(int(r).to_bytes(32, "little"))
        rc = ht().ht_ed25519_sign_with_r(k.ctypes.data, flags, d.ctypes.data, len(dom), m.ctypes.data, len(msg), rr.ctypes.data,
                                         sig.ctypes.data, ok.ctypes.data)
    assert rc == 0
    return sig.tobytes(), int(ok[0])


def ht_mul_base_scan(scalars):
    s = rows([int(k).to_bytes(32, "little") for k in scalars], 32)
    out = np.zeros_like(s)
    assert ht().ht_ed_mul_base_scan(s.ctypes.data, out.ctypes.data, len(scalars)) == 0
    return [out[i].tobytes() for i in range(len(scalars))]


def ht_sha512_segments(dom, a32, b32, msg):
    d, m = _buf(dom), _buf(msg)
    a, b = (None if a32 is None else _buf(a32)), (None if b32 is None else _buf(b32))
    out = np.zeros(64, np.uint8)
    assert ht().ht_sha512_segments(d.ctypes.data, len(dom), None if a is None else a.ctypes.data, None if b is None else b.ctypes.data,
                                   m.ctypes.data, len(msg), out.ctypes.data) == 0
    return out.tobytes()
