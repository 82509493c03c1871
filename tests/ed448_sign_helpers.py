"""Shared by the Ed448 signing tests: the message lengths at the edges of the SHAKE256 rate, a Keccak-f[1600] of a few lines, the
edge rows of the reduction mod n, the fixture (tests/golden/ed448_sign_kat.json, written by make_ed448_sign_kat.py from the
reference's own answers) and the bindings of the CPU twins of csrc/ed448_sign.hip.  The expectations are hashlib.shake_256, Python
integers and the plain-Python signer of ed448_helpers."""
import ctypes
import functools
import json
import os
import random

import numpy as np

import ed448_helpers as eh
from ed448_helpers import N

HERE = os.path.dirname(os.path.abspath(__file__))
EXPANDED, ONE_KEY, PREHASH = 1, 2, 4
DOM_MAX = 265
KEY_BYTES = 172
RATE = 136
OUT_LENS = (1, 56, 64, 114, 136, 137, 273)
PH_LENGTHS = (0, 1, 134, 135, 136, 137, 271, 272)      # the edges of SHAKE256(M, 64) itself
SIGN_CHECK_WORDS = {0: (50, 0, 50), 1: (29, 0, 14), 2: (28, 14, 14), 3: (43, 30, 30)}


# ---- message lengths.  SHAKE256 pads with 0x1f .. 0x80 inside the last 136-byte block: the edges are the TOTAL absorbed lengths
# 134 | 135 | 0 | 1 (mod 136): 0x1f in the last two bytes of a block (at 135 it meets 0x80: 0x9f), an empty last block, one byte in it.
def edge_lengths(prefix_len, longest=300):
    """the message lengths up to `longest` at which prefix_len + length is 0, 1, 134 or 135 (mod 136)"""
    return [n for n in range(longest + 1) if (prefix_len + n) % RATE in (0, 1, 134, 135)]


def sign_edge_lengths(ctx_len):
    """... of both hashes of a signature: the nonce hash absorbs dom (10 + ctx) || prefix (57) || M, the challenge hash
    dom || R || A (114) || M"""
    return sorted(set(edge_lengths(10 + ctx_len + 57)) | set(edge_lengths(10 + ctx_len + 114)))


def dom4(ctx=b"", ph=False):
    return eh.dom4(b"", ctx, ph)


# ---- Keccak-f[1600] on 25 integers (FIPS 202 section 3.2)
_RC = []
_r = 1
for _ in range(24):
    _c = 0
    for _j in range(7):
        _r = ((_r << 1) ^ ((_r >> 7) * 0x71)) % 256
        if _r & 2:
            _c ^= 1 << ((1 << _j) - 1)
    _RC.append(_c)
_M64 = (1 << 64) - 1


def _rol(x, n):
    return ((x << n) | (x >> (64 - n))) & _M64 if n else x


def keccak_f(lanes):
    a = [[lanes[x + 5 * y] for y in range(5)] for x in range(5)]
    for rc in _RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        x, y, cur = 1, 0, a[1][0]
        for t in range(24):
            x, y = y, (2 * x + 3 * y) % 5
            cur, a[x][y] = a[x][y], _rol(cur, (t + 1) * (t + 2) // 2 % 64)
        a = [[a[x][y] ^ (~a[(x + 1) % 5][y] & a[(x + 2) % 5][y] & _M64) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return [a[i % 5][i // 5] for i in range(25)]


def keccak_rows(count=8):
    """states [count, 25] as Python integers: zero, all ones, one bit, seeded"""
    rng = random.Random("keccak-f")
    rows_ = [[0] * 25, [_M64] * 25, [1] + [0] * 24, [0] * 24 + [1 << 63]]
    return rows_ + [[rng.getrandbits(64) for _ in range(25)] for _ in range(count - len(rows_))]


def lanes_words(states):
    return np.array([[(v >> (32 * h)) & 0xffffffff for v in st for h in (0, 1)] for st in states], np.uint32)


def words_lanes(row):
    return [int(row[2 * i]) | (int(row[2 * i + 1]) << 32) for i in range(25)]


# ---- the reduction.  mod_n_912 folds at 2^446 four times; the part above bit 446 is 466, 245, 24 and 1 bits wide in turn, so the
# multiples j of 2^446 at which a fold's high part gains a word or its last bit are j = 1, 2, 2^24 (third fold), 2^245 (second) and the
# top of the range
def mod_n_values(nrandom=2000):
    rng = random.Random("ed448-mod-n")
    top = 2**912 - 1
    vals = [0, 1, N - 1, N, N + 1, 2 * N - 1, 2**446 - 1, 2**446]
    for j in (1, 2, 3, 2**24 - 1, 2**24, 2**32, 2**245 - 1, 2**245, 2**256, 2**466 - 1):
        vals += [2**446 * j - 1, 2**446 * j + 1]
    vals += [top, top // N * N, top // N * N - 1]
    vals += [2**446 + 2**224 - 1, N + 2**224, 2 * N, 3 * N]
    vals += [rng.getrandbits(912) for _ in range(nrandom)]
    assert all(0 <= v <= top for v in vals)
    return vals


def muladd_triples(nrandom=500):
    rng = random.Random("ed448-muladd")
    edge = (0, 1, N - 1)
    return [(r, k, s) for r in edge for k in edge for s in edge] + [tuple(rng.randrange(N) for _ in range(3)) for _ in range(nrandom)]


def int_words(values, nwords):
    return np.array([[(v >> (32 * i)) & 0xffffffff for i in range(nwords)] for v in values], np.uint32).reshape(len(values), nwords)


def words_int(row):
    return sum(int(w) << (32 * i) for i, w in enumerate(row))


# ---- the signer: ed448_helpers.sign, and the same with the nonce given (None where r = 0 mod n: the reference throws)
@functools.lru_cache(maxsize=None)
def expand(seed):
    """scalar mod n (int), prefix, public key of a 57-byte seed"""
    s, prefix = eh.secret_scalar(seed)
    return s % N, prefix, eh.pt_encode(eh.pt_mul(eh.BASE, s % N))


def expanded_row(seed):
    scalar, prefix, pk = expand(bytes(seed))
    return scalar.to_bytes(56, "little") + prefix + pk + bytes(2)


@functools.lru_cache(maxsize=None)
def sign(msg, seed, ctx=b"", ph=False):
    return eh.sign(msg, seed, ctx, ph)


def sign_with_r(msg, seed, r, ctx=b"", ph=False):
    scalar, _, pk = expand(bytes(seed))
    if r % N == 0:
        return None
    rb = eh.pt_encode(eh.pt_mul(eh.BASE, r))
    k = eh.challenge(rb, pk, msg, ctx, ph) % N
    return rb + ((r + k * scalar) % N).to_bytes(57, "little")


# ---- fixtures
@functools.lru_cache(maxsize=None)
def kat():
    with open(os.path.join(HERE, "golden", "ed448_sign_kat.json")) as f:
        return json.load(f)


def kat_rows(variant=None, ctx_len=None):
    out = []
    for r in kat()["sign"]:
        if (variant is None or r["variant"] == variant) and (ctx_len is None or len(r["context"]) // 2 == ctx_len):
            out.append(r)
    return out


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
    lib.ht_shake256.argtypes = [vp, u32, vp, u32, vp, u32, vp, u64, vp, u32]
    lib.ht_ed448_sign_op.argtypes = [i32, vp, vp, vp]
    lib.ht_ed448_sign_widths.argtypes = [i32, vp, vp, vp]
    lib.ht_ed448_sign_widths.restype = None
    lib.ht_ed448_mod_n.argtypes = [vp, vp, i32]
    lib.ht_ed448_muladd.argtypes = [vp, vp, vp, vp, i32]
    lib.ht_ed448_expand.argtypes = [vp, vp, i32]
    lib.ht_ed448_sign.argtypes = [vp, i32, vp, u32, vp, u64, vp, vp]
    lib.ht_ed448_sign_with_r.argtypes = [vp, i32, vp, u32, vp, u64, vp, vp, vp]
    return lib


def _buf(b):
    """an aligned uint8 array holding b (at least one byte, so that its address is valid)"""
    a = np.zeros(max(len(b), 1) + 3 & ~3, np.uint8)
    a[:len(b)] = np.frombuffer(bytes(b), np.uint8)
    return a


def ht_shake256(dom, a, b, msg, out_len):
    """SHAKE256(dom || a || b || msg, out_len) through the four-segment absorb; a / b None: the segment is left out"""
    d, m = _buf(dom), _buf(msg)
    aa, bb = (None if a is None else _buf(a)), (None if b is None else _buf(b))
    out = np.full(out_len + 8, 0xAA, np.uint8)
    assert ht().ht_shake256(d.ctypes.data, len(dom), None if aa is None else aa.ctypes.data, 0 if a is None else len(a),
                            None if bb is None else bb.ctypes.data, 0 if b is None else len(b), m.ctypes.data, len(msg), out.ctypes.data,
                            out_len) == 0
    assert out[out_len:].tobytes() == b"\xaa" * 8, "the squeeze wrote past out_len"
    return out[:out_len].tobytes()


def ht_keccak_f(states):
    a = lanes_words(states)
    out = np.zeros_like(a)
    for i in range(a.shape[0]):
        assert ht().ht_ed448_sign_op(0, a[i].ctypes.data, None, out[i].ctypes.data) == 0
    return [words_lanes(r) for r in out]


def ht_mod_n(values):
    x = int_words(values, 29)
    out = np.zeros((len(values), 14), np.uint32)
    assert ht().ht_ed448_mod_n(x.ctypes.data, out.ctypes.data, len(values)) == 0
    return [words_int(r) for r in out]


def ht_muladd(triples):
    r, k, s = (int_words([t[j] for t in triples], 14) for j in range(3))
    out = np.zeros((len(triples), 14), np.uint32)
    assert ht().ht_ed448_muladd(r.ctypes.data, k.ctypes.data, s.ctypes.data, out.ctypes.data, len(triples)) == 0
    return [words_int(x) for x in out]


def ht_expand(seeds):
    s = rows(seeds, 57)
    out = np.zeros((len(seeds), KEY_BYTES), np.uint8)
    assert ht().ht_ed448_expand(s.ctypes.data, out.ctypes.data, len(seeds)) == 0
    return [out[i].tobytes() for i in range(len(seeds))]


def ht_sign(key, msg, flags=0, dom=None, r=None):
    """(114 signature bytes, ok) of one row; r: the nonce scalar to use instead of the derived one"""
    dom = dom4() if dom is None else dom
    k, m, d = _buf(key), _buf(msg), _buf(dom)
    sig, ok = np.full(116, 0xAA, np.uint8), np.full(1, 7, np.uint8)
    if r is None:
        rc = ht().ht_ed448_sign(k.ctypes.data, flags, d.ctypes.data, len(dom), m.ctypes.data, len(msg), sig.ctypes.data, ok.ctypes.data)
    else:
        rr = _buf(int(r).to_bytes(56, "little"))
        rc = ht().ht_ed448_sign_with_r(k.ctypes.data, flags, d.ctypes.data, len(dom), m.ctypes.data, len(msg), rr.ctypes.data,
                                       sig.ctypes.data, ok.ctypes.data)
    assert rc == 0 and sig[114:].tobytes() == b"\xaa\xaa"
    return sig[:114].tobytes(), int(ok[0])
