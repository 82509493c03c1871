"""Shared by the secp256k1 signing tests: a plain-Python model (hashlib + hmac + the oracle's curve) of RFC 6979 with the HMAC-SHA256
DRBG, ECDSA signing as secp256k1.sign does it, BIP-340 signing and the DER encoding; the fixtures (tests/golden/secp256k1_ecdsa.json
from the reference's vectors, tests/golden/secp256k1_sign_kat.json written by make_secp256k1_sign_kat.py from the reference's own
answers) and the bindings of the CPU twins of csrc/secp256k1_sign.hip."""
import ctypes
import functools
import hashlib
import hmac
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P = 2**256 - 2**32 - 977
LOW_S, ONE_KEY = 1, 4                      # NCG_ECDSA_LOW_S, NCG_SECP_SIGN_ONE_KEY
PK_COMPRESSED, PK_UNCOMPRESSED, PK_XONLY = 0, 1, 2
MSG_LENGTHS = (0, 1, 55, 56, 63, 64, 119, 120, 1000)
CHECK_WORDS = {0: (24, 1, 8), 1: (8, 1, 16), 2: (32, 1, 18), 3: (24, 1, 8), 4: (24, 1, 18)}


# ---- the curve: k G as affine integers (the oracle's point class, cached: the tests ask for the same points again and again)
@functools.lru_cache(maxsize=None)
def mul_base(k):
    from oracle.curves import Secp256k1
    return Secp256k1.BASE.multiply(k % N).toAffine()


def be(v):
    return int(v).to_bytes(32, "big")


# ---- RFC 6979 / createHmacDrbg(32, 32, hmac-sha256) of the reference (utils.ts:755-813)
def drbg_candidates(seed):
    """the candidates T0, T1, ... (32 bytes each) for a seed; one empty reseed between two candidates"""
    K, V = bytes(32), b"\x01" * 32
    mac = lambda key, msg: hmac.new(key, msg, hashlib.sha256).digest()  # noqa: E731
    K = mac(K, V + b"\x00" + seed)
    V = mac(K, V)
    K = mac(K, V + b"\x01" + seed)
    V = mac(K, V)
    while True:
        V = mac(K, V)
        yield V
        K = mac(K, V + b"\x00")
        V = mac(K, V)


def bits2int_modN(data):
    """weierstrass.ts:1440-1456 for a 256-bit order: the leading 256 bits, reduced"""
    if len(data) > 8192:
        raise ValueError("input is too large")
    num = int.from_bytes(data, "big")
    delta = len(data) * 8 - 256
    return (num >> delta if delta > 0 else num) % N


def normalise_hash(data):
    """the 32 bytes whose integer is bits2int(data): what the batch form hands to the device for prehash=False"""
    data = bytes(data)
    return data[:32] if len(data) >= 32 else data.rjust(32, b"\0")


def ecdsa_finish(k, x, y_odd, m, d, low_s):
    """k2sig (weierstrass.ts:1514-1542) from its inputs: (r, s, recid) or None where the candidate is refused"""
    if not 0 < k < N:
        return None
    r = x % N
    if r == 0:
        return None
    s = pow(k, -1, N) * (m + r * d) % N
    if s == 0:
        return None
    recid = (2 if x >= N else 0) | (1 if y_odd else 0)
    if low_s and s > N >> 1:
        s, recid = N - s, recid ^ 1
    return r, s, recid


def ecdsa_sign(msg, sk, lowS=True, prehash=True, extra=None, refuse_first=0):
    """(r, s, recid); refuse_first: the index of the first candidate that may be taken"""
    d = int.from_bytes(sk, "big")
    assert 0 < d < N
    h = hashlib.sha256(msg).digest() if prehash else bytes(msg)
    m = bits2int_modN(h)
    seed = be(d) + be(m) + (extra or b"")
    for j, T in enumerate(drbg_candidates(seed)):
        assert j < 1000
        if j < refuse_first:
            continue
        k = int.from_bytes(T, "big")
        if not 0 < k < N:
            continue
        x, y = mul_base(k)
        got = ecdsa_finish(k, x, y & 1, m, d, lowS)
        if got:
            return got


def compact(r, s):
    return be(r) + be(s)


def recovered(r, s, recid):
    return bytes([recid]) + be(r) + be(s)


def der(r, s):
    def enc(v):
        b = v.to_bytes((v.bit_length() + 7) // 8 or 1, "big")
        if b[0] & 0x80:
            b = b"\0" + b
        assert len(b) < 128
        return b"\x02" + bytes([len(b)]) + b
    body = enc(r) + enc(s)
    assert len(body) < 128
    return b"\x30" + bytes([len(body)]) + body


def public_key(sk, mode=PK_COMPRESSED):
    x, y = mul_base(int.from_bytes(sk, "big"))
    if mode == PK_XONLY:
        return be(x)
    if mode == PK_UNCOMPRESSED:
        return b"\x04" + be(x) + be(y)
    return bytes([2 | (y & 1)]) + be(x)


# ---- BIP-340 (secp256k1.ts:147-221)
def tagged(tag, *msgs):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + b"".join(msgs)).digest()


def schnorr_scalar(k_, y_odd, e, d):
    return ((N - k_ if y_odd else k_) + e * d) % N


def schnorr_sign(msg, sk, aux):
    """the 64 signature bytes, or None where k' = 0"""
    d_ = int.from_bytes(sk, "big")
    assert 0 < d_ < N and len(aux) == 32
    px, py = mul_base(d_)
    d = d_ if py % 2 == 0 else N - d_
    t = be(d ^ int.from_bytes(tagged("BIP0340/aux", aux), "big"))
    k_ = int.from_bytes(tagged("BIP0340/nonce", t, be(px), msg), "big") % N
    if k_ == 0:
        return None
    rx, ry = mul_base(k_)
    e = int.from_bytes(tagged("BIP0340/challenge", be(rx), be(px), msg), "big") % N
    return be(rx) + be(schnorr_scalar(k_, ry & 1, e, d))


# ---- fixtures
@functools.lru_cache(maxsize=None)
def kat():
    with open(os.path.join(HERE, "golden", "secp256k1_sign_kat.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def ecdsa_vectors():
    """the `valid` rows (d, m, signature) of the reference's ECDSA vectors: prehash false, lowS true"""
    with open(os.path.join(HERE, "golden", "secp256k1_ecdsa.json")) as f:
        return json.load(f)["valid"]


def kat_extra(row):
    return None if row["extraEntropy"] is None else bytes.fromhex(row["extraEntropy"])


def rand_bytes(n, seed):
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))


def edge_scalars():
    """the scalars the scan multiply is pinned at: the ends of the range, every power of two and its neighbours, the nibble patterns
    that make every window's digit extreme, and seeded values"""
    ks = [1, 2, 3, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2]
    for j in range(256):
        ks += [2**j - 1, 2**j, 2**j + 1]
    ks += [int("f" * 64, 16) % N, int("8" * 64, 16) % N]
    rng = random.Random("secp-scan-scalars")
    ks += [rng.randrange(1, N) for _ in range(64)]
    return [k for k in dict.fromkeys(ks) if 0 < k < N]


def blob(msgs):
    """messages back to back (uint8) and their n + 1 offsets (uint64)"""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    data = np.frombuffer(b"".join(msgs), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8)
    return data, off


def rows(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width).copy()


def words(v, n=8):
    """an integer as n little-endian 32-bit words"""
    return [(int(v) >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def from_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def bytes_words(b):
    """bytes as the words they are in memory"""
    return np.frombuffer(bytes(b), np.uint32).tolist()


def finish_row(k, x, m, d):
    return words(k) + words(x) + words(m) + words(d)


def rare_finish_cases():
    """(a row, b word, want (r, s, recid, accepted)) for every branch of the finish step that real inputs reach with probability 2^-128"""
    d, m = 0x1234567, 0x89ABCDEF
    k = 0xC0FFEE
    x, y = mul_base(k)
    cases = {}

    def add(name, k, x, y_odd, m, d, low_s):
        want = ecdsa_finish(k, x, y_odd, m, d, low_s)
        cases[name] = (finish_row(k, x, m, d), y_odd | (low_s << 1), (want + (1,)) if want else (0, 0, 0, 0))

    add("plain", k, x, y & 1, m, d, 0)
    add("k = 0", 0, x, 1, m, d, 1)
    add("k = n", N, x, 0, m, d, 1)
    add("k = 2^256 - 1", 2**256 - 1, x, 0, m, d, 0)
    add("r = 0: x = n", k, N, 0, m, d, 1)
    add("x in [n, p): recid 2", k, N + 5, 0, m, d, 0)
    add("x in [n, p): recid 3", k, P - 1, 1, m, d, 0)
    r = x % N
    add("s = 0", k, x, 0, (-r * d) % N, d, 1)
    for low_s in (0, 1):                       # one s in each half, with and without the rule
        for mm in range(2, 40):
            s = pow(k, -1, N) * (mm + r * d) % N
            if (s > N >> 1) and "high s, lowS %d" % low_s not in cases:
                add("high s, lowS %d" % low_s, k, x, y & 1, mm, d, low_s)
            if (s <= N >> 1) and "low s, lowS %d" % low_s not in cases:
                add("low s, lowS %d" % low_s, k, x, y & 1, mm, d, low_s)
    assert len(cases) == 12 and cases["r = 0: x = n"][2] == (0, 0, 0, 0) and cases["s = 0"][2] == (0, 0, 0, 0)
    assert cases["x in [n, p): recid 2"][2][2] == 2 and cases["x in [n, p): recid 3"][2][2] == 3
    return cases


# ---- the CPU twins (csrc/hosttest.hip)
@functools.lru_cache(maxsize=None)
def ht():
    import hosttest
    lib = hosttest.lib()
    vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    lib.ht_secp_sign_op.argtypes = [i32, i32, vp, vp, vp]
    lib.ht_secp_sign_widths.argtypes = [i32, vp, vp, vp]
    lib.ht_secp_public_key.argtypes = [vp, i32, vp, vp, i32]
    lib.ht_ecdsa_sign.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.ht_schnorr_sign.argtypes = [vp, vp, vp, u64, vp, vp]
    lib.ht_sha256_segments.argtypes = [vp, u32, vp, u32, vp, u64, vp]
    return lib


def _buf(b):
    """an aligned uint8 array holding b (at least one byte, so that its address is valid)"""
    a = np.zeros(max(len(b), 1) + 3 & ~3, np.uint8)
    a[:len(b)] = np.frombuffer(bytes(b), np.uint8)
    return a


def ht_widths(op):
    w = [ctypes.c_int(-1) for _ in range(3)]
    ht().ht_secp_sign_widths(op, *[ctypes.byref(x) for x in w])
    return tuple(x.value for x in w)


def ht_op(op, a_words, b_words=(0,), variant=0):
    """one row of the check table on the CPU -> (rc, the out words)"""
    wa, wb, wo = CHECK_WORDS.get(op, (1, 1, 16))
    a = np.array(list(a_words) + [0] * (wa - len(a_words)), np.uint32)
    b = np.array(list(b_words) + [0] * (wb - len(b_words)), np.uint32)
    out = np.zeros(max(wo, 1), np.uint32)
    rc = ht().ht_secp_sign_op(op, variant, a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return rc, [int(x) for x in out]


def ht_mul_base_scan(k):
    rc, out = ht_op(1, words(k))
    assert rc == 0
    return from_words(out[:8]), from_words(out[8:])


def ht_public_keys(sks, mode):
    s = rows(sks, 32)
    width = {PK_COMPRESSED: 33, PK_UNCOMPRESSED: 65, PK_XONLY: 32}[mode]
    out, ok = np.full((len(sks), width), 0xAA, np.uint8), np.full(len(sks), 7, np.uint8)
    assert ht().ht_secp_public_key(s.ctypes.data, mode, out.ctypes.data, ok.ctypes.data, len(sks)) == 0
    return [out[i].tobytes() for i in range(len(sks))], [int(x) for x in ok]


def ht_ecdsa_sign(sk, hash32, extra=None, low_s=True, refuse_first=0):
    """(64 signature bytes, recid, ok) of one row"""
    k, h = _buf(sk), _buf(hash32)
    e = None if extra is None else _buf(extra)
    sig, rec, ok = np.full(64, 0xAA, np.uint8), np.full(1, 9, np.uint8), np.full(1, 7, np.uint8)
    assert ht().ht_ecdsa_sign(k.ctypes.data, h.ctypes.data, None if e is None else e.ctypes.data, LOW_S if low_s else 0, refuse_first,
                              sig.ctypes.data, rec.ctypes.data, ok.ctypes.data) == 0
    return sig.tobytes(), int(rec[0]), int(ok[0])


def ht_schnorr_sign(sk, aux, msg):
    k, a, m = _buf(sk), _buf(aux), _buf(msg)
    sig, ok = np.full(64, 0xAA, np.uint8), np.full(1, 7, np.uint8)
    assert ht().ht_schnorr_sign(k.ctypes.data, a.ctypes.data, m.ctypes.data, len(msg), sig.ctypes.data, ok.ctypes.data) == 0
    return sig.tobytes(), int(ok[0])


def ht_sha256_segments(a, b, msg):
    m = _buf(msg)
    aa, bb = (None if a is None else _buf(a)), (None if b is None else _buf(b))
    out = np.zeros(32, np.uint8)
    assert ht().ht_sha256_segments(None if aa is None else aa.ctypes.data, len(a or b""), None if bb is None else bb.ctypes.data, len(b or b""),
                                   m.ctypes.data, len(msg), out.ctypes.data) == 0
    return out.tobytes()
