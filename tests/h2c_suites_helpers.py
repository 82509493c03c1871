"""Shared by the RFC 9380 tests of secp256k1 and edwards25519: the fixture tests/golden/h2c_suites_kat.json (the reference's own
answers), the inputs of its rows - the listed ones by name, the seeded ones from a counter hash, so that the file stores answers
only - expand_message_xmd / hash_to_field in plain Python (hashlib), big-integer models of the two maps for the exceptional inputs,
and the ctypes side of the ht_h2c_* host twins (csrc/hosttest.hip)."""
import ctypes
import hashlib
import json
import os

import numpy as np

import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
SECP_P = 2**256 - 2**32 - 977
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
ED_P = 2**255 - 19
ED_L = 2**252 + 27742317777372353535851937790883648493
SEEDED = 128
SUITES = {
    "secp256k1": {"id": 0, "curve": 0, "p": SECP_P, "n": SECP_N, "hash": hashlib.sha256, "ro": b"secp256k1_XMD:SHA-256_SSWU_RO_",
                  "nu": b"secp256k1_XMD:SHA-256_SSWU_NU_", "zero": (0, 0)},
    "ed25519": {"id": 1, "curve": 1, "p": ED_P, "n": ED_L, "hash": hashlib.sha512, "ro": b"edwards25519_XMD:SHA-512_ELL2_RO_",
                "nu": b"edwards25519_XMD:SHA-512_ELL2_NU_", "zero": (0, 1)},
}
SCALAR_DST = b"HashToScalar-"
_kat = None


def kat():
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "h2c_suites_kat.json")) as f:
            _kat = json.load(f)
    return _kat


def seeded_bytes(tag, i, n):
    """n bytes of row i of the family `tag`: SHA-512 in counter mode over a fixed label (the generator and the tests share it)"""
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(b"h2c-suites-kat/%s/%d/%d" % (tag.encode(), i, c)).digest()
        c += 1
    return out[:n]


# ---------------------------------------------------------------- the listed rows: (name, msg, dst, count)
MESSAGES = [("empty", b""), ("abc", b"abc"), ("abcdef", b"abcdef0123456789"), ("q133", b"q" * 133), ("a512", b"a" * 512)]


def boundary_lengths(suite):
    """message lengths that put the padded input of b_0 (a block of zeros, the message, 3 bytes, DST', 0x80 and the length field)
    one byte below, exactly at and one byte above a block boundary of the suite's hash, under the default DST"""
    H = SUITES[suite]["hash"]
    block, lenfield = H().block_size, (8 if H().block_size == 64 else 16)
    fixed = block + 3 + len(SUITES[suite]["ro"]) + 1 + 1 + lenfield
    at = (-fixed) % block + block
    return [at - 1, at, at + 1]


def listed_rows(suite):
    s = SUITES[suite]
    quux = b"QUUX-V01-CS02-with-"
    rows = []
    for name, msg in MESSAGES:
        rows += [("%s/rfc/ro" % name, msg, quux + s["ro"], 2), ("%s/rfc/nu" % name, msg, quux + s["nu"], 1),
                 ("%s/default/ro" % name, msg, s["ro"], 2), ("%s/default/nu" % name, msg, s["nu"], 1)]
    rows += [("dst300", b"abc", b"x" * 300, 2), ("dst1", b"abc", b"D", 2), ("dst255", b"abc", b"y" * 255, 1)]
    rows += [("boundary%+d" % (k - 1), seeded_bytes("boundary-" + suite, k, n), s["ro"], 2) for k, n in enumerate(boundary_lengths(suite))]
    rows += [("long1000", seeded_bytes("long-" + suite, 0, 1000), s["ro"], 2)]
    return rows


def scalar_rows(suite):
    """(name, msg, dst or None for the default)"""
    return [(name, msg, None) for name, msg in MESSAGES] + [("abc/custom", b"abc", b"QUUX-V01-CS02-with-" + SUITES[suite]["ro"])]


def edge_us(suite):
    p = SUITES[suite]["p"]
    return [0, 1, p - 1, p, p + 1, 2**256 - 1]


def _sqrt(v, p):
    """a square root of v mod p, or None"""
    v %= p
    if v == 0:
        return 0
    if pow(v, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(v, (p + 1) // 4, p)
    r = pow(v, (p + 3) // 8, p)                      # p = 5 (mod 8)
    if r * r % p != v:
        r = r * pow(2, (p - 1) // 4, p) % p
    return r


SWU_Z = SECP_P - 11
ELL2_J = 486662


def exception_us(suite):
    """the inputs of the exceptional branches, found with big integers: {name: u}.
    secp256k1: Z^2 u^4 + Z u^2 = 0 with u != 0, i.e. u^2 = -1 / Z = 1 / 11 (11 = (-1)(-11) is a square: p = 3 mod 4, Z a non-square).
    edwards25519: xd yd = 0 in step 7 of the map to Edwards form with u != 0: yd = xMn + xMd = 0, i.e. x = -1, which is x1 for
    u^2 = (J - 1) / 2 and x2 for u^2 = 1 / (2 (J - 1)); a candidate counts only where the map really takes that x (ed_map_model)."""
    if suite == "secp256k1":
        r = _sqrt(pow(-SWU_Z % SECP_P, -1, SECP_P), SECP_P)
        return {} if r is None else {"swu_tv2_zero+": r, "swu_tv2_zero-": SECP_P - r}
    out = {}
    for name, sq in (("x1", (ELL2_J - 1) * pow(2, -1, ED_P)), ("x2", pow(2 * (ELL2_J - 1), -1, ED_P))):
        r = _sqrt(sq, ED_P)
        if r is not None:
            for sign, u in (("+", r), ("-", ED_P - r)):
                if ed_map_model(u)[4]:
                    out["ell2_tv1_zero_%s%s" % (name, sign)] = u
    return out


def pair_rows(suite):
    """(u0, u1) of the count = 2 map: the doubling (u, u), the cancellation (u, p - u) and two generic pairs"""
    p = SUITES[suite]["p"]
    us = [5, int.from_bytes(seeded_bytes("pair-" + suite, 0, 32), "big") % p]
    rows = []
    for u in us:
        rows += [(u, u), (u, p - u)]
    return rows + [(us[0], us[1]), (1, 2)]


def seeded_row(suite, i):
    """row i of the suite's seeded family: ("hash", msg, dst, count) or ("map", u0, u1) with any values below 2^384"""
    s = SUITES[suite]
    kind = i % 4
    msg = seeded_bytes("msg-" + suite, i, 13 * i % 211)
    if kind == 0:
        return ("hash", msg, s["ro"], 2)
    if kind == 1:
        return ("hash", msg, s["nu"], 1)
    if kind == 2:
        return ("hash", msg, seeded_bytes("dst-" + suite, i, 1 + 7 * i % 255), 2)
    return ("map", int.from_bytes(seeded_bytes("u0-" + suite, i, 48), "big"), int.from_bytes(seeded_bytes("u1-" + suite, i, 48), "big"))


def seeded_answers(suite):
    """[(x, y, inf)] of the seeded rows"""
    flat = "".join(kat()[suite]["seeded"])
    rows = [flat[j:j + 130] for j in range(0, len(flat), 130)]
    assert len(rows) == SEEDED
    return [(int(r[:64], 16), int(r[64:128], 16), int(r[128:], 16)) for r in rows]


# ---------------------------------------------------------------- hashing in plain Python
def xmd(msg, dst, out_len, H):
    """expand_message_xmd (RFC 9380 section 5.3.1) with hashlib"""
    if len(dst) > 255:
        dst = H(b"H2C-OVERSIZE-DST-" + dst).digest()
    b, r = H().digest_size, H().block_size
    ell = -(-out_len // b)
    dp = dst + bytes([len(dst)])
    b0 = H(bytes(r) + msg + out_len.to_bytes(2, "big") + b"\x00" + dp).digest()
    bs = [H(b0 + b"\x01" + dp).digest()]
    for i in range(1, ell):
        bs.append(H(bytes(x ^ y for x, y in zip(b0, bs[-1])) + bytes([i + 1]) + dp).digest())
    return b"".join(bs)[:out_len]


def hash_to_field(suite, msg, dst, count, modulus=None):
    s = SUITES[suite]
    prb = xmd(msg, dst, 48 * count, s["hash"])
    return [int.from_bytes(prb[48 * j:48 * j + 48], "big") % (modulus or s["p"]) for j in range(count)]


def effective_dst(suite, dst):
    """what the device is given: an oversize DST hashed first"""
    return SUITES[suite]["hash"](b"H2C-OVERSIZE-DST-" + dst).digest() if len(dst) > 255 else dst


# ---------------------------------------------------------------- big-integer models of the maps (the exceptional inputs, ops 4 - 6)
SWU_A = 0x3F8731ABDD661ADCA08A5558F0F5D272E953D363CB6F0E5D405447C01A444533
SWU_B = 1771


def secp_swu_model(u):
    """mapToCurveSimpleSWU on E' (RFC 9380 section 6.6.2 / F.2): (x, y, took_exception)"""
    p, A, B, Z = SECP_P, SWU_A, SWU_B, SWU_Z
    u %= p
    tv1 = Z * u * u % p
    tv2 = (tv1 * tv1 + tv1) % p
    exc = tv2 == 0
    x1 = B * pow(Z * A, -1, p) % p if exc else (-B) * pow(A, -1, p) % p * (1 + pow(tv2, -1, p)) % p
    gx1 = (x1 ** 3 + A * x1 + B) % p
    y1 = _sqrt(gx1, p)
    if y1 is not None:
        x, y = x1, y1
    else:
        x = tv1 * x1 % p
        y = _sqrt((x ** 3 + A * x + B) % p, p)
    if u % 2 != y % 2:
        y = p - y
    return x, y, exc


def ed_map_model(u):
    """map_to_curve_elligator2_edwards25519 (RFC 9380 appendix G.2.1 / G.2.2) with inversions: (xn, xd, yn, yd, took_exception)
    where the point is (xn / xd, yn / yd)"""
    p, J = ED_P, ELL2_J
    u %= p
    c1 = _sqrt(-(J + 2), p)
    c1 = c1 if c1 % 2 == 0 else p - c1
    tv1 = 2 * u * u % p
    xd = (tv1 + 1) % p
    x1 = (-J) * pow(xd, -1, p) % p
    g = lambda x: (x ** 3 + J * x * x + x) % p  # noqa: E731
    y1 = _sqrt(g(x1), p)
    if y1 is not None:
        x, y, e3 = x1, y1, True
    else:
        x, e3 = x1 * tv1 % p, False
        y = _sqrt(g(x), p)
    if e3 != (y % 2 == 1):
        y = (p - y) % p
    xn_e, xd_e = x * c1 % p, y                                     # xn / xd = c1 xM / yM
    yn_e, yd_e = (x - 1) % p, (x + 1) % p
    if xd_e * yd_e % p == 0:
        return 0, 1, 1, 1, True
    return xn_e, xd_e, yn_e, yd_e, False


# ---------------------------------------------------------------- the host twins (csrc/hosttest.hip ht_h2c_*)
def _lib():
    L = hosttest.lib()
    vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    L.ht_h2c_xmd_sha256.argtypes = [ctypes.c_char_p, u64, ctypes.c_char_p, u32, u32, vp]
    L.ht_h2c_hash_to_field.argtypes = [i32, ctypes.c_char_p, u64, ctypes.c_char_p, u32, i32, vp]
    L.ht_h2c_hash_to_scalar.argtypes = [i32, ctypes.c_char_p, u64, ctypes.c_char_p, u32, vp]
    L.ht_h2c_map.argtypes = [i32, ctypes.c_char_p, i32, vp, vp]
    L.ht_h2c_hash.argtypes = [i32, ctypes.c_char_p, u64, ctypes.c_char_p, u32, i32, vp, vp]
    L.ht_h2c_check.argtypes = [i32, vp, vp]
    return L


def _point(out, inf):
    b = out.tobytes()
    return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little"), int(inf[0])


def ht_xmd_sha256(msg, dst, out_len):
    out = np.zeros(max(out_len, 1), dtype=np.uint8)
    rc = _lib().ht_h2c_xmd_sha256(msg, len(msg), dst, len(dst), out_len, out.ctypes.data)
    return rc, out.tobytes()[:out_len]


def ht_hash_to_field(suite, msg, dst, count):
    out = np.zeros(8 * count, dtype=np.uint32)
    assert _lib().ht_h2c_hash_to_field(SUITES[suite]["id"], msg, len(msg), dst, len(dst), count, out.ctypes.data) == 0
    b = out.tobytes()
    return [int.from_bytes(b[32 * j:32 * j + 32], "little") for j in range(count)]


def ht_hash_to_scalar(suite, msg, dst):
    out = np.zeros(8, dtype=np.uint32)
    assert _lib().ht_h2c_hash_to_scalar(SUITES[suite]["id"], msg, len(msg), dst, len(dst), out.ctypes.data) == 0
    return int.from_bytes(out.tobytes(), "little")


def ht_map(suite, us):
    """us: one or two integers below 2^384 -> (x, y, inf)"""
    out, inf = np.zeros(16, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
    raw = b"".join(int(u).to_bytes(48, "little") for u in us)
    assert _lib().ht_h2c_map(SUITES[suite]["id"], raw, len(us), out.ctypes.data, inf.ctypes.data) == 0
    return _point(out, inf)


def ht_hash(suite, msg, dst, count):
    out, inf = np.zeros(16, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
    assert _lib().ht_h2c_hash(SUITES[suite]["id"], msg, len(msg), dst, len(dst), count, out.ctypes.data, inf.ctypes.data) == 0
    return _point(out, inf)


def check_row(words):
    """integers (value, words it takes) -> one row of 24 uint32 words of ncg_h2c_check / ht_h2c_check"""
    raw = b"".join(int(v).to_bytes(4 * w, "little") for v, w in words)
    return np.frombuffer(raw + bytes(96 - len(raw)), dtype=np.uint32).copy()


def ht_check(op, row):
    """-> (rc, [three integers of 8 words each])"""
    out = np.zeros(24, dtype=np.uint32)
    rc = _lib().ht_h2c_check(op, np.ascontiguousarray(row, dtype=np.uint32).ctypes.data, out.ctypes.data)
    b = out.tobytes()
    return rc, [int.from_bytes(b[32 * j:32 * j + 32], "little") for j in range(3)]


def words_to_ints(out_row):
    b = np.ascontiguousarray(out_row, dtype=np.uint32).tobytes()
    return [int.from_bytes(b[32 * j:32 * j + 32], "little") for j in range(3)]


# ---------------------------------------------------------------- the reference, live (where its bundle and node exist)
LIVE_DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { secp256k1_hasher } from './secp256k1.mjs';
import { ed25519_hasher } from './ed25519.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hasher = job.suite === 'secp256k1' ? secp256k1_hasher : ed25519_hasher;
const h64 = (n) => n.toString(16).padStart(64, '0');
console.log(JSON.stringify(job.msgs.map((m) => {
  const msg = Uint8Array.from(Buffer.from(m, 'hex')), o = { DST: Uint8Array.from(Buffer.from(job.dst, 'hex')) };
  const p = job.count === 2 ? hasher.hashToCurve(msg, o) : hasher.encodeToCurve(msg, o), a = p.toAffine();
  return [h64(a.x), h64(a.y), p.equals(hasher.Point.ZERO) ? 1 : 0];
})));
"""


def live_reference(suite, msgs, dst, count):
    """[(x, y, inf)] of hashToCurve (count 2) / encodeToCurve (count 1) from the reference's own code, run now"""
    import subprocess
    import tempfile
    from oracle import refjs
    refjs.ref_dir()
    driver = os.path.join(refjs.hooked_dir(), "src", "h2c_suites_live_driver.mjs")
    with open(driver, "w") as f:
        f.write(LIVE_DRIVER)
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"suite": suite, "msgs": [m.hex() for m in msgs], "dst": dst.hex(), "count": count}, f)
        path = f.name
    try:
        res = subprocess.run([refjs.node(), driver, path], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert res.returncode == 0, (res.stderr or res.stdout)[-2000:]
    return [(int(x, 16), int(y, 16), inf) for x, y, inf in json.loads(res.stdout.strip().splitlines()[-1])]
