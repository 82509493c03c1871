"""RFC 9380 for secp256k1 and edwards25519 without a GPU: the CPU twins of the lane code of csrc/h2c_suites.hpp (ht_h2c_*) against
the reference's own answers (tests/golden/h2c_suites_kat.json), hashlib and big-integer models of the maps, and the rules of the
Python hashers (noble_curves_amd.h2c) with a fake engine.  Every comparison is exact."""
import hashlib
import os

import numpy as np
import pytest

import h2c_suites_helpers as hh
from noble_curves_amd import curve as GC
from noble_curves_amd import h2c as GH

SUITE_NAMES = sorted(hh.SUITES)
XMD_OUT_LENS = (1, 32, 33, 48, 96, 256)


def _want(row):
    return int(row["x"], 16), int(row["y"], 16), row["inf"]


def test_generator_pins_are_in_the_fixture():
    s, e = hh.kat()["secp256k1"], hh.kat()["ed25519"]
    abc = {r["name"]: r for r in s["hash"]}["abc/rfc/ro"]
    assert (abc["x"], abc["y"]) == ("3377e01eab42db296b512293120c6cee72b6ecf9f9205760bd9ff11fb3cb2c4b",
                                    "7f95890f33efebd1044d382a01b1bee0900fb6116f94688d487c6c7b9c8371f6")     # RFC 9380 J.8.1
    abc = {r["name"]: r for r in e["hash"]}["abc/rfc/ro"]
    assert (abc["x"], abc["y"]) == ("608040b42285cc0d72cbb3985c6b04c935370c7361f4b7fbdb1ae7f8c1a8ecad",
                                    "1a8395b88338f22e435bbd301183e7f20a5f9de643f11882fb237f88268a5531")     # RFC 9380 J.5.1
    assert s["map"][0]["x"] == "bf6ce2abc92f03c7abfb18752134acc036b8e8ef46a7ed2634a86727c12d6ac1"
    assert _want(e["map"][0]) == (0, 1, 1)
    assert s["scalar"][1]["out"] == "0afe998ff82d0b7ca5673a6c8dcaf2a0cd1361d1d1b2a4e4f57f4dc9a0305788"


def test_xmd_sha256_against_hashlib():
    msgs = [b"", b"abc", b"q" * 133, hh.seeded_bytes("xmd", 0, 1000)] + [hh.seeded_bytes("xmd", n, n) for n in (54, 55, 56, 63, 64, 65)]
    for msg in msgs:
        for dst in (b"D", b"QUUX-V01-CS02-with-expander-SHA256-128", b"y" * 255):
            for out_len in XMD_OUT_LENS:
                rc, got = hh.ht_xmd_sha256(msg, dst, out_len)
                assert rc == 0 and got == hh.xmd(msg, dst, out_len, hashlib.sha256), (len(msg), len(dst), out_len)
    assert hh.ht_xmd_sha256(b"", b"", 32)[0] == -1 and hh.ht_xmd_sha256(b"", b"D", 257)[0] == -1 and hh.ht_xmd_sha256(b"", b"D", 0)[0] == -1
    # RFC 9380 K.1: expand_message_xmd(SHA-256), msg = "", len_in_bytes = 0x20
    assert hh.ht_xmd_sha256(b"", b"QUUX-V01-CS02-with-expander-SHA256-128", 32)[1].hex() == \
        "68a985b87eb6b46952128911f2a4412bbc302a9d759667f87f7a21d803f07235"


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_reduction_of_48_bytes(suite):
    s = hh.SUITES[suite]
    p, n = s["p"], s["n"]
    vals = [0, 1, p - 1, p, p + 1, n - 1, n, n + 1, 2**256 - 1, 2**256, 2**384 - 1, 2**384 - p, (2**128 - 1) << 256] + \
        [int.from_bytes(hh.seeded_bytes("reduce-" + suite, i, 48), "big") for i in range(64)]
    for v in vals:
        rc, out = hh.ht_check(s["id"], hh.check_row([(v, 12)]))           # op 0 / 1: mod p
        assert rc == 0 and out == [v % p, 0, 0], hex(v)
        rc, out = hh.ht_check(2 + s["id"], hh.check_row([(v, 12)]))       # op 2 / 3: mod n / mod L
        assert rc == 0 and out == [v % n, 0, 0], hex(v)
    assert hh.ht_check(7, hh.check_row([(1, 12)])) == (-1, [0, 0, 0]) and hh.ht_check(-1, hh.check_row([(1, 12)]))[0] == -1


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_listed_rows_hash_to_field_and_full_lanes(suite):
    rows = hh.kat()[suite]["hash"]
    listed = hh.listed_rows(suite)
    assert [r["name"] for r in rows] == [name for name, _, _, _ in listed]
    for (name, msg, dst, count), r in zip(listed, rows):
        d = hh.effective_dst(suite, dst)
        u = [int(v, 16) for v in r["u"]]
        assert len(u) == count and u == hh.hash_to_field(suite, msg, dst, count), name
        assert hh.ht_hash_to_field(suite, msg, d, count) == u, name
        assert hh.ht_hash(suite, msg, d, count) == _want(r), name
        assert hh.ht_map(suite, u) == _want(r), name                        # the map half on the fixture's u


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_hash_to_scalar(suite):
    n = hh.SUITES[suite]["n"]
    for (name, msg, dst), r in zip(hh.scalar_rows(suite), hh.kat()[suite]["scalar"]):
        d = hh.SCALAR_DST if dst is None else dst
        want = int(r["out"], 16)
        assert name == r["name"] and want == hh.hash_to_field(suite, msg, d, 1, modulus=n)[0]
        assert hh.ht_hash_to_scalar(suite, msg, d) == want, name


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_map_edges_exceptions_and_pairs(suite):
    k, s = hh.kat()[suite], hh.SUITES[suite]
    assert [int(r["u"]) for r in k["map"]] == hh.edge_us(suite)
    for r in k["map"] + k["exceptions"]:
        assert hh.ht_map(suite, [int(r["u"])]) == _want(r), r["u"]
    assert {r["name"]: int(r["u"]) for r in k["exceptions"]} == hh.exception_us(suite)
    assert [(int(r["u0"]), int(r["u1"])) for r in k["pairs"]] == hh.pair_rows(suite)
    for r in k["pairs"]:
        assert hh.ht_map(suite, [int(r["u0"]), int(r["u1"])]) == _want(r), (r["u0"], r["u1"])
    # (u, u) doubles and (u, -u) cancels: sgn0(y) follows sgn0(u) on secp256k1; on edwards25519 the map ignores the sign of u
    dbl, neg = k["pairs"][0], k["pairs"][1]
    assert dbl["inf"] == 0 and int(dbl["u0"]) == int(dbl["u1"])
    if suite == "secp256k1":
        assert _want(neg) == (0, 0, 1)
    else:
        assert _want(neg) == _want(dbl)
    zero = [r for r in k["map"] if r["inf"]]
    assert all((int(r["x"], 16), int(r["y"], 16)) == s["zero"] for r in zero) and (suite == "secp256k1" or len(zero) == 2)


def test_secp256k1_swu_and_isogeny_pieces():
    p = hh.SECP_P
    exc = hh.exception_us("secp256k1")
    assert len(exc) == 2 and all(hh.secp_swu_model(u)[2] for u in exc.values())
    us = [0, 1, 2, p - 1, 5] + list(exc.values()) + [int.from_bytes(hh.seeded_bytes("swu", i, 48), "big") for i in range(24)]
    taken = set()
    for u in us:
        x, y, e = hh.secp_swu_model(u)
        taken.add(e)
        rc, (xn, xd, yy) = hh.ht_check(4, hh.check_row([(u, 12)]))
        assert rc == 0 and xd != 0 and xn * pow(xd, -1, p) % p == x and yy == y, hex(u)
        assert (y * y - x ** 3 - hh.SWU_A * x - hh.SWU_B) % p == 0 and y % 2 == (u % p) % 2
        rc, (X, Y, Z) = hh.ht_check(5, hh.check_row([(x, 8), (y, 8)]))      # the isogeny at (x', y'): a point of y^2 = x^3 + 7
        zi = pow(Z, -1, p)
        ax, ay = X * zi * zi % p, Y * zi ** 3 % p
        assert rc == 0 and Z != 0 and (ay * ay - ax ** 3 - 7) % p == 0
        assert hh.ht_map("secp256k1", [u]) == (ax, ay, 0)
    assert taken == {False, True}
    # The zero denominator: xden = (x - x0)^2 and yden(x0) = 0 with x0 in Fp, but g(x0) is not a square, so no point of E'(Fp)
    # gets there (E' has the prime order of E: no point of order 3).  The branch is driven at x' = x0 with an arbitrary y'.
    k1 = 0xedadc6f64383dc1df7c4b2d51b54225406d36b641f5e41bbc52a56612a8c6d14
    x0 = (-k1) * pow(2, -1, p) % p
    assert pow((x0 ** 3 + hh.SWU_A * x0 + hh.SWU_B) % p, (p - 1) // 2, p) == p - 1
    rc, (X, Y, Z) = hh.ht_check(5, hh.check_row([(x0, 8), (12345, 8)]))
    assert rc == 0 and Z == 0


def test_edwards25519_map_pieces():
    p = hh.ED_P
    assert hh.exception_us("ed25519") == {}                                 # u = 0 (mod p) is the only input of steps 8-12
    us = [0, p, 1, 2, p - 1, 5] + [int.from_bytes(hh.seeded_bytes("ell2", i, 48), "big") for i in range(24)]
    for u in us:
        xn, xd, yn, yd, e = hh.ed_map_model(u)
        x, y = xn * pow(xd, -1, p) % p, yn * pow(yd, -1, p) % p
        rc, (X, Y, Z) = hh.ht_check(6, hh.check_row([(u, 12)]))
        zi = pow(Z, -1, p)
        assert rc == 0 and Z != 0 and (X * zi % p, Y * zi % p) == (x, y), hex(u)
        assert e == (u % p == 0) and (not e or (x, y) == (0, 1))
        d = (-121665) * pow(121666, -1, p) % p
        assert (-x * x + y * y - 1 - d * x * x * y * y) % p == 0


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_seeded_rows(suite):
    want = hh.seeded_answers(suite)
    kinds = set()
    for i in range(hh.SEEDED):
        row = hh.seeded_row(suite, i)
        kinds.add((row[0], row[3] if row[0] == "hash" else 2))
        got = hh.ht_hash(suite, row[1], row[2], row[3]) if row[0] == "hash" else hh.ht_map(suite, [row[1], row[2]])
        assert got == want[i], i
    assert kinds == {("hash", 1), ("hash", 2), ("map", 2)}


# ---------------------------------------------------------------- the shim's rules, with an engine that records its calls
class FakeEngine:
    def __init__(self):
        self.calls = []

    def h2c_hash_batch(self, suite, msgs, dst, count):
        self.calls.append(("hash", suite, list(msgs), dst, count))
        out = np.zeros((len(msgs), 64), dtype=np.uint8)
        out[:, 0] = 7
        out[:, 32] = 9
        return out, np.zeros(len(msgs), dtype=np.uint8)

    def h2c_map_batch(self, suite, u48, count):
        self.calls.append(("map", suite, np.array(u48), count))
        n = np.asarray(u48).reshape(-1, count * 48).shape[0]
        return np.zeros((n, 64), dtype=np.uint8), np.ones(n, dtype=np.uint8)

    def h2c_hash_to_scalar_batch(self, suite, msgs, dst):
        self.calls.append(("scalar", suite, list(msgs), dst))
        out = np.zeros((len(msgs), 32), dtype=np.uint8)
        out[:, 0] = 5
        return out

    def map_to_curve_batch(self, curve, u, count):
        self.calls.append(("bls", curve, count))
        pb = 96 if curve == 2 else 192
        return np.zeros((u.shape[0], pb), dtype=np.uint8), np.ones(u.shape[0], dtype=np.uint8)


def _hasher(suite):
    src = GH.secp256k1_hasher if suite == "secp256k1" else GH.ed25519_hasher
    eng = FakeEngine()
    return GH.H2CSuiteHasher(src.Point, src._suite, src._defaults["DST"], src._defaults["encodeDST"], src._defaults["hash"], engine=eng), eng


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_shim_rules(suite):
    h, eng = _hasher(suite)
    s, k = hh.SUITES[suite], hh.kat()[suite]
    err = k["errors"]
    assert h.Point is (GC.secp256k1_Point if suite == "secp256k1" else GC.ed25519_Point)
    d = h.defaults
    ref = k["defaults"]
    assert (d["DST"], d["encodeDST"], str(d["p"]), d["m"], d["k"], d["expand"]) == \
        (ref["DST"], ref["encodeDST"], ref["p"], ref["m"], ref["k"], ref["expand"]) and d["hash"] == s["hash"]().name
    d["DST"] = "poisoned"
    assert h.defaults["DST"] == ref["DST"] and h.defaults is not h.defaults and k["defaults_is_copy"]
    # one call per batch, the suite's DSTs, count 2 / 1
    pts = h.hashToCurveBatch([b"a", b"", b"ccc"])
    assert eng.calls == [("hash", s["id"], [b"a", b"", b"ccc"], s["ro"], 2)] and [p.toAffine() for p in pts] == [(7, 9)] * 3
    assert isinstance(pts[0], h.Point)
    eng.calls.clear()
    h.encodeToCurve(bytearray(b"zz"))
    h.hashToCurve(b"m", {"DST": "custom"})
    h.hashToCurve(b"m", {"DST": b"custom", "p": 17, "m": 2, "hash": "md5"})     # only DST may be overridden
    assert eng.calls == [("hash", s["id"], [b"zz"], s["nu"], 1)] + [("hash", s["id"], [b"m"], b"custom", 2)] * 2
    eng.calls.clear()
    # an oversize DST is hashed first, with the suite's hash
    big = b"x" * 300
    h.hashToCurve(b"abc", {"DST": big})
    h.hashToScalar(b"abc", {"DST": big})
    hashed = s["hash"](b"H2C-OVERSIZE-DST-" + big).digest()
    assert [c[3] for c in eng.calls] == [hashed, hashed]
    h.hashToCurve(b"abc", {"DST": b"y" * 255})
    assert eng.calls[-1][3] == b"y" * 255
    eng.calls.clear()
    # hashToScalar: the default DST, integers out
    assert h.hashToScalarBatch([b"a", b"b"]) == [5, 5] and h.hashToScalar(b"a", {"DST": "T"}) == 5
    assert eng.calls == [("scalar", s["id"], [b"a", b"b"], b"HashToScalar-"), ("scalar", s["id"], [b"a"], b"T")]
    eng.calls.clear()
    # mapToCurve: integers only, reduced like Fp.create, one call
    zero = h.mapToCurveBatch([5, s["p"] + 6, 2**300])
    assert len(eng.calls) == 1 and eng.calls[0][0] == "map" and eng.calls[0][3] == 1
    assert [int.from_bytes(bytes(r), "little") for r in eng.calls[0][2]] == [5, 6, 2**300 % s["p"]]
    assert all(z is h.Point.ZERO for z in zero) and h.Point.ZERO.toAffine() == s["zero"]
    for bad in (5.0, True, [5], "5", None):
        with pytest.raises(ValueError) as e:
            h.mapToCurve(bad)
        assert str(e.value) == err["map_number"] == err["map_array"] == "expected bigint (m=1)"
    # the messages of the reference
    for call in (lambda: h.hashToCurve(b"x", {"DST": ""}), lambda: h.encodeToCurve(b"x", {"DST": b""}), lambda: h.hashToScalar(b"x", {"DST": ""})):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == err["empty_dst"] == err["empty_dst_bytes"] == err["scalar_empty_dst"] == "DST must be non-empty"
    for bad in ("abc", 5, None):
        for call in (h.hashToCurve, h.encodeToCurve, h.hashToScalar):
            with pytest.raises(TypeError) as e:
                call(bad)
            assert str(e.value).startswith('"msg" expected Uint8Array, got type=')
    assert err["msg_string"].startswith("expected Uint8Array, got type=")
    assert h.hashToCurveBatch([]) == [] and h.mapToCurveBatch([]) == [] and h.hashToScalarBatch([]) == [] and len(eng.calls) == 1


def test_bls12_381_hashers_unchanged():
    for h, cid, m in ((GH.bls12_381_G1_hasher, 2, 1), (GH.bls12_381_G2_hasher, 3, 2)):
        assert isinstance(h, GH.H2CHasher) and h.defaults["m"] == m and h.defaults["hash"] == "sha256" and h.defaults["k"] == 128
        assert h.defaults["DST"] == h.defaults["encodeDST"] == "BLS_SIG_BLS12381G%d_XMD:SHA-256_SSWU_RO_NUL_" % (cid - 1)
        eng = FakeEngine()
        g = GH.H2CHasher(h.Point, cid, m, h.defaults["DST"], engine=eng)
        assert g.hashToCurve("abc") is h.Point.ZERO and g.encodeToCurve(b"abc") is h.Point.ZERO      # a string is still read as ASCII
        assert eng.calls == [("bls", cid, 2), ("bls", cid, 1)]
        with pytest.raises(ValueError):
            g.mapToCurve(5.0 if m == 1 else [5])
    assert GH.hash_to_field(b"abc", 2, dict(GH.bls12_381_G1_hasher.defaults)) == \
        [[int.from_bytes(hh.xmd(b"abc", GH.bls12_381_G1_hasher.defaults["DST"].encode(), 128, hashlib.sha256)[64 * j:64 * j + 64], "big") % GH._P]
         for j in range(2)]


def test_against_the_reference_live():
    from oracle import refjs
    if not refjs.available() or not refjs.hooked_dir():
        pytest.skip("the reference bundle or node is not here")
    seed = int.from_bytes(os.urandom(8), "little")
    print("live reference seed", seed)                     # shown by pytest when the test fails: rerun with it
    rng = np.random.default_rng(seed)
    for suite in SUITE_NAMES:
        msgs = [rng.bytes(int(rng.integers(0, 200))) for _ in range(16)]
        dst = b"live-" + rng.bytes(int(rng.integers(1, 40)))
        for count in (2, 1):
            want = hh.live_reference(suite, msgs, dst, count)
            assert [hh.ht_hash(suite, m, dst, count) for m in msgs] == want, (seed, suite, count, [m.hex() for m in msgs], dst.hex())
