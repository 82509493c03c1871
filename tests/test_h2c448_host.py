"""RFC 9380 for edwards448 and the hash side of decaf448 without a GPU: the fixture tests/golden/h2c448_kat.json (the reference's own
answers) against the Python restatement of h2c448_helpers on every row, the CPU twins of the lane code of csrc/h2c448.hpp
(ht_h2c448_*) against the restatement, and the rules of the Python layer (noble_curves_amd.ed448.ed448_hasher,
noble_curves_amd.decaf448) with a fake engine.  Every comparison is exact."""
import hashlib

import numpy as np
import pytest

import h2c448_helpers as hh
from noble_curves_amd import decaf448 as GD
from noble_curves_amd import ed448 as GE
from noble_curves_amd import h2c as GH

P, N = hh.P, hh.N


def _pt(row):
    return int(row["x"], 16), int(row["y"], 16)


# ---------------------------------------------------------------- the fixture against the restatement
def test_fixture_pins_and_layout():
    k = hh.kat()
    decaf = {r["name"]: r["out"] for r in k["decaf"]}
    # the reference's inline vector (test/rfc9496-ristretto-decaf.test.ts, 'decaf448_hasher and wrapper helpers')
    assert k["pins"] == [{"name": "fill5", "out": decaf["fill5"]}]
    assert decaf["fill5"] == "1287dea7519af966cf537a58f614e8b39b93a7c0b989bcdb4f94af8f2573ab59589accb0d2a2097b5f30c1d721619470f21e78613bbfc4b6"
    assert [r["name"] for r in k["hash"]] == [r[0] for r in hh.listed_rows()]
    assert [r["name"] for r in k["xof"]] == [r[0] for r in hh.xof_rows()]
    assert [r["name"] for r in k["exceptions"]] == list(hh.exception_us()) and len(k["exceptions"]) >= 3
    assert all(len(k["seeded_" + name]) == hh.SEEDED for name in hh.SEEDED_SUITES + ("map",)) and len(k["seeded_pairs"]) == hh.SEEDED_PAIRS


def test_fixture_hash_rows_agree_with_the_restatement():
    for (name, msg, dst, count), row in zip(hh.listed_rows(), hh.kat()["hash"]):
        us = hh.hash_to_field(msg, dst, count)
        assert [int(u, 16) for u in row["u"]] == us, name
        assert _pt(row) == hh.map_to_curve(us), name
        assert row["zero"] == 0


def test_fixture_xof_and_scalar_rows_agree_with_the_restatement():
    k = hh.kat()
    for (name, msg, dst, n), row in zip(hh.xof_rows(), k["xof"]):
        assert bytes.fromhex(row["out"]) == hh.xof(msg, dst, n), name
    for (name, msg, dst), row, drow in zip(hh.scalar_rows(), k["scalar"], k["decaf_scalar"]):
        d = hh.SCALAR_DST if dst is None else dst
        assert int(row["out"], 16) == hh.hash_to_scalar(msg, d), name
        assert int(drow["out"], 16) == hh.decaf_hash_to_scalar(msg, d), name
    # the two compression lengths of an oversize DST differ: 56 bytes under k = 224, 64 under k = 256
    big = b"z" * 300
    assert hh.effective_dst(big, 224) == hashlib.shake_256(b"H2C-OVERSIZE-DST-" + big).digest(56)
    assert hh.effective_dst(big, 256) == hashlib.shake_256(b"H2C-OVERSIZE-DST-" + big).digest(64)
    assert hh.decaf_hash_to_scalar(b"abc", big) == int.from_bytes(hh.xof(b"abc", big, 64, 256), "little") % N


def test_fixture_map_rows_agree_with_the_restatement():
    k = hh.kat()
    for u, row in zip(hh.edge_us(), k["map"]):
        assert _pt(row) == hh.map_to_curve([u]) and row["zero"] == (1 if _pt(row) == (0, 1) else 0), u
    for (name, u), row in zip(hh.exception_us().items(), k["exceptions"]):
        assert hh.map_edwards448(u)[4] and _pt(row) == (0, 1) == hh.map_to_curve([u]) and row["zero"] == 1, name
    for u, h in zip(hh.seeded_us(), k["seeded_map"]):
        assert (int(h[:112], 16), int(h[112:], 16)) == hh.map_to_curve([u])
    # the fixture's pairs are mapToCurve(u0) + mapToCurve(u1) with the cofactor cleared on each: the same point as the tail's
    # 4 (Q0 + Q1); (u, p - u) is a doubling
    for (a, b), row in zip(hh.pair_rows(), k["pairs"]):
        assert _pt(row) == hh.map_to_curve([a, b]), (a, b)
    for a, b in hh.pair_rows()[:2]:
        assert hh.map_affine(a) == hh.map_affine(b)


def test_fixture_decaf_and_seeded_rows_agree_with_the_restatement():
    k = hh.kat()
    for (name, msg, dst), row in zip(hh.decaf_rows(), k["decaf"]):
        assert bytes.fromhex(row["out"]) == hh.decaf_hash_to_group(msg, dst), name
    for suite, count in (("ro", 2), ("nu", 1)):                                  # 128 seeded rows per suite, 8 DSTs each
        rows = [hh.seeded_row(suite, i) for i in range(hh.SEEDED)]
        assert len({d for _, d in rows}) == hh.SEEDED // hh.SEEDED_BATCH
        for i, ((msg, dst), want) in enumerate(zip(rows, hh.seeded_answers(suite))):
            assert hh.hash_to_curve(msg, dst, count) == want, (suite, i)
    for i, want in enumerate(hh.seeded_answers("decaf")):
        assert hh.decaf_hash_to_group(*hh.seeded_row("decaf", i)) == want, i
    for (a, b), want in zip(hh.seeded_pairs(), hh.seeded_pair_answers()):
        assert hh.map_to_curve([a, b]) == want


# ---------------------------------------------------------------- the CPU twins against the restatement
def test_twin_xof_against_hashlib():
    for name, msg, dst, n in hh.xof_rows():
        rc, got = hh.ht_xof(msg, hh.effective_dst(dst), n)
        assert rc == 0 and got == hh.xof(msg, dst, n), name
    for dst in (b"D", b"y" * 255):
        for r, n in zip((135, 136, 137), hh.boundary_lengths(dst)):
            msg = hh.seeded_bytes("twin-boundary", r, n)
            assert (len(msg) + 2 + len(dst) + 1) % 136 == r % 136
            for out_len in (1, 135, 136, 137, 272, 273):
                assert hh.ht_xof(msg, dst, out_len) == (0, hh.xof(msg, dst, out_len)), (len(dst), r, out_len)
    assert hh.ht_xof(b"", b"", 32)[0] == -1 and hh.ht_xof(b"", b"D", 65536)[0] == -1 and hh.ht_xof(b"", b"D", 0)[0] == -1


@pytest.mark.parametrize("op", range(hh.CHECK_OPS))
def test_twin_check_ops_against_the_restatement(op):
    vals, rows = hh.check_rows(op)
    for v, row in zip(vals, rows):
        rc, out = hh.ht_check(op, row)
        assert rc == 0 and hh.check_out_ints(op, out) == hh.check_expected(op, v), hex(v)
        assert not out[14 * hh.CHECK_OUT_ELEMS[op]:].any()


def test_twin_check_unknown_op():
    row = hh.check_row(0, 1)
    for op in (-1, hh.CHECK_OPS, 99):
        rc, out = hh.ht_check(op, row)
        assert rc == -1 and not out.any()


def test_twin_whole_rows():
    for name, msg, dst, count in hh.listed_rows():
        d = hh.effective_dst(dst)
        us = hh.hash_to_field(msg, dst, count)
        assert hh.ht_hash_to_field(msg, d, count) == us, name
        assert hh.ht_hash(msg, d, count) == hh.map_to_curve(us), name
    for name, msg, dst in hh.scalar_rows():
        dst = hh.SCALAR_DST if dst is None else dst
        assert hh.ht_hash_to_scalar(msg, hh.effective_dst(dst, 224)) == hh.hash_to_scalar(msg, dst), name
        assert hh.ht_decaf_hash_to_scalar(msg, hh.effective_dst(dst, 256)) == hh.decaf_hash_to_scalar(msg, dst), name
    for name, msg, dst in hh.decaf_rows():
        assert hh.ht_decaf_hash_to_group(msg, hh.effective_dst(dst)) == hh.decaf_hash_to_group(msg, dst), name
    for u in hh.edge_us() + list(hh.exception_us().values()) + hh.seeded_us()[:16]:
        assert hh.ht_map([u]) == hh.map_to_curve([u]), hex(u)
    for a, b in hh.pair_rows():
        assert hh.ht_map([a, b]) == hh.map_to_curve([a, b]), (a, b)


# ---------------------------------------------------------------- the Python layer with a fake engine
class FakeEngine:
    def __init__(self):
        self.calls = []

    def ed448_h2c_hash_batch(self, msgs, dst, count):
        self.calls.append(("hash", list(msgs), dst, count))
        out = np.zeros((len(msgs), 112), np.uint8)
        out[:, 0], out[:, 56] = 7, 9
        return out

    def ed448_h2c_map_batch(self, u56, count):
        self.calls.append(("map", np.array(u56), count))
        out = np.zeros((u56.shape[0], 112), np.uint8)
        out[:, 56] = 1
        return out

    def ed448_h2c_hash_to_scalar_batch(self, msgs, dst):
        self.calls.append(("scalar", list(msgs), dst))
        out = np.zeros((len(msgs), 56), np.uint8)
        out[:, 0] = 5
        return out

    def decaf448_hash_to_group_batch(self, msgs, dst):
        self.calls.append(("decaf", list(msgs), dst))
        return np.zeros((len(msgs), 56), np.uint8)

    def decaf448_hash_to_scalar_batch(self, msgs, dst):
        self.calls.append(("decaf_scalar", list(msgs), dst))
        out = np.zeros((len(msgs), 56), np.uint8)
        out[:, 0] = 6
        return out


def test_ed448_hasher_rules():
    eng = FakeEngine()
    h = GE._Ed448Hasher(engine=eng)
    k = hh.kat()
    err, ref = k["errors"], k["defaults"]
    assert isinstance(GE.ed448_hasher, GH.H2CDeviceHasher) and isinstance(GH.secp256k1_hasher, GH.H2CDeviceHasher) and h.Point is GE.ed448_Point and GE.ed448_Point.ZERO == (0, 1)
    d = h.defaults
    assert (d["DST"], d["encodeDST"], str(d["p"]), d["m"], d["k"], d["expand"]) == \
        (ref["DST"], ref["encodeDST"], ref["p"], ref["m"], ref["k"], ref["expand"]) == \
        (hh.RO.decode(), hh.NU.decode(), str(P), 1, 224, "xof")
    d["DST"] = "poisoned"
    assert h.defaults["DST"] == ref["DST"] and h.defaults is not h.defaults and k["defaults_is_copy"]
    assert h.hashToCurveBatch([b"a", b"", b"ccc"]) == [(7, 9)] * 3 and eng.calls == [("hash", [b"a", b"", b"ccc"], hh.RO, 2)]
    eng.calls.clear()
    h.encodeToCurve(bytearray(b"zz"))
    h.hashToCurve(b"m", {"DST": "custom"})
    h.hashToCurve(b"m", {"DST": b"custom", "p": 17, "m": 2, "hash": "md5"})     # only DST may be overridden
    assert eng.calls == [("hash", [b"zz"], hh.NU, 1)] + [("hash", [b"m"], b"custom", 2)] * 2
    eng.calls.clear()
    big = b"x" * 300                                                            # an oversize DST: SHAKE256 to 56 bytes (k = 224)
    h.hashToCurve(b"abc", {"DST": big})
    h.hashToScalar(b"abc", {"DST": big})
    assert [c[2] for c in eng.calls] == [hashlib.shake_256(b"H2C-OVERSIZE-DST-" + big).digest(56)] * 2
    h.hashToCurve(b"abc", {"DST": b"y" * 255})
    assert eng.calls[-1][2] == b"y" * 255
    eng.calls.clear()
    assert h.hashToScalarBatch([b"a", b"b"]) == [5, 5] and h.hashToScalar(b"a", {"DST": "T"}) == 5
    assert eng.calls == [("scalar", [b"a", b"b"], b"HashToScalar-"), ("scalar", [b"a"], b"T")]
    eng.calls.clear()
    zero = h.mapToCurveBatch([5, P + 6, 2**500])                                # reduced like Fp.create, one call
    assert len(eng.calls) == 1 and eng.calls[0][0] == "map" and eng.calls[0][2] == 1
    assert [int.from_bytes(bytes(r), "little") for r in eng.calls[0][1]] == [5, 6, 2**500 % P]
    assert all(z == h.Point.ZERO for z in zero)
    for bad in (5.0, True, [5], "5", None):
        with pytest.raises(ValueError) as e:
            h.mapToCurve(bad)
        assert str(e.value) == err["map_number"] == err["map_array"] == "expected bigint (m=1)"
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


def test_decaf448_device_hash_rules():
    eng, err = FakeEngine(), hh.kat()["errors"]
    big = b"w" * 300
    assert GD.hashToCurve_batch([b"a", bytearray(b"b")], engine=eng, device_hash=True) == [bytes(56)] * 2
    GD.hashToCurve_batch([b"a"], DST=big, engine=eng, device_hash=True)
    assert GD.hashToScalar_batch([b"a", b"b"], engine=eng) == [6, 6]
    assert GD.hashToScalar(b"a", DST=big, engine=eng, device_hash=True) == 6
    assert eng.calls == [("decaf", [b"a", b"b"], hh.DECAF_DST), ("decaf", [b"a"], hashlib.shake_256(b"H2C-OVERSIZE-DST-" + big).digest(56)),
                         ("decaf_scalar", [b"a", b"b"], b"HashToScalar-"),
                         ("decaf_scalar", [b"a"], hashlib.shake_256(b"H2C-OVERSIZE-DST-" + big).digest(64))]
    eng.calls.clear()
    assert GD.hashToScalar(b"abc") == hh.decaf_hash_to_scalar(b"abc") and GD.hashToScalar(b"abc", big) == hh.decaf_hash_to_scalar(b"abc", big)
    assert GD.hashToCurve_batch([], engine=eng, device_hash=True) == [] and GD.hashToScalar_batch([], engine=eng) == [] and not eng.calls
    for call in (lambda: GD.hashToCurve_batch([b"x"], DST="", engine=eng, device_hash=True), lambda: GD.hashToScalar_batch([b"x"], DST=b"", engine=eng),
                 lambda: GD.hashToScalar(b"x", DST="", engine=eng, device_hash=True)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == err["decaf_empty_dst"] == err["decaf_scalar_empty_dst"] == "DST must be non-empty"
    for call in (lambda: GD.hashToCurve_batch(["abc"], engine=eng, device_hash=True), lambda: GD.hashToScalar_batch([5], engine=eng)):
        with pytest.raises(TypeError) as e:
            call()
        assert str(e.value).startswith("expected Uint8Array, got type=")
    assert not eng.calls
