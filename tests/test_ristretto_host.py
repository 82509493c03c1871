"""ristretto255 on the CPU twins of csrc/ristretto.hip (the lane code the kernels run), against the reference's own answers
(tests/golden/ristretto255_kat.json) and the Python restatement of ristretto_helpers, bit for bit; the constants; the edge rows; the
argument checks and messages of the Python mirror."""
import numpy as np
import pytest

import ristretto_helpers as rh

P, L = rh.P, rh.L


def test_constants_against_the_reference_decimals():
    c = rh.kat()["constants"]
    want = [int(c[k]) for k in ("SQRT_AD_MINUS_ONE", "INVSQRT_A_MINUS_D", "ONE_MINUS_D_SQ", "D_MINUS_ONE_SQ")]
    assert rh.ht_consts() == want                                           # what the lane code holds (tools/gen_consts.py)
    assert [rh.SQRT_AD_MINUS_ONE, rh.INVSQRT_A_MINUS_D, rh.ONE_MINUS_D_SQ, rh.D_MINUS_ONE_SQ] == want


def test_decode_known_answers():
    rows = rh.kat()["decode"]
    out, ok = rh.ht_decode(rh.hex_rows([c["enc"] for c in rows]))
    for i, c in enumerate(rows):
        assert bool(ok[i]) == (c["error"] is None), c["name"]
        assert bytes(out[i]).hex() == rh.kat_affine(c), c["name"]
        d = rh.decode(bytes.fromhex(c["enc"]))                              # the restatement: value and the message
        assert (d if isinstance(d, str) else rh.wire([d])[0].tobytes().hex()) == (c["error"] or rh.kat_affine(c)), c["name"]
    assert sum(c["error"] == rh.ENC1 for c in rows) >= 12 and sum(c["error"] == rh.ENC2 for c in rows) >= 17
    assert sum(c["error"] is None for c in rows) >= 140 and sum(c["affine"] is not None for c in rows) >= 16 + rh.SEEDED_AFFINE


def test_encode_known_answers():
    rows = [c for c in rh.kat()["decode"] if c["error"] is None]
    pts = rh.hex_rows([rh.kat_affine(c) for c in rows], 64)
    assert [bytes(r).hex() for r in rh.ht_encode(pts)] == [c["bytes"] for c in rows]
    assert all(c["bytes"] == c["enc"] for c in rows)                        # fromBytes then toBytes is the identity map
    assert [rh.encode(rh.unwire(p)).hex() for p in pts[:40]] == [c["bytes"] for c in rows[:40]]
    small = rh.kat()["small_multiples"]
    assert small[1] == rh.kat()["base"] == rh.encode(rh.BASE).hex()
    assert [bytes(r).hex() for r in rh.ht_encode(rh.wire([(0, 1)] + rh.base_multiples(15)))] == small


def test_edge_encodings():
    edges = rh.edge_encodings()
    out, ok = rh.ht_decode(np.frombuffer(b"".join(e[1] for e in edges), np.uint8).reshape(-1, 32))
    want, want_ok = rh.expect_decode([e[1] for e in edges])
    assert np.array_equal(out, want) and np.array_equal(ok, want_ok)
    for (name, enc, verdict), o in zip(edges, ok):
        d = rh.decode(enc)
        assert (d if isinstance(d, str) else "ok") == verdict, name
        assert bool(o) == (verdict == "ok"), name
    assert rh.unwire(out[0]) == (0, 1)                                      # the identity decodes to (0, 1)


def test_random_rows_mixed():
    raw, (want, want_ok) = rh.mixed_encodings(512, "host")
    out, ok = rh.ht_decode(raw)
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)
    assert 200 < ok.sum() < 400                                             # both verdicts occur
    enc = rh.ht_encode(out[ok == 1])
    assert np.array_equal(enc, raw[ok == 1])


def test_torsion_cosets_encode_alike_and_equal():
    base = rh.base_multiples(64)
    assert 16 <= sum(rh.rotates(*p) for p in base) <= 48                    # both sides of the rotation are driven (30 of these 64)
    want = rh.ht_encode(rh.wire(base))
    assert [bytes(r) for r in want] == [rh.encode(p) for p in base]
    for t in rh.TORSION4:
        shifted = [rh.add(p, t) for p in base]
        assert np.array_equal(rh.ht_encode(rh.wire(shifted)), want)
        assert rh.ht_equals(rh.wire(base), rh.wire(shifted)).all()
    # the second clause of equals alone: P against P + (a point of order 4)
    for p in base[:8]:
        q = rh.add(p, rh.TORSION4[2])
        assert p[0] * q[1] % P != p[1] * q[0] % P and p[1] * q[1] % P == p[0] * q[0] % P
    dbl = [rh.add(p, p) for p in base]
    assert not rh.ht_equals(rh.wire(base), rh.wire(dbl)).any()
    assert not rh.ht_encode(rh.wire(rh.TORSION4)).any()                     # the four points of the identity's coset: 32 zero bytes
    # rows P + (a point of order 8): not the same element; against the restatement only
    t8 = rh.order8_point()
    odd = [rh.add(p, t8) for p in base[:16]]
    got = rh.ht_encode(rh.wire(odd))
    assert [bytes(r) for r in got] == [rh.encode(p) for p in odd]
    assert not (got == want[:16]).all(axis=1).any()


def test_encode_proj_matches_affine():
    base = rh.base_multiples(64) + rh.TORSION4
    rng = np.random.RandomState(7)
    rows = []
    for x, y in base:
        z = int.from_bytes(rng.bytes(32), "little") % (P - 1) + 1
        rows.append(b"".join(v.to_bytes(32, "little") for v in (x * z % P, y * z % P, z)))
    got = rh.ht_encode_proj(np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 96))
    assert np.array_equal(got, rh.ht_encode(rh.wire(base)))


def test_from_uniform_known_answers_and_edges():
    rows = rh.kat()["derive"]
    b = rh.hex_rows([c["in"] for c in rows], 64)
    out, aff = rh.ht_from_uniform(b, affine=True)
    assert [bytes(r).hex() for r in out] == [c["out"] for c in rows]
    assert np.array_equal(rh.ht_from_uniform(b), out)
    assert [bytes(r).hex() for r in rh.ht_encode(aff)] == [c["out"] for c in rows]
    for i in range(0, len(rows), 9):                                       # the representative itself, against the restatement
        assert rh.unwire(aff[i]) == rh.to_affine(rh.derive(bytes(b[i]))), i
    assert [rh.derive_bytes(bytes(r)).hex() for r in b[:40]] == [c["out"] for c in rows[:40]]
    import hashlib
    for c in rh.kat()["labels"]:
        assert rh.derive_bytes(hashlib.sha512(c["label"].encode()).digest()).hex() == c["out"]
    edges = rh.edge_uniform()
    got = rh.ht_from_uniform(np.frombuffer(b"".join(e[1] for e in edges), np.uint8).reshape(-1, 64))
    assert [bytes(r) for r in got] == [rh.derive_bytes(e[1]) for e in edges]
    assert not got[0].any()                                                 # both halves zero: the identity
    assert np.array_equal(got[2], got[3])                                   # bit 255 of a half is masked
    # both branches of the square test within the first 20 random rows
    sq = [rh.elligator(rh.half255(bytes(r[:32])))[1] for r in b[18:38]]
    assert any(sq) and not all(sq)


def test_hash_to_curve_rows_through_the_restatement_and_the_twin():
    rows = rh.kat()["hash"]
    xmd = [rh.expand_message_xmd(bytes.fromhex(c["msg"]), rh.DEFAULT_DST if c["dst"] is None else bytes.fromhex(c["dst"])) for c in rows[:-1]]
    got = rh.ht_from_uniform(np.frombuffer(b"".join(xmd), np.uint8).reshape(-1, 64))
    assert [bytes(r).hex() for r in got] == [c["out"] for c in rows[:-1]]


def test_multiply_known_answers_and_the_one_scalar_flag():
    rows = [c for c in rh.kat()["multiply"] if c["error"] is None]
    enc, ks = rh.hex_rows([c["enc"] for c in rows]), rh.scalars_le([int(c["k"]) for c in rows])
    out, ok = rh.ht_mul(enc, ks)
    assert ok.all() and [bytes(r).hex() for r in out] == [c["out"] for c in rows]
    assert {int(c["k"]) for c in rows} >= {1, 2, L - 1}
    bad = [c for c in rh.kat()["multiply"] if c["error"] in (rh.ENC1, rh.ENC2)]
    assert len(bad) == 2
    mixed = np.concatenate([enc[:3], rh.hex_rows([c["enc"] for c in bad]), enc[3:6]])
    k = ks[5:6]
    per_row = rh.ht_mul(mixed, np.repeat(k, 8, axis=0))
    flagged = rh.ht_mul(mixed, k, flags=1)
    assert np.array_equal(per_row[0], flagged[0]) and np.array_equal(per_row[1], flagged[1])
    assert list(flagged[1]) == [1, 1, 1, 0, 0, 1, 1, 1] and not flagged[0][3:5].any() and flagged[0][[0, 1, 2, 5, 6, 7]].any(axis=1).all()
    assert rh.ht().ht_ristretto_mul(mixed.ctypes.data, k.ctypes.data, 2, mixed.ctypes.data, mixed.ctypes.data, 1) == -1
    # k = 0 and k = L give the identity on the device path (the reference's range check is the mirror's)
    out, ok = rh.ht_mul(enc[:2], rh.scalars_le([0, L]))
    assert ok.all() and not out.any()
    assert [c["out"] for c in rh.kat()["equals"]] == [rh.equals(rh.decode(bytes.fromhex(c["a"])), rh.decode(bytes.fromhex(c["b"])))
                                                      for c in rh.kat()["equals"]]


@pytest.mark.parametrize("op", [0, 1, 2])
def test_pieces_on_raw_limbs(op):
    a, b = rh.op_rows(op)
    rh.check_op(op, a, b, rh.ht_op(op, a, b))


def test_unknown_piece():
    z = np.zeros(36, np.uint32)
    assert rh.ht().ht_ristretto_op(3, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -1


# ---------------------------------------------------------------- the Python mirror, the library calls stubbed by the host twin
class TwinEngine:
    """the engine methods noble_curves_amd.ristretto255 uses, on the CPU twins"""

    def ristretto_decode_batch(self, enc):
        out, ok = rh.ht_decode(enc)
        return out, ok.astype(bool)

    def ristretto_encode_batch(self, pts):
        return rh.ht_encode(pts)

    def ristretto_equals_batch(self, a, b):
        return rh.ht_equals(a, b).astype(bool)

    def ristretto_from_uniform_batch(self, b64, want_affine=False):
        if want_affine:
            return rh.ht_from_uniform(b64, affine=True)
        return rh.ht_from_uniform(b64), None

    def ristretto_mul_batch(self, enc, scalars, one_scalar=False):
        out, ok = rh.ht_mul(enc, scalars, 1 if one_scalar else 0)
        return out, ok.astype(bool)

    def ristretto_mul_base_batch(self, scalars):
        n = np.ascontiguousarray(scalars).reshape(-1, 32).shape[0]
        base = np.repeat(np.frombuffer(rh.encode(rh.BASE), np.uint8).reshape(1, 32), n, axis=0)
        return rh.ht_mul(base, scalars)[0]

    def ristretto_msm(self, enc, scalars):
        enc, scalars = np.ascontiguousarray(enc).reshape(-1, 32), np.ascontiguousarray(scalars).reshape(-1, 32)
        acc = (0, 1)
        for e, k in zip(enc, scalars):
            d = rh.decode(bytes(e))
            assert not isinstance(d, str)
            acc = rh.add(acc, rh.mul(d, int.from_bytes(bytes(k), "little")))
        return np.frombuffer(rh.encode(acc), np.uint8)

    def add_pairs_batch(self, curve, a, b, subtract=False):
        assert curve == 1
        out = [rh.add(rh.unwire(x), rh.unwire(y) if not subtract else ((P - rh.unwire(y)[0]) % P, rh.unwire(y)[1])) for x, y in zip(a, b)]
        return rh.wire(out), np.array([p == (0, 1) for p in out])


def _raises(exc, msg, f, *a, **kw):
    with pytest.raises(exc) as e:
        f(*a, engine=TwinEngine(), **kw)
    assert str(e.value) == msg, str(e.value)


def test_mirror_values():
    from noble_curves_amd import ristretto255 as r
    eng, k = TwinEngine(), rh.kat()
    Pt = r.Point
    assert Pt.BASE.toBytes(engine=eng).hex() == k["base"] and Pt.ZERO.toBytes(engine=eng) == bytes(32)
    small = k["small_multiples"]
    acc = Pt.ZERO
    for h in small[:6]:
        assert acc.toBytes(engine=eng).hex() == h and Pt.fromHex(h, engine=eng).equals(acc, engine=eng)
        acc = acc.add(Pt.BASE, engine=eng)
    assert Pt.ZERO.is0(engine=eng) and not Pt.BASE.is0(engine=eng)
    rows = k["decode"][:80]
    pts, ok = r.fromBytes_batch([bytes.fromhex(c["enc"]) for c in rows], engine=eng)
    assert ok == [c["error"] is None for c in rows] and [p is not None for p in pts] == ok
    good = [p for p in pts if p is not None]
    assert [b.hex() for b in r.toBytes_batch(good, engine=eng)] == [c["bytes"] for c in rows if c["error"] is None]
    assert all(r.equals_batch(good, good, engine=eng))
    mrows = [c for c in k["multiply"] if c["error"] is None]
    got, ok = r.multiply_batch([bytes.fromhex(c["enc"]) for c in mrows], [int(c["k"]) for c in mrows], engine=eng)
    assert [g.hex() for g in got] == [c["out"] for c in mrows] and all(ok)
    one, ok = r.multiply_batch([bytes.fromhex(c["enc"]) for c in mrows[:5]], int(mrows[3]["k"]), engine=eng)
    assert one[3].hex() == mrows[3]["out"]
    assert Pt.fromHex(mrows[1]["enc"], engine=eng).multiply(int(mrows[1]["k"]), engine=eng).toBytes(engine=eng).hex() == mrows[1]["out"]
    assert r.multiplyBase_batch([1, 2, 5], engine=eng) == [bytes.fromhex(small[i]) for i in (1, 2, 5)]
    assert r.msm([bytes.fromhex(small[2]), bytes.fromhex(small[3])], [3, 2], engine=eng).hex() == small[12]
    hrows = k["hash"]
    assert [b.hex() for b in r.hashToCurve_batch([bytes.fromhex(c["msg"]) for c in hrows[:20]], engine=eng)] == [c["out"] for c in hrows[:20]]
    c = hrows[300]
    assert r.hashToCurve(bytes.fromhex(c["msg"]), DST=bytes.fromhex(c["dst"]), engine=eng).toBytes(engine=eng).hex() == c["out"]
    c = hrows[-1]                                                           # an oversize DST is hashed first
    assert r.hashToCurve(bytes.fromhex(c["msg"]), DST=bytes.fromhex(c["dst"]), engine=eng).toBytes(engine=eng).hex() == c["out"]
    d = k["derive"][3]
    assert r.deriveToCurve(bytes.fromhex(d["in"]), engine=eng).toBytes(engine=eng).hex() == d["out"]
    assert [b.hex() for b in r.deriveToCurve_batch([bytes.fromhex(x["in"]) for x in k["derive"][:12]], engine=eng)] == \
        [x["out"] for x in k["derive"][:12]]


def test_mirror_errors():
    from noble_curves_amd import ristretto255 as r
    e, k = rh.kat()["errors"], rh.kat()
    Pt = r.Point
    for c in k["decode"]:
        if c["error"] is not None and not c["name"].startswith("random"):
            _raises(ValueError, c["error"], Pt.fromBytes, bytes.fromhex(c["enc"]))
    _raises(ValueError, e["length"], Pt.fromBytes, bytes(31))
    with pytest.raises(TypeError) as t:
        Pt.fromBytes("x", engine=TwinEngine())
    assert e["type"].endswith("got type=string") and "got type=str" in str(t.value)
    _raises(ValueError, e["derive_length"], r.deriveToCurve, bytes(63))
    _raises(ValueError, e["empty_dst"], r.hashToCurve, b"m", DST=b"")
    _raises(ValueError, e["multiply_zero"], Pt.BASE.multiply, 0)
    _raises(ValueError, e["multiply_order"], Pt.BASE.multiply, L)
    _raises(ValueError, e["multiply_zero"], r.multiply_batch, [bytes(32)], [0])
    _raises(ValueError, e["multiply_order"], r.multiplyBase_batch, [L])
    _raises(ValueError, e["hex_odd"], Pt.fromHex, "abc")
    _raises(ValueError, "arrays of points and scalars must have equal length", r.multiply_batch, [bytes(32)], [1, 2])
    assert r.fromBytes_batch([], engine=TwinEngine()) == ([], [])
