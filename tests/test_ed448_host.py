"""X448 and Ed448 on the CPU twins of csrc/ed448.hip (the lane code the kernels run), against the reference's own answers
(tests/golden/ed448_kat.json, ed448_wycheproof_old.json) and the Python restatement of ed448_helpers; the restatement against
the fixture; the raw-limb rows of every ncg_fe448_check op; and the argument checks of the Python mirror."""
import numpy as np
import pytest

import ed448_helpers as eh

ENG = eh.TwinEngine()


def _hex(rows):
    return [bytes(r).hex() for r in rows]


# ---------------------------------------------------------------- the restatement against the fixture
def test_restatement_reproduces_the_fixture():
    k = eh.kat()
    for c in k["scalar_mult"]:
        r = eh.scalar_mult(bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"]))
        assert (r.hex() if r else None) == c["out"], c["name"]
    for c in k["points"]:
        p = eh.pt_decode(bytes.fromhex(c["enc"]))
        if c["error"] is None:
            assert p == (int(c["x"], 16), int(c["y"], 16)) and eh.on_curve(p) and eh.pt_encode(p).hex() == c["enc"], c["name"]
        else:
            assert isinstance(p, str) and p in c["error"], (c["name"], p, c["error"])
    for c in k["to_montgomery"]:
        r = eh.to_montgomery(bytes.fromhex(c["publicKey"]))
        assert (r.hex() if r else None) == c["out"], c["name"]
    for c in k["ed_public_keys"]:
        assert eh.public_key(bytes.fromhex(c["secretKey"])).hex() == c["out"]
    for c in k["signatures"]:
        ctx = bytes.fromhex(c["context"] or "")
        assert eh.sign(bytes.fromhex(c["msg"]), bytes.fromhex(c["seed"]), ctx, c["ph"]).hex() == c["sig"]
        assert eh.public_key(bytes.fromhex(c["seed"])).hex() == c["publicKey"]
    for c in k["to_montgomery_secret"]:
        assert eh.to_montgomery_secret(bytes.fromhex(c["secretKey"])).hex() == c["out"]
    for c in k["public_keys"]:
        assert eh.scalar_mult(bytes.fromhex(c["scalar"]), eh.le56(5)).hex() == c["out"]
    x = u = eh.le56(5)
    for i in range(1, 1001):
        x, u = eh.scalar_mult(x, u), x
        assert str(i) not in k["iterated"] or x.hex() == k["iterated"][str(i)], i
    assert [eh.pt_encode(t).hex() for t in eh.TORSION] == [k["torsion"][0], k["torsion"][1], k["torsion"][3], k["torsion"][2]]
    assert all(eh.is_small_order(t) for t in eh.TORSION) and not eh.is_small_order(eh.BASE)
    assert eh.pt_mul(eh.BASE, eh.N) == eh.IDENTITY and eh.on_curve(eh.BASE)
    for v in eh.LOW_ORDER:
        assert eh.ladder(v, eh.clamp(b"\x55" * 56)) == 0


def _fixture_verify_rows():
    k = eh.kat()
    out = []
    for c in k["verify"]:
        base = k["signatures"][c["row"]]
        msg = bytes.fromhex(base["msg"] if c["msg"] is None else c["msg"])
        out.append((bytes.fromhex(base["sig"]), msg, bytes.fromhex(base["publicKey"]), bytes.fromhex(c["context"] or ""), c["ph"], c["ok"]))
    return out


def _wycheproof_rows():
    out = []
    for g in eh.wycheproof()["testGroups"]:
        pk = bytes.fromhex(g["key"]["pk"])
        for t in g["tests"]:
            out.append((bytes.fromhex(t["sig"]), bytes.fromhex(t["msg"]), pk, t["result"] == "valid"))
    return out


def test_restatement_verifies_like_the_reference():
    for sig, msg, pk, ctx, ph, ok in _fixture_verify_rows():
        assert eh.verify(sig, msg, pk, ctx, ph) == ok
    for sig, msg, pk, ok in _wycheproof_rows():
        assert (len(sig) == 114 and eh.verify(sig, msg, pk)) == ok


# ---------------------------------------------------------------- X448
def test_scalar_mult_known_answers():
    rows = eh.kat()["scalar_mult"]
    want, want_ok = eh.kat_expected(rows)
    out, ok = ENG.x448_batch(eh.hex_rows([c["scalar"] for c in rows]), eh.hex_rows([c["u"] for c in rows]))
    assert np.array_equal(ok, want_ok.astype(bool)) and np.array_equal(out, want)
    assert {c["error"] for c in rows if c["out"] is None} == {eh.INVALID}
    assert sum(c["out"] is None for c in rows) == 5          # 0, 1, p - 1, p, p + 1


def test_random_rows_against_the_ladder_and_one_scalar():
    s, u = eh.rand_rows(96, "host-s"), eh.rand_rows(96, "host-u")
    u[7] = 0
    u[9] = np.frombuffer(eh.le56(eh.P + 1), np.uint8)
    want, want_ok = eh.expect_x448(s, u)
    out, ok = ENG.x448_batch(s, u)
    assert np.array_equal(ok, want_ok.astype(bool)) and np.array_equal(out, want) and ok.sum() == 94
    flagged = ENG.x448_batch(s[:1], u, one_scalar=True)
    per_row = ENG.x448_batch(np.repeat(s[:1], 96, axis=0), u)
    assert np.array_equal(per_row[0], flagged[0]) and np.array_equal(per_row[1], flagged[1])
    assert eh.ht().ht_x448(s.ctypes.data, u.ctypes.data, 2, u.ctypes.data, u.ctypes.data, 1) == -1


def test_iterated_to_1000():
    it = eh.kat()["iterated"]
    k = u = eh.le56(5)
    for i in range(1, 1001):
        out, ok = ENG.x448_batch(eh.rows([k], 56), eh.rows([u], 56))
        assert ok[0]
        k, u = bytes(out[0]), k
        if str(i) in it:
            assert k.hex() == it[str(i)], i


def test_base_against_the_ladder_at_five_and_the_edwards_route():
    rows = eh.kat()["public_keys"]
    want, want_ok = eh.kat_expected(rows)
    s = eh.hex_rows([c["scalar"] for c in rows])
    out, ok = ENG.x448_base_batch(s)
    assert np.array_equal(ok, want_ok.astype(bool)) and np.array_equal(out, want) and ok.all()
    # the reference's Edwards hook: u = y^2 / x^2 of [clamp(s)]B
    clamped = eh.rows([eh.le56(eh.clamp(bytes(r))) for r in s[:6]], 56)
    mont, mok = ENG.ed448_to_montgomery_batch(ENG.ed448_mul_base_batch(clamped))
    assert mok.all() and np.array_equal(mont, out[:6])


# ---------------------------------------------------------------- Ed448 codecs, group law, multiply
def test_decode_known_answers_edges_and_round_trip():
    pts = eh.kat()["points"]
    enc = [bytes.fromhex(c["enc"]) for c in pts] + eh.decode_edge_rows()
    aff, ok = ENG.ed448_decode_batch(eh.rows(enc, 57))
    for i, e in enumerate(enc):
        w = eh.pt_decode(e)
        assert ok[i] == (not isinstance(w, str)), i
        assert bytes(aff[i]) == (bytes(112) if isinstance(w, str) else eh.le56(w[0]) + eh.le56(w[1])), i
    assert [bool(x) for x in ok[:len(pts)]] == [c["error"] is None for c in pts]
    good = eh.rows([e for i, e in enumerate(enc) if ok[i]], 57)
    assert np.array_equal(ENG.ed448_encode_batch(ENG.ed448_decode_batch(good)[0]), good)
    assert (~ok).sum() >= 15


def test_add_pairs_every_edge_pair():
    pts = eh.edge_points()
    pa, pb = [p for p in pts for q in pts], [q for p in pts for q in pts]
    got = ENG.ed448_add_pairs_batch(eh.affine_rows(pa), eh.affine_rows(pb))
    assert np.array_equal(got, eh.affine_rows([eh.pt_add(p, q) for p, q in zip(pa, pb)]))
    got = ENG.ed448_add_pairs_batch(eh.affine_rows(pa), eh.affine_rows(pb), True)
    assert np.array_equal(got, eh.affine_rows([eh.pt_add(p, eh.pt_neg(q)) for p, q in zip(pa, pb)]))


def test_multiply_edge_points_and_scalars():
    pk = [(p, k) for p in eh.edge_points() for k in eh.EDGE_SCALARS]
    got, ok = ENG.ed448_mul_batch(eh.rows([eh.pt_encode(p) for p, k in pk], 57), eh.rows([eh.le56(k) for p, k in pk], 56))
    assert ok.all() and _hex(got) == [eh.pt_encode(eh.pt_mul(p, k)).hex() for p, k in pk]
    ks = eh.rand_rows(6, "k")
    base = eh.rows([eh.pt_encode(eh.BASE)] * 6, 57)
    gb = ENG.ed448_mul_base_batch(ks)
    assert _hex(gb) == [eh.pt_encode(eh.pt_mul(eh.BASE, int.from_bytes(bytes(k), "little"))).hex() for k in ks]
    assert np.array_equal(ENG.ed448_mul_batch(base, ks)[0], gb)
    assert np.array_equal(ENG.ed448_mul_batch(base, ks[:1], one_scalar=True)[0], np.repeat(gb[:1], 6, axis=0))
    bad, bok = ENG.ed448_mul_batch(eh.rows([eh.P.to_bytes(57, "little")], 57), ks[:1])
    assert not bok[0] and not bad.any()
    keys = eh.kat()["ed_public_keys"][:4]
    heads = [eh.le56(eh.secret_scalar(bytes.fromhex(c["secretKey"]))[0]) for c in keys]
    assert _hex(ENG.ed448_mul_base_batch(eh.rows(heads, 56))) == [c["out"] for c in keys]


def test_to_montgomery_known_answers_and_rejections():
    rows = eh.kat()["to_montgomery"]
    want, want_ok = eh.kat_expected(rows)
    out, ok = ENG.ed448_to_montgomery_batch(eh.hex_rows([c["publicKey"] for c in rows], 57))
    assert np.array_equal(ok, want_ok.astype(bool)) and np.array_equal(out, want)
    assert (want_ok == 0).sum() == 11


# ---------------------------------------------------------------- verification
def test_verify_rules():
    sig, pk, k, want = eh.verify_arrays(len(eh.verify_rows()))
    got = ENG.ed448_verify_batch(sig, pk, k)
    assert np.array_equal(got, want.astype(bool)) and got.any() and not got.all()


def test_verify_reference_rows_and_wycheproof():
    rows = [(s, p, eh.challenge(s[:57], p, m, c, ph) % eh.N, ok) for s, m, p, c, ph, ok in _fixture_verify_rows()]
    rows += [(s, p, eh.challenge(s[:57], p, m) % eh.N, ok) for s, m, p, ok in _wycheproof_rows() if len(s) == 114]
    got = ENG.ed448_verify_batch(eh.rows([r[0] for r in rows], 114), eh.rows([r[1] for r in rows], 57), eh.rows([eh.le56(r[2]) for r in rows], 56))
    assert [bool(x) for x in got] == [r[3] for r in rows]
    assert got.any() and not got.all() and len(rows) > 50


# ---------------------------------------------------------------- the pieces on raw limbs
@pytest.mark.parametrize("op,variant", [(op, 0) for op in range(11)] + [(8, 1)])
def test_fe448_op_on_raw_limbs(op, variant):
    a, b = eh.fe448_rows(op, 256)
    eh.check_fe448(op, variant, a, b, eh.ht_op(op, variant, a, b))


def test_fe448_op_table_and_unknown_ops():
    from noble_curves_amd._native import FE448_CHECK_WORDS
    import ctypes
    assert FE448_CHECK_WORDS == {op: v[:3] for op, v in eh.FE448_OPS.items()}
    for op in list(range(-1, 13)):
        w = [ctypes.c_int(-1) for _ in range(3)]
        eh.ht().ht_fe448_widths(op, *[ctypes.byref(x) for x in w])
        assert tuple(x.value for x in w) == FE448_CHECK_WORDS.get(op, (0, 0, 0)), op
    z = np.zeros(64, np.uint32)
    assert eh.ht().ht_fe448_op(11, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -1
    a, b = eh.fe448_rows(8, 4)
    assert np.array_equal(eh.ht_op(8, 3, a, b), eh.ht_op(8, 1, a, b))      # the upper variant bits are ignored


# ---------------------------------------------------------------- the Python mirror, the library calls stubbed by the host twin
def _raises(exc, msg, f, *a, **kw):
    with pytest.raises(exc) as e:
        f(*a, engine=ENG, **kw)
    assert str(e.value) == msg, str(e.value)


def test_mirror_x448():
    from noble_curves_amd.ed448 import x448
    k = eh.kat()
    assert x448.GuBytes == eh.le56(5)
    rows = k["scalar_mult"]
    got, ok = x448.scalarMult_batch([bytes.fromhex(c["scalar"]) for c in rows], [bytes.fromhex(c["u"]) for c in rows], engine=ENG)
    assert [g.hex() if g else None for g in got] == [c["out"] for c in rows] and ok == [c["out"] is not None for c in rows]
    alice, bob = (bytes.fromhex(c["scalar"]) for c in k["public_keys"][:2])
    apub, bpub = x448.getPublicKey(alice, engine=ENG), x448.getPublicKey(bob, engine=ENG)
    assert [apub.hex(), bpub.hex()] == [c["out"] for c in k["public_keys"][:2]]
    assert x448.getSharedSecret(alice, bpub, engine=ENG) == x448.scalarMult(bob, apub, engine=ENG) == bytes.fromhex(k["scalar_mult"][2]["out"])
    many, ok = x448.getSharedSecret_batch(alice, [bpub, apub, bytes(56)], engine=ENG)
    assert many[0] == x448.getSharedSecret(alice, bpub, engine=ENG) and many[2] is None and ok == [True, True, False]
    assert x448.getPublicKey_batch([alice, bob], engine=ENG)[0] == [apub, bpub]
    e = k["errors"]
    good = b"\x01" * 56
    _raises(ValueError, e["u_length"], x448.scalarMult, good, bytes(55))
    _raises(ValueError, e["scalar_length"], x448.scalarMult, bytes(57), x448.GuBytes)
    _raises(ValueError, e["both_bad"], x448.scalarMult, bytes(57), bytes(55))
    _raises(ValueError, e["low_order_before_scalar"], x448.scalarMult, bytes(57), bytes(56))
    _raises(ValueError, e["public_key_length"], x448.getPublicKey, bytes(55))
    _raises(ValueError, eh.INVALID, x448.getSharedSecret, good, eh.le56(eh.P + 1))
    _raises(TypeError, e["u_type"], x448.scalarMult, good, "x")
    _raises(ValueError, "arrays of scalars and u coordinates must have equal length", x448.scalarMult_batch, [good], [good, good])
    assert x448.scalarMult_batch([], [], engine=ENG) == ([], [])


def test_mirror_ed448():
    from noble_curves_amd import ed448 as m
    k = eh.kat()
    assert list(m.ED448_TORSION_SUBGROUP) == k["torsion"]
    for lib, ph in ((m.ed448, False), (m.ed448ph, True)):
        rows = [r for r in _fixture_verify_rows() if r[4] == ph]
        by_ctx = {}
        for r in rows:
            by_ctx.setdefault(r[3], []).append(r)
        for ctx, rs in by_ctx.items():
            assert lib.verify_batch([r[0] for r in rs], [r[1] for r in rs], [r[2] for r in rs], context=ctx, engine=ENG) == [r[5] for r in rs]
    sig, msg, pk = _fixture_verify_rows()[0][:3]
    assert m.ed448.verify(sig, msg, pk, engine=ENG) is True and m.ed448.verify(sig, msg + b"!", pk, engine=ENG) is False
    assert m.ed448.verify(sig, msg, pk, context=b"c", engine=ENG) is False
    keys = k["ed_public_keys"]
    assert [x.hex() for x in m.ed448.getPublicKey_batch([bytes.fromhex(c["secretKey"]) for c in keys], engine=ENG)] == [c["out"] for c in keys]
    for c in k["to_montgomery_secret"]:
        assert m.ed448.utils.toMontgomerySecret(bytes.fromhex(c["secretKey"])).hex() == c["out"]
    rows = k["to_montgomery"]
    got, ok = m.ed448.utils.toMontgomery_batch([bytes.fromhex(c["publicKey"]) for c in rows], engine=ENG)
    assert [g.hex() if g else None for g in got] == [c["out"] for c in rows]
    for c in rows:
        if c["out"] is None:
            _raises(ValueError, c["error"], m.ed448.utils.toMontgomery, bytes.fromhex(c["publicKey"]))
    e = k["errors"]
    _raises(ValueError, e["signature_length"], m.ed448.verify, bytes(113), b"\0", pk)
    _raises(ValueError, e["verify_public_key_length"], m.ed448.verify, sig, b"\0", bytes(56))
    _raises(TypeError, e["message_type"], m.ed448.verify, sig, "x", pk)
    # the context is looked at only by a row that got past decoding, s < n and the small-order test (edwards.ts:964-984)
    long_ctx, n57 = bytes(256), eh.N.to_bytes(57, "little")
    for bad_sig, bad_pk in ((sig, eh.P.to_bytes(57, "little")), (eh.P.to_bytes(57, "little") + sig[57:], pk), (sig[:57] + n57, pk),
                            (sig, bytes.fromhex(k["torsion"][2]))):
        assert m.ed448.verify(bad_sig, msg, bad_pk, context=long_ctx, engine=ENG) is False
    _raises(ValueError, e["context_too_long"], m.ed448.verify, sig, b"\0", pk, context=bytes(256))
    _raises(ValueError, "ed448: zip215 is not supported", m.ed448.verify, sig, msg, pk, zip215=True)
    _raises(ValueError, e["secret_key_length"], m.ed448.getPublicKey, bytes(56))
    with pytest.raises(ValueError) as err:
        m.ed448.utils.toMontgomerySecret(bytes(56))
    assert str(err.value) == e["to_montgomery_secret_length"]
    for sg, ms, pk2, ok2 in _wycheproof_rows():
        if len(sg) != 114:
            with pytest.raises(ValueError):
                m.ed448.verify(sg, ms, pk2, engine=ENG)


def test_mirror_point():
    from noble_curves_amd.ed448 import ed448_Point as pt
    k = eh.kat()
    pts = k["points"]
    got, ok = pt.fromBytes_batch([bytes.fromhex(c["enc"]) for c in pts], engine=ENG)
    assert ok == [c["error"] is None for c in pts]
    assert [g for g in got if g] == [(int(c["x"], 16), int(c["y"], 16)) for c in pts if c["error"] is None]
    for c in pts:
        if c["error"]:
            _raises(ValueError, c["error"], pt.fromBytes, bytes.fromhex(c["enc"]))
    assert [b.hex() for b in pt.toBytes_batch([g for g in got if g], engine=ENG)] == [c["enc"] for c in pts if c["error"] is None]
    g = eh.pt_encode(eh.BASE)
    assert pt.multiplyBase_batch([1, 2, eh.N - 1], engine=ENG) == pt.multiplyUnsafe_batch([g] * 3, [1, 2, eh.N - 1], engine=ENG)[0]
    assert pt.multiplyUnsafe_batch([g, g], 0, engine=ENG)[0] == [eh.pt_encode(eh.IDENTITY)] * 2
    assert pt.add_batch([g, g, eh.P.to_bytes(57, "little")], [g, eh.pt_encode(eh.pt_neg(eh.BASE)), g], engine=ENG) == \
        ([eh.pt_encode(eh.pt_mul(eh.BASE, 2)), eh.pt_encode(eh.IDENTITY), None], [True, True, False])
    e = k["errors"]
    _raises(ValueError, e["multiply_zero"], pt.multiply_batch, [g], [0])
    _raises(ValueError, e["multiply_n"], pt.multiplyBase_batch, [eh.N])
    _raises(ValueError, e["multiply_unsafe_n"], pt.multiplyUnsafe_batch, [g], [eh.N])
    _raises(ValueError, e["point_length"], pt.fromBytes_batch, [bytes(56)])
