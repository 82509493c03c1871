"""decaf448 WITHOUT a GPU: the Python restatement of decaf448_helpers against the reference's own answers
(tests/golden/decaf448_kat.json), the CPU twins of the lane code (csrc/decaf448.hpp through hosttest.hip) against both, bit for bit,
and the argument errors of the Python shim running on the twins."""
import random

import numpy as np
import pytest

import decaf448_helpers as dh
import ed448_helpers as eh

ENG = dh.TwinEngine()
P, N = dh.P, dh.N


# ---------------------------------------------------------------- the restatement against the fixture
def test_constants_as_generated_and_as_the_lane_code_holds_them():
    c = dh.kat()["consts"]
    assert dh.SQRT_MINUS_D == int(c["sqrt_minus_d"]) and dh.INVSQRT_MINUS_D == int(c["invsqrt_minus_d"])
    assert dh.ONE_MINUS_D == int(c["one_minus_d"]) == (1 - dh.D) % P and dh.ONE_MINUS_TWO_D == int(c["one_minus_two_d"]) == (1 - 2 * dh.D) % P
    base = (int(dh.kat()["base"]["x"], 16), int(dh.kat()["base"]["y"], 16))
    assert base == dh.BASE and (int(dh.kat()["ed_base"]["x"], 16), int(dh.kat()["ed_base"]["y"], 16)) == eh.BASE
    assert dh.ht_consts() == [dh.ONE_MINUS_D, dh.ONE_MINUS_TWO_D, dh.SQRT_MINUS_D, dh.INVSQRT_MINUS_D, base[0], base[1]]
    from noble_curves_amd import decaf448 as m
    assert m.Point.BASE.toAffine() == base and m.Point.ZERO.toAffine() == (0, 1)


def test_restatement_reproduces_the_fixture():
    k = dh.kat()
    for kk, enc, p in dh.multiples():
        assert eh.pt_mul(dh.BASE, kk) == p and dh.encode(p) == enc and dh.decode(enc) != dh.ENC2, kk
    assert [c["enc"] for c in k["multiples"][:2]] == ["00" * 56, "66" * 28 + "33" * 28]
    rejected = 0
    for c in k["decode"]:
        got = dh.decode(bytes.fromhex(c["enc"]))
        if c["error"]:
            assert got == c["error"], c["name"]
            rejected += 1
        else:
            assert got == (int(c["x"], 16), int(c["y"], 16)) and dh.encode(got).hex() == c["enc"], c["name"]
    assert rejected >= 30 and {c["error"] for c in k["decode"]} == {None, dh.RANGE, dh.ENC1, dh.ENC2}
    for c in k["mul"]:
        kk, enc = int(c["k"], 16), bytes.fromhex(c["enc"])
        for how, lo in (("multiply", 1), ("multiplyUnsafe", 0)):
            r = c[how]
            if r["error"] is None:
                assert lo <= kk < N and dh.mul_enc(enc, kk).hex() == r["out"], (how, c["k"])
            else:
                assert isinstance(dh.decode(enc), str) or not lo <= kk < N
    assert any(int(c["k"], 16) == 0 and c["multiplyUnsafe"]["out"] == "00" * 56 for c in k["mul"])
    for c in k["add"]:
        a, b = dh.decode(bytes.fromhex(c["a"])), dh.decode(bytes.fromhex(c["b"]))
        assert dh.encode(eh.pt_add(a, b)).hex() == c["add"] and dh.encode(eh.pt_add(a, eh.pt_neg(b))).hex() == c["subtract"]
        assert dh.encode(eh.pt_neg(a)).hex() == c["negate"] and dh.encode(eh.pt_add(a, a)).hex() == c["double"]
    for c in k["equals"]:
        assert dh.equals((int(c["x1"], 16), int(c["y1"], 16)), (int(c["x2"], 16), int(c["y2"], 16))) is c["equal"]
    assert {c["equal"] for c in k["equals"]} == {True, False}
    for c in k["encode_affine"]:
        assert dh.encode((int(c["x"], 16), int(c["y"], 16))).hex() == c["enc"]
    # the small-order points: (0, 1) and (0, -1) are the identity; (+-1, 0) are not folded onto it, they give p - 1
    assert [c["enc"] for c in k["encode_affine"][:4]] == ["00" * 56] * 2 + [dh.le56(P - 1).hex()] * 2
    for c in k["encode_ext"]:
        assert dh.encode_ext(*(int(c[n], 16) for n in "XYZT")).hex() == c["enc"]
    for c in k["derive"]:
        assert dh.encode(dh.derive(bytes.fromhex(c["uniform"]))).hex() == c["enc"]
    for c in k["hash"]:
        dst = {} if c["dst"] is None else {"dst": bytes.fromhex(c["dst"])}
        msg = bytes.fromhex(c["msg"])
        assert dh.hash_to_curve(msg, **dst).hex() == c["curve"] and dh.hash_to_scalar(msg, **dst) == int(c["scalar"], 16)
    assert any(c["dst"] and len(c["dst"]) > 510 for c in k["hash"])


# ---------------------------------------------------------------- the CPU twins
def test_decode_twin_against_fixture_and_round_trip():
    enc, aff, ok = dh.decode_rows()
    got, gok = ENG.decaf448_decode_batch(enc)
    assert np.array_equal(gok, ok.astype(bool)) and np.array_equal(got, aff) and not got[~gok].any()
    assert np.array_equal(ENG.decaf448_encode_batch(got[gok]), enc[gok])


def test_encode_twin_whole_cosets_and_projective_scale():
    aff, want = dh.encode_rows()
    assert np.array_equal(ENG.decaf448_encode_batch(aff), want)
    rng = random.Random("decaf-proj")
    xyz, wantp = [], []
    for _, enc, (x, y) in dh.multiples():
        for z in (1, 2, P - 1, rng.randrange(1, P)):
            xyz.append(dh.le56(x * z % P) + dh.le56(y * z % P) + dh.le56(z))
            wantp.append(enc)
    assert np.array_equal(dh.ht_encode_proj(dh.rows(xyz, 168)), dh.rows(wantp, 56))


def test_equals_twin():
    a, b, want = dh.equals_rows()
    assert np.array_equal(ENG.decaf448_equals_batch(a, b), want.astype(bool))
    assert ENG.decaf448_equals_batch(a, a).all()


def test_from_uniform_twin():
    uni, want = dh.derive_rows()
    assert np.array_equal(ENG.decaf448_from_uniform_batch(uni), want)


def test_multiply_twin_rows_one_scalar_and_base():
    enc, ks, want, ok = dh.mul_rows()
    got, gok = ENG.decaf448_mul_batch(enc, ks)
    assert np.array_equal(gok, ok.astype(bool)) and np.array_equal(got, want) and not gok.all()
    one, ook = ENG.decaf448_mul_batch(enc[:12], ks[3:4], one_scalar=True)
    rep, rok = ENG.decaf448_mul_batch(enc[:12], np.repeat(ks[3:4], 12, axis=0))
    assert np.array_equal(one, rep) and np.array_equal(ook, rok)
    scal = [kk for kk, _, _ in dh.multiples()] + [N, 2**448 - 1]
    base = ENG.decaf448_mul_base_batch(dh.rows([dh.le56(kk) for kk in scal], 56))
    assert [bytes(r) for r in base] == [dh.encode(eh.pt_mul(dh.BASE, kk)) for kk in scal]
    assert [bytes(r).hex() for r in base[:27]] == [c["enc"] for c in dh.kat()["multiples"]]


def test_decode_add_pairs_encode_is_the_reference_add():
    k = dh.kat()["add"]
    a, _ = ENG.decaf448_decode_batch(dh.rows([bytes.fromhex(c["a"]) for c in k], 56))
    b, _ = ENG.decaf448_decode_batch(dh.rows([bytes.fromhex(c["b"]) for c in k], 56))
    assert [bytes(r).hex() for r in ENG.decaf448_encode_batch(ENG.ed448_add_pairs_batch(a, b))] == [c["add"] for c in k]
    assert [bytes(r).hex() for r in ENG.decaf448_encode_batch(ENG.ed448_add_pairs_batch(a, b, True))] == [c["subtract"] for c in k]


def test_random_encodings_sweep():
    """even canonical strings: the twin and the restatement agree on every row; the accepted share is only counted"""
    rng = random.Random("decaf-sweep")
    enc = [dh.le56((rng.getrandbits(448) % P) & ~1) for _ in range(64)]
    got, ok = ENG.decaf448_decode_batch(dh.rows(enc, 56))
    accepted = 0
    for i, e in enumerate(enc):
        want = dh.decode(e)
        assert bool(ok[i]) == (not isinstance(want, str)), i
        if ok[i]:
            accepted += 1
            assert bytes(got[i]) == dh.le56(want[0]) + dh.le56(want[1])
    print("accepted %d of %d even canonical strings" % (accepted, len(enc)))


@pytest.mark.parametrize("op", [0, 1, 2])
def test_decaf448_op_on_raw_limbs(op):
    a, b = dh.check_rows(op)
    dh.check_decaf448(op, a, b, dh.ht_op(op, a, b))


def test_decaf448_op_table_and_unknown_ops():
    import ctypes
    from noble_curves_amd._native import DECAF448_CHECK_WORDS
    assert DECAF448_CHECK_WORDS == dh.DECAF448_OPS
    for op in (-1, 0, 1, 2, 3, 11):
        w = (ctypes.c_int * 3)()
        dh.ht().ht_decaf448_widths(op, ctypes.byref(w, 0), ctypes.byref(w, 4), ctypes.byref(w, 8))
        assert tuple(w) == dh.DECAF448_OPS.get(op, (0, 0, 0))
    z = np.zeros(64, np.uint32)
    out = np.full(64, 7, np.uint32)
    assert dh.ht().ht_decaf448_op(3, z.ctypes.data, z.ctypes.data, out.ctypes.data) == -1 and (out == 7).all()


# ---------------------------------------------------------------- the Python shim on the twins
def test_mirror_point_and_hasher():
    from noble_curves_amd import decaf448 as m
    k = dh.kat()
    Pt = m.Point
    for c in k["multiples"][:20]:
        kk = int(c["k"], 16)
        p = Pt.BASE.multiplyUnsafe(kk, ENG)
        assert p.toAffine() == (int(c["x"], 16), int(c["y"], 16)) and p.toHex(ENG) == c["enc"]
        q = Pt.fromHex(c["enc"], ENG)
        assert q.equals(p, ENG) and q.toBytes(ENG).hex() == c["enc"] and q.is0(ENG) == (kk == 0)
    for c in k["add"]:
        a, b = Pt.fromHex(c["a"], ENG), Pt.fromHex(c["b"], ENG)
        assert a.add(b, ENG).toHex(ENG) == c["add"] and a.subtract(b, ENG).toHex(ENG) == c["subtract"]
        assert a.negate().toHex(ENG) == c["negate"] and a.double(ENG).toHex(ENG) == c["double"]
    for c in k["mul"]:
        kk = int(c["k"], 16)
        for how in ("multiply", "multiplyUnsafe"):
            r = c[how]
            try:
                got = getattr(Pt.fromHex(c["enc"], ENG), how)(kk, ENG).toHex(ENG)
                assert r["error"] is None and got == r["out"]
            except ValueError as e:
                assert str(e) == r["error"], (how, c["k"])
    pts, ok = m.fromBytes_batch([bytes.fromhex(c["enc"]) for c in k["decode"]], ENG)
    assert ok == [c["error"] is None for c in k["decode"]] and [p is not None for p in pts] == ok
    for c in k["decode"]:
        if c["error"]:
            with pytest.raises(ValueError) as e:
                Pt.fromBytes(bytes.fromhex(c["enc"]), ENG)
            assert str(e.value) == c["error"], c["name"]
    good = [p for p in pts if p is not None]
    assert [b.hex() for b in m.toBytes_batch(good, ENG)] == [c["enc"] for c in k["decode"] if c["error"] is None]
    assert m.equals_batch(good, good, ENG) == [True] * len(good) and m.equals_batch(good[:2], good[1:3], ENG) == [False, False]
    rows = [c for c in k["mul"] if c["multiply"]["error"] is None]
    out, mok = m.multiply_batch([bytes.fromhex(c["enc"]) for c in rows], [int(c["k"], 16) for c in rows], ENG)
    assert [o.hex() for o in out] == [c["multiply"]["out"] for c in rows] and all(mok)
    out1, _ = m.multiply_batch([Pt.fromHex(c["enc"], ENG) for c in rows[:4]], 5, ENG)
    assert out1 == [dh.mul_enc(bytes.fromhex(c["enc"]), 5) for c in rows[:4]]
    bad, bok = m.multiply_batch([bytes.fromhex(k["decode"][30]["enc"])], [3], ENG)
    assert bad == [None] and bok == [False]
    assert [b.hex() for b in m.multiplyBase_batch([int(c["k"], 16) for c in k["multiples"][1:8]], ENG)] == [c["enc"] for c in k["multiples"][1:8]]
    d = k["derive"]
    assert [b.hex() for b in m.deriveToCurve_batch([bytes.fromhex(c["uniform"]) for c in d], ENG)] == [c["enc"] for c in d]
    assert m.deriveToCurve(bytes.fromhex(d[0]["uniform"]), ENG).toHex(ENG) == d[0]["enc"]
    for c in k["hash"]:
        dst = None if c["dst"] is None else bytes.fromhex(c["dst"]).decode("ascii") if c["dst_is_text"] else bytes.fromhex(c["dst"])
        msg = bytes.fromhex(c["msg"])
        assert m.hashToCurve_batch([msg], dst, ENG)[0].hex() == c["curve"] == m.hashToCurve(msg, dst, ENG).toHex(ENG)
        assert m.hashToScalar(msg, dst) == int(c["scalar"], 16)
    assert m.fromBytes_batch([], ENG) == ([], []) and m.toBytes_batch([], ENG) == [] and m.multiplyBase_batch([], ENG) == []


def test_mirror_argument_errors():
    from noble_curves_amd import decaf448 as m
    err = dh.kat()["errors"]
    Pt = m.Point

    def msg(f, kind=ValueError):
        with pytest.raises(kind) as e:
            f()
        return str(e.value)

    assert msg(lambda: Pt.fromBytes(bytes(55), ENG)) == err["length"] and msg(lambda: Pt.fromBytes(bytes(57), ENG)) == err["length_57"]
    assert msg(lambda: Pt.fromBytes("00", ENG), TypeError) == err["type"]
    assert msg(lambda: m.deriveToCurve(bytes(111), ENG)) == err["derive_length"]
    assert msg(lambda: Pt.BASE.equals((0, 1), ENG), TypeError) == err["equals_other"]
    assert msg(lambda: Pt.BASE.add((0, 1), ENG), TypeError) == err["add_other"] == msg(lambda: Pt.BASE.subtract(None, ENG), TypeError)
    assert msg(lambda: Pt.BASE.multiply(0, ENG)) == err["multiply_zero"] and msg(lambda: Pt.BASE.multiply(N, ENG)) == err["multiply_n"]
    assert msg(lambda: Pt.BASE.multiplyUnsafe(N, ENG)) == err["multiply_unsafe_n"]
    assert msg(lambda: Pt.BASE.multiplyUnsafe(-1, ENG)) == err["multiply_unsafe_negative"]
    assert msg(lambda: m.multiply_batch([bytes(56)], [0], ENG)) == err["multiply_zero"]
    assert msg(lambda: m.multiplyBase_batch([N], ENG)) == err["multiply_n"]
    assert msg(lambda: m.hashToCurve(b"x", "", ENG)) == err["empty_dst"] and msg(lambda: m.hashToScalar(b"x", b"")) == err["empty_dst_scalar"]
    assert msg(lambda: Pt.fromHex("0", ENG)) == err["from_hex_odd"]
    # the batch forms check every scalar, then every length, before anything is sent (as ristretto255's do); an encoding that
    # does not decode is a None in the result, not an error
    assert msg(lambda: m.multiply_batch([bytes(55)], [1], ENG)) == err["length"]
    assert msg(lambda: m.multiply_batch([bytes(55)], [0], ENG)) == err["multiply_zero"]
    assert msg(lambda: m.equals_batch([Pt.BASE], [], ENG)) == "arrays of points must have equal length"
