"""ristretto255 ON THE DEVICE: ncg_ristretto_{decode,encode,equals,from_uniform,mul,mul_base}_batch (host and _dev forms),
ncg_ristretto_msm and the pieces of ncg_field_check field 17, against the reference's own answers
(tests/golden/ristretto255_kat.json), the Python restatement (ristretto_helpers) and the CPU twin - bit for bit, no tolerances."""
import ctypes

import numpy as np
import pytest
import torch

import ristretto_helpers as rh
from noble_curves_amd import NativeError, get_engine

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
P, L = rh.P, rh.L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fill(shape, v):
    return torch.full(shape, v, dtype=torch.uint8, device="cuda")


def _decode_dev(eng, enc):
    n = enc.shape[0]
    d, out, ok = _dev(enc), _fill((n, 64), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_ristretto_decode_batch_dev(eng.h, n, d.data_ptr(), out.data_ptr(), ok.data_ptr(), None) == OK
    torch.cuda.synchronize()
    return out.cpu().numpy(), ok.cpu().numpy()


def _encode_dev(eng, pts):
    n = pts.shape[0]
    d, out = _dev(pts), _fill((n, 32), 0xAA)
    assert eng.lib.ncg_ristretto_encode_batch_dev(eng.h, n, d.data_ptr(), out.data_ptr(), None) == OK
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _mul_dev(eng, enc, ks, flags=0):
    n = enc.shape[0]
    de, dk, out, ok = _dev(enc), _dev(ks), _fill((n, 32), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_ristretto_mul_batch_dev(eng.h, n, de.data_ptr(), dk.data_ptr(), flags, out.data_ptr(), ok.data_ptr(), None) == OK
    torch.cuda.synchronize()
    return out.cpu().numpy(), ok.cpu().numpy()


# ---------------------------------------------------------------- decode
def test_decode_known_answers_host_and_dev_forms():
    eng, rows = get_engine(), rh.kat()["decode"]
    enc = rh.hex_rows([c["enc"] for c in rows])
    want = rh.hex_rows([rh.kat_affine(c) for c in rows], 64)
    want_ok = np.array([c["error"] is None for c in rows])
    out, ok = eng.ristretto_decode_batch(enc)
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)
    out, ok = _decode_dev(eng, enc)
    assert np.array_equal(ok, want_ok.astype(np.uint8)) and np.array_equal(out, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
def test_decode_batch_sizes_valid_and_invalid_mixed(n):
    raw, (want, want_ok) = rh.mixed_encodings(4096, "gpu")
    out, ok = _decode_dev(get_engine(), raw[:n])
    assert np.array_equal(ok, want_ok[:n]) and np.array_equal(out, want[:n])
    assert not out[ok == 0].any()                                           # a rejected row is zero, its neighbours untouched
    if n >= 63:
        assert 0 < ok.sum() < n


def test_decode_edge_rows_in_one_wave():
    eng = get_engine()
    raw, (want, want_ok) = rh.mixed_encodings(4096, "gpu")
    raw, want, want_ok = raw[:64].copy(), want[:64].copy(), want_ok[:64].copy()
    edges = rh.edge_encodings()
    for j, (name, enc, verdict) in enumerate(edges):
        i = 1 + 5 * j                                                       # lanes 1, 6, 11, ...
        raw[i] = np.frombuffer(enc, np.uint8)
        w, o = rh.expect_decode([enc])
        want[i], want_ok[i] = w[0], o[0]
        assert bool(o[0]) == (verdict == "ok"), name
    out, ok = _decode_dev(eng, raw)
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)
    assert rh.unwire(out[1]) == (0, 1) and ok[1] == 1                       # 32 zero bytes: the identity, (0, 1)
    assert ok[6] == 0 and ok[16] == 0 and ok[21] == 0 and ok[36] == 0       # even sqrt(-1), p - 1, p, bit 255


# ---------------------------------------------------------------- encode and equals
def test_encode_known_answers_and_torsion_cosets():
    eng = get_engine()
    rows = [c for c in rh.kat()["decode"] if c["error"] is None]
    pts = rh.hex_rows([rh.kat_affine(c) for c in rows], 64)
    want = rh.hex_rows([c["bytes"] for c in rows])
    assert np.array_equal(eng.ristretto_encode_batch(pts), want) and np.array_equal(_encode_dev(eng, pts), want)
    assert not eng.ristretto_encode_batch(rh.wire(rh.TORSION4)).any()       # (0, 1), (0, -1), (i, 0), (-i, 0): 32 zero bytes
    base = rh.base_multiples(64)
    assert 16 <= sum(rh.rotates(*p) for p in base) <= 48                    # both sides of the rotation
    ref = eng.ristretto_encode_batch(rh.wire(base))
    assert [bytes(r) for r in ref] == [rh.encode(p) for p in base]
    for t in rh.TORSION4:
        shifted = rh.wire([rh.add(p, t) for p in base])
        assert np.array_equal(_encode_dev(eng, shifted), ref)
        assert eng.ristretto_equals_batch(rh.wire(base), shifted).all()
    t8 = rh.order8_point()
    odd = [rh.add(p, t8) for p in base[:16]]
    got = eng.ristretto_encode_batch(rh.wire(odd))
    assert [bytes(r) for r in got] == [rh.encode(p) for p in odd] and np.array_equal(got, rh.ht_encode(rh.wire(odd)))


def test_equals_clauses_and_dev_form():
    eng = get_engine()
    base = rh.base_multiples(64)
    a = rh.wire(base)
    b = rh.wire([rh.add(p, rh.TORSION4[2]) for p in base[:32]] + [rh.add(p, p) for p in base[32:]])
    for p in base[:4]:                                                      # the second clause alone decides the first half
        q = rh.add(p, rh.TORSION4[2])
        assert p[0] * q[1] % P != p[1] * q[0] % P and p[1] * q[1] % P == p[0] * q[0] % P
    want = np.array([1] * 32 + [0] * 32, np.uint8)
    assert np.array_equal(eng.ristretto_equals_batch(a, b), want.astype(bool))
    da, db, out = _dev(a), _dev(b), _fill((64,), 7)
    assert eng.lib.ncg_ristretto_equals_batch_dev(eng.h, 64, da.data_ptr(), db.data_ptr(), out.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(rh.ht_equals(a, b), want)


# ---------------------------------------------------------------- from_uniform
def test_from_uniform_known_answers_edges_and_representative():
    eng, rows = get_engine(), rh.kat()["derive"]
    b = rh.hex_rows([c["in"] for c in rows], 64)
    want = rh.hex_rows([c["out"] for c in rows])
    out, aff = eng.ristretto_from_uniform_batch(b, want_affine=True)
    assert np.array_equal(out, want) and np.array_equal(eng.ristretto_from_uniform_batch(b)[0], want)
    tw_out, tw_aff = rh.ht_from_uniform(b, affine=True)
    assert np.array_equal(aff, tw_aff) and np.array_equal(eng.ristretto_encode_batch(aff), want)
    n = len(rows)
    db, dout, daff = _dev(b), _fill((n, 32), 0xAA), _fill((n, 64), 0xAA)
    assert eng.lib.ncg_ristretto_from_uniform_batch_dev(eng.h, n, db.data_ptr(), dout.data_ptr(), daff.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), want) and np.array_equal(daff.cpu().numpy(), tw_aff)
    edges = rh.edge_uniform()
    got = eng.ristretto_from_uniform_batch(np.frombuffer(b"".join(e[1] for e in edges), np.uint8).reshape(-1, 64))[0]
    assert [bytes(r) for r in got] == [rh.derive_bytes(e[1]) for e in edges]
    assert not got[0].any() and np.array_equal(got[2], got[3])             # zero halves: the identity; bit 255 of a half is masked
    sq = [rh.elligator(rh.half255(bytes(r[:32])))[1] for r in b[18:38]]     # both branches of the square test among 20 rows
    assert any(sq) and not all(sq)
    hrows = rh.kat()["hash"][:-1]
    xmd = [rh.expand_message_xmd(bytes.fromhex(c["msg"]), rh.DEFAULT_DST if c["dst"] is None else bytes.fromhex(c["dst"])) for c in hrows]
    got = eng.ristretto_from_uniform_batch(np.frombuffer(b"".join(xmd), np.uint8).reshape(-1, 64))[0]
    assert [bytes(r).hex() for r in got] == [c["out"] for c in hrows]


# ---------------------------------------------------------------- mul and mul_base
def test_mul_known_answers_one_scalar_and_rejected_rows():
    eng = get_engine()
    rows = [c for c in rh.kat()["multiply"] if c["error"] is None]
    enc, ks = rh.hex_rows([c["enc"] for c in rows]), rh.scalars_le([int(c["k"]) for c in rows])
    want = rh.hex_rows([c["out"] for c in rows])
    out, ok = eng.ristretto_mul_batch(enc, ks)
    assert ok.all() and np.array_equal(out, want)
    out, ok = _mul_dev(eng, enc, ks)
    assert ok.all() and np.array_equal(out, want)
    raw, (_, want_ok) = rh.mixed_encodings(4096, "gpu")
    raw, want_ok = raw[:130].copy(), want_ok[:130].copy()
    raw[64], want_ok[64] = np.frombuffer((P - 1).to_bytes(32, "little"), np.uint8), 0      # a rejected encoding mid-wave
    k = ks[3:4]
    per_row = _mul_dev(eng, raw, np.repeat(k, 130, axis=0))
    flagged = _mul_dev(eng, raw, k, flags=1)
    assert np.array_equal(per_row[0], flagged[0]) and np.array_equal(per_row[1], flagged[1]) and np.array_equal(flagged[1], want_ok)
    assert not flagged[0][want_ok == 0].any() and flagged[0][want_ok == 1].any(axis=1).all()
    host = eng.ristretto_mul_batch(raw, k, one_scalar=True)
    assert np.array_equal(host[0], flagged[0]) and np.array_equal(host[1], want_ok.astype(bool))
    tw = rh.ht_mul(raw, k, flags=1)
    assert np.array_equal(tw[0], flagged[0]) and np.array_equal(tw[1], want_ok)


def test_mul_base_equals_mul_of_the_encoded_basepoint():
    eng = get_engine()
    ks = rh.rand_bytes(300, 32, "mul-base")
    ks[:, 31] &= 0x0F                                                       # below 2^252 < L
    ks[0], ks[1], ks[2] = rh.scalars_le([1, 2, L - 1])
    ks[3] = 0                                                               # k = 0: the identity, 32 zero bytes
    base = np.repeat(np.frombuffer(rh.encode(rh.BASE), np.uint8).reshape(1, 32), 300, axis=0)
    want, ok = eng.ristretto_mul_batch(base, ks)
    got = eng.ristretto_mul_base_batch(ks)
    assert ok.all() and np.array_equal(got, want) and not got[3].any()
    small = rh.kat()["small_multiples"]
    assert bytes(got[0]).hex() == small[1] and bytes(got[1]).hex() == small[2]
    assert bytes(got[2]) == rh.encode(((P - rh.BASE[0]) % P, rh.BASE[1]))   # (L - 1) B = -B
    dk, out = _dev(ks), _fill((300, 32), 0xAA)
    assert eng.lib.ncg_ristretto_mul_base_batch_dev(eng.h, 300, dk.data_ptr(), out.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    for i in (4, 5, 6):                                                     # and against the restatement's double-and-add
        assert bytes(got[i]) == rh.encode(rh.mul(rh.BASE, int.from_bytes(bytes(ks[i]), "little")))


# ---------------------------------------------------------------- msm
@pytest.fixture(scope="module")
def msm_rows():
    """1000 valid encodings (multiples of the basepoint shifted through the cosets), their multipliers, and scalars with 0, 1 and
    L - 1 among them - the sum is tracked as one multiple of B"""
    rng = np.random.RandomState(11)
    base = rh.base_multiples(64)
    idx = rng.randint(0, 64, 1000)
    enc = np.frombuffer(b"".join(rh.encode(rh.add(base[i], rh.TORSION4[j % 4])) for j, i in enumerate(idx)), np.uint8).reshape(1000, 32).copy()
    ks = [int.from_bytes(rng.bytes(32), "little") % L for _ in range(1000)]
    ks[0], ks[1], ks[2] = L - 1, 1, 0
    return enc, ks, [int(i) + 1 for i in idx]


@pytest.mark.parametrize("n", [1, 2, 65, 1000])
def test_msm_against_the_sum(msm_rows, n):
    enc, ks, mult = msm_rows
    total = sum(k * m for k, m in zip(ks[:n], mult[:n])) % L
    want = rh.encode(rh.mul(rh.BASE, total))
    eng = get_engine()
    assert eng.ristretto_msm(enc[:n], rh.scalars_le(ks[:n])).tobytes() == want
    de, dk = _dev(enc[:n]), _dev(rh.scalars_le(ks[:n]))
    out, bad = np.full(32, 0xAA, np.uint8), ctypes.c_int64(5)
    assert eng.lib.ncg_ristretto_msm_dev(eng.h, n, de.data_ptr(), dk.data_ptr(), out.ctypes.data, ctypes.byref(bad), None) == OK
    assert out.tobytes() == want and bad.value == -1


def test_msm_zero_sum_and_bad_encodings(msm_rows):
    enc, ks, _ = msm_rows
    eng = get_engine()
    k = ks[5]
    pair = np.stack([enc[7], enc[7]])
    assert not eng.ristretto_msm(pair, rh.scalars_le([k, L - k])).any()     # k P + (L - k) P: the identity, 32 zero bytes
    assert not eng.ristretto_msm(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8)).any()      # the empty sum likewise
    sc = rh.scalars_le(ks[:100])
    for at in (0, 99):
        e = enc[:100].copy()
        e[at] = np.frombuffer((P - 1).to_bytes(32, "little"), np.uint8)
        with pytest.raises(NativeError, match="invalid ristretto255 encoding at index %d" % at) as err:
            eng.ristretto_msm(e, sc)
        assert err.value.bad_index == at
    big = rh.scalars_le([L] + ks[1:100])                                    # a scalar at the group order: the rule of ncg_msm
    with pytest.raises(NativeError, match="invalid scalar at index 0"):
        eng.ristretto_msm(enc[:100], big)


# ---------------------------------------------------------------- the Python mirror on the real engine
def test_python_mirror_on_the_device():
    from noble_curves_amd import ristretto255 as r
    k, Pt = rh.kat(), r.Point
    small = k["small_multiples"]
    acc = Pt.ZERO
    for hx in small[:5]:                                                    # Point.add through ncg_add_pairs_batch on representatives
        assert acc.toHex() == hx and Pt.fromHex(hx).equals(acc)
        acc = acc.add(Pt.BASE)
    assert acc.subtract(Pt.BASE).toHex() == small[4] and Pt.ZERO.is0() and not Pt.BASE.is0()
    assert Pt.BASE.multiply(7).toHex() == small[7]
    with pytest.raises(ValueError, match="invalid ristretto255 encoding 2"):
        Pt.fromBytes((P - 1).to_bytes(32, "little"))
    with pytest.raises(ValueError, match="invalid ristretto255 encoding 1"):
        Pt.fromBytes(P.to_bytes(32, "little"))
    hrows = k["hash"]
    assert [b.hex() for b in r.hashToCurve_batch([bytes.fromhex(c["msg"]) for c in hrows[:16]])] == [c["out"] for c in hrows[:16]]
    c = hrows[300]
    assert r.hashToCurve(bytes.fromhex(c["msg"]), DST=bytes.fromhex(c["dst"])).toHex() == c["out"]
    assert r.msm([bytes.fromhex(small[2]), bytes.fromhex(small[3])], [3, 2]).hex() == small[12]
    with pytest.raises(ValueError, match="invalid ristretto255 encoding 2"):
        r.msm([bytes.fromhex(small[2]), (P - 1).to_bytes(32, "little")], [3, 2])
    got, ok = r.multiply_batch([bytes.fromhex(small[1]), (P - 1).to_bytes(32, "little")], 9)
    assert got == [bytes.fromhex(small[9]), None] and ok == [True, False]
    assert r.multiplyBase_batch([9, 15]) == [bytes.fromhex(small[9]), bytes.fromhex(small[15])]


# ---------------------------------------------------------------- field_check 17 and the argument table
@pytest.mark.parametrize("op", [0, 1, 2])
def test_field_check_device_against_host_twin(op):
    a, b = rh.op_rows(op)
    out = get_engine().field_check(rh.FIELD_RISTRETTO, op, 0, a, b)
    rh.check_op(op, a, b, out)
    assert np.array_equal(out, rh.ht_op(op, a, b))                          # raw limbs, bit for bit


def test_field_check_unknown_op_leaves_out_zero():
    a, b = rh.op_rows(0)
    assert not get_engine().field_check(rh.FIELD_RISTRETTO, 3, 0, a[:4], b[:4]).any()


def test_argument_table():
    """NULL pointers, n = 0 and unknown flag bits for the fourteen entry points.  Safe whatever the library does: every non-NULL
    pointer is a zeroed 4 KB buffer (device memory for the _dev forms, host memory for what the header says is host memory) and
    n = 1, so a missing check runs on valid memory and fails the test."""
    eng = get_engine()
    Lb, h = eng.lib, eng.h
    hbuf = np.zeros(4096, dtype=np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    err = lambda: (Lb.ncg_last_error(h) or b"").decode()  # noqa: E731
    bad = ctypes.c_int64(0)

    def fresh():                                                            # a call that is to succeed reads zero rows: the identity
        hbuf[:64] = 0
        dbuf[:64] = 0
        torch.cuda.synchronize()
    # B a required buffer, O an optional one, H a required HOST buffer in both forms, I the bad-index pointer (optional), F flags, S stream
    specs = [("ncg_ristretto_decode_batch", "B B B"), ("ncg_ristretto_decode_batch_dev", "B B B S"),
             ("ncg_ristretto_encode_batch", "B B"), ("ncg_ristretto_encode_batch_dev", "B B S"),
             ("ncg_ristretto_equals_batch", "B B B"), ("ncg_ristretto_equals_batch_dev", "B B B S"),
             ("ncg_ristretto_from_uniform_batch", "B B O"), ("ncg_ristretto_from_uniform_batch_dev", "B B O S"),
             ("ncg_ristretto_mul_batch", "B B F B B"), ("ncg_ristretto_mul_batch_dev", "B B F B B S"),
             ("ncg_ristretto_mul_base_batch", "B B"), ("ncg_ristretto_mul_base_batch_dev", "B B S"),
             ("ncg_ristretto_msm", "B B H I"), ("ncg_ristretto_msm_dev", "B B H I S")]
    for fn, tmpl in specs:
        f, toks = getattr(Lb, fn), tmpl.split()
        buf = dbuf.data_ptr() if fn.endswith("_dev") else hbuf.ctypes.data
        msm = "msm" in fn

        def args(over=None, toks=toks, buf=buf):
            base = {"B": buf, "O": None, "H": hbuf.ctypes.data + 2048, "I": ctypes.byref(bad), "F": 0, "S": None}
            return [(over or {}).get(i, base[t]) for i, t in enumerate(toks)]

        assert f(None, 1, *args()) == INVALID, fn
        empty = [None if t in "BO" else a for t, a in zip(toks, args())]
        assert f(h, 0, *empty) == OK, fn                                    # n = 0 needs no input buffer ...
        if msm:                                                             # ... but the empty sum is WRITTEN, as ncg_msm does
            hbuf[2048:2080] = 0xAA
            assert f(h, 0, *empty) == OK and not hbuf[2048:2080].any(), fn
            assert f(h, 0, *[None if t in "BOH" else a for t, a in zip(toks, args())]) == INVALID and "NULL output" in err(), fn
        for i, t in enumerate(toks):
            if t in "BH":
                assert f(h, 1, *args({i: None})) == INVALID, (fn, i)
                assert "NULL buffer" in err(), (fn, i, err())
            if t == "F":
                for flags in (2, 3, 1 << 8, -2):
                    assert f(h, 1, *args({i: flags})) == INVALID, (fn, flags)
                    assert "unknown flag" in err(), (fn, flags, err())
                assert f(h, 0, *args({i: 2})) == INVALID, fn                # the flag rule comes before the empty batch
                fresh()
                assert f(h, 1, *args({i: 1})) == OK, fn
            if t == "I":
                fresh()
                assert f(h, 1, *args({i: None})) == OK, fn                  # the bad-index pointer is optional
        fresh()
        assert f(h, 1, *args()) == OK, (fn, err())                          # a zero row is the identity: a valid element
    torch.cuda.synchronize()
    assert not hbuf[64:2048].any() and not hbuf[2080:].any() and not dbuf.cpu().numpy()[64:].any()
