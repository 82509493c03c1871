"""X448 and Ed448 ON THE DEVICE: the ncg_x448_* / ncg_ed448_* entry points (host and _dev forms) and ncg_fe448_check, against the
reference's own answers (tests/golden/ed448_kat.json, ed448_wycheproof_old.json), the Python restatement of ed448_helpers and
the CPU twin, bit for bit.  Every case runs at n in {1, 64, 65, 299}: rows are built once and cycled to n."""
import ctypes

import numpy as np
import pytest
import torch

import ed448_helpers as eh
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
SIZES = [1, 64, 65, 299]
_cache = {}


def once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _odd(a):
    """the same bytes at an odd host address"""
    raw = np.empty(a.nbytes + 1, np.uint8)
    raw[1:] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return raw[1:]


def both(fn, n, ins, mid, out_shapes):
    """fn (host form) and fn_dev on the same rows; the host form's first input sits at an odd address.  `mid`: the integer
    arguments between the inputs and the outputs.  Both forms must agree bit for bit; returns the outputs [uint8 arrays]."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    hin = [_odd(ins[0])] + [np.ascontiguousarray(x) for x in ins[1:]]
    hout = [np.full(s, 0xA5, np.uint8) for s in out_shapes]
    rc = getattr(L, fn)(h, n, *[x.ctypes.data for x in hin], *mid, *[o.ctypes.data for o in hout])
    assert rc == OK, (L.ncg_last_error(h) or b"").decode()
    din = [_dev(x) for x in ins]
    dout = [torch.full(s, 0x5A, dtype=torch.uint8, device="cuda") for s in out_shapes]
    rc = getattr(L, fn + "_dev")(h, n, *[t.data_ptr() for t in din], *mid, *[t.data_ptr() for t in dout], None)
    assert rc == OK, (L.ncg_last_error(h) or b"").decode()
    torch.cuda.synchronize()
    for a, b in zip(hout, dout):
        assert np.array_equal(a, b.cpu().numpy()), fn + ": the host form and the _dev form differ"
    return hout


# ---------------------------------------------------------------- ncg_fe448_check
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op,variant", [(op, 0) for op in range(11)] + [(8, 1)])
def test_fe448_check_device_against_restatement_and_twin(op, variant, n):
    a, b = once(("fe", op), lambda: eh.fe448_rows(op, 300))
    a, b = a[:n], b[:n]
    out = get_engine().fe448_check(op, variant, a, b)
    eh.check_fe448(op, variant, a, b, out)
    m = min(n, 24)
    assert np.array_equal(out[:m], eh.ht_op(op, variant, a[:m], b[:m]))     # raw limbs, bit for bit


def test_fe448_check_unknown_op_and_batch_limit():
    eng = get_engine()
    z = np.ones((3, 64), np.uint32)
    assert eng.fe448_check(11, 0, z, z).shape == (3, 16) and not eng.fe448_check(11, 0, z, z).any()
    assert not eng.fe448_check(-1, 0, z, z).any()
    assert eng.lib.ncg_fe448_check(eng.h, 0, 0, (1 << 24) + 1, None, None, None) == INVALID
    assert "too large" in (eng.lib.ncg_last_error(eng.h) or b"").decode()


# ---------------------------------------------------------------- X448
def _x448_rows():
    k = eh.kat()["scalar_mult"]
    fixed = [c for c in k if not c["name"].startswith("random")] + k[-8:]
    s = np.concatenate([eh.hex_rows([c["scalar"] for c in fixed]), eh.rand_rows(40, "gpu-s")])
    u = np.concatenate([eh.hex_rows([c["u"] for c in fixed]), eh.rand_rows(40, "gpu-u")])
    want, want_ok = eh.expect_x448(s, u)
    fw, fok = eh.kat_expected(fixed)
    assert np.array_equal(want[:len(fixed)], fw) and np.array_equal(want_ok[:len(fixed)], fok)
    return s, u, want, want_ok


@pytest.mark.parametrize("n", SIZES)
def test_x448_rows_host_and_dev_forms(n):
    s, u, want, want_ok = (eh.cycle(x, n) for x in once("x448", _x448_rows))
    out, ok = both("ncg_x448_batch", n, [s, u], [0], [(n, 56), (n,)])
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)
    assert not out[ok == 0].any()
    if n > 1:
        assert ok.any() and not ok.all()


@pytest.mark.parametrize("n", SIZES)
def test_x448_one_scalar_and_base(n):
    s, u, want, want_ok = (eh.cycle(x, n) for x in once("x448", _x448_rows))
    s1 = np.ascontiguousarray(s[:1])
    per_row = both("ncg_x448_batch", n, [np.repeat(s1, n, axis=0), u], [0], [(n, 56), (n,)])
    flagged = both("ncg_x448_batch", n, [s1, u], [1], [(n, 56), (n,)])
    assert np.array_equal(per_row[0], flagged[0]) and np.array_equal(per_row[1], flagged[1])
    five = eh.rows([eh.le56(5)] * n, 56)
    base = both("ncg_x448_base_batch", n, [s], [], [(n, 56), (n,)])
    lad = both("ncg_x448_batch", n, [s, five], [0], [(n, 56), (n,)])
    assert base[1].all() and np.array_equal(base[0], lad[0])
    # the reference's Edwards hook: u = y^2 / x^2 of [clamp(s)]B
    eng = get_engine()
    clamped = eh.rows([eh.le56(eh.clamp(bytes(r))) for r in s], 56)
    mont, mok = eng.ed448_to_montgomery_batch(eng.ed448_mul_base_batch(clamped))
    assert mok.all() and np.array_equal(mont, base[0])


def test_x448_public_keys_and_chain_of_100():
    eng, k = get_engine(), eh.kat()
    rows = k["public_keys"]
    want, want_ok = eh.kat_expected(rows)
    out, ok = eng.x448_base_batch(eh.hex_rows([c["scalar"] for c in rows]))
    assert np.array_equal(ok, want_ok.astype(bool)) and np.array_equal(out, want)
    key = u = eh.rows([eh.le56(5)], 56)
    for i in range(1, 101):
        out, ok = eng.x448_batch(key, u)
        assert ok[0]
        key, u = out, key
        if i in (1, 100):
            assert key.tobytes().hex() == k["iterated"][str(i)], i


# ---------------------------------------------------------------- decode / encode
def _decode_rows():
    enc = [bytes.fromhex(c["enc"]) for c in eh.kat()["points"]] + eh.decode_edge_rows()
    want = [eh.pt_decode(e) for e in enc]
    aff = eh.rows([bytes(112) if isinstance(w, str) else eh.le56(w[0]) + eh.le56(w[1]) for w in want], 112)
    ok = np.array([0 if isinstance(w, str) else 1 for w in want], np.uint8)
    fixture = [c["error"] is None for c in eh.kat()["points"]]
    assert [bool(x) for x in ok[:len(fixture)]] == fixture
    return eh.rows(enc, 57), aff, ok


@pytest.mark.parametrize("n", SIZES)
def test_decode_encode(n):
    enc, aff, ok = (eh.cycle(x, n) for x in once("decode", _decode_rows))
    got, gok = both("ncg_ed448_decode_batch", n, [enc], [], [(n, 112), (n,)])
    assert np.array_equal(gok, ok) and np.array_equal(got, aff)
    valid = ok == 1
    if valid.any():
        m = int(valid.sum())
        back, = both("ncg_ed448_encode_batch", m, [np.ascontiguousarray(got[valid])], [], [(m, 57)])
        assert np.array_equal(back, enc[valid])               # encode(decode(e)) = e
    if n >= 64:
        assert (ok == 0).sum() >= 15


# ---------------------------------------------------------------- add pairs, multiply
def _add_rows():
    pts = eh.edge_points()
    pa, pb = [p for p in pts for q in pts], [q for p in pts for q in pts]
    return (eh.affine_rows(pa), eh.affine_rows(pb), eh.affine_rows([eh.pt_add(p, q) for p, q in zip(pa, pb)]),
            eh.affine_rows([eh.pt_add(p, eh.pt_neg(q)) for p, q in zip(pa, pb)]))


@pytest.mark.parametrize("n", SIZES)
def test_add_pairs(n):
    a, b, want_add, want_sub = (eh.cycle(x, n) for x in once("add", _add_rows))
    assert np.array_equal(both("ncg_ed448_add_pairs_batch", n, [a, b], [0], [(n, 112)])[0], want_add)
    assert np.array_equal(both("ncg_ed448_add_pairs_batch", n, [a, b], [1], [(n, 112)])[0], want_sub)


def _mul_rows():
    pk = [(p, k) for p in eh.edge_points() for k in eh.EDGE_SCALARS]
    rng_k = eh.rand_rows(10, "gpu-k")
    pk += [(eh.pt_mul(eh.BASE, 3 + i), int.from_bytes(bytes(rng_k[i]), "little")) for i in range(10)]
    enc = eh.rows([eh.pt_encode(p) for p, k in pk], 57)
    ks = eh.rows([eh.le56(k) for p, k in pk], 56)
    want = eh.rows([eh.pt_encode(eh.pt_mul(p, k)) for p, k in pk], 57)
    ok = np.ones(len(pk), np.uint8)
    enc[5], want[5], ok[5] = np.frombuffer(eh.P.to_bytes(57, "little"), np.uint8), 0, 0      # a refused encoding among them
    return enc, ks, want, ok


@pytest.mark.parametrize("n", SIZES)
def test_multiply(n):
    enc, ks, want, ok = (eh.cycle(x, n) for x in once("mul", _mul_rows))
    got, gok = both("ncg_ed448_mul_batch", n, [enc, ks], [0], [(n, 57), (n,)])
    assert np.array_equal(gok, ok) and np.array_equal(got, want)
    one = both("ncg_ed448_mul_batch", n, [enc, np.ascontiguousarray(ks[:1])], [1], [(n, 57), (n,)])
    rep = both("ncg_ed448_mul_batch", n, [enc, np.repeat(ks[:1], n, axis=0)], [0], [(n, 57), (n,)])
    assert np.array_equal(one[0], rep[0]) and np.array_equal(one[1], rep[1])
    base = eh.rows([eh.pt_encode(eh.BASE)] * n, 57)
    mb, = both("ncg_ed448_mul_base_batch", n, [ks], [], [(n, 57)])
    assert np.array_equal(mb, both("ncg_ed448_mul_batch", n, [base, ks], [0], [(n, 57), (n,)])[0])


@pytest.mark.parametrize("n", SIZES)
def test_to_montgomery(n):
    rows = eh.kat()["to_montgomery"]
    want, want_ok = (eh.cycle(x, n) for x in eh.kat_expected(rows))
    keys = eh.cycle(eh.hex_rows([c["publicKey"] for c in rows], 57), n)
    out, ok = both("ncg_ed448_to_montgomery_batch", n, [keys], [], [(n, 56), (n,)])
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)


# ---------------------------------------------------------------- verification
def _reference_verify_rows():
    k = eh.kat()
    out = []
    for c in k["verify"]:
        base = k["signatures"][c["row"]]
        msg = bytes.fromhex(base["msg"] if c["msg"] is None else c["msg"])
        sig, pk = bytes.fromhex(base["sig"]), bytes.fromhex(base["publicKey"])
        out.append((sig, pk, eh.challenge(sig[:57], pk, msg, bytes.fromhex(c["context"] or ""), c["ph"]) % eh.N, c["ok"]))
    for g in eh.wycheproof()["testGroups"]:
        pk = bytes.fromhex(g["key"]["pk"])
        for t in g["tests"]:
            sig, msg = bytes.fromhex(t["sig"]), bytes.fromhex(t["msg"])
            if len(sig) == 114:
                out.append((sig, pk, eh.challenge(sig[:57], pk, msg) % eh.N, t["result"] == "valid"))
    return (eh.rows([r[0] for r in out], 114), eh.rows([r[1] for r in out], 57), eh.rows([eh.le56(r[2]) for r in out], 56),
            np.array([r[3] for r in out], np.uint8))


@pytest.mark.parametrize("n", SIZES)
def test_verify_rules(n):
    sig, pk, k, want = once(("verify", n), lambda: eh.verify_arrays(n))
    if n == 1:                                                  # one accepted and one refused row
        for i in (0, int(np.argmin(want))):
            got, = both("ncg_ed448_verify_batch", 1, [sig[i:i + 1], pk[i:i + 1], k[i:i + 1]], [], [(1,)])
            assert got[0] == want[i]
        return
    ok, = both("ncg_ed448_verify_batch", n, [sig, pk, k], [], [(n,)])
    assert np.array_equal(ok, want) and ok.any() and not ok.all()


def test_verify_reference_and_wycheproof_rows():
    sig, pk, k, want = _reference_verify_rows()
    n = len(want)
    ok, = both("ncg_ed448_verify_batch", n, [sig, pk, k], [], [(n,)])
    assert np.array_equal(ok, want) and ok.any() and not ok.all() and n > 50


# ---------------------------------------------------------------- argument checks
# (function, template: B a required buffer, W a buffer of 56-byte rows (4-byte aligned in the _dev form), F the flags, I an integer)
SPECS = [("ncg_x448_batch", "W W F W B"), ("ncg_x448_base_batch", "W W B"), ("ncg_ed448_decode_batch", "B W B"),
         ("ncg_ed448_encode_batch", "W B"), ("ncg_ed448_add_pairs_batch", "W W I W"), ("ncg_ed448_mul_batch", "B W F B B"),
         ("ncg_ed448_mul_base_batch", "W B"), ("ncg_ed448_to_montgomery_batch", "B W B"), ("ncg_ed448_verify_batch", "B B W B")]


def test_argument_table():
    """NULL ctx, each required buffer NULL, n = 0 with every buffer NULL, unknown flags, n = 2^31 on the host forms and a misaligned
    device pointer for 56-byte rows.  Safe whatever the library does: every non-NULL pointer is a zeroed 4 KB buffer (device memory
    for the _dev forms) and n = 1, so a missing check runs on valid memory and fails the test instead of faulting."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    hbuf = np.zeros(4096, dtype=np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    err = lambda: (L.ncg_last_error(h) or b"").decode()  # noqa: E731
    checked = 0
    for name, tmpl in SPECS:
        for dev in (False, True):
            fn = name + ("_dev" if dev else "")
            f, toks = getattr(L, fn), tmpl.split() + (["S"] if dev else [])
            buf = dbuf.data_ptr() if dev else hbuf.ctypes.data

            def args(over=None, toks=toks, buf=buf):
                return [(over or {}).get(i, buf if t in "BW" else 0 if t in "FI" else None) for i, t in enumerate(toks)]

            assert f(None, 1, *args()) == INVALID, fn
            assert f(h, 0, *[None if t in "BW" else a for t, a in zip(toks, args())]) == OK, fn      # n = 0 touches nothing
            for i, t in enumerate(toks):
                if t in "BW":
                    assert f(h, 1, *args({i: None})) == INVALID, (fn, i)
                    assert "NULL buffer" in err(), (fn, i, err())
                    checked += 1
                if t == "W" and dev:
                    for off in (1, 2, 3):
                        assert f(h, 1, *args({i: buf + off})) == INVALID, (fn, i, off)
                        assert "4-byte aligned" in err(), (fn, i, err())
                        checked += 1
                if t == "F":
                    for bad in (2, 3, 1 << 8, -2):
                        assert f(h, 1, *args({i: bad})) == INVALID, (fn, bad)
                        assert "unknown flag" in err(), (fn, bad, err())
                    assert f(h, 0, *args({i: 2})) == INVALID, fn     # the flag rule comes before the empty batch
                    assert f(h, 1, *args({i: 1})) == OK, fn
            if not dev:
                assert f(h, 1 << 31, *[None if t in "BW" else a for t, a in zip(toks, args())]) == INVALID, fn
                assert "too large" in err(), (fn, err())
            assert f(h, 1, *args()) == OK, (fn, err())               # zero rows: refused by value, not by status
    for a in ((None, hbuf.ctypes.data, hbuf.ctypes.data), (hbuf.ctypes.data, None, hbuf.ctypes.data), (hbuf.ctypes.data, hbuf.ctypes.data, None)):
        assert L.ncg_fe448_check(h, 0, 0, 1, *a) == INVALID and "NULL buffer" in err()
    assert L.ncg_fe448_check(None, 0, 0, 1, hbuf.ctypes.data, hbuf.ctypes.data, hbuf.ctypes.data) == INVALID
    assert L.ncg_fe448_check(h, 0, 0, 0, None, None, None) == OK
    assert L.ncg_sync(h) == OK
    torch.cuda.synchronize()
    assert checked > 80
    assert not hbuf[128:].any() and not dbuf.cpu().numpy()[128:].any()


# ---------------------------------------------------------------- the Python shim on the device
def test_shim_on_the_device():
    from noble_curves_amd import ed448 as m
    k = eh.kat()
    rows = k["scalar_mult"][:24]
    got, ok = m.x448.scalarMult_batch([bytes.fromhex(c["scalar"]) for c in rows], [bytes.fromhex(c["u"]) for c in rows])
    assert [g.hex() if g else None for g in got] == [c["out"] for c in rows] and ok == [c["out"] is not None for c in rows]
    alice, bob = (bytes.fromhex(c["scalar"]) for c in k["public_keys"][:2])
    apub, bpub = m.x448.getPublicKey(alice), m.x448.getPublicKey(bob)
    assert [apub.hex(), bpub.hex()] == [c["out"] for c in k["public_keys"][:2]]
    assert m.x448.getSharedSecret(alice, bpub) == m.x448.scalarMult(bob, apub) == bytes.fromhex(k["scalar_mult"][2]["out"])
    many, ok = m.x448.getSharedSecret_batch(alice, [bpub, bytes(56)])
    assert many[1] is None and ok == [True, False]
    with pytest.raises(ValueError) as e:
        m.x448.scalarMult(alice, eh.le56(eh.P))
    assert str(e.value) == eh.INVALID
    with pytest.raises(ValueError) as e:
        m.x448.scalarMult(bytes(57), bytes(55))
    assert str(e.value) == k["errors"]["both_bad"]
    sigs = k["signatures"]
    plain = [c for c in sigs if not c["ph"] and c["context"] is None]
    v = m.ed448.verify_batch([bytes.fromhex(c["sig"]) for c in plain] + [bytes.fromhex(plain[0]["sig"])],
                             [bytes.fromhex(c["msg"]) for c in plain] + [b"other"],
                             [bytes.fromhex(c["publicKey"]) for c in plain] + [bytes.fromhex(plain[0]["publicKey"])])
    assert v == [True] * len(plain) + [False]
    ph = next(c for c in sigs if c["ph"] and c["context"])
    args = (bytes.fromhex(ph["sig"]), bytes.fromhex(ph["msg"]), bytes.fromhex(ph["publicKey"]))
    assert m.ed448ph.verify(*args, context=bytes.fromhex(ph["context"])) is True
    assert m.ed448ph.verify(*args) is False and m.ed448.verify(*args, context=bytes.fromhex(ph["context"])) is False
    with pytest.raises(ValueError) as e:
        m.ed448.verify(*args, context=bytes(256))
    assert str(e.value) == k["errors"]["context_too_long"]
    keys = k["ed_public_keys"][:3]
    assert [x.hex() for x in m.ed448.getPublicKey_batch([bytes.fromhex(c["secretKey"]) for c in keys])] == [c["out"] for c in keys]
    mont = k["to_montgomery"]
    got, ok = m.ed448.utils.toMontgomery_batch([bytes.fromhex(c["publicKey"]) for c in mont])
    assert [g.hex() if g else None for g in got] == [c["out"] for c in mont]
    g = eh.pt_encode(eh.BASE)
    assert m.ed448_Point.multiplyBase_batch([1, 2]) == [g, eh.pt_encode(eh.pt_mul(eh.BASE, 2))]
    assert m.ed448_Point.add_batch([g], [g])[0] == m.ed448_Point.multiplyUnsafe_batch([g], [2])[0]
    pts, ok = m.ed448_Point.fromBytes_batch([g, eh.P.to_bytes(57, "little")])
    assert pts == [eh.BASE, None] and m.ed448_Point.toBytes_batch([eh.BASE]) == [g]
