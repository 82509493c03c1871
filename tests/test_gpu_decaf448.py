"""decaf448 ON THE DEVICE: the ncg_decaf448_* entry points (host and _dev forms) and ncg_decaf448_check, against the reference's own
answers (tests/golden/decaf448_kat.json), the Python restatement of decaf448_helpers and the CPU twin, bit for bit.  Every case
runs at n in {1, 64, 65, 299}: rows are built once and cycled to n."""
import numpy as np
import pytest
import torch

import decaf448_helpers as dh
import ed448_helpers as eh
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
SIZES = [1, 64, 65, 299]
TWIN = dh.TwinEngine()
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


def twin_sample(n):
    """the rows the (slow) CPU twin is asked about"""
    return slice(0, min(n, 24))


# ---------------------------------------------------------------- ncg_decaf448_check
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", [0, 1, 2])
def test_check_device_against_restatement_and_twin(op, n):
    a0, b0 = once(("check", op), lambda: dh.check_rows(op))
    a, b = dh.cycle(a0, n), dh.cycle(b0, n)
    out = get_engine().decaf448_check(op, a, b)
    m = min(n, a0.shape[0])
    dh.check_decaf448(op, a[:m], b[:m], out[:m])
    assert np.array_equal(out, dh.cycle(out[:m], n))                          # a cycled row gives the same answer in every lane
    s = twin_sample(n)
    assert np.array_equal(out[s], dh.ht_op(op, a[s], b[s]))                   # raw limbs, bit for bit


def test_check_unknown_op_and_batch_limit():
    eng = get_engine()
    z = np.ones((3, 64), np.uint32)
    assert eng.decaf448_check(3, z, z).shape == (3, 16) and not eng.decaf448_check(3, z, z).any()
    assert not eng.decaf448_check(-1, z, z).any() and not eng.decaf448_check(11, z, z).any()
    assert eng.lib.ncg_decaf448_check(eng.h, 0, 0, (1 << 24) + 1, None, None, None) == INVALID
    assert "too large" in (eng.lib.ncg_last_error(eng.h) or b"").decode()


# ---------------------------------------------------------------- decode / encode / equals
@pytest.mark.parametrize("n", SIZES)
def test_decode_and_round_trip(n):
    full = once("decode", dh.decode_rows)
    if n == 1:                                                                # the single lane on a refused row as well
        bad = int(np.argmin(full[2]))
        got, gok = both("ncg_decaf448_decode_batch", 1, [np.ascontiguousarray(full[0][bad:bad + 1])], [], [(1, 112), (1,)])
        assert not gok.any() and not got.any()
    enc, aff, ok = (dh.cycle(x, n) for x in full)
    got, gok = both("ncg_decaf448_decode_batch", n, [enc], [], [(n, 112), (n,)])
    assert np.array_equal(gok, ok) and np.array_equal(got, aff) and not got[ok == 0].any()
    s = twin_sample(n)
    tw, twok = TWIN.decaf448_decode_batch(enc[s])
    assert np.array_equal(got[s], tw) and np.array_equal(gok[s].astype(bool), twok)
    valid = ok == 1
    m = int(valid.sum())
    back, = both("ncg_decaf448_encode_batch", m, [np.ascontiguousarray(got[valid])], [], [(m, 56)])
    assert np.array_equal(back, enc[valid])                                   # encode(decode(e)) = e
    if n >= 64:
        assert (ok == 0).sum() >= 30 and valid.sum() >= 20


@pytest.mark.parametrize("n", SIZES)
def test_encode_whole_cosets(n):
    aff, want = (dh.cycle(x, n) for x in once("encode", dh.encode_rows))
    got, = both("ncg_decaf448_encode_batch", n, [aff], [], [(n, 56)])
    assert np.array_equal(got, want)
    s = twin_sample(n)
    assert np.array_equal(got[s], TWIN.decaf448_encode_batch(aff[s]))


@pytest.mark.parametrize("n", SIZES)
def test_equals(n):
    a, b, want = (dh.cycle(x, n) for x in once("equals", dh.equals_rows))
    got, = both("ncg_decaf448_equals_batch", n, [a, b], [], [(n,)])
    assert np.array_equal(got, want)
    assert np.array_equal(got, TWIN.decaf448_equals_batch(a, b).astype(np.uint8))
    if n > 1:
        assert got.any() and not got.all()


@pytest.mark.parametrize("n", SIZES)
def test_decode_add_pairs_encode_is_the_reference_add(n):
    k = dh.kat()["add"]
    ea, eb = (dh.cycle(dh.rows([bytes.fromhex(c[x]) for c in k], 56), n) for x in "ab")
    want_add, want_sub = (dh.cycle(dh.rows([bytes.fromhex(c[x]) for c in k], 56), n) for x in ("add", "subtract"))
    a, oka = both("ncg_decaf448_decode_batch", n, [ea], [], [(n, 112), (n,)])
    b, okb = both("ncg_decaf448_decode_batch", n, [eb], [], [(n, 112), (n,)])
    assert oka.all() and okb.all()
    eng = get_engine()
    assert np.array_equal(both("ncg_decaf448_encode_batch", n, [eng.ed448_add_pairs_batch(a, b)], [], [(n, 56)])[0], want_add)
    assert np.array_equal(both("ncg_decaf448_encode_batch", n, [eng.ed448_add_pairs_batch(a, b, True)], [], [(n, 56)])[0], want_sub)


# ---------------------------------------------------------------- hash to group
@pytest.mark.parametrize("n", SIZES)
def test_from_uniform(n):
    uni, want = (dh.cycle(x, n) for x in once("derive", dh.derive_rows))
    got, = both("ncg_decaf448_from_uniform_batch", n, [uni], [], [(n, 56)])
    assert np.array_equal(got, want)
    s = twin_sample(n)
    assert np.array_equal(got[s], TWIN.decaf448_from_uniform_batch(uni[s]))


# ---------------------------------------------------------------- multiply
@pytest.mark.parametrize("n", SIZES)
def test_multiply_rows_one_scalar_and_base(n):
    enc, ks, want, ok = (dh.cycle(x, n) for x in once("mul", dh.mul_rows))
    got, gok = both("ncg_decaf448_mul_batch", n, [enc, ks], [0], [(n, 56), (n,)])
    assert np.array_equal(gok, ok) and np.array_equal(got, want) and not got[ok == 0].any()
    s = slice(0, min(n, 6))
    tw, twok = TWIN.decaf448_mul_batch(enc[s], ks[s])
    assert np.array_equal(got[s], tw) and np.array_equal(gok[s].astype(bool), twok)
    k1 = np.ascontiguousarray(once("mul", dh.mul_rows)[1][7:8])
    one = both("ncg_decaf448_mul_batch", n, [enc, k1], [1], [(n, 56), (n,)])
    rep = both("ncg_decaf448_mul_batch", n, [enc, np.repeat(k1, n, axis=0)], [0], [(n, 56), (n,)])
    assert np.array_equal(one[0], rep[0]) and np.array_equal(one[1], rep[1]) and np.array_equal(one[1], ok)
    base = dh.rows([dh.encode(dh.BASE)] * n, 56)
    mb, = both("ncg_decaf448_mul_base_batch", n, [ks], [], [(n, 56)])
    assert np.array_equal(mb, both("ncg_decaf448_mul_batch", n, [base, ks], [0], [(n, 56), (n,)])[0])
    if n >= 64:
        assert (ok == 0).any() and (ok == 1).sum() > 40


def test_multiples_of_base_from_the_fixture():
    m = dh.kat()["multiples"]
    ks = dh.rows([dh.le56(int(c["k"], 16)) for c in m], 56)
    out, = both("ncg_decaf448_mul_base_batch", len(m), [ks], [], [(len(m), 56)])
    assert [bytes(r).hex() for r in out] == [c["enc"] for c in m] and not out[0].any()          # k = 0: 56 zero bytes


# ---------------------------------------------------------------- argument checks
# (function, template: W a buffer of 56-byte rows (4-byte aligned in the _dev form), B a byte buffer, F the flags)
SPECS = [("ncg_decaf448_decode_batch", "W W B"), ("ncg_decaf448_encode_batch", "W W"), ("ncg_decaf448_equals_batch", "W W B"),
         ("ncg_decaf448_from_uniform_batch", "W W"), ("ncg_decaf448_mul_batch", "W W F W B"), ("ncg_decaf448_mul_base_batch", "W W")]


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
                return [(over or {}).get(i, buf if t in "BW" else 0 if t == "F" else None) for i, t in enumerate(toks)]

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
            assert f(h, 1, *args()) == OK, (fn, err())               # a zero row: the identity's encoding, a valid input everywhere
    for a in ((None, hbuf.ctypes.data, hbuf.ctypes.data), (hbuf.ctypes.data, None, hbuf.ctypes.data), (hbuf.ctypes.data, hbuf.ctypes.data, None)):
        assert L.ncg_decaf448_check(h, 0, 0, 1, *a) == INVALID and "NULL buffer" in err()
    assert L.ncg_decaf448_check(None, 0, 0, 1, hbuf.ctypes.data, hbuf.ctypes.data, hbuf.ctypes.data) == INVALID
    assert L.ncg_decaf448_check(h, 0, 0, 0, None, None, None) == OK
    assert L.ncg_sync(h) == OK
    torch.cuda.synchronize()
    assert checked == 71                                             # 32 NULL-buffer cases and 39 misaligned device pointers
    assert not hbuf[256:].any() and not dbuf.cpu().numpy()[256:].any()


# ---------------------------------------------------------------- the Python shim on the device
def test_shim_on_the_device():
    from noble_curves_amd import decaf448 as m
    k = dh.kat()
    Pt = m.Point
    mult = k["multiples"]
    assert [b.hex() for b in m.multiplyBase_batch([int(c["k"], 16) for c in mult[1:]])] == [c["enc"] for c in mult[1:]]
    c = mult[20]
    p = Pt.BASE.multiply(int(c["k"], 16))
    assert p.toAffine() == (int(c["x"], 16), int(c["y"], 16)) and p.toHex() == c["enc"] and not p.is0()
    assert Pt.BASE.multiplyUnsafe(0).is0() and Pt.ZERO.toBytes() == bytes(56)
    a = k["add"][0]
    pa, pb = Pt.fromHex(a["a"]), Pt.fromHex(a["b"])
    assert pa.add(pb).toHex() == a["add"] and pa.subtract(pb).toHex() == a["subtract"] and pa.double().toHex() == a["double"]
    assert pa.negate().toHex() == a["negate"] and pa.add(pb).equals(pb.add(pa)) and not pa.equals(pb)
    dec = k["decode"]
    pts, ok = m.fromBytes_batch([bytes.fromhex(x["enc"]) for x in dec])
    assert ok == [x["error"] is None for x in dec]
    assert [b.hex() for b in m.toBytes_batch([q for q in pts if q])] == [x["enc"] for x in dec if x["error"] is None]
    for x in (dec[16], dec[16 + 7], dec[16 + 14]):                             # not canonical, negative, a non-square ratio
        with pytest.raises(ValueError) as e:
            Pt.fromBytes(bytes.fromhex(x["enc"]))
        assert str(e.value) == x["error"]
    rows = [x for x in k["mul"] if x["multiply"]["error"] is None]
    out, mok = m.multiply_batch([bytes.fromhex(x["enc"]) for x in rows], [int(x["k"], 16) for x in rows])
    assert [o.hex() for o in out] == [x["multiply"]["out"] for x in rows] and all(mok)
    out, mok = m.multiply_batch([bytes.fromhex(rows[0]["enc"]), bytes.fromhex(dec[16 + 14]["enc"])], 7)
    assert out == [dh.mul_enc(bytes.fromhex(rows[0]["enc"]), 7), None] and mok == [True, False]
    d = k["derive"]
    assert [b.hex() for b in m.deriveToCurve_batch([bytes.fromhex(x["uniform"]) for x in d])] == [x["enc"] for x in d]
    for x in k["hash"]:
        dst = None if x["dst"] is None else bytes.fromhex(x["dst"]).decode("ascii") if x["dst_is_text"] else bytes.fromhex(x["dst"])
        assert m.hashToCurve(bytes.fromhex(x["msg"]), dst).toHex() == x["curve"]
    assert [b.hex() for b in m.hashToCurve_batch([bytes.fromhex(x["msg"]) for x in k["hash"] if x["dst"] is None])] == \
        [x["curve"] for x in k["hash"] if x["dst"] is None]
    with pytest.raises(ValueError) as e:
        Pt.BASE.multiply(0)
    assert str(e.value) == k["errors"]["multiply_zero"]
