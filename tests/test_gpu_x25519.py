"""X25519 and ed25519.utils.toMontgomery ON THE DEVICE: ncg_x25519_batch, ncg_x25519_base_batch, ncg_ed25519_to_montgomery_batch
(host and _dev forms) and the ladder pieces of ncg_field_check field 16, against the reference's own answers
(tests/golden/x25519_kat.json), the Python restatement of the ladder (x25519_helpers) and the CPU twin, bit for bit.  The Wycheproof
X25519 file the reference's test reads is an absent submodule of the reference and is left out."""
import numpy as np
import pytest
import torch

import x25519_helpers as xh
from noble_curves_amd import get_engine
from noble_curves_amd._native import ED25519

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
P = xh.P


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _x25519_dev(eng, s, u, flags=0):
    n = u.shape[0]
    ds, du = _dev(s), _dev(u)
    out, ok = torch.full((n, 32), 0xAA, dtype=torch.uint8, device="cuda"), torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    assert eng.lib.ncg_x25519_batch_dev(eng.h, n, ds.data_ptr(), du.data_ptr(), flags, out.data_ptr(), ok.data_ptr(), None) == OK
    torch.cuda.synchronize()
    return out.cpu().numpy(), ok.cpu().numpy()


def test_known_answers_host_and_dev_forms():
    eng, rows = get_engine(), xh.kat()["scalar_mult"]
    s, u = xh.hex_rows([c["scalar"] for c in rows]), xh.hex_rows([c["u"] for c in rows])
    want, want_ok = xh.kat_expected(rows)
    out, ok = eng.x25519_batch(s, u)
    assert np.array_equal(ok, want_ok.astype(bool)) and np.array_equal(out, want)
    out, ok = _x25519_dev(eng, s, u)
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)


@pytest.fixture(scope="module")
def big():
    """4 096 seeded rows and the restatement's answers, computed once"""
    s, u = xh.rand_rows(4096, "gpu-s"), xh.rand_rows(4096, "gpu-u")
    return s, u, xh.expect(s, u)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
def test_batch_sizes_against_the_ladder(big, n):
    s, u, (want, want_ok) = big
    out, ok = _x25519_dev(get_engine(), s[:n], u[:n])
    assert np.array_equal(ok, want_ok[:n]) and np.array_equal(out, want[:n])


def test_rejected_rows_among_valid_ones_in_one_wave(big):
    s, u, (want, want_ok) = big
    u, want, want_ok = u[:64].copy(), want[:64].copy(), want_ok[:64].copy()
    low = [v.to_bytes(32, "little") for v in xh.LOW_ORDER] + [P.to_bytes(32, "little"), (P + 1).to_bytes(32, "little"),
                                                              ((1 << 255) | 1).to_bytes(32, "little")]
    for j, enc in enumerate(low):
        i = 1 + 7 * j                                       # lanes 1, 8, 15, ...: every one between two valid rows
        u[i], want[i], want_ok[i] = np.frombuffer(enc, np.uint8), 0, 0
    out, ok = _x25519_dev(get_engine(), s[:64], u)
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)
    assert not out[ok == 0].any() and (ok == 0).sum() == len(low)


def test_one_scalar_flag(big):
    s, u, _ = big
    eng = get_engine()
    u = u[:130].copy()
    u[64] = 0
    per_row = _x25519_dev(eng, np.repeat(s[:1], 130, axis=0), u)
    flagged = _x25519_dev(eng, s[:1], u, flags=1)
    assert np.array_equal(per_row[0], flagged[0]) and np.array_equal(per_row[1], flagged[1])
    host = eng.x25519_batch(s[:1], u, one_scalar=True)
    assert np.array_equal(host[0], flagged[0]) and np.array_equal(host[1], flagged[1].astype(bool))
    assert flagged[1].sum() == 129 and flagged[1][64] == 0


def test_rfc7748_chain_of_1000():
    """one lane, 10 chained calls of 100 dependent steps each, checked at every 100th value of the fixture"""
    eng, it = get_engine(), xh.kat()["iterated"]
    k = u = np.frombuffer((9).to_bytes(32, "little"), np.uint8).reshape(1, 32)
    for i in range(1, 1001):
        out, ok = eng.x25519_batch(k, u)
        assert ok[0]
        k, u = out, k
        if i == 1 or i % 100 == 0:
            assert k.tobytes().hex() == it[str(i)], i


def test_commutativity_through_the_base_entry_point():
    eng = get_engine()
    a, b = xh.rand_rows(256, "comm-a"), xh.rand_rows(256, "comm-b")
    apub, aok = eng.x25519_base_batch(a)
    bpub, bok = eng.x25519_base_batch(b)
    assert aok.all() and bok.all()
    nine = np.zeros((256, 32), np.uint8)
    nine[:, 0] = 9
    lad, lok = eng.x25519_batch(a, nine)                    # the table path against the ladder at u = 9
    assert lok.all() and np.array_equal(lad, apub)
    ab, ok1 = eng.x25519_batch(a, bpub)
    ba, ok2 = eng.x25519_batch(b, apub)
    assert ok1.all() and ok2.all() and np.array_equal(ab, ba)
    rows = xh.kat()["public_keys"]
    want, want_ok = xh.kat_expected(rows)
    ds = _dev(xh.hex_rows([c["scalar"] for c in rows]))
    out, ok = torch.zeros((len(rows), 32), dtype=torch.uint8, device="cuda"), torch.zeros(len(rows), dtype=torch.uint8, device="cuda")
    assert eng.lib.ncg_x25519_base_batch_dev(eng.h, len(rows), ds.data_ptr(), out.data_ptr(), ok.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy(), want_ok) and np.array_equal(out.cpu().numpy(), want)


def test_to_montgomery():
    eng, rows = get_engine(), xh.kat()["to_montgomery"]
    want, want_ok = xh.kat_expected(rows)
    keys = xh.hex_rows([c["publicKey"] for c in rows])
    out, ok = eng.ed25519_to_montgomery_batch(keys)
    assert np.array_equal(ok, want_ok.astype(bool)) and np.array_equal(out, want)
    dk = _dev(keys)
    dout, dok = torch.full((len(rows), 32), 0xAA, dtype=torch.uint8, device="cuda"), torch.full((len(rows),), 7, dtype=torch.uint8, device="cuda")
    assert eng.lib.ncg_ed25519_to_montgomery_batch_dev(eng.h, len(rows), dk.data_ptr(), dout.data_ptr(), dok.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(dok.cpu().numpy(), want_ok) and np.array_equal(dout.cpu().numpy(), want)
    # 4 096 keys [k]B from the fixed-base multiply, k clamped like an X25519 secret: u = (1 + y) / (1 - y) on integers ...
    raw = xh.rand_rows(4096, "mont")
    ks = np.frombuffer(b"".join(xh.clamp(bytes(r)).to_bytes(32, "little") for r in raw), np.uint8).reshape(4096, 32)
    pts, inf = eng.mul_base_batch(ED25519, ks)
    assert not inf.any()
    enc, eok = eng.encode_points_batch(ED25519, pts)
    assert eok.all()
    out, ok = eng.ed25519_to_montgomery_batch(enc)
    assert ok.all()
    for i in range(4096):
        y = int.from_bytes(pts[i, 32:].tobytes(), "little")
        assert out[i].tobytes() == ((1 + y) * pow(1 - y, P - 2, P) % P).to_bytes(32, "little"), i
    # ... and the same value as the X25519 public key of that secret (toMontgomery(getPublicKey) == getPublicKey(toMontgomerySecret))
    pub, pok = eng.x25519_base_batch(raw[:64])
    assert pok.all() and np.array_equal(pub, out[:64])


@pytest.mark.parametrize("swap", [0, 1])
def test_field_check_step_device_against_host_twin(swap):
    a, b = xh.step_rows()
    out = get_engine().field_check(xh.FIELD_X25519, 0, swap, a, b)
    xh.check_step(a, b, out, swap)
    assert np.array_equal(out, xh.ht_op(0, swap, a, b))     # raw limbs, bit for bit


def test_field_check_decoders_device_against_host_twin():
    eng = get_engine()
    us, ks = xh.edge_u_rows(), xh.edge_scalar_rows()
    au, ak = xh.words36(us), xh.words36(ks)
    zu, zk = np.zeros((len(us), 9), np.uint32), np.zeros((len(ks), 9), np.uint32)
    out = eng.field_check(xh.FIELD_X25519, 1, 0, au, zu)
    xh.check_decode_u(us, out)
    assert np.array_equal(out, xh.ht_op(1, 0, au, zu))
    out = eng.field_check(xh.FIELD_X25519, 2, 0, ak, zk)
    xh.check_decode_scalar(ks, out)
    assert np.array_equal(out, xh.ht_op(2, 0, ak, zk))
    assert not eng.field_check(xh.FIELD_X25519, 3, 0, ak, zk).any()     # an unknown op leaves out zero


def test_argument_table():
    """NULL pointers, n = 0 and an unknown flag bit for the six entry points.  Safe whatever the library does: every non-NULL pointer
    is a zeroed 4 KB buffer (device memory for the _dev forms) and n = 1, so a missing check runs on valid memory and fails the test."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    hbuf = np.zeros(4096, dtype=np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    err = lambda: (L.ncg_last_error(h) or b"").decode()  # noqa: E731
    # (function, argument template: B a required buffer, F the flags, S the stream)
    specs = [("ncg_x25519_batch", "B B F B B"), ("ncg_x25519_batch_dev", "B B F B B S"),
             ("ncg_x25519_base_batch", "B B B"), ("ncg_x25519_base_batch_dev", "B B B S"),
             ("ncg_ed25519_to_montgomery_batch", "B B B"), ("ncg_ed25519_to_montgomery_batch_dev", "B B B S")]
    for fn, tmpl in specs:
        f, toks = getattr(L, fn), tmpl.split()
        buf = dbuf.data_ptr() if fn.endswith("_dev") else hbuf.ctypes.data

        def args(over=None, toks=toks, buf=buf):
            return [(over or {}).get(i, buf if t == "B" else 0 if t == "F" else None) for i, t in enumerate(toks)]

        assert f(None, 1, *args()) == INVALID, fn
        assert f(h, 0, *[None if t == "B" else a for t, a in zip(toks, args())]) == OK, fn      # n = 0 touches nothing
        for i, t in enumerate(toks):
            if t == "B":
                assert f(h, 1, *args({i: None})) == INVALID, (fn, i)
                assert "NULL buffer" in err(), (fn, i, err())
            if t == "F":
                for bad in (2, 3, 1 << 8, -2):
                    assert f(h, 1, *args({i: bad})) == INVALID, (fn, bad)
                    assert "unknown flag" in err(), (fn, bad, err())
                assert f(h, 0, *args({i: 2})) == INVALID, fn     # the flag rule comes before the empty batch
                assert f(h, 1, *args({i: 1})) == OK, fn
        assert f(h, 1, *args()) == OK, (fn, err())               # a zero row: refused by value, not by status
    torch.cuda.synchronize()
    assert not hbuf[32:].any() and not dbuf.cpu().numpy()[32:].any()
