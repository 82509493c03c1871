"""SHAKE256, Ed448 signing and Ed448 verification from messages ON THE DEVICE: ncg_shake256_batch, ncg_ed448_public_key_batch,
ncg_ed448_expand_key_batch, ncg_ed448_sign_batch, ncg_ed448_challenge_batch_dev, ncg_ed448_verify_batch_msgs (host and _dev forms),
ncg_ed448_sign_check and the Python mirror, byte for byte against hashlib, Python integers, the plain-Python signer of ed448_helpers
(pinned to the reference's answers by test_ed448_sign_host.py) and the fixture tests/golden/ed448_sign_kat.json."""
import hashlib

import numpy as np
import pytest
import torch

import ed448_helpers as eh
import ed448_sign_helpers as sh
from ed448_helpers import N
from ed448_sign_helpers import EXPANDED, ONE_KEY, PREHASH
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
NMAX = 129
SIZES = [1, 63, 64, 65, 129]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _err(eng):
    return (eng.lib.ncg_last_error(eng.h) or b"").decode()


def _ctx(r):
    return bytes.fromhex(r["context"])


# ---- 1. the pieces on raw rows
@pytest.mark.parametrize("n", SIZES)
def test_check_keccak_f(n):
    states = sh.keccak_rows(NMAX)[:n]
    out = get_engine().ed448_sign_check(0, sh.lanes_words(states), np.zeros((n, 1), np.uint32))
    assert out.shape == (n, 50)
    assert [sh.words_lanes(r) for r in out] == [sh.keccak_f(s) for s in states]


def test_check_mod_n():
    vals = sh.mod_n_values()
    out = get_engine().ed448_sign_check(1, sh.int_words(vals, 29), np.zeros((len(vals), 1), np.uint32))
    assert out.shape == (len(vals), 14)
    for v, row in zip(vals, out):
        assert sh.words_int(row) == v % N, hex(v)


@pytest.mark.parametrize("n", SIZES)
def test_check_mod_n_and_muladd_batch_sizes(n):
    eng = get_engine()
    vals = sh.mod_n_values(NMAX)[:n]
    out = eng.ed448_sign_check(1, sh.int_words(vals, 29), np.zeros((n, 1), np.uint32))
    assert [sh.words_int(r) for r in out] == [v % N for v in vals]
    tr = sh.muladd_triples(NMAX)[:n]
    a = np.concatenate([sh.int_words([t[0] for t in tr], 14), sh.int_words([t[1] for t in tr], 14)], axis=1)
    out = eng.ed448_sign_check(2, a, sh.int_words([t[2] for t in tr], 14))
    assert [sh.words_int(r) for r in out] == [(r + k * s) % N for r, k, s in tr]


def test_check_muladd():
    tr = sh.muladd_triples()
    a = np.concatenate([sh.int_words([t[0] for t in tr], 14), sh.int_words([t[1] for t in tr], 14)], axis=1)
    out = get_engine().ed448_sign_check(2, a, sh.int_words([t[2] for t in tr], 14))
    assert out.shape == (len(tr), 14)
    for (r, k, s), row in zip(tr, out):
        assert sh.words_int(row) == (r + k * s) % N, (r, k, s)


def test_check_unknown_op_and_limits():
    eng = get_engine()
    out = eng.ed448_sign_check(4, np.ones((3, 4), np.uint32), np.ones((3, 4), np.uint32))
    assert out.shape == (3, 16) and not out.any()
    b = np.zeros(64, np.uint32)
    assert eng.lib.ncg_ed448_sign_check(eng.h, 0, 0, (1 << 24) + 1, b.ctypes.data, b.ctypes.data, b.ctypes.data) == INVALID
    assert "too large" in _err(eng)
    assert eng.lib.ncg_ed448_sign_check(eng.h, 0, 0, 1, b.ctypes.data, None, b.ctypes.data) == INVALID
    assert eng.lib.ncg_ed448_sign_check(eng.h, 0, 0, 0, None, None, None) == OK


# ---- 2. a signature with the nonce given: the only way to r = 0
def test_check_sign_with_a_given_nonce():
    eng = get_engine()
    seeds = [sh.rand_bytes(57, "gpu-r-seed-%d" % i) for i in range(4)]
    rs = [0, 1, 0, N - 1, 1, 0x1234567]
    rows = [(seeds[i % 4], rs[i], sh.rand_bytes(64, "gpu-r-msg-%d" % i)) for i in range(len(rs))]
    a = np.frombuffer(b"".join(sh.expanded_row(s) for s, _, _ in rows), np.uint32).reshape(len(rows), 43)
    b = np.frombuffer(b"".join(r.to_bytes(56, "little") + m for _, r, m in rows), np.uint32).reshape(len(rows), 30)
    out = eng.ed448_sign_check(3, a, b)
    assert out.shape == (len(rows), 30)
    for (seed, r, msg), row in zip(rows, out):
        raw = row.tobytes()
        want = sh.sign_with_r(msg, seed, r)
        if r == 0:
            assert want is None and raw == bytes(120)            # ok = 0 and 114 zero bytes
        else:
            assert raw[:114] == want and raw[114:116] == bytes(2) and int(row[29]) == 1
        if r == 1:
            assert raw[:57] == eh.pt_encode(eh.BASE)


# ---- 3. SHAKE256
SHAKE_LENGTHS = (0, 1, 134, 135, 136, 137, 271, 272, 1000)


@pytest.fixture(scope="module")
def shake_msgs():
    return [sh.rand_bytes(SHAKE_LENGTHS[i % len(SHAKE_LENGTHS)], "gpu-shake-%d" % i) for i in range(NMAX)]


@pytest.mark.parametrize("out_len", sh.OUT_LENS)
def test_shake256_host_and_dev_forms(shake_msgs, out_len):
    eng = get_engine()
    want = sh.rows([hashlib.shake_256(m).digest(out_len) for m in shake_msgs], out_len)
    blob, off = sh.blob(shake_msgs)
    got = eng.shake256_batch(blob, off, out_len)
    assert got.shape == want.shape and np.array_equal(got, want)
    dblob, doff = _dev(blob), _dev(off.view(np.int64))
    out = torch.full((NMAX * out_len + 8,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.shake256_batch_dev(NMAX, dblob.data_ptr(), doff.data_ptr(), out_len, out.data_ptr(), None)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(o[:NMAX * out_len].reshape(NMAX, out_len), want) and (o[NMAX * out_len:] == 0xAA).all()


def test_shake256_empty_messages_and_a_null_buffer():
    eng, n = get_engine(), 65
    off = np.zeros(n + 1, np.uint64)
    out = np.zeros((n, 64), np.uint8)
    assert eng.lib.ncg_shake256_batch(eng.h, n, None, off.ctypes.data, 64, out.ctypes.data) == OK, _err(eng)
    assert np.array_equal(out, np.tile(np.frombuffer(hashlib.shake_256(b"").digest(64), np.uint8), (n, 1)))
    doff = _dev(off.view(np.int64))
    dout = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert eng.lib.ncg_shake256_batch_dev(eng.h, n, None, doff.data_ptr(), 64, dout.data_ptr(), None) == OK, _err(eng)
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), out)
    from noble_curves_amd import ed448 as m
    assert m.ed448.shake256_batch([b"", b"abc"], 57) == [hashlib.shake_256(x).digest(57) for x in (b"", b"abc")]


# ---- 4. the fixture, bit for bit
def _sign_host(eng, keys, flags, dom, msgs):
    blob, off = sh.blob(msgs)
    n = len(msgs)
    sig, ok = np.full((n, 114), 0xAA, np.uint8), np.full(n, 7, np.uint8)
    rc = eng.lib.ncg_ed448_sign_batch(eng.h, n, keys.ctypes.data, flags, dom, len(dom), blob.ctypes.data if blob.size else None,
                                      off.ctypes.data, sig.ctypes.data, ok.ctypes.data)
    assert rc == OK, _err(eng)
    return sig, ok


def _sign_dev(eng, keys, flags, dom, msgs, stream=None):
    blob, off = sh.blob(msgs)
    n = len(msgs)
    dk, doff = _dev(keys), _dev(off.view(np.int64))
    dblob = _dev(blob) if blob.size else None
    sig = torch.full((n * 114 + 8,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = eng.lib.ncg_ed448_sign_batch_dev(eng.h, n, dk.data_ptr(), flags, dom, len(dom), dblob.data_ptr() if dblob is not None else None,
                                          doff.data_ptr(), sig.data_ptr(), ok.data_ptr(), stream.cuda_stream if stream is not None else None)
    assert rc == OK, _err(eng)
    torch.cuda.synchronize()
    s = sig.cpu().numpy()
    assert (s[n * 114:] == 0xAA).all()
    return s[:n * 114].reshape(n, 114), ok.cpu().numpy()


def test_public_keys_and_expanded_rows_against_the_fixture():
    eng, keys = get_engine(), sh.kat()["keys"]
    n = len(keys)
    s = sh.rows([bytes.fromhex(k["secretKey"]) for k in keys], 57)
    want = sh.rows([int(k["scalar"], 16).to_bytes(56, "little") + bytes.fromhex(k["prefix"]) + bytes.fromhex(k["publicKey"]) + bytes(2)
                    for k in keys], sh.KEY_BYTES)
    assert np.array_equal(eng.ed448_public_key_batch(s), want[:, 113:170])
    assert np.array_equal(eng.ed448_expand_key_batch(s), want)
    ds = _dev(s)
    pk = torch.full((n, 57), 0xAA, dtype=torch.uint8, device="cuda")
    rows = torch.full((n, sh.KEY_BYTES), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.ed448_public_key_batch_dev(n, ds.data_ptr(), pk.data_ptr())
    eng.ed448_expand_key_batch_dev(n, ds.data_ptr(), rows.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(pk.cpu().numpy(), want[:, 113:170]) and np.array_equal(rows.cpu().numpy(), want)


@pytest.mark.parametrize("variant,clen", [("ed448", 0), ("ed448", 1), ("ed448", 255), ("ed448ph", 0), ("ed448ph", 1), ("ed448ph", 255)])
@pytest.mark.parametrize("expanded", [0, EXPANDED])
def test_sign_fixture_rows_per_row_keys(variant, clen, expanded):
    eng = get_engine()
    rows = sh.kat_rows(variant, clen)
    assert rows
    ph = variant == "ed448ph"
    dom = sh.dom4(_ctx(rows[0]), ph)
    assert all(_ctx(r) == _ctx(rows[0]) for r in rows)
    seeds = [bytes.fromhex(r["secretKey"]) for r in rows]
    keys = sh.rows([sh.expanded_row(s) for s in seeds], sh.KEY_BYTES) if expanded else sh.rows(seeds, 57)
    msgs = [bytes.fromhex(r["msg"]) for r in rows]
    want = sh.rows([bytes.fromhex(r["sig"]) for r in rows], 114)
    flags = expanded | (PREHASH if ph else 0)
    sig, ok = _sign_host(eng, keys, flags, dom, msgs)
    assert ok.dtype == np.uint8 and (ok == 1).all() and np.array_equal(sig, want)
    dsig, dok = _sign_dev(eng, keys, flags, dom, msgs)
    assert (dok == 1).all() and np.array_equal(dsig, sig)


@pytest.mark.parametrize("expanded", [0, EXPANDED])
def test_sign_fixture_rows_one_key(expanded):
    eng = get_engine()
    for variant, clen in (("ed448", 0), ("ed448", 255), ("ed448ph", 0)):
        ph = variant == "ed448ph"
        rows = sh.kat_rows(variant, clen)
        seed = rows[0]["secretKey"]
        rows = [r for r in rows if r["secretKey"] == seed]
        assert len(rows) >= 2
        key = sh.rows([sh.expanded_row(bytes.fromhex(seed)) if expanded else bytes.fromhex(seed)], sh.KEY_BYTES if expanded else 57)
        sig, ok = _sign_dev(eng, key, expanded | ONE_KEY | (PREHASH if ph else 0), sh.dom4(_ctx(rows[0]), ph), [bytes.fromhex(r["msg"]) for r in rows])
        assert (ok == 1).all() and np.array_equal(sig, sh.rows([bytes.fromhex(r["sig"]) for r in rows], 114))


# ---- 5. seeded rows against the signer, accepted by the EXISTING verifier given host-hashed challenges
@pytest.fixture(scope="module")
def seeded():
    """NMAX (seed, msg, sig) under the context b"gpu" with the signer's signature; computed once"""
    ctx = b"gpu"
    lens = sh.sign_edge_lengths(len(ctx))
    out = []
    for i in range(NMAX):
        seed = sh.rand_bytes(57, "gpu-seed-%d" % (i % 7))
        msg = sh.rand_bytes(lens[i % len(lens)] if i % 2 else (11 * i) % 83, "gpu-msg-%d" % i)
        out.append((seed, msg, sh.sign(msg, seed, ctx)))
    return ctx, out


@pytest.mark.parametrize("n", [1, 65, 129])
def test_seeded_rows_sign_then_verify(seeded, n):
    eng = get_engine()
    ctx, rows = seeded
    rows = rows[:n]
    seeds, msgs = [r[0] for r in rows], [r[1] for r in rows]
    sig, ok = _sign_host(eng, sh.rows(seeds, 57), 0, sh.dom4(ctx), msgs)
    assert (ok == 1).all() and ok.shape == (n,)                 # a row silently refused cannot hide
    assert np.array_equal(sig, sh.rows([r[2] for r in rows], 114))
    pk = eng.ed448_public_key_batch(sh.rows(seeds, 57))
    ks = sh.rows([(eh.challenge(sig[i, :57].tobytes(), pk[i].tobytes(), msgs[i], ctx) % N).to_bytes(56, "little") for i in range(n)], 56)
    assert eng.ed448_verify_batch(sig, pk, ks).all()


def test_side_stream(seeded):
    eng, st = get_engine(), torch.cuda.Stream()
    ctx, rows = seeded
    rows = rows[:65]
    sig, ok = _sign_dev(eng, sh.rows([r[0] for r in rows], 57), 0, sh.dom4(ctx), [r[1] for r in rows], stream=st)
    assert (ok == 1).all() and np.array_equal(sig, sh.rows([r[2] for r in rows], 114))


# ---- 6. the challenge alone
def _challenge_dev(eng, sig, pk, dom, msgs, prehash):
    blob, off = sh.blob(msgs)
    n = len(msgs)
    dsig, dpk, doff = _dev(sig), _dev(pk), _dev(off.view(np.int64))
    dblob = _dev(blob) if blob.size else None
    k = torch.full((n, 56), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.ed448_challenge_batch_dev(n, dsig.data_ptr(), dpk.data_ptr(), dom, dblob.data_ptr() if dblob is not None else None, doff.data_ptr(),
                                  k.data_ptr(), prehash=prehash)
    torch.cuda.synchronize()
    return k.cpu().numpy()


@pytest.mark.parametrize("variant,clen", [("ed448", 0), ("ed448", 1), ("ed448", 255), ("ed448ph", 0)])
def test_challenge_on_the_fixture_edge_lengths(variant, clen):
    rows = sh.kat_rows(variant, clen)
    ph = variant == "ed448ph"
    ctx = _ctx(rows[0])
    pub = {k["secretKey"]: bytes.fromhex(k["publicKey"]) for k in sh.kat()["keys"]}
    sig = sh.rows([bytes.fromhex(r["sig"]) for r in rows], 114)
    pk = sh.rows([pub[r["secretKey"]] for r in rows], 57)
    msgs = [bytes.fromhex(r["msg"]) for r in rows]
    got = _challenge_dev(get_engine(), sig, pk, sh.dom4(ctx, ph), msgs, ph)
    want = sh.rows([(eh.challenge(sig[i, :57].tobytes(), pk[i].tobytes(), msgs[i], ctx, ph) % N).to_bytes(56, "little")
                    for i in range(len(rows))], 56)
    assert np.array_equal(got, want)


# ---- 7, 8. verification from messages against the host-hash path
def _verify_rows(ctx, ph):
    """(sig, msg, pk) rows: valid ones, a flipped bit in R / S / A / the message, s >= n, small-order A, undecodable R"""
    rows = []
    for i in range(12):
        seed = sh.rand_bytes(57, "gpu-v-seed-%d" % (i % 3))
        msg = sh.rand_bytes((37 * i) % 150, "gpu-v-msg-%d" % i)
        rows.append((sh.sign(msg, seed, ctx, ph), msg, sh.expand(seed)[2]))
    sig, msg, pk = rows[1]
    s0 = int.from_bytes(sig[57:], "little")
    rows += [(eh.flip(sig, 3), msg, pk), (eh.flip(sig, 60), msg, pk), (sig, msg, eh.flip(pk, 5)), (sig, msg + b"!", pk), (sig, msg[:-1], pk),
             (sig[:57] + (s0 + N).to_bytes(57, "little"), msg, pk), (sig[:57] + N.to_bytes(57, "little"), msg, pk),
             (sig[:113] + b"\x01", msg, pk), (eh.P.to_bytes(57, "little") + sig[57:], msg, pk),
             (bytes(56) + b"\x7f" + sig[57:], msg, pk)]
    rows += [(eh.pt_encode(eh.pt_mul(eh.BASE, 5)) + (5).to_bytes(57, "little"), msg, eh.pt_encode(t)) for t in eh.TORSION]
    return rows


@pytest.mark.parametrize("ctx,ph", [(b"", False), (b"verify-ctx", False), (b"", True), (b"ph-ctx", True)])
def test_verify_from_messages_equals_the_host_hash_path(ctx, ph):
    eng = get_engine()
    rows = _verify_rows(ctx, ph)
    rows = [rows[i % len(rows)] for i in range(65)]
    sig, pk = sh.rows([r[0] for r in rows], 114), sh.rows([r[2] for r in rows], 57)
    msgs = [r[1] for r in rows]
    ks = sh.rows([(eh.challenge(r[0][:57], r[2], r[1], ctx, ph) % N).to_bytes(56, "little") for r in rows], 56)
    want = eng.ed448_verify_batch(sig, pk, ks)
    assert want[:12].all() and not want[12:26].any()
    blob, off = sh.blob(msgs)
    dom = sh.dom4(ctx, ph)
    got = eng.ed448_verify_batch_msgs(sig, pk, blob, off, dom, prehash=ph)
    assert got.shape == want.shape and np.array_equal(got, want)
    dsig, dpk, dblob, doff = _dev(sig), _dev(pk), _dev(blob), _dev(off.view(np.int64))
    ok = torch.full((65,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.ed448_verify_batch_msgs_dev(65, dsig.data_ptr(), dpk.data_ptr(), dom, dblob.data_ptr(), doff.data_ptr(), ok.data_ptr(), prehash=ph)
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy().astype(bool), want)           # the _dev form equals the host form
    # a signature does not verify under the other variant's domain
    other = eng.ed448_verify_batch_msgs(sig, pk, blob, off, sh.dom4(ctx, not ph), prehash=ph)
    assert not other.any()


# ---- 9. argument checks
def test_argument_table():
    """NULL pointers, n = 0, n = 2^31, unknown flag bits, the dom rules and out_len for every new entry point.  Safe whatever the
    library does: every non-NULL pointer is a 256-byte slice of a zeroed 4 KB buffer (device memory for the _dev forms; dom is host
    memory in both) and n = 1, so a missing check runs on valid memory and fails the test."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    hbuf = np.zeros(4096, dtype=np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    # B a required buffer, M the message blob (may be NULL when every message is empty), F / V the flags (sign: 0..7, verify: 0 or 4),
    # D dom, N dom_len, O out_len, S the stream
    specs = [("ncg_shake256_batch", "M B O B"), ("ncg_shake256_batch_dev", "M B O B S"),
             ("ncg_ed448_challenge_batch_dev", "B B V D N M B B S"),
             ("ncg_ed448_verify_batch_msgs", "B B V D N M B B"), ("ncg_ed448_verify_batch_msgs_dev", "B B V D N M B B S"),
             ("ncg_ed448_public_key_batch", "B B"), ("ncg_ed448_public_key_batch_dev", "B B S"),
             ("ncg_ed448_expand_key_batch", "B B"), ("ncg_ed448_expand_key_batch_dev", "B B S"),
             ("ncg_ed448_sign_batch", "B F D N M B B B"), ("ncg_ed448_sign_batch_dev", "B F D N M B B B S")]
    for fn, tmpl in specs:
        f, toks = getattr(L, fn), tmpl.split()
        buf = dbuf.data_ptr() if fn.endswith("_dev") else hbuf.ctypes.data

        def args(over=None, toks=toks, buf=buf):   # every buffer its own 256-byte slice: an output never lands on the offsets
            base = {"F": 0, "V": 0, "D": None, "N": 0, "O": 64, "S": None}
            return [(over or {}).get(i, buf + 256 * i if t in "BM" else base[t]) for i, t in enumerate(toks)]

        assert f(None, 1, *args()) == INVALID, fn
        assert f(h, 0, *[None if t in "BM" else a for t, a in zip(toks, args())]) == OK, fn      # n = 0 touches nothing
        assert f(h, 1 << 31, *args()) == INVALID and "too large" in _err(eng), (fn, _err(eng))   # before any buffer is read
        for i, t in enumerate(toks):
            if t == "B":
                assert f(h, 1, *args({i: None})) == INVALID, (fn, i)
                assert "NULL buffer" in _err(eng), (fn, i, _err(eng))
            if t in "FV":
                good = range(8) if t == "F" else (0, 4)
                for bad in (8, 15, 1 << 8, -8) + ((1, 2, 3) if t == "V" else ()):
                    assert f(h, 1, *args({i: bad})) == INVALID, (fn, bad)
                    assert "unknown flag" in _err(eng), (fn, bad, _err(eng))
                assert f(h, 0, *args({i: 8})) == INVALID, fn     # the flag rule comes before the empty batch
                for g in good:
                    assert f(h, 1, *args({i: g})) == OK, (fn, g, _err(eng))
            if t == "N":
                assert f(h, 1, *args({i - 1: hbuf.ctypes.data, i: 266})) == INVALID, fn
                assert "dom_len" in _err(eng), (fn, _err(eng))
                assert f(h, 1, *args({i: 1})) == INVALID, fn     # dom = NULL with dom_len = 1
                assert "NULL buffer" in _err(eng), (fn, _err(eng))
                assert f(h, 1, *args({i - 1: hbuf.ctypes.data, i: 265})) == OK, (fn, _err(eng))
            if t == "O":
                for bad in (0, 65536):
                    assert f(h, 1, *args({i: bad})) == INVALID and "out_len" in _err(eng), (fn, bad, _err(eng))
                assert f(h, 0, *args({i: 0})) == INVALID, fn
            if t == "M":
                assert f(h, 1, *args({i: None})) == OK, (fn, _err(eng))     # one empty message needs no blob
        assert f(h, 1, *args()) == OK, (fn, _err(eng))
    torch.cuda.synchronize()
    for b in (hbuf.reshape(16, 256), dbuf.cpu().numpy().reshape(16, 256)):
        assert not b[:, 172:].any() and not b[9:].any()         # at most one key row per slice, nothing past the last argument


def test_offsets_and_alignment():
    eng = get_engine()
    L, h = eng.lib, eng.h
    b = np.zeros(1024, np.uint8)
    off = np.array([0, 5, 3], np.uint64)
    p = b.ctypes.data
    assert L.ncg_shake256_batch(h, 2, p, off.ctypes.data, 32, p + 256) == INVALID and "offsets must not decrease" in _err(eng)
    assert L.ncg_ed448_sign_batch(h, 2, p, 0, None, 0, p + 256, off.ctypes.data, p + 512, p + 768) == INVALID
    assert "offsets must not decrease" in _err(eng)
    assert L.ncg_ed448_verify_batch_msgs(h, 2, p, p + 256, 0, None, 0, p + 512, off.ctypes.data, p + 768) == INVALID
    assert "offsets must not decrease" in _err(eng)
    off = np.array([0, 5], np.uint64)
    assert L.ncg_shake256_batch(h, 1, None, off.ctypes.data, 32, p + 256) == INVALID and "NULL message buffer" in _err(eng)
    # expanded key rows and challenges are words on the device: a misaligned pointer is refused, not dereferenced
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    doff = _dev(np.zeros(2, np.int64))
    torch.cuda.synchronize()
    q = d.data_ptr()
    assert L.ncg_ed448_sign_batch_dev(h, 1, q + 1, EXPANDED, None, 0, None, doff.data_ptr(), q + 512, q + 1024, None) == INVALID
    assert "4-byte aligned" in _err(eng)
    assert L.ncg_ed448_expand_key_batch_dev(h, 1, q, q + 258, None) == INVALID and "4-byte aligned" in _err(eng)
    assert L.ncg_ed448_challenge_batch_dev(h, 1, q, q + 256, 0, None, 0, None, doff.data_ptr(), q + 513, None) == INVALID
    assert "4-byte aligned" in _err(eng)
    # packed rows may sit at any address: seeds, public keys and signatures at odd pointers
    dom = sh.dom4()
    assert L.ncg_ed448_sign_batch_dev(h, 1, q + 1, 0, dom, len(dom), None, doff.data_ptr(), q + 513, q + 1024, None) == OK, _err(eng)
    assert L.ncg_ed448_public_key_batch_dev(h, 1, q + 1, q + 2049, None) == OK, _err(eng)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert got[513:627].tobytes() == eh.sign(b"", bytes(57)) and got[2049:2106].tobytes() == eh.public_key(bytes(57))


# ---- 10. the Python mirror
def test_python_mirror_against_the_fixture():
    from noble_curves_amd import ed448 as m
    kat = sh.kat()
    for k in kat["keys"][:3]:
        sk = bytes.fromhex(k["secretKey"])
        assert m.ed448.getPublicKey(sk).hex() == k["publicKey"]
        ext = m.ed448.getExtendedPublicKey(sk)
        assert (ext["head"].hex(), ext["prefix"].hex(), ext["scalar"], ext["pointBytes"].hex()) == \
            (k["head"], k["prefix"], int(k["scalar"], 16), k["pointBytes"])
    sks = [bytes.fromhex(k["secretKey"]) for k in kat["keys"]]
    assert [p.hex() for p in m.ed448.getPublicKey_batch(sks)] == [k["publicKey"] for k in kat["keys"]]
    pub = {k["secretKey"]: bytes.fromhex(k["publicKey"]) for k in kat["keys"]}
    ns = {"ed448": m.ed448, "ed448ph": m.ed448ph}
    for r in kat["sign"][::5]:
        sk, msg, ctx = bytes.fromhex(r["secretKey"]), bytes.fromhex(r["msg"]), _ctx(r)
        sig = ns[r["variant"]].sign(msg, sk, context=ctx)
        assert sig.hex() == r["sig"], r
        for dh in (False, True):
            assert ns[r["variant"]].verify(sig, msg, pub[r["secretKey"]], context=ctx, device_hash=dh) is True
            assert ns[r["variant"]].verify(sig, msg + b"x", pub[r["secretKey"]], context=ctx, device_hash=dh) is False
    msgs = [b"m%d" % i for i in range(5)]
    assert m.ed448.sign_batch(msgs, sks[:5]) == [sh.sign(x, s) for x, s in zip(msgs, sks)]
    assert m.ed448.sign_batch(msgs, sks[0], context=b"c") == [sh.sign(x, sks[0], b"c") for x in msgs]
    rows = m.ed448.expand_keys(sks[:5])
    assert m.ed448.sign_batch(msgs, rows, expanded=True) == [sh.sign(x, s) for x, s in zip(msgs, sks)]
    assert m.ed448ph.sign_batch(msgs, rows[0], expanded=True) == [sh.sign(x, sks[0], b"", True) for x in msgs]


@pytest.mark.parametrize("ctx,ph", [(b"", False), (b"mirror", False), (b"", True)])
def test_python_verify_batch_device_hash_equals_the_default(ctx, ph):
    from noble_curves_amd import ed448 as m
    ns = m.ed448ph if ph else m.ed448
    rows = _verify_rows(ctx, ph)
    sigs, msgs, pks = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    want = ns.verify_batch(sigs, msgs, pks, context=ctx)
    assert want[:12] == [True] * 12 and not any(want[12:])
    assert ns.verify_batch(sigs, msgs, pks, context=ctx, device_hash=True) == want
    # a context above 255 bytes keeps its host handling: rows that cannot verify are False, a row that could raises like the reference
    for dh in (False, True):
        assert ns.verify_batch(sigs[20:26], msgs[20:26], pks[20:26], context=bytes(256), device_hash=dh) == [False] * 6   # R, A refused
        with pytest.raises(ValueError) as e:
            ns.verify_batch(sigs[:1], msgs[:1], pks[:1], context=bytes(256), device_hash=dh)
        assert str(e.value) == "context must be smaller than 255, got: 256"
