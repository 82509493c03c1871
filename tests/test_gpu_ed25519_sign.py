"""Ed25519 signing ON THE DEVICE: ncg_ed25519_public_key_batch, ncg_ed25519_expand_key_batch and ncg_ed25519_sign_batch (host and
_dev forms) and the Python namespaces, byte for byte against the plain-Python signer of ed25519_sign_helpers (itself pinned to the
reference's vectors and fixture by test_ed25519_sign_host.py), the reference's 160 sign vectors and its ed25519ctx / ed25519ph
answers (tests/golden/ed25519_sign_kat.json)."""
import numpy as np
import pytest
import torch

import ed25519_sign_helpers as sh
from ed25519_sign_helpers import EXPANDED, ONE_KEY, PREHASH
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
NMAX = 257
CTX255 = bytes((7 * i + 1) & 255 for i in range(255))
# name -> (context, prehash); "plain" has no domain at all
VARIANTS = {"plain": (None, False), "ctx0": (b"", False), "ctx1": (b"\xa5", False), "ctx255": (CTX255, False), "ph": (None, True)}


def _dom(name):
    context, prehash = VARIANTS[name]
    return b"" if name == "plain" else sh.dom2(context, prehash)


def _lengths(name):
    """NMAX message lengths: 0, 1000, both sides of every block edge of the two hashes under this domain (for plain ed25519: 79 / 80,
    207 / 208, 47 / 48, 175 / 176), and of the prehash itself for ed25519ph; the rest short"""
    head = [0, 1000] + sh.edge_lengths(len(_dom(name))) + ([111, 112, 239, 240] if VARIANTS[name][1] else [])
    return head + [(13 * i) % 97 for i in range(NMAX - len(head))]


@pytest.fixture(scope="module")
def seeds():
    return [sh.rand_bytes(32, "gpu-seed-%d" % i) for i in range(NMAX)]


@pytest.fixture(scope="module")
def cases(seeds):
    """per variant: the messages, the signer's signatures under per-row keys, and under seeds[0] alone; computed once"""
    out = {}
    for name, (context, prehash) in VARIANTS.items():
        msgs = [sh.rand_bytes(n, "gpu-msg-%s-%d" % (name, i)) for i, n in enumerate(_lengths(name))]
        ctx = None if name == "plain" else context
        per_row = [sh.sign(m, s, ctx, prehash) for m, s in zip(msgs, seeds)]
        one_key = [sh.sign(m, seeds[0], ctx, prehash) for m in msgs]
        out[name] = (msgs, sh.rows(per_row, 64), sh.rows(one_key, 64))
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sign_host(eng, keys, flags, dom, msgs):
    blob, off = sh.blob(msgs)
    n = len(msgs)
    sig, ok = np.full((n, 64), 0xAA, np.uint8), np.full(n, 7, np.uint8)
    rc = eng.lib.ncg_ed25519_sign_batch(eng.h, n, keys.ctypes.data, flags, dom if dom else None, len(dom),
                                        blob.ctypes.data if blob.size else None, off.ctypes.data, sig.ctypes.data, ok.ctypes.data)
    assert rc == OK, eng.lib.ncg_last_error(eng.h)
    return sig, ok


def _sign_dev(eng, keys, flags, dom, msgs, stream=None):
    blob, off = sh.blob(msgs)
    n = len(msgs)
    dk, doff = _dev(keys), _dev(off.view(np.int64))
    dblob = _dev(blob) if blob.size else None
    sig = torch.full((n, 64), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = eng.lib.ncg_ed25519_sign_batch_dev(eng.h, n, dk.data_ptr(), flags, dom if dom else None, len(dom),
                                            dblob.data_ptr() if dblob is not None else None, doff.data_ptr(), sig.data_ptr(),
                                            ok.data_ptr(), stream.cuda_stream if stream is not None else None)
    assert rc == OK, eng.lib.ncg_last_error(eng.h)
    torch.cuda.synchronize()
    return sig.cpu().numpy(), ok.cpu().numpy()


def _keys(seeds, flags):
    ks = seeds[:1] if flags & ONE_KEY else seeds
    return sh.rows([sh.expanded_row(s) for s in ks], 96) if flags & EXPANDED else sh.rows(ks, 32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_batch_sizes_plain_seeds_dev_form(cases, seeds, n):
    msgs, want, _ = cases["plain"]
    sig, ok = _sign_dev(get_engine(), _keys(seeds[:n], 0), 0, b"", msgs[:n])
    assert sig.shape == want[:n].shape and ok.all() and np.array_equal(sig, want[:n])


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("kflags", [0, EXPANDED, ONE_KEY, EXPANDED | ONE_KEY])
def test_bytes_against_the_signer_host_and_dev_forms(cases, seeds, name, kflags):
    eng = get_engine()
    msgs, per_row, one_key = cases[name]
    want = one_key if kflags & ONE_KEY else per_row
    flags = kflags | (PREHASH if VARIANTS[name][1] else 0)
    keys, dom = _keys(seeds, kflags), _dom(name)
    host_sig, host_ok = _sign_host(eng, keys, flags, dom, msgs)
    dev_sig, dev_ok = _sign_dev(eng, keys, flags, dom, msgs)
    assert host_sig.shape == dev_sig.shape == want.shape == (NMAX, 64)
    assert host_ok.all() and dev_ok.all()
    assert np.array_equal(host_sig, want)
    assert np.array_equal(dev_sig, host_sig)           # the _dev form equals the host form bit for bit
    if kflags & ONE_KEY:                                # ONE_KEY equals the same key repeated
        rep = np.repeat(keys, NMAX, axis=0)
        rep_sig, rep_ok = _sign_dev(eng, rep, flags & ~ONE_KEY, dom, msgs)
        assert rep_sig.shape == dev_sig.shape and rep_ok.all() and np.array_equal(rep_sig, dev_sig)


def test_side_stream(cases, seeds):
    eng, st = get_engine(), torch.cuda.Stream()
    for name in ("plain", "ctx255", "ph"):
        msgs, want, _ = cases[name]
        flags = PREHASH if VARIANTS[name][1] else 0
        sig, ok = _sign_dev(eng, _keys(seeds[:130], 0), flags, _dom(name), msgs[:130], stream=st)
        assert sig.shape == want[:130].shape and ok.all() and np.array_equal(sig, want[:130])
    sd = _dev(sh.rows(seeds[:130], 32))
    pk = torch.zeros((130, 32), dtype=torch.uint8, device="cuda")
    rows = torch.zeros((130, 96), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert eng.lib.ncg_ed25519_public_key_batch_dev(eng.h, 130, sd.data_ptr(), pk.data_ptr(), st.cuda_stream) == OK
    assert eng.lib.ncg_ed25519_expand_key_batch_dev(eng.h, 130, sd.data_ptr(), rows.data_ptr(), st.cuda_stream) == OK
    torch.cuda.synchronize()
    want_rows = sh.rows([sh.expanded_row(s) for s in seeds[:130]], 96)
    assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(pk.cpu().numpy(), want_rows[:, 64:])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_public_keys_and_expanded_rows(seeds, n):
    eng = get_engine()
    want = sh.rows([sh.expanded_row(s) for s in seeds[:n]], 96)
    s = sh.rows(seeds[:n], 32)
    assert np.array_equal(eng.ed25519_public_key_batch(s), want[:, 64:])
    assert np.array_equal(eng.ed25519_expand_key_batch(s), want)
    ds = _dev(s)
    pk = torch.full((n, 32), 0xAA, dtype=torch.uint8, device="cuda")
    rows = torch.full((n, 96), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert eng.lib.ncg_ed25519_public_key_batch_dev(eng.h, n, ds.data_ptr(), pk.data_ptr(), None) == OK
    assert eng.lib.ncg_ed25519_expand_key_batch_dev(eng.h, n, ds.data_ptr(), rows.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(pk.cpu().numpy(), want[:, 64:]) and np.array_equal(rows.cpu().numpy(), want)


def test_seeds_at_any_address_expanded_rows_on_words(cases, seeds):
    """seeds are read byte by byte, so a device pointer to them may be odd; expanded rows and signatures are words and refused there"""
    eng, n = get_engine(), 65
    msgs, want, _ = cases["plain"]
    blob, off = sh.blob(msgs[:n])
    raw = torch.zeros(n * 96 + 4, dtype=torch.uint8, device="cuda")
    raw[1:1 + n * 32] = _dev(sh.rows(seeds[:n], 32)).reshape(-1)
    dblob, doff = _dev(blob), _dev(off.view(np.int64))
    sig = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    ok = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    pk = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L, h = eng.lib, eng.h
    assert L.ncg_ed25519_sign_batch_dev(h, n, raw.data_ptr() + 1, 0, None, 0, dblob.data_ptr(), doff.data_ptr(), sig.data_ptr(), ok.data_ptr(), None) == OK
    assert L.ncg_ed25519_public_key_batch_dev(h, n, raw.data_ptr() + 1, pk.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert ok.cpu().numpy().all() and np.array_equal(sig.cpu().numpy(), want[:n])
    assert np.array_equal(pk.cpu().numpy(), sh.rows([sh.expand(s)[2] for s in seeds[:n]], 32))
    err = lambda: (L.ncg_last_error(h) or b"").decode()  # noqa: E731
    assert L.ncg_ed25519_sign_batch_dev(h, n, raw.data_ptr() + 1, EXPANDED, None, 0, dblob.data_ptr(), doff.data_ptr(), sig.data_ptr(), ok.data_ptr(),
                                        None) == INVALID and "4-byte aligned" in err()
    assert L.ncg_ed25519_sign_batch_dev(h, n, raw.data_ptr(), 0, None, 0, dblob.data_ptr(), doff.data_ptr(), sig.data_ptr() + 2, ok.data_ptr(),
                                        None) == INVALID and "4-byte aligned" in err()
    assert L.ncg_ed25519_public_key_batch_dev(h, n, raw.data_ptr(), pk.data_ptr() + 1, None) == INVALID and "4-byte aligned" in err()


def test_golden_vectors_in_one_call_each():
    """the reference's 160 sk / pk / msg / sig rows: one ncg_ed25519_public_key_batch and one ncg_ed25519_sign_batch"""
    eng, vec = get_engine(), sh.vectors()
    assert len(vec) == 160
    s = sh.rows([v["sk"][:32] for v in vec], 32)
    pk = np.zeros((160, 32), np.uint8)
    assert eng.lib.ncg_ed25519_public_key_batch(eng.h, 160, s.ctypes.data, pk.ctypes.data) == OK
    assert np.array_equal(pk, sh.rows([v["pk"] for v in vec], 32))
    sig, ok = _sign_host(eng, s, 0, b"", [v["msg"] for v in vec])
    assert ok.all() and np.array_equal(sig, sh.rows([v["sig"][:64] for v in vec], 64))


def test_round_trip_through_the_batch_verifier(cases, seeds):
    eng = get_engine()
    msgs, _, _ = cases["plain"]
    s = sh.rows(seeds, 32)
    sig, ok = _sign_host(eng, s, 0, b"", msgs)
    pk = eng.ed25519_public_key_batch(s)
    blob, off = sh.blob(msgs)
    assert ok.all() and eng.ed25519_verify_batch_msgs(sig, pk, blob, off, zip215=False).all()
    # the signature over message i against message i + 1 (the last against the first): every row fails
    shifted = msgs[1:] + msgs[:1]
    assert all(a != b for a, b in zip(msgs, shifted))
    blob, off = sh.blob(shifted)
    assert not eng.ed25519_verify_batch_msgs(sig, pk, blob, off, zip215=False).any()


def test_argument_table():
    """NULL pointers, n = 0, unknown flag bits and the dom rules for the six entry points.  Safe whatever the library does: every
    non-NULL pointer is a 256-byte slice of a zeroed 4 KB buffer (device memory for the _dev forms; dom is host memory in both) and
    n = 1, so a missing check runs on valid memory and fails the test."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    hbuf = np.zeros(4096, dtype=np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    err = lambda: (L.ncg_last_error(h) or b"").decode()  # noqa: E731
    # B a required buffer, M the message blob (may be NULL when every message is empty), F the flags, D dom, N dom_len, S the stream
    specs = [("ncg_ed25519_public_key_batch", "B B"), ("ncg_ed25519_public_key_batch_dev", "B B S"),
             ("ncg_ed25519_expand_key_batch", "B B"), ("ncg_ed25519_expand_key_batch_dev", "B B S"),
             ("ncg_ed25519_sign_batch", "B F D N M B B B"), ("ncg_ed25519_sign_batch_dev", "B F D N M B B B S")]
    for fn, tmpl in specs:
        f, toks = getattr(L, fn), tmpl.split()
        buf = dbuf.data_ptr() if fn.endswith("_dev") else hbuf.ctypes.data

        def args(over=None, toks=toks, buf=buf):   # every buffer its own 256-byte slice: an output never lands on the offsets
            base = {"F": 0, "D": None, "N": 0, "S": None}
            return [(over or {}).get(i, buf + 256 * i if t in "BM" else base[t]) for i, t in enumerate(toks)]

        assert f(None, 1, *args()) == INVALID, fn
        assert f(h, 0, *[None if t in "BM" else a for t, a in zip(toks, args())]) == OK, fn      # n = 0 touches nothing
        for i, t in enumerate(toks):
            if t == "B":
                assert f(h, 1, *args({i: None})) == INVALID, (fn, i)
                assert "NULL buffer" in err(), (fn, i, err())
            if t == "F":
                for bad in (8, 15, 1 << 8, -8):
                    assert f(h, 1, *args({i: bad})) == INVALID, (fn, bad)
                    assert "unknown flag" in err(), (fn, bad, err())
                assert f(h, 0, *args({i: 8})) == INVALID, fn     # the flag rule comes before the empty batch
                for good in range(8):
                    assert f(h, 1, *args({i: good})) == OK, (fn, good, err())
            if t == "N":
                assert f(h, 1, *args({i - 1: hbuf.ctypes.data, i: 290})) == INVALID, fn
                assert "dom_len" in err(), (fn, err())
                assert f(h, 1, *args({i: 1})) == INVALID, fn     # dom = NULL with dom_len = 1
                assert "NULL buffer" in err(), (fn, err())
                assert f(h, 1, *args({i - 1: hbuf.ctypes.data, i: 289})) == OK, (fn, err())
            if t == "M":
                assert f(h, 1, *args({i: None})) == OK, (fn, err())     # one empty message needs no blob
        assert f(h, 1, *args()) == OK, (fn, err())
    torch.cuda.synchronize()
    for b in (hbuf.reshape(16, 256), dbuf.cpu().numpy().reshape(16, 256)):
        assert not b[:, 96:].any() and not b[9:].any()          # at most one 96-byte row per slice, nothing past the last argument


def test_python_namespaces_against_the_fixture():
    from noble_curves_amd import ed25519 as ed
    kat = sh.kat()
    for k in kat["keys"][:4]:
        sk = bytes.fromhex(k["secretKey"])
        assert ed.getPublicKey(sk).hex() == k["publicKey"]
        ext = ed.getExtendedPublicKey(sk)
        assert (ext["head"].hex(), ext["prefix"].hex(), ext["scalar"], ext["pointBytes"].hex()) == \
            (k["head"], k["prefix"], int(k["scalar"], 16), k["pointBytes"])
    assert [p.hex() for p in ed.getPublicKey_batch([bytes.fromhex(k["secretKey"]) for k in kat["keys"]])] == [k["publicKey"] for k in kat["keys"]]
    pub = {k["secretKey"]: bytes.fromhex(k["publicKey"]) for k in kat["keys"]}
    ns = {"ed25519": ed, "ed25519ctx": ed.ed25519ctx, "ed25519ph": ed.ed25519ph}
    for r in kat["sign"]:
        sk, msg, ctx = bytes.fromhex(r["secretKey"]), bytes.fromhex(r["msg"]), sh.kat_context(r)
        kw = {} if ctx is None else {"context": ctx}
        sig = ns[r["variant"]].sign(msg, sk, **kw)
        assert sig.hex() == r["sig"], r
        assert ns[r["variant"]].verify(sig, msg, pub[r["secretKey"]], **kw) is True
        assert ns[r["variant"]].verify(sig, msg + b"x", pub[r["secretKey"]], **kw) is False
    # the batch forms: one key for all, a list of keys, expanded rows; a signature of one variant does not verify under another
    sk = [bytes.fromhex(k["secretKey"]) for k in kat["keys"][:5]]
    msgs = [b"m%d" % i for i in range(5)]
    assert ed.sign_batch(msgs, sk) == [sh.sign(m, s) for m, s in zip(msgs, sk)]
    assert ed.sign_batch(msgs, sk[0]) == [sh.sign(m, sk[0]) for m in msgs]
    rows = ed.expand_keys(sk)
    assert ed.ed25519ctx.sign_batch(msgs, rows, context=b"c", expanded=True) == [sh.sign(m, s, b"c") for m, s in zip(msgs, sk)]
    assert ed.ed25519ph.sign_batch(msgs, rows[0], expanded=True) == [sh.sign(m, sk[0], None, True) for m in msgs]
    sig = ed.ed25519ctx.sign(msgs[0], sk[0], context=b"c")
    assert ed.verify(sig, msgs[0], pub[sk[0].hex()], context=b"c") is True
    assert ed.verify(sig, msgs[0], pub[sk[0].hex()]) is False
    assert ed.ed25519ph.verify(sig, msgs[0], pub[sk[0].hex()], context=b"c") is False
    assert ed.verify(ed.ed25519ph.sign(msgs[1], sk[1]), msgs[1], pub[sk[1].hex()], prehash=True) is True
