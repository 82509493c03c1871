"""secp256k1 signing ON THE DEVICE: ncg_secp256k1_public_key_batch, ncg_ecdsa_sign_batch[_msgs], ncg_schnorr_sign_batch (host and _dev
forms), ncg_secp256k1_sign_check and the Python namespaces, byte for byte against the plain-Python model of secp256k1_sign_helpers
(itself pinned to the reference's vectors and fixture by test_secp256k1_sign_host.py) and the reference's own answers
(tests/golden/secp256k1_sign_kat.json), then round trips through the batch verifiers and the key recovery."""
import hashlib

import numpy as np
import pytest
import torch

import secp256k1_sign_helpers as sh
from secp256k1_sign_helpers import LOW_S, N, ONE_KEY, PK_COMPRESSED, PK_UNCOMPRESSED, PK_XONLY
from noble_curves_amd import get_engine
from noble_curves_amd._native import SECP256K1

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -4
NMAX = 299


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _err(eng):
    return (eng.lib.ncg_last_error(eng.h) or b"").decode()


@pytest.fixture(scope="module")
def keys():
    return [sh.be(1), sh.be(N - 1)] + [sh.be(int.from_bytes(sh.rand_bytes(32, "gpu-sk-%d" % i), "big") % (N - 1) + 1) for i in range(NMAX - 2)]


@pytest.fixture(scope="module")
def msgs():
    """NMAX messages: both sides of every SHA-256 block edge of the prehash (55 | 56 mod 64) and of the BIP-340 hashes, the rest short"""
    head = list(sh.MSG_LENGTHS) + [183, 184]
    return [sh.rand_bytes(n, "gpu-msg-%d" % i) for i, n in enumerate(head + [(13 * i) % 97 for i in range(NMAX - len(head))])]


@pytest.fixture(scope="module")
def extras():
    return [sh.rand_bytes(32, "gpu-extra-%d" % i) for i in range(NMAX)]


@pytest.fixture(scope="module")
def model(keys, msgs, extras):
    """the model's answers, computed once: ECDSA over SHA-256 of the messages (lowS) with per-row keys, with keys[2] alone, with extra
    entropy and without lowS; BIP-340 with per-row keys and with keys[2] alone"""
    def ecdsa(ks, low_s=True, ex=None, n=NMAX):
        got = [sh.ecdsa_sign(msgs[i], ks[i], low_s, True, ex[i] if ex else None) for i in range(n)]
        return sh.rows([sh.compact(r, s) for r, s, _ in got], 64), np.array([c for _, _, c in got], np.uint8)
    return {"ecdsa": ecdsa(keys), "ecdsa_one": ecdsa([keys[2]] * NMAX), "ecdsa_extra": ecdsa(keys, ex=extras, n=65),
            "ecdsa_high": ecdsa(keys, low_s=False, n=65),
            "schnorr": sh.rows([sh.schnorr_sign(m, k, a) for m, k, a in zip(msgs, keys, extras)], 64),
            "schnorr_one": sh.rows([sh.schnorr_sign(m, keys[2], a) for m, a in zip(msgs[:65], extras)], 64)}


# ---------------------------------------------------------------- callers of the C ABI
def _ecdsa_host(eng, sk, msgs=None, hashes=None, extra=None, flags=LOW_S, recid=True):
    n = len(msgs) if hashes is None else hashes.shape[0]
    sig, rec, ok = np.full((n, 64), 0xAA, np.uint8), np.full(n, 9, np.uint8), np.full(n, 7, np.uint8)
    xp, rp = (None if extra is None else extra.ctypes.data), (rec.ctypes.data if recid else None)
    if hashes is None:
        blob, off = sh.blob(msgs)
        rc = eng.lib.ncg_ecdsa_sign_batch_msgs(eng.h, SECP256K1, n, sk.ctypes.data, blob.ctypes.data if blob.size else None, off.ctypes.data, xp,
                                               flags, sig.ctypes.data, rp, ok.ctypes.data)
    else:
        rc = eng.lib.ncg_ecdsa_sign_batch(eng.h, SECP256K1, n, sk.ctypes.data, hashes.ctypes.data, xp, flags, sig.ctypes.data, rp, ok.ctypes.data)
    assert rc == OK, _err(eng)
    return sig, rec, ok


def _ecdsa_dev(eng, sk, msgs=None, hashes=None, extra=None, flags=LOW_S, recid=True, stream=None, sk_ptr=None):
    n = len(msgs) if hashes is None else hashes.shape[0]
    dsk = _dev(sk)
    dx = None if extra is None else _dev(extra)
    sig = torch.full((n, 64), 0xAA, dtype=torch.uint8, device="cuda")
    rec = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    st = stream.cuda_stream if stream is not None else None
    xp, rp = (None if dx is None else dx.data_ptr()), (rec.data_ptr() if recid else None)
    if hashes is None:
        blob, off = sh.blob(msgs)
        dblob, doff = (_dev(blob) if blob.size else None), _dev(off.view(np.int64))
        torch.cuda.synchronize()
        rc = eng.lib.ncg_ecdsa_sign_batch_msgs_dev(eng.h, SECP256K1, n, sk_ptr or dsk.data_ptr(), dblob.data_ptr() if dblob is not None else None,
                                                   doff.data_ptr(), xp, flags, sig.data_ptr(), rp, ok.data_ptr(), st)
    else:
        dh = _dev(hashes)
        torch.cuda.synchronize()
        rc = eng.lib.ncg_ecdsa_sign_batch_dev(eng.h, SECP256K1, n, sk_ptr or dsk.data_ptr(), dh.data_ptr(), xp, flags, sig.data_ptr(), rp,
                                              ok.data_ptr(), st)
    assert rc == OK, _err(eng)
    torch.cuda.synchronize()
    return sig.cpu().numpy(), rec.cpu().numpy(), ok.cpu().numpy()


def _schnorr_host(eng, sk, aux, msgs, flags=0):
    blob, off = sh.blob(msgs)
    n = len(msgs)
    sig, ok = np.full((n, 64), 0xAA, np.uint8), np.full(n, 7, np.uint8)
    rc = eng.lib.ncg_schnorr_sign_batch(eng.h, n, sk.ctypes.data, aux.ctypes.data, blob.ctypes.data if blob.size else None, off.ctypes.data, flags,
                                        sig.ctypes.data, ok.ctypes.data)
    assert rc == OK, _err(eng)
    return sig, ok


def _schnorr_dev(eng, sk, aux, msgs, flags=0, stream=None):
    blob, off = sh.blob(msgs)
    n = len(msgs)
    dsk, da, doff = _dev(sk), _dev(aux), _dev(off.view(np.int64))
    dblob = _dev(blob) if blob.size else None
    sig = torch.full((n, 64), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = eng.lib.ncg_schnorr_sign_batch_dev(eng.h, n, dsk.data_ptr(), da.data_ptr(), dblob.data_ptr() if dblob is not None else None, doff.data_ptr(),
                                            flags, sig.data_ptr(), ok.data_ptr(), stream.cuda_stream if stream is not None else None)
    assert rc == OK, _err(eng)
    torch.cuda.synchronize()
    return sig.cpu().numpy(), ok.cpu().numpy()


# ---------------------------------------------------------------- ncg_secp256k1_sign_check
def test_check_scan_multiply_edge_scalars():
    ks = sh.edge_scalars()
    out = get_engine().secp256k1_sign_check(1, np.array([sh.words(k) for k in ks], np.uint32), np.zeros((len(ks), 1), np.uint32))
    assert out.shape == (len(ks), 16)
    for k, row in zip(ks, out):
        assert (sh.from_words(row[:8]), sh.from_words(row[8:])) == sh.mul_base(k), hex(k)
    bad = [0, N, N + 1, 2**256 - 1]                  # replaced by 1: no fault, no garbage address
    out = get_engine().secp256k1_sign_check(1, np.array([sh.words(k) for k in bad], np.uint32), np.zeros((4, 1), np.uint32))
    assert all((sh.from_words(r[:8]), sh.from_words(r[8:])) == sh.mul_base(1) for r in out)


def test_check_finish_rare_branches_and_schnorr_scalar():
    eng = get_engine()
    cases = sh.rare_finish_cases()
    a = np.array([c[0] for c in cases.values()], np.uint32)
    b = np.array([[c[1]] for c in cases.values()], np.uint32)
    out = eng.secp256k1_sign_check(2, a, b)
    for (name, c), row in zip(cases.items(), out):
        assert (sh.from_words(row[:8]), sh.from_words(row[8:16]), int(row[16]), int(row[17])) == c[2], name
    rows = [(1, 0, 0, 1), (N - 1, 1, N - 1, N - 1), (N - 1, 0, N - 1, N - 1), (0x1234 ** 9 % N, 1, 0x777 ** 20 % N, 0x4321 ** 11 % N)]
    out = eng.secp256k1_sign_check(3, np.array([sh.words(k) + sh.words(e) + sh.words(d) for k, _, e, d in rows], np.uint32),
                                   np.array([[o] for _, o, _, _ in rows], np.uint32))
    assert [sh.from_words(r) for r in out] == [sh.schnorr_scalar(k, o, e, d) for k, o, e, d in rows]


@pytest.mark.parametrize("extra", [0, 1])
def test_check_drbg_candidates_and_retry(extra):
    eng = get_engine()
    seeds = [sh.rand_bytes(96, "gpu-drbg-%d" % i) for i in range(3)]
    a = np.array([sh.bytes_words(s) for s in seeds], np.uint32)
    for j in range(4):
        out = eng.secp256k1_sign_check(0, a, np.zeros((3, 1), np.uint32), variant=(j << 1) | extra)
        for s, row in zip(seeds, out):
            gen = sh.drbg_candidates(s if extra else s[:64])
            want = [next(gen) for _ in range(j + 1)][-1]
            assert row.tobytes() == want, (extra, j)
    # the whole row with the first candidates refused: sk || hash || extra
    sk, h, ex = sh.rand_bytes(32, "retry-key"), sh.rand_bytes(32, "retry-hash"), sh.rand_bytes(32, "retry-extra")
    for refuse in range(4):
        r, s, recid = sh.ecdsa_sign(h, sk, True, False, ex if extra else None, refuse_first=refuse)
        out = eng.secp256k1_sign_check(4, np.array([sh.bytes_words(sk + h + ex)] * 2, np.uint32), np.ones((2, 1), np.uint32), variant=(refuse << 1) | extra)
        for row in out:
            assert row[:16].tobytes() == sh.compact(r, s) and (int(row[16]), int(row[17])) == (recid, 1), (extra, refuse)


def test_check_table_edges():
    eng = get_engine()
    z = np.zeros((3, 1), np.uint32)
    for op in (5, 11, -1):
        out = eng.secp256k1_sign_check(op, z, z)
        assert out.shape == (3, 16) and not out.any()
    hbuf = np.zeros(4096, np.uint8)
    p = hbuf.ctypes.data
    L, h = eng.lib, eng.h
    assert L.ncg_secp256k1_sign_check(h, 0, 0, (1 << 24) + 1, p, p, p) == INVALID and "too large" in _err(eng)
    assert L.ncg_secp256k1_sign_check(h, 0, 4 << 1, 1, p, p + 512, p + 1024) == INVALID and "variant" in _err(eng)
    assert L.ncg_secp256k1_sign_check(h, 4, 9, 1, p, p + 512, p + 1024) == INVALID and "variant" in _err(eng)
    for i in range(3):
        a = [p, p + 512, p + 1024]
        a[i] = None
        assert L.ncg_secp256k1_sign_check(h, 1, 0, 1, *a) == INVALID and "NULL buffer" in _err(eng)
    assert L.ncg_secp256k1_sign_check(None, 1, 0, 1, p, p + 512, p + 1024) == INVALID
    assert L.ncg_secp256k1_sign_check(h, 1, 0, 0, None, None, None) == OK


# ---------------------------------------------------------------- fixture rows, one call per variant
def test_fixture_public_keys():
    eng, kat = get_engine(), sh.kat()
    sk = sh.rows([bytes.fromhex(k["secretKey"]) for k in kat["keys"]], 32)
    n = sk.shape[0]
    for mode, name, width in ((PK_COMPRESSED, "compressed", 33), (PK_UNCOMPRESSED, "uncompressed", 65), (PK_XONLY, "xonly", 32)):
        out, ok = eng.secp256k1_public_key_batch(sk, mode)
        assert ok.all() and [bytes(r).hex() for r in out] == [k[name] for k in kat["keys"]]
        dsk = _dev(sk)
        dout = torch.full((n, width), 0xAA, dtype=torch.uint8, device="cuda")
        dok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert eng.lib.ncg_secp256k1_public_key_batch_dev(eng.h, n, dsk.data_ptr(), mode, dout.data_ptr(), dok.data_ptr(), None) == OK
        torch.cuda.synchronize()
        assert np.array_equal(dout.cpu().numpy(), out) and dok.cpu().numpy().all()


@pytest.mark.parametrize("prehash", [True, False])
@pytest.mark.parametrize("low_s", [True, False])
@pytest.mark.parametrize("extra", [True, False])
def test_fixture_ecdsa_host_and_dev_forms(prehash, low_s, extra):
    eng = get_engine()
    rows = [r for r in sh.kat()["ecdsa"] if (r["prehash"], r["lowS"], r["extraEntropy"] is not None) == (prehash, low_s, extra)]
    assert len(rows) == len(sh.MSG_LENGTHS)
    sk = sh.rows([bytes.fromhex(r["secretKey"]) for r in rows], 32)
    ms = [bytes.fromhex(r["msg"]) for r in rows]
    ex = sh.rows([sh.kat_extra(r) for r in rows], 32) if extra else None
    kw = {"msgs": ms} if prehash else {"hashes": sh.rows([sh.normalise_hash(m) for m in ms], 32)}
    flags = LOW_S if low_s else 0
    sig, rec, ok = _ecdsa_host(eng, sk, extra=ex, flags=flags, **kw)
    dsig, drec, dok = _ecdsa_dev(eng, sk, extra=ex, flags=flags, **kw)
    assert ok.all() and dok.all() and np.array_equal(sig, dsig) and np.array_equal(rec, drec)
    assert [bytes(s).hex() for s in sig] == [r["compact"] for r in rows]
    assert [(bytes([c]) + bytes(s)).hex() for c, s in zip(rec, sig)] == [r["recovered"] for r in rows]


def test_fixture_schnorr_host_and_dev_forms():
    eng, rows = get_engine(), sh.kat()["schnorr"]
    sk = sh.rows([bytes.fromhex(r["secretKey"]) for r in rows], 32)
    aux = sh.rows([bytes.fromhex(r["auxRand"]) for r in rows], 32)
    ms = [bytes.fromhex(r["msg"]) for r in rows]
    sig, ok = _schnorr_host(eng, sk, aux, ms)
    dsig, dok = _schnorr_dev(eng, sk, aux, ms)
    assert ok.all() and dok.all() and np.array_equal(sig, dsig) and [bytes(s).hex() for s in sig] == [r["sig"] for r in rows]


def test_reference_vectors_in_one_call():
    """the 404 `valid` rows of the reference's ECDSA vectors: prehash false, lowS true"""
    eng, vec = get_engine(), sh.ecdsa_vectors()
    sk = sh.rows([bytes.fromhex(v["d"].rjust(64, "0")) for v in vec], 32)
    H = sh.rows([sh.normalise_hash(bytes.fromhex(v["m"])) for v in vec], 32)
    sig, _, ok = _ecdsa_host(eng, sk, hashes=H)
    assert ok.all() and [bytes(s).hex() for s in sig] == [v["signature"] for v in vec]


# ---------------------------------------------------------------- batch sizes, ONE_KEY, recid, streams, addresses
@pytest.mark.parametrize("n", [1, 63, 64, 65, NMAX])
def test_batch_sizes_against_the_model(model, keys, msgs, extras, n):
    eng = get_engine()
    sk, aux = sh.rows(keys[:n], 32), sh.rows(extras[:n], 32)
    sig, rec, ok = _ecdsa_dev(eng, sk, msgs=msgs[:n])
    assert sig.shape == (n, 64) and ok.all() and np.array_equal(sig, model["ecdsa"][0][:n]) and np.array_equal(rec, model["ecdsa"][1][:n])
    ssig, sok = _schnorr_dev(eng, sk, aux, msgs[:n])
    assert ssig.shape == (n, 64) and sok.all() and np.array_equal(ssig, model["schnorr"][:n])
    want = sh.rows([sh.public_key(k) for k in keys[:n]], 33)
    out, pok = eng.secp256k1_public_key_batch(sk)
    assert pok.all() and np.array_equal(out, want)


def test_one_key_against_per_row_keys(model, keys, msgs, extras):
    eng = get_engine()
    one = sh.rows(keys[2:3], 32)
    sig, rec, ok = _ecdsa_host(eng, one, msgs=msgs, flags=LOW_S | ONE_KEY)
    dsig, drec, dok = _ecdsa_dev(eng, one, msgs=msgs, flags=LOW_S | ONE_KEY)
    rsig, rrec, rok = _ecdsa_dev(eng, np.repeat(one, NMAX, axis=0), msgs=msgs)
    assert ok.all() and dok.all() and rok.all()
    assert np.array_equal(sig, model["ecdsa_one"][0]) and np.array_equal(rec, model["ecdsa_one"][1])
    assert np.array_equal(dsig, sig) and np.array_equal(rsig, sig) and np.array_equal(drec, rec) and np.array_equal(rrec, rec)
    aux = sh.rows(extras[:65], 32)
    ssig, sok = _schnorr_host(eng, one, aux, msgs[:65], ONE_KEY)
    dssig, dsok = _schnorr_dev(eng, one, aux, msgs[:65], ONE_KEY)
    rssig, rsok = _schnorr_dev(eng, np.repeat(one, 65, axis=0), aux, msgs[:65])
    assert sok.all() and dsok.all() and rsok.all() and np.array_equal(ssig, model["schnorr_one"])
    assert np.array_equal(dssig, ssig) and np.array_equal(rssig, ssig)


def test_extra_entropy_high_s_and_null_recid(model, keys, msgs, extras):
    eng, n = get_engine(), 65
    sk, ex = sh.rows(keys[:n], 32), sh.rows(extras[:n], 32)
    sig, rec, ok = _ecdsa_dev(eng, sk, msgs=msgs[:n], extra=ex)
    assert ok.all() and np.array_equal(sig, model["ecdsa_extra"][0]) and np.array_equal(rec, model["ecdsa_extra"][1])
    sig, rec, ok = _ecdsa_host(eng, sk, msgs=msgs[:n], flags=0)
    assert ok.all() and np.array_equal(sig, model["ecdsa_high"][0]) and np.array_equal(rec, model["ecdsa_high"][1])
    assert any(int.from_bytes(bytes(s[32:]), "big") > N >> 1 for s in sig)
    for fn in (_ecdsa_host, _ecdsa_dev):               # out_recid NULL: the same signatures, the array untouched
        sig2, rec2, ok2 = fn(eng, sk, msgs=msgs[:n], flags=0, recid=False)
        assert ok2.all() and np.array_equal(sig2, sig) and (rec2 == 9).all()


def test_side_stream(model, keys, msgs, extras):
    eng, st, n = get_engine(), torch.cuda.Stream(), 130
    sk, aux = sh.rows(keys[:n], 32), sh.rows(extras[:n], 32)
    sig, rec, ok = _ecdsa_dev(eng, sk, msgs=msgs[:n], stream=st)
    assert ok.all() and np.array_equal(sig, model["ecdsa"][0][:n]) and np.array_equal(rec, model["ecdsa"][1][:n])
    H = sh.rows([hashlib.sha256(m).digest() for m in msgs[:n]], 32)
    sig, rec, ok = _ecdsa_dev(eng, sk, hashes=H, stream=st)
    assert ok.all() and np.array_equal(sig, model["ecdsa"][0][:n])
    ssig, sok = _schnorr_dev(eng, sk, aux, msgs[:n], stream=st)
    assert sok.all() and np.array_equal(ssig, model["schnorr"][:n])
    dsk = _dev(sk)
    out = torch.zeros((n, 33), dtype=torch.uint8, device="cuda")
    pok = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert eng.lib.ncg_secp256k1_public_key_batch_dev(eng.h, n, dsk.data_ptr(), PK_COMPRESSED, out.data_ptr(), pok.data_ptr(), st.cuda_stream) == OK
    torch.cuda.synchronize()
    assert pok.cpu().numpy().all() and np.array_equal(out.cpu().numpy(), sh.rows([sh.public_key(k) for k in keys[:n]], 33))


def test_inputs_at_odd_host_addresses(model, keys, msgs, extras):
    """every row is read byte by byte: keys, hashes, aux rows and outputs may sit at any address"""
    eng, n = get_engine(), 65
    L, h = eng.lib, eng.h
    raw = np.zeros(n * 32 * 3 + n * 64 + 2 * n + 64, np.uint8)
    off0 = 1 - raw.ctypes.data % 2                                                                   # an odd address inside raw
    o_sk, o_h, o_x, o_sig, o_rec, o_ok = off0, off0 + n * 32, off0 + n * 64, off0 + n * 96, off0 + n * 160, off0 + n * 161
    assert (raw.ctypes.data + o_sk) % 2 == 1 and (raw.ctypes.data + o_sig) % 2 == 1
    raw[o_sk:o_sk + n * 32] = sh.rows(keys[:n], 32).reshape(-1)
    raw[o_h:o_h + n * 32] = sh.rows([hashlib.sha256(m).digest() for m in msgs[:n]], 32).reshape(-1)
    raw[o_x:o_x + n * 32] = sh.rows(extras[:n], 32).reshape(-1)
    p = raw.ctypes.data
    assert L.ncg_ecdsa_sign_batch(h, SECP256K1, n, p + o_sk, p + o_h, p + o_x, LOW_S, p + o_sig, p + o_rec, p + o_ok) == OK, _err(eng)
    assert raw[o_ok:o_ok + n].all() and np.array_equal(raw[o_sig:o_sig + n * 64].reshape(n, 64), model["ecdsa_extra"][0])
    assert np.array_equal(raw[o_rec:o_rec + n], model["ecdsa_extra"][1])
    blob, off = sh.blob(msgs[:n])
    raw[o_sig:o_sig + n * 65] = 0
    assert L.ncg_schnorr_sign_batch(h, n, p + o_sk, p + o_x, blob.ctypes.data, off.ctypes.data, 0, p + o_sig, p + o_ok) == OK, _err(eng)
    assert raw[o_ok:o_ok + n].all() and np.array_equal(raw[o_sig:o_sig + n * 64].reshape(n, 64), model["schnorr"][:n])
    out = np.zeros(n * 33 + 1, np.uint8)
    assert L.ncg_secp256k1_public_key_batch(h, n, p + o_sk, PK_COMPRESSED, out.ctypes.data + 1, p + o_ok) == OK, _err(eng)
    assert np.array_equal(out[1:].reshape(n, 33), sh.rows([sh.public_key(k) for k in keys[:n]], 33))


def test_invalid_keys_leave_their_neighbours_alone(model, keys, msgs, extras):
    eng, n = get_engine(), 70
    bad = {0: 0, 31: N, 64: 2**256 - 1, 69: N + 1}
    ks = [sh.be(bad[i]) if i in bad else keys[i] for i in range(n)]
    sk, aux = sh.rows(ks, 32), sh.rows(extras[:n], 32)
    good = np.array([i not in bad for i in range(n)])
    for sig, rec, ok in (_ecdsa_host(eng, sk, msgs=msgs[:n]), _ecdsa_dev(eng, sk, msgs=msgs[:n])):
        assert np.array_equal(ok.astype(bool), good) and not sig[~good].any() and not rec[~good].any()
        assert np.array_equal(sig[good], model["ecdsa"][0][:n][good]) and np.array_equal(rec[good], model["ecdsa"][1][:n][good])
    for sig, ok in (_schnorr_host(eng, sk, aux, msgs[:n]), _schnorr_dev(eng, sk, aux, msgs[:n])):
        assert np.array_equal(ok.astype(bool), good) and not sig[~good].any() and np.array_equal(sig[good], model["schnorr"][:n][good])
    for mode, width in ((PK_COMPRESSED, 33), (PK_UNCOMPRESSED, 65), (PK_XONLY, 32)):
        out, ok = eng.secp256k1_public_key_batch(sk, mode)
        assert np.array_equal(ok, good) and not out[~good].any()
        assert np.array_equal(out[good], sh.rows([sh.public_key(k, mode) for i, k in enumerate(ks) if i not in bad], width))
    # a refused ONE key refuses every row
    sig, rec, ok = _ecdsa_dev(eng, sh.rows([sh.be(N)], 32), msgs=msgs[:5], flags=LOW_S | ONE_KEY)
    assert not ok.any() and not sig.any()


# ---------------------------------------------------------------- round trips through the verifiers
def test_round_trips(keys, msgs, extras):
    eng = get_engine()
    sk, aux = sh.rows(keys, 32), sh.rows(extras, 32)
    pub, pok = eng.secp256k1_public_key_batch(sk)
    pub65, _ = eng.secp256k1_public_key_batch(sk, PK_UNCOMPRESSED)
    xonly, _ = eng.secp256k1_public_key_batch(sk, PK_XONLY)
    assert pok.all()
    H = sh.rows([hashlib.sha256(m).digest() for m in msgs], 32)
    shifted = msgs[1:] + msgs[:1]
    assert all(a != b for a, b in zip(msgs, shifted))
    for low_s in (True, False):
        sig, rec, ok = _ecdsa_host(eng, sk, msgs=msgs, flags=LOW_S if low_s else 0)
        assert ok.all()
        assert eng.ecdsa_verify_batch_msgs(sig, msgs, pub, low_s=low_s).all() and eng.ecdsa_verify_batch(sig, H, pub65, low_s=low_s).all()
        assert not eng.ecdsa_verify_batch_msgs(sig, shifted, pub, low_s=low_s).any()
        pts, rok = eng.ecdsa_recover_batch(np.concatenate([rec.reshape(-1, 1), sig], axis=1), H)
        assert rok.all()
        # the recovered point is the signer's key: x and y little-endian in the wire point, big-endian in the SEC1 key
        assert np.array_equal(pts[:, 31::-1], pub65[:, 1:33]) and np.array_equal(pts[:, :31:-1], pub65[:, 33:])
    ssig, sok = _schnorr_host(eng, sk, aux, msgs)
    assert sok.all() and eng.schnorr_verify_batch_msgs(ssig, msgs, xonly).all() and not eng.schnorr_verify_batch_msgs(ssig, shifted, xonly).any()


# ---------------------------------------------------------------- arguments
def test_argument_table():
    """NULL pointers, n = 0, unknown flag bits and refused curves for the eight entry points.  Safe whatever the library does: every
    non-NULL pointer is a 256-byte slice of a zeroed 4 KB buffer (device memory for the _dev forms) and n = 1, so a missing check runs
    on valid memory and fails the test."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    hbuf = np.zeros(4096, dtype=np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    # C the curve, B a required buffer, O an optional one, M the message blob (may be NULL when every message is empty), F sign flags
    # (known: the bits of `known`), P the public-key mode, S the stream
    specs = [("ncg_secp256k1_public_key_batch", "B P B B", 0), ("ncg_secp256k1_public_key_batch_dev", "B P B B S", 0),
             ("ncg_ecdsa_sign_batch", "C B B O F B O B", 5), ("ncg_ecdsa_sign_batch_dev", "C B B O F B O B S", 5),
             ("ncg_ecdsa_sign_batch_msgs", "C B M B O F B O B", 5), ("ncg_ecdsa_sign_batch_msgs_dev", "C B M B O F B O B S", 5),
             ("ncg_schnorr_sign_batch", "B B M B F B B", 4), ("ncg_schnorr_sign_batch_dev", "B B M B F B B S", 4)]
    for fn, tmpl, known in specs:
        f, toks = getattr(L, fn), tmpl.split()
        buf = dbuf.data_ptr() if fn.endswith("_dev") else hbuf.ctypes.data
        nfirst = 1 if toks[0] == "C" else 0       # n follows the curve where there is one

        def call(ctx, n, over=None, toks=toks, buf=buf, nfirst=nfirst, f=f):
            base = {"C": SECP256K1, "F": 0, "P": 0, "S": None}
            a = [(over or {}).get(i, buf + 256 * i if t in "BMO" else base[t]) for i, t in enumerate(toks)]
            return f(ctx, *a[:nfirst], n, *a[nfirst:])

        assert call(None, 1) == INVALID, fn
        assert call(h, 0, {i: None for i, t in enumerate(toks) if t in "BMO"}) == OK, fn      # n = 0 touches nothing
        for i, t in enumerate(toks):
            if t == "B":
                assert call(h, 1, {i: None}) == INVALID, (fn, i)
                assert "NULL buffer" in _err(eng), (fn, i, _err(eng))
            if t in "OM":
                assert call(h, 1, {i: None}) == OK, (fn, i, _err(eng))       # optional, or one empty message
            if t == "F":
                for bad in (2, 8, 15, 1 << 8, -8):
                    assert call(h, 1, {i: bad}) == INVALID, (fn, bad)
                    assert "unknown flag" in _err(eng), (fn, bad, _err(eng))
                assert call(h, 0, {i: 8}) == INVALID, fn     # the flag rule comes before the empty batch
                for good in (0, 1, 4, 5):
                    if good & ~known == 0:
                        assert call(h, 1, {i: good}) == OK, (fn, good, _err(eng))
            if t == "P":
                for bad in (3, -1, 1 << 8):
                    assert call(h, 1, {i: bad}) == INVALID and "unknown flags" in _err(eng), (fn, bad)
                for good in (0, 1, 2):
                    assert call(h, 1, {i: good}) == OK, (fn, good, _err(eng))
            if t == "C":
                for bad in (2, 4, 5, 9):
                    assert call(h, 1, {i: bad}) == UNSUPPORTED and "secp256k1 only" in _err(eng), (fn, bad)
        assert call(h, 1) == OK, (fn, _err(eng))
    torch.cuda.synchronize()
    for b in (hbuf.reshape(16, 256), dbuf.cpu().numpy().reshape(16, 256)):
        assert not b[:, 65:].any() and not b[9:].any()          # at most one row per slice, nothing past the last argument


# ---------------------------------------------------------------- the Python namespaces
def test_python_namespaces_against_the_fixture():
    from noble_curves_amd import ecdsa as ec, schnorr as sn
    kat = sh.kat()
    err = kat["errors"]
    sks = [bytes.fromhex(k["secretKey"]) for k in kat["keys"]]
    assert [p.hex() for p in ec.getPublicKeyBatch(sks)] == [k["compressed"] for k in kat["keys"]]
    assert [p.hex() for p in ec.getPublicKeyBatch(sks, isCompressed=False)] == [k["uncompressed"] for k in kat["keys"]]
    assert [p.hex() for p in sn.getPublicKey_batch(sks)] == [k["xonly"] for k in kat["keys"]]
    assert ec.getPublicKey(sks[0]).hex() == kat["keys"][0]["compressed"] and sn.getPublicKey(sks[1]).hex() == kat["keys"][1]["xonly"]
    pub = {k["secretKey"]: bytes.fromhex(k["compressed"]) for k in kat["keys"]}
    for fmt in ("compact", "recovered", "der"):
        for prehash in (True, False):
            for low_s in (True, False):
                rows = [r for r in kat["ecdsa"] if (r["prehash"], r["lowS"]) == (prehash, low_s)]
                for ex in (True, False):
                    sub = [r for r in rows if (r["extraEntropy"] is not None) == ex]
                    got = ec.sign_batch([bytes.fromhex(r["msg"]) for r in sub], [bytes.fromhex(r["secretKey"]) for r in sub], lowS=low_s,
                                        prehash=prehash, format=fmt, extraEntropy=[sh.kat_extra(r) for r in sub] if ex else False,
                                        verify=(fmt == "compact"))
                    assert [g.hex() for g in got] == [r[fmt] for r in sub], (fmt, prehash, low_s, ex)
    r0 = kat["ecdsa"][0]
    sig = ec.sign(bytes.fromhex(r0["msg"]), bytes.fromhex(r0["secretKey"]))
    assert sig.hex() == r0["compact"] and ec.verify(sig, bytes.fromhex(r0["msg"]), pub[r0["secretKey"]]) is True
    rec = ec.sign_batch([bytes.fromhex(r0["msg"])], [bytes.fromhex(r0["secretKey"])], format="recovered")
    assert ec.recoverPublicKeyBatch(rec, [bytes.fromhex(r0["msg"])]) == [pub[r0["secretKey"]]]
    ms = [b"m%d" % i for i in range(5)]
    assert ec.sign_batch(ms, sks[3]) == [sh.compact(*sh.ecdsa_sign(m, sks[3])[:2]) for m in ms]                  # one key for all
    fresh = ec.sign_batch(ms, sks[3], extraEntropy=True, verify=True)                                           # os.urandom per row
    assert len(set(fresh)) == 5 and all(a != b for a, b in zip(fresh, ec.sign_batch(ms, sks[3])))
    rows = kat["schnorr"]
    got = sn.sign_batch([bytes.fromhex(r["msg"]) for r in rows], [bytes.fromhex(r["secretKey"]) for r in rows],
                        [bytes.fromhex(r["auxRand"]) for r in rows])
    assert [g.hex() for g in got] == [r["sig"] for r in rows]
    assert sn.sign(bytes.fromhex(rows[0]["msg"]), bytes.fromhex(rows[0]["secretKey"]), bytes.fromhex(rows[0]["auxRand"])).hex() == rows[0]["sig"]
    s1, s2 = sn.sign(b"msg", sks[4]), sn.sign(b"msg", sks[4])                                                    # fresh aux by default
    assert s1 != s2 and sn.verify_batch([s1, s2], [b"msg", b"msg"], [sn.getPublicKey(sks[4])] * 2) == [True, True]
    assert sn.sign_batch(ms, sks[4], bytes(32), verify=False) == [sh.schnorr_sign(m, sks[4], bytes(32)) for m in ms]
    assert ec.sign_batch([], []) == [] and sn.sign_batch([], []) == [] and ec.getPublicKeyBatch([]) == []

    def raises(exc, message, f, *a, **kw):
        with pytest.raises(exc) as e:
            f(*a, **kw)
        assert str(e.value) == message, (str(e.value), message)

    m, good = bytes(32), sh.be(3)
    raises(ValueError, err["ecdsa_secret_key_0"], ec.sign, m, sh.be(0))
    raises(ValueError, err["ecdsa_secret_key_n"], ec.sign, m, sh.be(N))
    raises(ValueError, err["ecdsa_secret_key_max"], ec.sign, m, sh.be(2**256 - 1))
    raises(ValueError, err["ecdsa_secret_key_length_31"], ec.sign, m, bytes(31))
    raises(ValueError, err["ecdsa_secret_key_length_33"], ec.sign, m, bytes(33))
    raises(TypeError, err["ecdsa_message_not_bytes"], ec.sign, "abc", good)
    raises(ValueError, err["public_key_secret_key_0"], ec.getPublicKey, sh.be(0))
    raises(ValueError, err["public_key_secret_key_n"], ec.getPublicKey, sh.be(N))
    raises(ValueError, err["public_key_secret_key_max"], ec.getPublicKey, sh.be(2**256 - 1))
    raises(ValueError, err["public_key_secret_key_length_31"], ec.getPublicKey, bytes(31))
    raises(ValueError, err["public_key_secret_key_length_33"], ec.getPublicKey, bytes(33))
    raises(ValueError, err["schnorr_secret_key_0"], sn.sign, m, sh.be(0), m)
    raises(ValueError, err["schnorr_secret_key_n"], sn.sign, m, sh.be(N), m)
    raises(ValueError, err["schnorr_secret_key_max"], sn.sign, m, sh.be(2**256 - 1), m)
    raises(ValueError, err["schnorr_secret_key_length_31"], sn.sign, m, bytes(31), m)
    raises(ValueError, err["schnorr_secret_key_length_33"], sn.sign, m, bytes(33), m)
    raises(ValueError, err["schnorr_public_key_secret_key_0"], sn.getPublicKey, sh.be(0))
    raises(ValueError, err["schnorr_public_key_secret_key_length_31"], sn.getPublicKey, bytes(31))
    raises(ValueError, err["schnorr_aux_rand_length_31"], sn.sign, m, good, bytes(31))
    raises(TypeError, err["schnorr_message_not_bytes"], sn.sign, "abc", good, m)
    with pytest.raises(ValueError, match="only 32-byte extra entropy is offered in batch"):
        ec.sign_batch([m], [good], extraEntropy=[bytes(31)])
    with pytest.raises(ValueError, match="input is too large"):
        ec.sign_batch([bytes(8193)], [good], prehash=False)
    assert len(ec.sign_batch([bytes(8192), b"", b"\x01"], good, prehash=False)) == 3
