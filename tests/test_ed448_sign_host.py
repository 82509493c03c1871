"""SHAKE256, the reduction mod the Ed448 group order and Ed448 signing on the CPU twins of csrc/keccak.hpp and csrc/ed448_sign.hpp
(the lane code the kernels run), and the argument checks of the Python mirror, without a GPU.  The expectations are hashlib, Python
integers and the plain-Python signer of ed448_helpers, itself checked first against the reference's own answers for ed448 / ed448ph
(tests/golden/ed448_sign_kat.json)."""
import hashlib
import random

import numpy as np
import pytest

import ed448_helpers as eh
import ed448_sign_helpers as sh
from ed448_helpers import N
from ed448_sign_helpers import EXPANDED, PREHASH


def _ctx(r):
    return bytes.fromhex(r["context"])


def test_signer_reproduces_the_fixture():
    kat = sh.kat()
    assert len(kat["keys"]) == 30
    for k in kat["keys"]:
        seed = bytes.fromhex(k["secretKey"])
        s, prefix = eh.secret_scalar(seed)
        assert s.to_bytes(57, "little").hex() == k["head"] and prefix.hex() == k["prefix"]
        assert s % N == int(k["scalar"], 16) and eh.public_key(seed).hex() == k["publicKey"] == k["pointBytes"]
    assert {r["variant"] for r in kat["sign"]} == {"ed448", "ed448ph"}
    for r in kat["sign"]:
        got = eh.sign(bytes.fromhex(r["msg"]), bytes.fromhex(r["secretKey"]), _ctx(r), r["variant"] == "ed448ph")
        assert got.hex() == r["sig"], r
    for clen in (0, 1, 255):                 # the fixture has every edge length of both hashes under each context
        have = {len(r["msg"]) // 2 for r in sh.kat_rows("ed448", clen)}
        assert set(sh.sign_edge_lengths(clen)) | {0, 1000} <= have, clen
        for fixed in (10 + clen + 57, 10 + clen + 114):
            assert {(fixed + n) % 136 for n in have} >= {0, 1, 134, 135}
    assert set(sh.PH_LENGTHS) <= {len(r["msg"]) // 2 for r in sh.kat_rows("ed448ph", 0)}
    assert {len(_ctx(r)) for r in sh.kat_rows("ed448ph")} == {0, 1, 255}


def test_keccak_f_against_the_restatement():
    lanes = [0] * 25                          # the restatement itself: SHAKE256 of the empty message is one permutation
    lanes[0], lanes[16] = 0x1f, 0x80 << 56
    assert b"".join(v.to_bytes(8, "little") for v in sh.keccak_f(lanes))[:136] == hashlib.shake_256(b"").digest(136)
    states = sh.keccak_rows(12)
    assert sh.ht_keccak_f(states) == [sh.keccak_f(s) for s in states]


# the splits of `total` bytes over (dom, a, b, msg) that the kernels use: the message alone (k_shake256, prehash, expand), dom ||
# prefix || M (nonce), dom || R || A || M (challenge, finish) under the three context lengths, and empty segments
def _splits(total):
    out = [(0, None, None), (0, 0, None), (0, 0, 0)]
    for dom_len in (10, 11, 265):
        out += [(dom_len, 57, None), (dom_len, 57, 57)]
    for dom_len, a, b in out:
        mlen = total - dom_len - (a or 0) - (b or 0)
        if mlen >= 0:
            yield dom_len, a, b, mlen


def test_shake256_segments_against_hashlib():
    rng = random.Random("shake-segments")
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    ran = 0
    for total in list(range(301)) + [1000]:
        data = rb(total)
        want = hashlib.shake_256(data).digest(273)
        for dom_len, a, b, mlen in _splits(total):
            p1 = dom_len + (a or 0)
            p2 = p1 + (b or 0)
            for out_len in sh.OUT_LENS:
                got = sh.ht_shake256(data[:dom_len], None if a is None else data[dom_len:p1], None if b is None else data[p1:p2], data[p2:],
                                     out_len)
                assert got == want[:out_len], (total, dom_len, a, b, out_len)
                ran += 1
    assert ran > 10000


@pytest.mark.parametrize("out_len", sh.OUT_LENS)
def test_shake256_output_lengths(out_len):
    for total in (0, 1, 134, 135, 136, 137, 271, 272, 300, 1000):
        data = sh.rand_bytes(total, "out-%d" % total)
        assert sh.ht_shake256(b"", None, None, data, out_len) == hashlib.shake_256(data).digest(out_len), total
        if total >= 124:
            assert sh.ht_shake256(data[:10], data[10:67], data[67:124], data[124:], out_len) == hashlib.shake_256(data).digest(out_len), total


def test_mod_n_against_python():
    vals = sh.mod_n_values()
    assert len(vals) > 2030
    got = sh.ht_mod_n(vals)
    for v, g in zip(vals, got):
        assert g == v % N, hex(v)


def test_muladd_against_python():
    triples = sh.muladd_triples()
    assert len(triples) == 527
    got = sh.ht_muladd(triples)
    for (r, k, s), g in zip(triples, got):
        assert g == (r + k * s) % N, (r, k, s)


def test_check_widths():
    for op, want in sh.SIGN_CHECK_WORDS.items():
        w = [np.zeros(1, np.int32) for _ in range(3)]
        sh.ht().ht_ed448_sign_widths(op, *[x.ctypes.data for x in w])
        assert tuple(int(x[0]) for x in w) == want
    w = [np.full(1, 9, np.int32) for _ in range(3)]
    sh.ht().ht_ed448_sign_widths(4, *[x.ctypes.data for x in w])
    assert [int(x[0]) for x in w] == [0, 0, 0]


def test_expand_against_the_fixture():
    keys = sh.kat()["keys"]
    seeds = [bytes.fromhex(k["secretKey"]) for k in keys]
    got = sh.ht_expand(seeds)
    assert got == [sh.expanded_row(s) for s in seeds]
    for k, row in zip(keys, got):
        assert len(row) == sh.KEY_BYTES and row[170:] == bytes(2)
        assert int.from_bytes(row[:56], "little") == int(k["scalar"], 16) != 0
        assert row[56:113].hex() == k["prefix"] and row[113:170].hex() == k["publicKey"]


@pytest.mark.parametrize("expanded", [0, EXPANDED])
def test_sign_fixture_rows_on_the_twin(expanded):
    for r in sh.kat()["sign"]:
        ph = r["variant"] == "ed448ph"
        seed = bytes.fromhex(r["secretKey"])
        key = sh.expanded_row(seed) if expanded else seed
        sig, ok = sh.ht_sign(key, bytes.fromhex(r["msg"]), expanded | (PREHASH if ph else 0), sh.dom4(_ctx(r), ph))
        assert ok == 1 and sig.hex() == r["sig"], r


def test_sign_with_a_given_nonce():
    seed, msg = sh.rand_bytes(57, "r-seed"), b"nonce"
    for flags, key in ((0, seed), (EXPANDED, sh.expanded_row(seed))):
        sig, ok = sh.ht_sign(key, msg, flags, r=0)
        assert ok == 0 and sig == bytes(114)
        sig, ok = sh.ht_sign(key, msg, flags, r=1)
        assert ok == 1 and sig[:57] == eh.pt_encode(eh.BASE) and sig == sh.sign_with_r(msg, seed, 1)
        sig, ok = sh.ht_sign(key, msg, flags, r=N - 1)
        assert ok == 1 and sig == sh.sign_with_r(msg, seed, N - 1)
    assert sh.sign_with_r(msg, seed, 0) is None
    # the twin refuses what the C ABI refuses
    b = sh._buf(bytes(172))
    assert sh.ht().ht_ed448_sign(b.ctypes.data, 8, b.ctypes.data, 10, b.ctypes.data, 0, b.ctypes.data, b.ctypes.data) == -1
    assert sh.ht().ht_ed448_sign(b.ctypes.data, 2, b.ctypes.data, 10, b.ctypes.data, 0, b.ctypes.data, b.ctypes.data) == -1
    assert sh.ht().ht_ed448_sign(b.ctypes.data, 0, b.ctypes.data, 266, b.ctypes.data, 0, b.ctypes.data, b.ctypes.data) == -1


# ---- the Python mirror: every check happens before the device is touched (a sentinel engine fails the test if it is reached)
class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError("the device was reached: " + name)


def test_python_layer_messages():
    from noble_curves_amd import ed448 as m
    err, eng, sk, msg = sh.kat()["errors"], _NoEngine(), bytes(57), b"abc"
    assert err["secret_key_length_56"] == '"secretKey" expected Uint8Array of length 57, got length=56'
    assert err["context_256"] == err["context_256_ph"] == "context must be smaller than 255, got: 256" and err["context_255"] is None
    with pytest.raises(ValueError) as e:
        m.ed448.sign(msg, bytes(58), engine=eng)
    assert str(e.value) == err["secret_key_length_58"]
    with pytest.raises(ValueError) as e:
        m.ed448ph.sign(msg, bytes(114), context=msg, engine=eng)
    assert str(e.value) == err["secret_key_length_114"]
    with pytest.raises(ValueError) as e:
        m.ed448.expand_keys([sk, bytes(56)], engine=eng)
    assert str(e.value) == err["secret_key_length_56"]
    with pytest.raises(ValueError) as e:
        m.ed448.sign_batch([msg, msg], [sk, bytes(56)], engine=eng)
    assert str(e.value) == err["secret_key_length_56"]
    for ns, name in ((m.ed448, "context_256"), (m.ed448ph, "context_256_ph")):
        with pytest.raises(ValueError) as e:
            ns.sign(msg, sk, context=bytes(256), engine=eng)
        assert str(e.value) == err[name]
        with pytest.raises(ValueError) as e:
            ns.sign_batch([msg], sk, context=bytes(256), engine=eng)
        assert str(e.value) == err[name]
    with pytest.raises(TypeError):
        m.ed448.sign(msg, "not bytes", engine=eng)
    with pytest.raises(ValueError):
        m.ed448.sign_batch([msg, msg], [sk], engine=eng)
    with pytest.raises(ValueError):
        m.ed448.shake256_batch([msg], 0, engine=eng)


def test_python_sign_goes_through_the_engine():
    from noble_curves_amd import ed448 as m
    calls = []

    class Fake:
        def ed448_sign_batch(self, K, blob, off, dom, expanded, one_key, prehash):
            calls.append((K.copy(), bytes(blob), list(off), dom, expanded, one_key, prehash))
            n = len(off) - 1
            return np.zeros((n, 114), np.uint8), np.array([i != 1 for i in range(n)])

    sk = bytes(range(57))
    assert m.ed448ph.sign_batch([b"ab", b"", b"c"], sk, context=b"ctx", engine=Fake()) == [bytes(114), None, bytes(114)]
    K, blob, off, dom, expanded, one_key, prehash = calls[0]
    assert K.tobytes() == sk and blob == b"abc" and off == [0, 2, 2, 3] and dom == sh.dom4(b"ctx", True)
    assert (expanded, one_key, prehash) == (False, True, True)

    class Refuses:
        def ed448_sign_batch(self, K, blob, off, dom, expanded, one_key, prehash):
            return np.zeros((1, 114), np.uint8), np.zeros(1, bool)

    with pytest.raises(ValueError) as e:
        m.ed448.sign(b"m", sk, engine=Refuses())
    assert str(e.value) == "invalid scalar: expected 1 <= sc < curve.n"
