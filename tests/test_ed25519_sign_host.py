"""Ed25519 signing on the CPU twins of csrc/ed25519_sign.hip (the lane code the kernels run) and the argument checks of the Python
mirror, without a GPU.  The expectation is a plain-Python signer (ed25519_sign_helpers), itself checked first against the reference's
160 sign vectors and against the reference's own answers for ed25519 / ed25519ctx / ed25519ph (tests/golden/ed25519_sign_kat.json)."""
import hashlib
import random

import pytest

import ed25519_sign_helpers as sh
from ed25519_sign_helpers import EXPANDED, L, PREHASH


def test_signer_reproduces_the_reference_vectors():
    vec = sh.vectors()
    assert len(vec) == 160
    for i, v in enumerate(vec):
        seed = v["sk"][:32]
        assert sh.expand(seed)[2] == v["pk"], i
        assert sh.sign(v["msg"], seed) == v["sig"][:64], i


def test_signer_reproduces_the_fixture():
    kat = sh.kat()
    for k in kat["keys"]:
        scalar, prefix, pk = sh.expand(bytes.fromhex(k["secretKey"]))
        assert (pk.hex(), prefix.hex(), scalar) == (k["publicKey"], k["prefix"], int(k["scalar"], 16))
    assert {r["variant"] for r in kat["sign"]} == {"ed25519", "ed25519ctx", "ed25519ph"}
    assert {len(sh.kat_context(r)) for r in kat["sign"] if r["variant"] == "ed25519ctx"} == {0, 1, 255}
    for r in kat["sign"]:
        got = sh.sign(bytes.fromhex(r["msg"]), bytes.fromhex(r["secretKey"]), sh.kat_context(r) if r["variant"] != "ed25519" else None,
                      r["variant"] == "ed25519ph")
        assert got.hex() == r["sig"], r
    for dom_len in (0, 34, 35, 289):       # the fixture has every edge length of its domains
        variant, clen = ("ed25519", None) if dom_len == 0 else ("ed25519ctx", dom_len - 34)
        have = {len(r["msg"]) // 2 for r in kat["sign"] if r["variant"] == variant and (clen is None or len(sh.kat_context(r)) == clen)}
        assert set(sh.edge_lengths(dom_len)) <= have, dom_len


# total lengths at the edges of the 17-byte padding rule; a dom longer than the total cannot reach it, so each edge is also taken one
# and two blocks later (the same residues mod 128), where every dom length fits
TOTALS = [0, 111, 112, 239, 240, 367] + [368, 495, 496, 623, 624]


@pytest.mark.parametrize("dom_len", [0, 34, 289])
def test_sha512_segments_against_hashlib(dom_len):
    rng = random.Random("segments-%d" % dom_len)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    ran = set()
    for total in TOTALS:
        for nseg in (0, 1, 2):             # no per-row segment, one (the nonce hash), two (the challenge hash)
            mlen = total - dom_len - 32 * nseg
            if mlen < 0:
                continue
            dom, a, b, msg = rb(dom_len), rb(32), rb(32), rb(mlen)
            a32, b32 = (a if nseg >= 1 else None), (b if nseg == 2 else None)
            want = hashlib.sha512(dom + (a32 or b"") + (b32 or b"") + msg).digest()
            assert sh.ht_sha512_segments(dom, a32, b32, msg) == want, (dom_len, total, nseg)
            ran.add(total)
    assert ran == {t for t in TOTALS if t >= dom_len}
    if dom_len == 0:                       # b32 alone, and a long message
        assert sh.ht_sha512_segments(b"", None, b"\x07" * 32, b"") == hashlib.sha512(b"\x07" * 32).digest()
        assert sh.ht_sha512_segments(b"", None, None, b"x" * 1000) == hashlib.sha512(b"x" * 1000).digest()


def _digits_scalar(digits):
    """the odd scalar whose signed 4-bit digits (least significant first) are `digits`"""
    return sum(d << (4 * i) for i, d in enumerate(digits))


def test_mul_base_scan_against_the_oracle():
    from oracle.curves import Ed25519
    rng = random.Random("scan")
    ks = [0, 1, 2, 3, 8, L - 1, L - 2, 2**252, 2**253 - 1]
    # the recoding of a scalar below 2^253 has the top digit +1 over 63 free digits: all +15 (2^253 - 1), all -15 (1), alternating
    ks += [_digits_scalar([15] * 63 + [1]), _digits_scalar([-15] * 63 + [1]), _digits_scalar([15, -15] * 31 + [15, 1]),
           _digits_scalar([-15, 15] * 31 + [-15, 1])]
    assert ks[9] == 2**253 - 1 and ks[10] == 1
    ks += [k - 1 for k in ks[9:]]         # the even neighbours: the same walks, then the was_even correction
    rnd = [rng.randrange(L) for _ in range(64)]
    rnd[:32] = [k | 1 for k in rnd[:32]]
    rnd[32:] = [k & ~1 for k in rnd[32:]]
    ks += rnd
    assert all(0 <= k < 2**255 for k in ks)
    got = sh.ht_mul_base_scan(ks)
    for k, g in zip(ks, got):
        assert g == Ed25519.BASE.multiplyUnsafe(k % L).toBytes(), hex(k)     # 2^252 and 2^253 - 1 lie above L: B has order L


def test_expand_against_the_signer():
    seeds = [bytes.fromhex(k["secretKey"]) for k in sh.kat()["keys"]]
    assert sh.ht_expand(seeds) == [sh.expanded_row(s) for s in seeds]
    for k, row in zip(sh.kat()["keys"], sh.ht_expand(seeds)):
        assert row[64:].hex() == k["publicKey"] and row[32:64].hex() == k["prefix"]
        assert int.from_bytes(row[:32], "little") == int(k["scalar"], 16)


VARIANTS = [("plain", None, False), ("ctx0", b"", False), ("ctx1", b"\x5a", False), ("ctx255", bytes(range(255)), False),
            ("ph", None, True), ("ph-ctx", b"context", True)]


@pytest.mark.parametrize("expanded", [0, EXPANDED])
@pytest.mark.parametrize("name,context,prehash", VARIANTS)
def test_sign_against_the_signer(name, context, prehash, expanded):
    plain = name == "plain"
    dom = b"" if plain else sh.dom2(context, prehash)
    lengths = sorted(set(sh.edge_lengths(len(dom))) | {0, 1, 111, 112, 1000})
    for i, n in enumerate(lengths):
        seed = sh.rand_bytes(32, "seed-%s-%d" % (name, i % 3))
        msg = sh.rand_bytes(n, "msg-%s-%d" % (name, n))
        key = sh.expanded_row(seed) if expanded else seed
        sig, ok = sh.ht_sign(key, msg, expanded | (PREHASH if prehash else 0), dom)
        assert ok == 1 and sig == sh.sign(msg, seed, None if plain else context, prehash), (name, n)


def test_sign_fixture_rows_on_the_twin():
    for r in sh.kat()["sign"]:
        ph = r["variant"] == "ed25519ph"
        dom = b"" if r["variant"] == "ed25519" else sh.dom2(sh.kat_context(r), ph)
        sig, ok = sh.ht_sign(bytes.fromhex(r["secretKey"]), bytes.fromhex(r["msg"]), PREHASH if ph else 0, dom)
        assert ok == 1 and sig.hex() == r["sig"], r


def test_sign_with_a_given_nonce():
    seed, msg = sh.rand_bytes(32, "r-seed"), b"nonce"
    for flags, key in ((0, seed), (EXPANDED, sh.expanded_row(seed))):
        sig, ok = sh.ht_sign(key, msg, flags, r=0)
        assert ok == 0 and sig == bytes(64)
        for r in (1, L - 1):
            sig, ok = sh.ht_sign(key, msg, flags, r=r)
            assert ok == 1 and sig == sh.sign(msg, seed, r=r), r
    assert sh.sign(msg, seed, r=0) is None
    # the twin refuses what the C ABI refuses
    b = sh._buf(bytes(96))
    assert sh.ht().ht_ed25519_sign(b.ctypes.data, 8, b.ctypes.data, 0, b.ctypes.data, 0, b.ctypes.data, b.ctypes.data) == -1
    assert sh.ht().ht_ed25519_sign(b.ctypes.data, 2, b.ctypes.data, 0, b.ctypes.data, 0, b.ctypes.data, b.ctypes.data) == -1
    assert sh.ht().ht_ed25519_sign(b.ctypes.data, 0, b.ctypes.data, 290, b.ctypes.data, 0, b.ctypes.data, b.ctypes.data) == -1


# ---- the Python mirror: every check happens before the device is touched (a sentinel engine fails the test if it is reached)
class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError("the device was reached: " + name)


def test_python_layer_messages():
    from noble_curves_amd import ed25519 as ed
    err, eng, sk, m = sh.kat()["errors"], _NoEngine(), bytes(32), b"abc"
    with pytest.raises(ValueError) as e:
        ed.getPublicKey(bytes(31), engine=eng)
    assert str(e.value) == err["secret_key_length_31"]
    with pytest.raises(ValueError) as e:
        ed.sign(m, bytes(33), engine=eng)
    assert str(e.value) == err["secret_key_length_33"]
    with pytest.raises(ValueError) as e:
        ed.ed25519ctx.sign(m, bytes(64), context=m, engine=eng)
    assert str(e.value) == err["secret_key_length_64"]
    with pytest.raises(ValueError) as e:
        ed.getPublicKey_batch([sk, bytes(31)], engine=eng)
    assert str(e.value) == err["secret_key_length_31"]
    with pytest.raises(ValueError) as e:
        ed.sign(m, sk, context=b"\x01", engine=eng)
    assert str(e.value) == err["context_on_plain"] == "Contexts/pre-hash are not supported"
    with pytest.raises(ValueError) as e:
        ed.sign_batch([m], sk, context=b"\x01", engine=eng)
    assert str(e.value) == err["context_on_plain"]
    for ns in (ed.ed25519ctx, ed.ed25519ph):
        with pytest.raises(ValueError) as e:
            ns.sign(m, sk, context=bytes(256), engine=eng)
        assert str(e.value) == err["context_256"] == err["context_256_ph"] == "Context is too big"
        with pytest.raises(ValueError) as e:
            ns.verify(bytes(64), m, sk, context=bytes(256), engine=eng)
        assert str(e.value) == err["context_256"]
    with pytest.raises(TypeError):
        ed.sign(m, "not bytes", engine=eng)
    with pytest.raises(ValueError):
        ed.sign_batch([m, m], [sk], engine=eng)
    assert err["empty_context_on_plain"] is None      # the reference takes an empty context on plain ed25519: so does _dom
    assert ed._dom(b"", False, False) == b"" and ed._dom(None, False, True) == sh.dom2(b"", False)
    assert ed._dom(b"ab", True, True) == sh.dom2(b"ab", True)


def test_python_single_sign_raises_on_a_refused_row():
    from noble_curves_amd import ed25519 as ed
    import numpy as np

    class Refuses:
        def ed25519_sign_batch(self, K, blob, off, dom, expanded, one_key, prehash):
            return np.zeros((1, 64), np.uint8), np.zeros(1, bool)

    with pytest.raises(ValueError) as e:
        ed.sign(b"m", bytes(32), engine=Refuses())
    assert str(e.value) == "invalid scalar: expected 1 <= sc < curve.n"
    assert ed.sign_batch([b"m"], bytes(32), engine=Refuses()) == [None]
