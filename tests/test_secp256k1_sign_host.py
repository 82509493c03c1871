"""secp256k1 signing on the CPU twins of csrc/secp256k1_sign.hip (the lane code the kernels run), without a GPU.  The expectation is
a plain-Python model (secp256k1_sign_helpers: hmac + hashlib + the oracle's curve), itself checked first against the 404 `valid` rows
of the reference's ECDSA vectors and against the reference's own answers (tests/golden/secp256k1_sign_kat.json)."""
import hashlib
import hmac
import random

import pytest

import secp256k1_sign_helpers as sh
from secp256k1_sign_helpers import N, PK_COMPRESSED, PK_UNCOMPRESSED, PK_XONLY


# ---------------------------------------------------------------- the model against the reference
def test_model_reproduces_the_reference_vectors():
    rows = sh.ecdsa_vectors()
    assert len(rows) == 404
    for i, v in enumerate(rows):
        r, s, _ = sh.ecdsa_sign(bytes.fromhex(v["m"]), bytes.fromhex(v["d"].rjust(64, "0")), lowS=True, prehash=False)
        assert sh.compact(r, s).hex() == v["signature"], i


def test_model_reproduces_the_fixture():
    kat = sh.kat()
    assert len(kat["keys"]) >= 32 and {int(k["secretKey"], 16) for k in kat["keys"]} >= {1, N - 1}
    for k in kat["keys"]:
        sk = bytes.fromhex(k["secretKey"])
        assert (sh.public_key(sk, PK_COMPRESSED).hex(), sh.public_key(sk, PK_UNCOMPRESSED).hex(), sh.public_key(sk, PK_XONLY).hex()) == \
            (k["compressed"], k["uncompressed"], k["xonly"])
    combos = set()
    for row in kat["ecdsa"]:
        msg, sk, extra = bytes.fromhex(row["msg"]), bytes.fromhex(row["secretKey"]), sh.kat_extra(row)
        r, s, recid = sh.ecdsa_sign(msg, sk, row["lowS"], row["prehash"], extra)
        assert (sh.compact(r, s).hex(), sh.recovered(r, s, recid).hex(), sh.der(r, s).hex()) == (row["compact"], row["recovered"], row["der"]), row
        combos.add((row["prehash"], row["lowS"], extra is not None, len(msg)))
    assert combos == {(p, l, e, n) for p in (True, False) for l in (True, False) for e in (True, False) for n in sh.MSG_LENGTHS}
    for row in kat["schnorr"]:
        assert sh.schnorr_sign(bytes.fromhex(row["msg"]), bytes.fromhex(row["secretKey"]), bytes.fromhex(row["auxRand"])).hex() == row["sig"], row
    assert {(row["auxRand"] == "00" * 32, len(row["msg"]) // 2) for row in kat["schnorr"]} == {(z, n) for z in (True, False) for n in sh.MSG_LENGTHS}


def test_der_matches_the_parser():
    from noble_curves_amd.ecdsa import der_to_rs, rs_to_der
    rng = random.Random("der")
    for bits in (1, 7, 8, 127, 128, 247, 248, 255, 256):
        for _ in range(4):
            r, s = rng.getrandbits(bits) | 1 << (bits - 1), rng.getrandbits(bits) | 1
            assert sh.der(r, s) == rs_to_der(r, s) and der_to_rs(rs_to_der(r, s)) == (r, s)


# ---------------------------------------------------------------- hashes and the DRBG
def test_sha256_segments_against_hashlib():
    rng = random.Random("sha256-segments")
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    for total in (0, 1, 55, 56, 63, 64, 119, 120, 183, 184, 1000):     # 55 | 56 (mod 64): the edges of the 9-byte padding rule
        for na, nb in ((0, 0), (32, 0), (64, 32), (33, 64)):
            if total < na + nb:
                continue
            a, b, msg = rb(na), rb(nb), rb(total - na - nb)
            assert sh.ht_sha256_segments(a or None, b or None, msg) == hashlib.sha256(a + b + msg).digest(), (total, na, nb)


@pytest.mark.parametrize("extra", [0, 1])
def test_drbg_candidates_against_hmac(extra):
    rng = random.Random("drbg-%d" % extra)
    for _ in range(3):
        seed = bytes(rng.randrange(256) for _ in range(96))
        used = seed if extra else seed[:64]
        # the model's generator restated with the hmac module alone, so that the twin is not only compared with our own code
        K, V = bytes(32), b"\x01" * 32
        mac = lambda k, m: hmac.new(k, m, hashlib.sha256).digest()  # noqa: E731
        K = mac(K, V + b"\0" + used); V = mac(K, V); K = mac(K, V + b"\1" + used); V = mac(K, V)   # noqa: E702
        gen = sh.drbg_candidates(used)
        for j in range(4):
            V = mac(K, V)
            want = V
            assert next(gen) == want
            rc, out = sh.ht_op(0, sh.bytes_words(seed), variant=(j << 1) | extra)
            assert rc == 0 and b"".join(int(w).to_bytes(4, "little") for w in out) == want, (extra, j)
            K = mac(K, V + b"\0"); V = mac(K, V)   # noqa: E702
    assert sh.ht_op(0, [0] * 24, variant=4 << 1)[0] == -1       # j = 4 is outside the table


# ---------------------------------------------------------------- the scan multiply
def test_scan_multiply_edge_scalars():
    ks = sh.edge_scalars()
    assert {1, 2, 3, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2, 2**255, 2**255 + 1, 2**255 - 1} <= set(ks) and len(ks) > 800
    for k in ks:
        assert sh.ht_mul_base_scan(k) == sh.mul_base(k), hex(k)


def test_scan_multiply_refused_scalars_are_safe():
    g = sh.mul_base(1)
    for k in (0, N, N + 1, 2**256 - 1):          # replaced by 1: the callers refuse such scalars themselves
        assert sh.ht_mul_base_scan(k) == g


# ---------------------------------------------------------------- the finish steps with injected inputs
def test_ecdsa_finish_rare_branches():
    for name, (a, b, want) in sh.rare_finish_cases().items():
        rc, out = sh.ht_op(2, a, [b])
        assert rc == 0 and (sh.from_words(out[:8]), sh.from_words(out[8:16]), out[16], out[17]) == want, name


def test_schnorr_scalar_half():
    rng = random.Random("schnorr-scalar")
    cases = [(1, 0, 0, 1), (N - 1, 1, N - 1, N - 1), (N - 1, 0, N - 1, N - 1)] + \
        [(rng.randrange(1, N), rng.randrange(2), rng.randrange(N), rng.randrange(1, N)) for _ in range(16)]
    for k_, odd, e, d in cases:
        rc, out = sh.ht_op(3, sh.words(k_) + sh.words(e) + sh.words(d), [odd])
        assert rc == 0 and sh.from_words(out) == sh.schnorr_scalar(k_, odd, e, d)


def test_unknown_ops():
    assert sh.ht_widths(5) == (0, 0, 0) and sh.ht_widths(-1) == (0, 0, 0)
    assert sh.ht_op(5, [0])[0] == -1 and sh.ht_op(-1, [0])[0] == -1
    for op, w in sh.CHECK_WORDS.items():
        assert sh.ht_widths(op) == w


# ---------------------------------------------------------------- whole rows on the twins
def test_twin_public_keys():
    kat = sh.kat()
    sks = [bytes.fromhex(k["secretKey"]) for k in kat["keys"]]
    for mode, name in ((PK_COMPRESSED, "compressed"), (PK_UNCOMPRESSED, "uncompressed"), (PK_XONLY, "xonly")):
        got, ok = sh.ht_public_keys(sks, mode)
        assert [g.hex() for g in got] == [k[name] for k in kat["keys"]] and ok == [1] * len(sks)
    bad = [sh.be(0), sh.be(N), sh.be(2**256 - 1), sh.be(7)]
    got, ok = sh.ht_public_keys(bad, PK_COMPRESSED)
    assert ok == [0, 0, 0, 1] and got[:3] == [bytes(33)] * 3 and got[3] == sh.public_key(sh.be(7))


def test_twin_reproduces_the_reference_vectors():
    for i, v in enumerate(sh.ecdsa_vectors()):
        sig, _, ok = sh.ht_ecdsa_sign(bytes.fromhex(v["d"].rjust(64, "0")), sh.normalise_hash(bytes.fromhex(v["m"])))
        assert ok == 1 and sig.hex() == v["signature"], i


def test_twin_reproduces_the_fixture():
    kat = sh.kat()
    for row in kat["ecdsa"]:
        msg, sk = bytes.fromhex(row["msg"]), bytes.fromhex(row["secretKey"])
        h = hashlib.sha256(msg).digest() if row["prehash"] else sh.normalise_hash(msg)
        sig, recid, ok = sh.ht_ecdsa_sign(sk, h, sh.kat_extra(row), row["lowS"])
        assert ok == 1 and sig.hex() == row["compact"] and (bytes([recid]) + sig).hex() == row["recovered"], row
    for row in kat["schnorr"]:
        sig, ok = sh.ht_schnorr_sign(bytes.fromhex(row["secretKey"]), bytes.fromhex(row["auxRand"]), bytes.fromhex(row["msg"]))
        assert ok == 1 and sig.hex() == row["sig"], row


def test_twin_takes_the_next_candidates():
    """the retry loop: with the first candidates refused the row is the model's with the same candidates skipped"""
    sk, h, extra = sh.rand_bytes(32, "retry-key"), sh.rand_bytes(32, "retry-hash"), sh.rand_bytes(32, "retry-extra")
    seen = set()
    for refuse in (0, 1, 2, 3):
        for ex in (None, extra):
            r, s, recid = sh.ecdsa_sign(h, sk, True, False, ex, refuse_first=refuse)
            assert sh.ht_ecdsa_sign(sk, h, ex, True, refuse) == (sh.compact(r, s), recid, 1)
            row = sh.bytes_words(sk + h + extra)
            rc, out = sh.ht_op(4, row, [1], variant=(refuse << 1) | (ex is not None))
            assert rc == 0 and b"".join(int(w).to_bytes(4, "little") for w in out[:16]) == sh.compact(r, s) and out[16:] == [recid, 1]
            seen.add(sh.compact(r, s))
    assert len(seen) == 8


def test_twin_refuses_bad_keys():
    h, aux = sh.rand_bytes(32, "h"), sh.rand_bytes(32, "aux")
    for d in (0, N, 2**256 - 1):
        assert sh.ht_ecdsa_sign(sh.be(d), h) == (bytes(64), 0, 0)
        assert sh.ht_schnorr_sign(sh.be(d), aux, b"msg") == (bytes(64), 0)

