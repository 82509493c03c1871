"""The ristretto255 OPRF without a GPU: the plain-Python model of tests/oprf_helpers.py against the reference's recorded answers
(tests/golden/ristretto255_oprf_kat.json) and the anchors of RFC 9497 A.1, then the CPU twins of the lane code of csrc/oprf.hpp
(ht_oprf_*) against the model, and the argument checks of the mirror that need no device."""
import random

import numpy as np
import pytest

import oprf_helpers as oh
import ristretto_helpers as rh

L = oh.L
H = bytes.fromhex


def rows_of(block):
    """(input, rng bytes of the row's blind, row) of every row of a fixture mode block"""
    inputs = oh.seeded_inputs()
    for b in block["batches"]:
        rng = H(b["rng"])
        for j, i in enumerate(b["idx"]):
            yield inputs[i], rng[48 * j:48 * j + 48], {k: b[k][j] for k in ("blind", "blinded", "evaluated", "output", "evaluate")}, b


def block_key(block):
    """(scalar the server multiplies by, whether inverted, info) of a fixture block"""
    mode, info = block["mode"], H(block["info"])
    sk = int.from_bytes(H(block["skS"]), "little")
    if mode == 2:
        return (sk + oh.poprf_m(info)) % L, True, info
    return sk, False, None


# ---------------------------------------------------------------- the model against the reference's answers
def test_model_anchors():
    k = oh.kat()
    assert k["name"] == "ristretto255-SHA512"
    a = k["anchor"][0]
    assert a["skS"] == "5ebcea5ee37023ccb9fc2d2019f9d7737be85591ae8652ffa9ef0f4d37063b0e" and a["input"] == "00"
    assert a["blind"] == "64d37aed22a27f5191de1c1d69fadb899d8862b58eb4220029e036ec4c1f6706"
    assert a["blinded"] == "609a0ae68c15a3cf6903766461307e5c8bb2f95e7e6550e1ffa2dc99e412803c"
    assert a["evaluated"] == "7ec6578ae5120958eb2db1745758ff379e77cb64fe77b0b2d8cc917ea0869c7e"
    assert a["output"] == ("527759c3d9366f277d8c6020418d96bb393ba2afb20ff90df23fb7708264e2f3ab9135e3bd69955851de4b1f9fe8a0973396719b7912ba9ee8aa7d0b5e24bcf6")
    assert k["anchor_keys"][1]["skS"] == "e6f73f344b79b379f1a0dd37e07ff62e38d9f71345ce62ae3a9bc60b04ccd909"
    assert k["anchor_keys"][1]["pkS"] == "c803e2cc6b05fc15064549b5920659ca4a77b2cca6f04f6b357009335476ad4e"
    blind = oh.random_scalar(H(a["rng"]))
    assert oh.le32(blind).hex() == a["blind"]
    assert oh.blind(0, H(a["input"]), blind).hex() == a["blinded"]
    assert oh.mul_row(H(a["blinded"]), H(a["skS"])) == (0, H(a["evaluated"]))
    assert oh.finalize(0, H(a["input"]), H(a["blind"]), H(a["evaluated"])) == (0, H(a["output"]))
    assert oh.evaluate(0, H(a["input"]), H(a["skS"])) == (0, H(a["output"]))
    for row in k["anchor_keys"]:
        sk, pk = oh.derive_key_pair(row["mode"], H(k["seed"]), H(k["key_info"]))
        assert (sk.hex(), pk.hex()) == (row["skS"], row["pkS"])


def test_model_reproduces_fixture():
    k = oh.kat()
    assert [b["mode"] for b in k["modes"]] == [0, 1, 2, 2, 2] and [len(H(b["info"])) for b in k["modes"]] == [0, 0, 0, 9, 300]
    seen = set()
    for block in k["modes"]:
        mode = block["mode"]
        assert oh.derive_key_pair(mode, H(k["seed"]), H(k["key_info"])) == (H(block["skS"]), H(block["pkS"]))
        scalar, invert, info = block_key(block)
        for inp, rng, row, _ in rows_of(block):
            seen.add(len(inp))
            blind = oh.random_scalar(rng)
            assert oh.le32(blind).hex() == row["blind"]
            assert oh.blind(mode, inp, blind).hex() == row["blinded"]
            assert oh.mul_row(H(row["blinded"]), oh.le32(scalar), invert) == (0, H(row["evaluated"]))
            assert oh.finalize(mode, inp, H(row["blind"]), H(row["evaluated"]), info) == (0, H(row["output"]))
            assert oh.evaluate(mode, inp, oh.le32(scalar), invert, info) == (0, H(row["evaluate"])) and row["evaluate"] == row["output"]
        sizes = [len(b["idx"]) for b in block["batches"]]
        assert sizes[:4] == [1, 2, 3, 5]
    assert seen == {0, 1, 17, 67, 68, 84, 200, 1000}


def proof_batches():
    for block in oh.kat()["modes"]:
        if block["mode"] == 0:
            continue
        for b in block["batches"][:4]:
            mode, n = block["mode"], len(b["idx"])
            scalar, _, _ = block_key(block)
            B = H(block["pkS"]) if mode == 1 else H(b["tweakedKey"])
            C, D = [H(x) for x in b["blinded"]], [H(x) for x in b["evaluated"]]
            if mode == 2:
                C, D = D, C
            yield mode, scalar, B, C, D, oh.random_scalar(H(b["rng"])[48 * n:48 * n + 48]), H(b["proof"])


def test_model_proofs():
    for mode, k, B, C, D, r, proof in proof_batches():
        assert rh.encode(rh.mul(rh.BASE, k)) == B
        assert oh.generate_proof(mode, k, B, C, D, r) == proof
        assert oh.verify_proof(mode, B, C, D, proof)
        if len(C) > 1:
            assert not oh.verify_proof(mode, B, C[1:] + C[:1], D, proof)
        assert not oh.verify_proof(mode, B, C, D, bytes(64))


def test_model_seeded_hashes():
    k = oh.kat()["seeded"]
    h2s = "".join(k["hash_to_scalar"])
    assert len(h2s) == 64 * 64 and len(k["xmd"]) == 64
    for i in range(64):
        want = oh.hash_to_scalar(oh.seeded_scalar_msg(i), b"HashToScalar-" + oh.ctx_of(i % 3))
        assert oh.le32(want).hex() == h2s[64 * i:64 * i + 64]
        msg, dst, n = oh.seeded_xmd_row(i)
        assert rh.expand_message_xmd(msg, dst, n).hex() == k["xmd"][i] and len(k["xmd"][i]) == 2 * n
    assert {len(x) // 2 for x in k["xmd"]} == set(oh.XMD_OUT_LENS)


# ---------------------------------------------------------------- the lane code on the CPU against the model
def test_xmd_lane_block_boundaries():
    """b_0 hashes 128 + len(msg) + 3 + len(DST) + 1 bytes: the message lengths that bring this to 111, 112, 127 and 128 mod 128 (the
    padding fits / needs another block, the block is full / one over), and the same one block later"""
    rng = random.Random("oprf-xmd")
    for dl in (1, 40, 255):
        dst = bytes(rng.getrandbits(8) for _ in range(dl))
        for target in (111, 112, 127, 128):
            for extra in (0, 128):
                n = (target - (132 + dl)) % 128 + extra
                assert (128 + n + 3 + dl + 1) % 128 == target % 128
                msg = bytes(rng.getrandbits(8) for _ in range(n))
                for out_len in (64, 65) if extra else (1, 256):
                    assert oh.ht_xmd(msg, dst, out_len) == rh.expand_message_xmd(msg, dst, out_len), (dl, n, out_len)


def test_xmd_and_hash_twins_on_seeded_rows():
    k = oh.kat()["seeded"]
    h2s = "".join(k["hash_to_scalar"])
    for i in range(64):
        msg, dst, n = oh.seeded_xmd_row(i)
        assert oh.ht_xmd(msg, dst, n).hex() == k["xmd"][i]
        assert oh.ht_hash_to_scalar(oh.seeded_scalar_msg(i), b"HashToScalar-" + oh.ctx_of(i % 3)).hex() == h2s[64 * i:64 * i + 64]
    for c in rh.kat()["hash"][:40]:
        if c["dst"] is not None and len(bytes.fromhex(c["dst"])) > 255:
            continue
        dst = rh.DEFAULT_DST if c["dst"] is None else H(c["dst"])
        enc, aff = oh.ht_hash_to_group(H(c["msg"]), dst, affine=True)
        assert enc.hex() == c["out"] and rh.encode(rh.unwire(np.frombuffer(aff, np.uint8))) == enc


def scalar_rows():
    rng = random.Random("oprf-scalars")
    return [1, 2, L - 1, L - 2, 2**252] + [rng.randrange(1, L) for _ in range(256)]


def test_scalar_product_inverse_add_sub():
    ks = scalar_rows()
    other = ks[1:] + ks[:1]
    a, b = rh.scalars_le(ks), rh.scalars_le(other)
    prod, inv = oh.ht_check(0, 0, a, b), oh.ht_check(1, 0, a, b)
    add, sub = oh.ht_check(4, 0, a, b), oh.ht_check(5, 0, a, b)
    for i, (x, y) in enumerate(zip(ks, other)):
        assert int.from_bytes(bytes(prod[i]), "little") == x * y % L, i
        assert int.from_bytes(bytes(inv[i]), "little") == pow(x, -1, L), i
        assert int.from_bytes(bytes(add[i]), "little") == (x + y) % L, i
        assert int.from_bytes(bytes(sub[i]), "little") == (x - y) % L, i


def test_zero_and_order_are_rejected():
    base = rh.encode(rh.BASE)
    for bad in (0, L, L + 1, 2**256 - 1):
        assert oh.ht_mul(base, oh.le32(bad)) == (oh.BAD_SCALAR, bytes(32))
        assert oh.ht_mul(base, oh.le32(bad), oh.INVERT) == (oh.BAD_SCALAR, bytes(32))
        assert oh.ht_blind(0, b"x", oh.le32(bad)) == (oh.BAD_SCALAR, bytes(32))
        assert oh.ht_finalize(0, b"x", oh.le32(bad), base) == (oh.BAD_SCALAR, bytes(64))
        assert oh.ht_evaluate(1, b"x", oh.le32(bad)) == (oh.BAD_SCALAR, bytes(64))
    assert oh.ht_mul(base, oh.le32(L - 1))[0] == 0


def secret_mul_points():
    """the base point, points whose encoder rotates and points whose encoder does not, and each of them plus every four-torsion point"""
    pts = rh.base_multiples(24)
    rot, plain = [p for p in pts if rh.rotates(*p)], [p for p in pts if not rh.rotates(*p)]
    assert rot and plain
    return [rh.BASE] + rot[:2] + plain[:2]


def test_mul_secret_against_model():
    pts = secret_mul_points()
    ks = oh.edge_scalars()
    assert len(ks) == 72
    for j, p in enumerate(pts):      # every scalar on every point, and on its whole coset
        want = [rh.encode(rh.mul(p, k)) for k in ks]
        for t in rh.TORSION4:
            q = rh.add(p, t)
            got = oh.ht_check(2, 0, np.repeat(rh.wire([q]), len(ks), axis=0), rh.scalars_le(ks))
            assert [bytes(r) for r in got] == want, (j, t)


def test_fused_rows_against_model():
    rng = random.Random("oprf-rows")
    inputs = oh.seeded_inputs()
    info = b"public info"
    for mode in (0, 1, 2):
        for inp in inputs[:5]:
            blind, sk = rng.randrange(1, L), rng.randrange(1, L)
            st, blinded = oh.ht_blind(mode, inp, oh.le32(blind))
            assert (st, blinded) == (0, oh.blind(mode, inp, blind))
            inv = mode == 2
            st, ev = oh.ht_mul(blinded, oh.le32(sk), oh.INVERT if inv else 0)
            assert (st, ev) == oh.mul_row(blinded, oh.le32(sk), inv)
            i = info if mode == 2 else None
            assert oh.ht_finalize(mode, inp, oh.le32(blind), ev, i) == oh.finalize(mode, inp, oh.le32(blind), ev, i)
            assert oh.ht_evaluate(mode, inp, oh.le32(sk), oh.INVERT if inv else 0, i) == oh.evaluate(mode, inp, oh.le32(sk), inv, i)
            assert oh.ht_finalize(mode, inp, oh.le32(blind), ev, i)[1] == oh.ht_evaluate(mode, inp, oh.le32(sk), oh.INVERT if inv else 0, i)[1]
    # mode 2 with an empty info still hashes its two length bytes
    assert oh.ht_evaluate(2, b"a", oh.le32(5), 0, b"") == oh.evaluate(2, b"a", oh.le32(5), False, b"")
    assert oh.ht_evaluate(2, b"a", oh.le32(5), 0, b"")[1] != oh.ht_evaluate(1, b"a", oh.le32(5), 0, None)[1]


def test_fused_rows_on_fixture():
    for block in oh.kat()["modes"]:
        mode = block["mode"]
        scalar, invert, info = block_key(block)
        fl = oh.INVERT if invert else 0
        for inp, rng, row, _ in list(rows_of(block))[:11]:
            assert oh.ht_blind(mode, inp, H(row["blind"])) == (0, H(row["blinded"]))
            assert oh.ht_mul(H(row["blinded"]), oh.le32(scalar), fl) == (0, H(row["evaluated"]))
            assert oh.ht_finalize(mode, inp, H(row["blind"]), H(row["evaluated"]), info) == (0, H(row["output"]))
            assert oh.ht_evaluate(mode, inp, oh.le32(scalar), fl, info) == (0, H(row["output"]))


def test_rejected_elements():
    base = rh.encode(rh.BASE)
    k = oh.le32(7)
    bad1, bad2 = b"\x01" + bytes(31), next(e for _, e, w in rh.edge_encodings() if w == rh.ENC2)
    for enc, st in ((bytes(32), oh.IDENTITY), (bad1, oh.BAD_ENCODING), (bad2, oh.BAD_ENCODING), (base, 0)):
        assert oh.ht_mul(enc, k)[0] == st == oh.mul_row(enc, k)[0]
        assert oh.ht_finalize(0, b"in", k, enc)[0] == st
        if st:
            assert oh.ht_mul(enc, k)[1] == bytes(32) and oh.ht_finalize(0, b"in", k, enc)[1] == bytes(64)
    # the element is looked at before the scalar
    assert oh.ht_mul(bytes(32), oh.le32(0))[0] == oh.IDENTITY and oh.ht_mul(bad1, oh.le32(L))[0] == oh.BAD_ENCODING


def test_composites_and_proof_twins():
    for mode, k, B, C, D, r, proof in proof_batches():
        want = oh.composite_scalars(mode, B, C, D)
        got, st = oh.ht_composite(mode, B, C, D)
        assert [int.from_bytes(g, "little") for g in got] == want and not any(st)
        M = rh.encode(oh.msm(C, want))
        assert oh.ht_proof(mode, oh.le32(k), B, M, oh.le32(r)) == (0, proof)
        five = [B, M, rh.encode(rh.mul(rh.decode(M), k)), rh.encode(rh.mul(rh.BASE, r)), rh.encode(rh.mul(rh.decode(M), r))]
        assert oh.ht_challenge(mode, five) == proof[:32]
    mode, k, B, C, D, r, proof = next(proof_batches())
    got, st = oh.ht_composite(mode, B, [bytes(32)] + C, [D[0]] + [b"\x01" + bytes(31)])
    assert list(st) == [oh.IDENTITY, oh.BAD_ENCODING] and got[0] == got[1] == bytes(32)
    assert oh.ht_proof(mode, oh.le32(0), B, C[0], oh.le32(r))[0] == -1 and oh.ht_proof(mode, oh.le32(k), B, C[0], oh.le32(L))[0] == -1


# ---------------------------------------------------------------- the mirror's argument checks that need no device
def test_mirror_argument_checks():
    from noble_curves_amd.oprf import ristretto255_oprf as O
    err = oh.kat()["errors"]
    assert O.name == oh.kat()["name"]
    with pytest.raises(ValueError) as e:
        O.oprf.blind(bytes(65536))
    assert str(e.value) == err["input_long"]
    with pytest.raises(ValueError) as e:
        O.oprf.deriveKeyPair(bytes(31), b"")
    assert str(e.value) == err["seed_length"]
    with pytest.raises(TypeError) as e:
        O.oprf.blind(b"\x00", 5)
    assert str(e.value) == err["rng_type"].replace("number", "int")
    ei = oh.kat()["error_inputs"]
    with pytest.raises(ValueError) as e:
        O.oprf.finalize(b"\x00", oh.le32(L), H(ei["blinded"]))
    assert str(e.value) == err["blind_order"]
    with pytest.raises(ValueError) as e:
        O.voprf.blindEvaluateBatch(H(ei["skS"]), H(ei["pkS"]), H(ei["blinded"]))
    assert str(e.value) == err["expected_array"]
    for method in ("generateKeyPair", "deriveKeyPair", "blind", "blindEvaluate", "finalize", "evaluate", "blind_batch", "blindEvaluate_batch",
                   "finalize_batch", "evaluate_batch"):
        assert callable(getattr(O.oprf, method)) and callable(getattr(O.voprf, method)), method
    assert callable(O.voprf.blindEvaluateBatch) and callable(O.voprf.finalizeBatch) and callable(O.poprf)
