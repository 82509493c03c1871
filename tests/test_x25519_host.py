"""X25519 and ed25519.utils.toMontgomery on the CPU twins of csrc/x25519.hip (the lane code the kernels run), against the
reference's own answers (tests/golden/x25519_kat.json) and the Python restatement of the ladder; and the argument checks of the
Python mirror.  The Wycheproof X25519 file the reference's test reads is an absent submodule of the reference and is left out."""
import numpy as np
import pytest

import x25519_helpers as xh


def test_scalar_mult_known_answers():
    rows = xh.kat()["scalar_mult"]
    want, want_ok = xh.kat_expected(rows)
    out, ok = xh.ht_x25519(xh.hex_rows([c["scalar"] for c in rows]), xh.hex_rows([c["u"] for c in rows]))
    assert np.array_equal(ok, want_ok)
    assert np.array_equal(out, want)
    assert {c["error"] for c in rows if c["out"] is None} == {xh.INVALID}
    assert sum(c["out"] is None for c in rows) >= 14      # the low-order set in all its encodings


def test_restatement_reproduces_the_fixture():
    """the oracle of the random batches is itself checked against the reference: every edge row, the RFC 7748 products and the chain"""
    rows = [c for c in xh.kat()["scalar_mult"] if not c["name"].startswith("random")][:60]
    for c in rows:
        r = xh.scalar_mult(bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"]))
        assert (r.hex() if r else None) == c["out"], c["name"]
    k = u = (9).to_bytes(32, "little")
    for _ in range(100):
        k, u = xh.scalar_mult(k, u), k
    assert k.hex() == xh.kat()["iterated"]["100"]
    for v in xh.LOW_ORDER:
        assert xh.ladder(v, xh.clamp(b"\x55" * 32)) == 0


def test_random_rows_against_the_ladder():
    s, u = xh.rand_rows(512, "host-s"), xh.rand_rows(512, "host-u")
    want, want_ok = xh.expect(s, u)
    out, ok = xh.ht_x25519(s, u)
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)
    assert ok.all()                                         # random input is never refused


def test_one_scalar_flag():
    s, u = xh.rand_rows(1, "one-s"), xh.rand_rows(40, "one-u")
    u[7] = 0                                                # a refused row among them
    per_row = xh.ht_x25519(np.repeat(s, 40, axis=0), u)
    flagged = xh.ht_x25519(s, u, flags=1)
    assert np.array_equal(per_row[0], flagged[0]) and np.array_equal(per_row[1], flagged[1])
    assert flagged[1][7] == 0 and not flagged[0][7].any() and flagged[1].sum() == 39
    assert xh.ht().ht_x25519(s.ctypes.data, u.ctypes.data, 2, u.ctypes.data, u.ctypes.data, 1) == -1


def test_base_against_the_ladder_at_nine():
    s = xh.rand_rows(128, "base")
    s[0], s[1] = 0, 255
    nine = np.zeros((128, 32), np.uint8)
    nine[:, 0] = 9
    want, want_ok = xh.ht_x25519(s, nine)
    out, ok = xh.ht_x25519_base(s)
    assert ok.all() and want_ok.all() and np.array_equal(out, want)
    rows = xh.kat()["public_keys"]
    out, ok = xh.ht_x25519_base(xh.hex_rows([c["scalar"] for c in rows]))
    want, want_ok = xh.kat_expected(rows)
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)


@pytest.mark.parametrize("swap", [0, 1])
def test_step_on_raw_limbs(swap):
    a, b = xh.step_rows()
    xh.check_step(a, b, xh.ht_op(0, swap, a, b), swap)


def test_step_ignores_the_upper_variant_bits():
    a, b = xh.step_rows()
    assert np.array_equal(xh.ht_op(0, 3, a[:8], b[:8]), xh.ht_op(0, 1, a[:8], b[:8]))


def test_decode_u_and_decode_scalar():
    us, ks = xh.edge_u_rows(), xh.edge_scalar_rows()
    zb = np.zeros((max(len(us), len(ks)), 9), np.uint32)
    out = xh.ht_op(1, 0, xh.words36(us), zb[:len(us)])
    xh.check_decode_u(us, out)
    assert (out[:, 8] == 0).sum() >= 14
    xh.check_decode_scalar(ks, xh.ht_op(2, 0, xh.words36(ks), zb[:len(ks)]))
    assert xh.ht().ht_x25519_op(3, 0, zb.ctypes.data, zb.ctypes.data, zb.ctypes.data) == -1


def test_to_montgomery_known_answers_and_rejections():
    rows = xh.kat()["to_montgomery"]
    want, want_ok = xh.kat_expected(rows)
    out, ok = xh.ht_to_montgomery(xh.hex_rows([c["publicKey"] for c in rows]))
    assert np.array_equal(ok, want_ok) and np.array_equal(out, want)
    assert (want_ok == 0).sum() == 7 and (want_ok == 1).sum() == 65


# ---------------------------------------------------------------- the Python mirror, the library calls stubbed by the host twin
class TwinEngine:
    """the three engine methods of noble_curves_amd._native.Engine on the CPU twins"""

    def x25519_batch(self, scalars, us, one_scalar=False):
        out, ok = xh.ht_x25519(scalars, us, 1 if one_scalar else 0)
        return out, ok.astype(bool)

    def x25519_base_batch(self, scalars):
        out, ok = xh.ht_x25519_base(scalars)
        return out, ok.astype(bool)

    def ed25519_to_montgomery_batch(self, pks):
        out, ok = xh.ht_to_montgomery(pks)
        return out, ok.astype(bool)


def _raises(exc, msg, f, *a):
    with pytest.raises(exc) as e:
        f(*a, engine=TwinEngine())
    assert str(e.value) == msg, str(e.value)


def test_mirror_values():
    from noble_curves_amd import ed25519 as ed
    from noble_curves_amd import x25519 as x
    eng, k = TwinEngine(), xh.kat()
    assert x.GuBytes == (9).to_bytes(32, "little")
    rows = k["scalar_mult"][:40]
    got, ok = x.scalarMult_batch([bytes.fromhex(c["scalar"]) for c in rows], [bytes.fromhex(c["u"]) for c in rows], engine=eng)
    assert [g.hex() if g else None for g in got] == [c["out"] for c in rows] and ok == [c["out"] is not None for c in rows]
    alice, bob = (bytes.fromhex(c["scalar"]) for c in k["public_keys"][:2])
    apub, bpub = x.getPublicKey(alice, engine=eng), x.getPublicKey(bob, engine=eng)
    assert [apub.hex(), bpub.hex()] == [c["out"] for c in k["public_keys"][:2]]
    assert x.getSharedSecret(alice, bpub, engine=eng) == x.scalarMult(bob, apub, engine=eng) == bytes.fromhex(k["scalar_mult"][2]["out"])
    many, ok = x.getSharedSecret_batch(alice, [bpub, apub, b"\0" * 32], engine=eng)     # one secret, many keys
    assert many[0] == x.getSharedSecret(alice, bpub, engine=eng) and many[2] is None and ok == [True, True, False]
    assert x.getPublicKey_batch([alice, bob], engine=eng)[0] == [apub, bpub]
    for c in k["to_montgomery_secret"][:4]:
        assert ed.toMontgomerySecret(bytes.fromhex(c["secretKey"])).hex() == c["out"]
    seed = bytes.fromhex(k["to_montgomery_secret"][0]["secretKey"])
    assert ed.toMontgomery(bytes.fromhex(k["to_montgomery"][0]["publicKey"]), engine=eng) == x.getPublicKey(ed.toMontgomerySecret(seed), engine=eng)
    rows = k["to_montgomery"]
    got, ok = ed.toMontgomery_batch([bytes.fromhex(c["publicKey"]) for c in rows], engine=eng)
    assert [g.hex() if g else None for g in got] == [c["out"] for c in rows]
    for c in rows:
        if c["out"] is None:
            _raises(ValueError, c["error"], ed.toMontgomery, bytes.fromhex(c["publicKey"]))


def test_mirror_argument_errors_and_their_order():
    from noble_curves_amd import x25519 as x
    e = xh.kat()["errors"]
    good, nine = b"\x01" * 32, x.GuBytes
    _raises(ValueError, e["u_length"], x.scalarMult, good, b"\0" * 31)
    _raises(ValueError, e["scalar_length"], x.scalarMult, b"\0" * 33, nine)
    _raises(ValueError, e["both_bad"], x.scalarMult, b"\0" * 33, b"\0" * 31)                # the peer's key is checked first
    _raises(ValueError, e["low_order_before_scalar"], x.scalarMult, b"\0" * 33, b"\0" * 32)  # ... and refused before the scalar is read
    _raises(ValueError, e["public_key_length"], x.getPublicKey, b"\0" * 31)
    _raises(ValueError, xh.INVALID, x.getSharedSecret, good, b"\x01" + b"\0" * 31)
    with pytest.raises(TypeError):
        x.scalarMult(good, "x", engine=TwinEngine())
    _raises(ValueError, e["both_bad"], x.scalarMult_batch, [good, b"\0" * 33], [nine, b"\0" * 31])
    _raises(ValueError, "arrays of scalars and u coordinates must have equal length", x.scalarMult_batch, [good], [nine, nine])
    assert x.scalarMult_batch([], [], engine=TwinEngine()) == ([], [])
