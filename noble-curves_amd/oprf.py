"""RFC 9497 host shim: the reference's `ristretto255_oprf` (src/ed25519.ts:682, built by createOPRF of src/abstract/oprf.ts) with
batch forms - OPRF (mode 0), VOPRF (mode 1) and POPRF (mode 2) over ristretto255-SHA512.

Every step with a group element in it runs in the HIP kernels of csrc/oprf.hip through `ncg_oprf_*`: the hashes to the group and to
scalars (expand_message_xmd on the device), the blinding, the evaluation and unblinding multiplies (which take their SECRET scalars
without a table lookup by digit), the Finalize hash, the composite scalars and the DLEQ proof.  The shim does the argument checks
of the reference and raises its messages; POPRF's m = hashToScalar("Info" || len || info), t = skS + m and the single inversions of the
server are host integers.  `rng` is a callable rng(n) -> n bytes; a blind is int.from_bytes(rng(48), 'little') % (L - 1) + 1, the
reference's mapHashToField, so the reference's answers are reproduced with a recorded rng.  No constant-time claim is made."""
import os

import numpy as np

from ._native import get_engine
from .ed25519 import L

NAME = "ristretto255-SHA512"
_P = 2**255 - 19


def _abytes(b, length=None, title=""):
    """utils abytes(value, length, title)"""
    pre = '"%s" ' % title if title else ""
    if not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError("%sexpected Uint8Array%s, got type=%s" % (pre, "" if length is None else " of length %d" % length, type(b).__name__))
    b = bytes(b)
    if length is not None and len(b) != length:
        raise ValueError("%sexpected Uint8Array of length %d, got length=%d" % (pre, length, len(b)))
    return b


def _input(title, b):
    b = _abytes(b, None, title)
    if len(b) > 0xFFFF:
        raise ValueError('"%s" expected Uint8Array of length <= 65535, got length=%d' % (title, len(b)))
    return b


def _i2osp2(n):
    return int(n).to_bytes(2, "big")


def _ctx(mode):
    return b"OPRFV1-" + bytes([mode]) + b"-" + NAME.encode()


def _scalar(b):
    """Fn.fromBytes: 32 bytes, below L"""
    b = _abytes(b, 32)
    k = int.from_bytes(b, "little")
    if k >= L:
        raise ValueError("invalid field element: outside of range 0..ORDER")
    return k


def _le32(k):
    return int(k).to_bytes(32, "little")


def _random_scalar(rng):
    if not callable(rng):
        raise TypeError('"rng" expected function, got type=' + type(rng).__name__)
    return int.from_bytes(bytes(rng(48)), "little") % (L - 1) + 1


def _enc_error(b):
    s = int.from_bytes(b, "little")
    return "invalid ristretto255 encoding 1" if s >= _P or s & 1 else "invalid ristretto255 encoding 2"


def _raise_status(st, label, rows, invert=False):
    """the reference's message for the FIRST refused row, whatever its status"""
    for i, s in enumerate(st):
        if s == 1:
            raise ValueError(_enc_error(bytes(rows[i])))
        if s == 2:
            raise ValueError(label + " point at infinity")
        if s == 3:   # Fn.inv of zero, or Point.multiply of zero
            raise ValueError("invert: expected non-zero number" if invert else "invalid scalar: expected 1 <= sc < curve.n")


def _wire_points(label, rows, eng):
    """wirePoint for every row: decodes and is not the identity"""
    rows = [_abytes(r, 32) for r in rows]
    for r in rows:
        if r == bytes(32):
            raise ValueError(label + " point at infinity")
    if rows:
        _, ok = eng.ristretto_decode_batch(np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 32))
        for r, good in zip(rows, ok):
            if not good:
                raise ValueError(_enc_error(r))
    return rows


class _Mode:
    """the functions the three modes share; `engine` may be given to every call"""

    def __init__(self, mode, info=None):
        self._mode, self._info = mode, info

    def generateKeyPair(self, engine=None):
        sk = np.frombuffer(_le32(_random_scalar(os.urandom)), np.uint8)
        out, _ = (engine or get_engine()).oprf_mul_batch(_BASE_ENC, sk, one_scalar=True)   # the secret key through the masked multiply
        return {"secretKey": sk.tobytes(), "publicKey": out[0].tobytes()}

    def deriveKeyPair(self, seed, keyInfo, engine=None):
        seed = _abytes(seed, 32, "seed")
        keyInfo = _input("keyInfo", keyInfo)
        eng = engine or get_engine()
        dst = b"DeriveKeyPair" + _ctx(self._mode)
        for counter in range(256):
            sk = eng.ristretto_hash_to_scalar_batch([seed + _i2osp2(len(keyInfo)) + keyInfo + bytes([counter])], dst)[0]
            if sk.any():
                out, st = eng.oprf_mul_batch(_BASE_ENC, sk, one_scalar=True)   # the secret key through the masked multiply
                return {"secretKey": sk.tobytes(), "publicKey": out[0].tobytes()}
        raise ValueError("Cannot derive key")

    def blind_batch(self, inputs, rng=os.urandom, engine=None):
        """blind() for every input: (list of blind bytes, list of blinded elements)"""
        inputs = [_input("input", i) for i in inputs]
        blinds = [_le32(_random_scalar(rng)) for _ in inputs]
        if not inputs:
            return [], []
        out, st = (engine or get_engine()).oprf_blind_batch(self._mode, inputs, np.frombuffer(b"".join(blinds), np.uint8))
        if st.any():
            raise ValueError("Input point at infinity")
        return blinds, [r.tobytes() for r in out]

    def _unblind_batch(self, inputs, blinds, evaluated, eng):
        ks = [_scalar(b) for b in blinds]
        evaluated = [_abytes(e, 32) for e in evaluated]
        if not inputs:
            return []
        out, st = (eng or get_engine()).oprf_finalize_batch(self._mode, inputs, np.frombuffer(b"".join(_le32(k) for k in ks), np.uint8),
                                          np.frombuffer(b"".join(evaluated), np.uint8), self._info)
        _raise_status(st, "evaluated", evaluated, True)
        return [r.tobytes() for r in out]

    def _evaluate(self, scalar, invert, inputs, eng):
        inputs = [_input("input", i) for i in inputs]
        if not inputs:
            return []
        out, st = (eng or get_engine()).oprf_evaluate_batch(self._mode, inputs, np.frombuffer(_le32(scalar), np.uint8), invert, self._info)
        for s in st:
            if s == 3:
                raise ValueError("invert: expected non-zero number" if invert else "invalid scalar: expected 1 <= sc < curve.n")
            if s:
                raise ValueError("Input point at infinity")
        return [r.tobytes() for r in out]

    def _mul_one(self, label, elements, scalar, invert, eng):
        """every wire element times the one secret scalar (or its inverse)"""
        elements = [_abytes(e, 32) for e in elements]
        if not elements:
            return []
        out, st = (eng or get_engine()).oprf_mul_batch(np.frombuffer(b"".join(elements), np.uint8), np.frombuffer(_le32(scalar), np.uint8), one_scalar=True, invert=invert)
        _raise_status(st, label, elements, invert)
        return [r.tobytes() for r in out]

    def _proof(self, k, B, C, D, rng, eng):
        r = _random_scalar(rng)
        return eng.oprf_generate_proof(self._mode, _le32(k), B, np.frombuffer(b"".join(C), np.uint8), np.frombuffer(b"".join(D), np.uint8), _le32(r))

    def _verify(self, B, C, D, proof, eng):
        proof = _abytes(proof, 64)
        for half in (proof[:32], proof[32:]):
            _scalar(half)
        if not eng.oprf_verify_proof(self._mode, B, np.frombuffer(b"".join(C), np.uint8), np.frombuffer(b"".join(D), np.uint8), proof):
            raise ValueError("proof verification failed")


_BASE_ENC = np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), np.uint8)


def _items(items):
    if not isinstance(items, (list, tuple)):
        raise ValueError("expected array")
    return list(items)


class _OPRF(_Mode):
    def __init__(self):
        super().__init__(0)

    def blind(self, input, rng=os.urandom, engine=None):
        b, e = self.blind_batch([input], rng, engine)
        return {"blind": b[0], "blinded": e[0]}

    def blindEvaluate_batch(self, secretKey, blinded, engine=None):
        return self._mul_one("blinded", _items(blinded), _scalar(secretKey), False, engine)

    def blindEvaluate(self, secretKey, blinded, engine=None):
        return self.blindEvaluate_batch(secretKey, [blinded], engine)[0]

    def finalize_batch(self, inputs, blinds, evaluated, engine=None):
        return self._unblind_batch([_input("input", i) for i in inputs], blinds, evaluated, engine)

    def finalize(self, input, blind, evaluated, engine=None):
        return self.finalize_batch([input], [blind], [evaluated], engine)[0]

    def evaluate_batch(self, secretKey, inputs, engine=None):
        return self._evaluate(_scalar(secretKey), False, inputs, engine)

    def evaluate(self, secretKey, input, engine=None):
        return self.evaluate_batch(secretKey, [input], engine)[0]


class _VOPRF(_Mode):
    def __init__(self):
        super().__init__(1)

    def blind(self, input, rng=os.urandom, engine=None):
        b, e = self.blind_batch([input], rng, engine)
        return {"blind": b[0], "blinded": e[0]}

    def blindEvaluateBatch(self, secretKey, publicKey, blinded, rng=os.urandom, engine=None):
        blinded = _items(blinded)
        eng = engine or get_engine()
        sk = _scalar(secretKey)
        pk = _wire_points("public key", [publicKey], eng)[0]
        evaluated = self._mul_one("blinded", blinded, sk, False, eng)
        return {"evaluated": evaluated, "proof": self._proof(sk, pk, [bytes(b) for b in blinded], evaluated, rng, eng)}

    blindEvaluate_batch = blindEvaluateBatch

    def blindEvaluate(self, secretKey, publicKey, blinded, rng=os.urandom, engine=None):
        res = self.blindEvaluateBatch(secretKey, publicKey, [blinded], rng, engine)
        return {"evaluated": res["evaluated"][0], "proof": res["proof"]}

    def finalizeBatch(self, items, publicKey, proof, engine=None):
        items = _items(items)
        eng = engine or get_engine()
        pk = _wire_points("public key", [publicKey], eng)[0]
        blinded = _wire_points("blinded", [i["blinded"] for i in items], eng)
        evaluated = _wire_points("evaluated", [i["evaluated"] for i in items], eng)
        self._verify(pk, blinded, evaluated, proof, eng)
        return self._unblind_batch([_input("input", i["input"]) for i in items], [i["blind"] for i in items], evaluated, eng)

    finalize_batch = finalizeBatch

    def finalize(self, input, blind, evaluated, blinded, publicKey, proof, engine=None):
        return self.finalizeBatch([{"input": input, "blind": blind, "evaluated": evaluated, "blinded": blinded}], publicKey, proof, engine)[0]

    def evaluate_batch(self, secretKey, inputs, engine=None):
        return self._evaluate(_scalar(secretKey), False, inputs, engine)

    def evaluate(self, secretKey, input, engine=None):
        return self.evaluate_batch(secretKey, [input], engine)[0]


class _POPRF(_Mode):
    def __init__(self, info, engine=None):
        super().__init__(2, _input("info", info))
        eng = engine or get_engine()
        self._m = int.from_bytes(eng.ristretto_hash_to_scalar_batch([b"Info" + _i2osp2(len(self._info)) + self._info],
                                                                    b"HashToScalar-" + _ctx(2))[0].tobytes(), "little")

    def _tweaked(self, publicKey, eng):
        """T + pkS with T = m G: m is public, so the public multiply and the Edwards addition of the ristretto255 shim serve"""
        from . import ristretto255 as rc
        pk = _wire_points("public key", [publicKey], eng)[0]
        tw = rc.Point.fromBytes(pk, eng).add(rc.Point.BASE.multiply(self._m, eng) if self._m else rc.Point.ZERO, eng).toBytes(eng)
        if tw == bytes(32):
            raise ValueError("tweakedKey point at infinity")
        return tw

    def blind_batch(self, inputs, publicKey, rng=os.urandom, engine=None):
        """(blinds, blinded, tweakedKey)"""
        eng = engine or get_engine()
        inputs = [_input("input", i) for i in inputs]
        tw = self._tweaked(publicKey, eng)
        b, e = super().blind_batch(inputs, rng, eng)
        return b, e, tw

    def blind(self, input, publicKey, rng=os.urandom, engine=None):
        b, e, tw = self.blind_batch([input], publicKey, rng, engine)
        return {"blind": b[0], "blinded": e[0], "tweakedKey": tw}

    def _t(self, secretKey):
        t = (_scalar(secretKey) + self._m) % L
        if t == 0:
            raise ValueError("invert: expected non-zero number")
        return t

    def blindEvaluateBatch(self, secretKey, blinded, rng=os.urandom, engine=None):
        blinded = _items(blinded)
        eng = engine or get_engine()
        t = self._t(secretKey)
        evaluated = self._mul_one("blinded", blinded, t, True, eng)
        tweaked = eng.oprf_mul_batch(_BASE_ENC, np.frombuffer(_le32(t), np.uint8), one_scalar=True)[0][0].tobytes()
        return {"evaluated": evaluated, "proof": self._proof(t, tweaked, evaluated, [bytes(b) for b in blinded], rng, eng)}

    blindEvaluate_batch = blindEvaluateBatch

    def blindEvaluate(self, secretKey, blinded, rng=os.urandom, engine=None):
        res = self.blindEvaluateBatch(secretKey, [blinded], rng, engine)
        return {"evaluated": res["evaluated"][0], "proof": res["proof"]}

    def finalizeBatch(self, items, proof, tweakedKey, engine=None):
        items = _items(items)
        eng = engine or get_engine()
        inputs = [_input("input", i["input"]) for i in items]
        evaluated = _wire_points("evaluated", [i["evaluated"] for i in items], eng)
        tw = _wire_points("tweakedKey", [tweakedKey], eng)[0]
        blinded = _wire_points("blinded", [i["blinded"] for i in items], eng)
        self._verify(tw, evaluated, blinded, proof, eng)
        return self._unblind_batch(inputs, [i["blind"] for i in items], evaluated, eng)

    finalize_batch = finalizeBatch

    def finalize(self, input, blind, evaluated, blinded, proof, tweakedKey, engine=None):
        return self.finalizeBatch([{"input": input, "blind": blind, "evaluated": evaluated, "blinded": blinded}], proof, tweakedKey, engine)[0]

    def evaluate_batch(self, secretKey, inputs, engine=None):
        return self._evaluate(self._t(secretKey), True, inputs, engine)

    def evaluate(self, secretKey, input, engine=None):
        return self.evaluate_batch(secretKey, [input], engine)[0]


class _Suite:
    name = NAME

    def __init__(self):
        self.oprf, self.voprf = _OPRF(), _VOPRF()

    def poprf(self, info, engine=None):
        return _POPRF(info, engine)


ristretto255_oprf = _Suite()
