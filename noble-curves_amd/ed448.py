"""Ed448 / X448 host shim with the reference's call shapes, checks, check order and messages (src/ed448.ts over
src/abstract/montgomery.ts and src/abstract/edwards.ts).

`x448`: scalarMult / getSharedSecret / getPublicKey and their `_batch` forms (`ncg_x448_batch`, `ncg_x448_base_batch`): the
u coordinate (the peer's key) is checked before the scalar (montgomery.ts:324-326); clamping, the reduction of u mod p, the
low-order test and the 448-step ladder run in HIP kernels.  `_batch` forms return (list of bytes-or-None, list of bool), None
where the reference throws 'invalid private or public key received'; `scalars` may be ONE bytes value against many peers.

`ed448` / `ed448ph`: getPublicKey[_batch], getExtendedPublicKey, expand_keys, sign / sign_batch, verify / verify_batch,
shake256_batch, utils.toMontgomery[_batch] and utils.toMontgomerySecret.  THE HASHES RUN ON THE DEVICE (Keccak-f[1600], one message
per lane): the key expansion SHAKE256(secretKey, 114), the prehash of ed448ph, the nonce r = SHAKE256(dom4 || prefix || PH(M), 114)
mod n and the challenge k = SHAKE256(dom4 || R || A || PH(M), 114) mod n (`ncg_ed448_public_key_batch`, `ncg_ed448_expand_key_batch`,
`ncg_ed448_sign_batch`, `ncg_ed448_verify_batch_msgs`, `ncg_shake256_batch`).  verify_batch hashes the challenge with hashlib on the
host by default, as it always has, and on the device with `device_hash=True`; the decoding of A and R, the small-order test, s < n
and the cofactored equation run on the device either way.  The signing multiplications double, always add and select, so no branch or
address follows a key or a nonce; no constant-time claim is made.  `zip215=True` is not supported.

`ed448_Point`: fromBytes_batch / toBytes_batch / multiplyUnsafe_batch / multiplyBase_batch / add_batch on encodings, with the
range errors of multiply / multiplyUnsafe raised here.

decaf448 and its hasher, the prime-order group of this curve, live in `noble_curves_amd.decaf448`.

`ed448_hasher`: the reference's RFC 9380 hasher (edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_, ed448.ts:313-417) with `*Batch` forms; the
hash (expand_message_xof over SHAKE256), the two Elligator maps, the sum, the cofactor and the affine conversion run on the device
(`ncg_ed448_h2c_*`).  Points are affine (x, y) pairs, the identity `ed448_Point.ZERO` = (0, 1).

Out of scope, not provided by this module: `E448` (the NIST Edwards model of Curve448), FROST
and OPRF suites, an MSM over Ed448, and a fixed-base table (multiplyBase runs the variable-base kernel on the base
point).
"""
import hashlib

import numpy as np

from . import h2c as _h2c
from ._native import ED448_KEY_BYTES, get_engine

P = 2**448 - 2**224 - 1
N = 2**446 - 13818066809895115352007386748515426880336692474882178609894547503885
_D = P - 39081
INVALID = "invalid private or public key received"
LOW_ORDER_U = frozenset((0, 1, P - 1))                   # montgomery.ts:303-313
# ED448_TORSION_SUBGROUP (ed448.ts:738-743): the hex encodings of the four points of order 1, 2, 4, 4
ED448_TORSION_SUBGROUP = tuple(b.hex() for b in ((1).to_bytes(57, "little"), (P - 1).to_bytes(57, "little"), bytes(57), bytes(56) + b"\x80"))


def _abytes(b, length, title):
    """utils abytes(value, length, title) with the reference's wording, the type named as JavaScript's typeof names it"""
    if not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
        kind = "string" if isinstance(b, str) else "boolean" if isinstance(b, bool) else "number" if isinstance(b, (int, float)) else "object"
        raise TypeError('"%s" expected Uint8Array%s, got type=%s' % (title, "" if length is None else " of length %d" % length, kind))
    b = bytes(b)
    if length is not None and len(b) != length:
        raise ValueError('"%s" expected Uint8Array of length %d, got length=%d' % (title, length, len(b)))
    return b


def _result(out, ok):
    ok = [bool(x) for x in ok]
    return [out[i].tobytes() if ok[i] else None for i in range(len(ok))], ok


def _rows(items, width, title):
    out = np.zeros((len(items), width), np.uint8)
    for i, b in enumerate(items):
        out[i] = np.frombuffer(_abytes(b, width, title), np.uint8)
    return out


def _adjust(b):
    """adjustScalarBytes (ed448.ts:122-130) on 56 or 57 bytes"""
    b = bytearray(b)
    b[0] &= 252
    b[55] |= 128
    if len(b) > 56:
        b[56] = 0
    return bytes(b)


class x448:
    """x448 of src/ed448.ts:284-311"""
    GuBytes = (5).to_bytes(56, "little")

    @staticmethod
    def scalarMult_batch(scalars, us, engine=None):
        """x448.scalarMult for every (scalar, u) pair.  `scalars` may be ONE bytes value: that secret against every u."""
        one = isinstance(scalars, (bytes, bytearray, memoryview))
        if not one and len(scalars) != len(us):
            raise ValueError("arrays of scalars and u coordinates must have equal length")
        U = np.zeros((len(us), 56), np.uint8)
        S = np.zeros((1 if one else len(us), 56), np.uint8)
        for i in range(len(us)):   # row by row, the u coordinate first (montgomery.ts:324-326)
            U[i] = np.frombuffer(_abytes(us[i], 56, "uCoordinate"), np.uint8)
            if not one:
                S[i] = np.frombuffer(_abytes(scalars[i], 56, "scalar"), np.uint8)
        if one:
            S[0] = np.frombuffer(_abytes(scalars, 56, "scalar"), np.uint8)
        return _result(*(engine or get_engine()).x448_batch(S, U, one_scalar=one))

    @staticmethod
    def getSharedSecret_batch(secretKeys, publicKeys, engine=None):
        return x448.scalarMult_batch(secretKeys, publicKeys, engine)

    @staticmethod
    def getPublicKey_batch(secretKeys, engine=None):
        return _result(*(engine or get_engine()).x448_base_batch(_rows(secretKeys, 56, "scalar")))

    @staticmethod
    def scalarMult(scalar, u, engine=None):
        """a batch of one, with the reference's errors in the reference's order"""
        u = _abytes(u, 56, "uCoordinate")
        if int.from_bytes(u, "little") % P in LOW_ORDER_U:
            raise ValueError(INVALID)
        out, ok = x448.scalarMult_batch([_abytes(scalar, 56, "scalar")], [u], engine)
        if not ok[0]:
            raise ValueError(INVALID)
        return out[0]

    @staticmethod
    def getSharedSecret(secretKey, publicKey, engine=None):
        return x448.scalarMult(secretKey, publicKey, engine)

    @staticmethod
    def getPublicKey(secretKey, engine=None):
        out, ok = x448.getPublicKey_batch([secretKey], engine)
        if not ok[0]:
            raise ValueError(INVALID)
        return out[0]


def _dom4(data, ctx, phflag):
    """ed448.ts:190-201"""
    if len(ctx) > 255:
        raise ValueError("context must be smaller than 255, got: %d" % len(ctx))
    return b"SigEd448" + bytes([1 if phflag else 0, len(ctx)]) + ctx + data


def _decode_error(enc):
    """the message of the error Point.fromBytes throws for an encoding the device refused (rare path: host integers), or None"""
    y = int.from_bytes(enc[:56] + bytes([enc[56] & 0x7f]), "little")
    if y >= P:
        return "expected valid point.y: 0 <= n < %d, got %d" % (P, y)
    u, v = (y * y - 1) % P, (_D * y * y - 1) % P
    x2 = u * pow(v, P - 2, P) % P
    if x2 and pow(x2, (P - 1) // 2, P) != 1:
        return "bad point: invalid y coordinate"
    if x2 == 0 and enc[56] & 0x80:
        return "bad point: x=0 and x_0=1"
    return None


class _Utils:
    @staticmethod
    def toMontgomery_batch(publicKeys, engine=None):
        """u = y^2 / x^2 of Point.fromBytes(publicKey) for every key (`ncg_ed448_to_montgomery_batch`)"""
        return _result(*(engine or get_engine()).ed448_to_montgomery_batch(_rows(publicKeys, 57, "point")))

    @staticmethod
    def toMontgomery(publicKey, engine=None):
        out, ok = _Utils.toMontgomery_batch([publicKey], engine)
        if not ok[0]:
            raise ValueError(_decode_error(_abytes(publicKey, 57, "point")) or "invert: expected non-zero number")
        return out[0]

    @staticmethod
    def toMontgomerySecret(secretKey):
        """ed448.ts:181-188: the clamped first 56 bytes of SHAKE256(secretKey, 114), on the host"""
        if not isinstance(secretKey, (bytes, bytearray, memoryview, np.ndarray)):
            raise TypeError("expected Uint8Array of length 57, got type=%s" % type(secretKey).__name__)
        if len(bytes(secretKey)) != 57:
            raise ValueError("expected Uint8Array of length 57, got length=%d" % len(bytes(secretKey)))
        return _adjust(hashlib.shake_256(bytes(secretKey)).digest(114)[:57])[:56]


class _EdDSA:
    """ed4(opts) of ed448.ts:206-215: `prehash` False = ed448, True = ed448ph"""
    utils = _Utils

    def __init__(self, prehash):
        self.prehash = prehash

    def challenge(self, r_bytes, pk_bytes, msg, context=b""):
        """hashDomainToScalar (edwards.ts:900-906) of an already prehashed message, reduced mod n"""
        return int.from_bytes(hashlib.shake_256(_dom4(bytes(r_bytes) + bytes(pk_bytes) + bytes(msg), context, self.prehash)).digest(114),
                              "little") % N

    def verify_batch(self, sigs, msgs, publicKeys, context=b"", zip215=False, engine=None, device_hash=False):
        """list of bool, one per (signature, message, publicKey) triple, all under one context.  device_hash=True hashes the
        challenges (and the prehash of ed448ph) on the device (`ncg_ed448_verify_batch_msgs`) instead of with hashlib here; the rows
        under a context longer than 255 bytes keep their host handling either way."""
        n = len(sigs)
        if len(msgs) != n or len(publicKeys) != n:
            raise ValueError("arrays of signatures, messages and public keys must have equal length")
        if not isinstance(zip215, bool):
            raise TypeError('"zip215" expected boolean')
        if zip215:
            raise ValueError("ed448: zip215 is not supported")
        context = _abytes(context, None, "context")
        long_context = len(context) > 255
        S, A, K = np.zeros((n, 114), np.uint8), np.zeros((n, 57), np.uint8), np.zeros((n, 56), np.uint8)
        raw = []
        for i in range(n):
            sig = _abytes(sigs[i], 114, "signature")
            msg = _abytes(msgs[i], None, "message")
            pk = _abytes(publicKeys[i], 57, "publicKey")
            raw.append(msg)
            if self.prehash and not device_hash:
                msg = hashlib.shake_256(msg).digest(64)
            S[i], A[i] = np.frombuffer(sig, np.uint8), np.frombuffer(pk, np.uint8)
            if long_context:
                # edwards.ts:964-984: dom4 refuses the context only for a row that got past the decoding of A and R, s < n and the
                # small-order test; every other row is False without the context being looked at (rare path: host integers)
                if (_decode_error(pk) is None and _decode_error(sig[:57]) is None and int.from_bytes(sig[57:], "little") < N
                        and pk.hex() not in ED448_TORSION_SUBGROUP):
                    _dom4(b"", context, self.prehash)
                continue
            if not device_hash:
                K[i] = np.frombuffer(self.challenge(sig[:57], pk, msg, context).to_bytes(56, "little"), np.uint8)
        if long_context:
            return [False] * n
        if device_hash:
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum([len(m) for m in raw], dtype=np.uint64)
            blob = np.frombuffer(b"".join(raw), np.uint8) if off[-1] else np.zeros(0, np.uint8)
            ok = (engine or get_engine()).ed448_verify_batch_msgs(S, A, blob, off, _dom4(b"", context, self.prehash), prehash=self.prehash)
            return [bool(x) for x in ok]
        return [bool(x) for x in (engine or get_engine()).ed448_verify_batch(S, A, K)]

    def verify(self, sig, msg, publicKey, context=b"", zip215=False, engine=None, device_hash=False):
        """eddsa.verify (edwards.ts:942): one signature = a batch of one"""
        return self.verify_batch([sig], [msg], [publicKey], context, zip215, engine, device_hash)[0]

    def getPublicKey_batch(self, secretKeys, engine=None):
        """getExtendedPublicKey(secretKey).pointBytes (edwards.ts:871-897) for every key: SHAKE256, the clamp, the reduction mod n and
        [scalar]B on the device (`ncg_ed448_public_key_batch`).  An engine that has only the multiply (the CPU twins of the host
        tests) gets the head hashed here, as before the device had a Keccak: the bytes are the same."""
        eng = engine or get_engine()
        if hasattr(eng, "ed448_public_key_batch"):
            K = _rows(secretKeys, 57, "secretKey")
            out = eng.ed448_public_key_batch(K)
            K[:] = 0
            return [out[i].tobytes() for i in range(len(secretKeys))]
        K = np.zeros((len(secretKeys), 56), np.uint8)
        for i, sk in enumerate(secretKeys):
            head = _adjust(hashlib.shake_256(_abytes(sk, 57, "secretKey")).digest(114)[:57])
            K[i] = np.frombuffer(head[:56], np.uint8)
        out = eng.ed448_mul_base_batch(K)
        return [out[i].tobytes() for i in range(len(secretKeys))]

    def getPublicKey(self, secretKey, engine=None):
        return self.getPublicKey_batch([secretKey], engine)[0]

    @staticmethod
    def expand_keys(secretKeys, engine=None):
        """172-byte rows scalar (56, below n) || prefix (57) || publicKey (57) || 2 zero bytes (uint8 [n, 172]) for repeated use with
        sign_batch(..., expanded=True) (`ncg_ed448_expand_key_batch`)"""
        K = _rows(secretKeys, 57, "secretKey")
        out = (engine or get_engine()).ed448_expand_key_batch(K)
        K[:] = 0
        return out

    def getExtendedPublicKey(self, secretKey, engine=None):
        """head, prefix, scalar, pointBytes of the reference's getExtendedPublicKey (edwards.ts:871-892); prefix, scalar and pointBytes
        come from the device, head is the clamped first 57 bytes of SHAKE256(secretKey, 114) (the device keeps it only reduced mod n)"""
        row = self.expand_keys([secretKey], engine)[0].tobytes()
        head = _adjust(hashlib.shake_256(bytes(secretKey)).digest(114)[:57])
        return {"head": head, "prefix": row[56:113], "scalar": int.from_bytes(row[:56], "little"), "pointBytes": row[113:170]}

    def sign_batch(self, msgs, secretKeys, context=b"", engine=None, expanded=False):
        """sign per message, all under one context (`ncg_ed448_sign_batch`).  secretKeys: ONE key for every message (bytes, or one
        172-byte row with expanded=True) or a list / array as long as msgs.  Returns a list of 114-byte signatures; None where the
        device refused the row (r = 0 mod n, where the reference throws)."""
        ms = [_abytes(m, None, "message") for m in msgs]
        width = ED448_KEY_BYTES if expanded else 57
        one = isinstance(secretKeys, (bytes, bytearray, memoryview)) or (isinstance(secretKeys, np.ndarray) and secretKeys.ndim == 1)
        keys = [secretKeys] if one else secretKeys
        if not one and len(keys) != len(ms):
            raise ValueError("arrays of messages and secret keys must have equal length")
        K = _rows(keys, width, "secretKey")
        dom = _dom4(b"", _abytes(context, None, "context"), self.prehash)
        off = np.zeros(len(ms) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in ms], dtype=np.uint64)
        blob = np.frombuffer(b"".join(ms), np.uint8) if off[-1] else np.zeros(0, np.uint8)
        sig, ok = (engine or get_engine()).ed448_sign_batch(K, blob, off, dom, expanded=expanded, one_key=one, prehash=self.prehash)
        K[:] = 0
        return [sig[i].tobytes() if ok[i] else None for i in range(len(ms))]

    def sign(self, msg, secretKey, context=b"", engine=None):
        """eddsa.sign (edwards.ts:909-930): a batch of one; raises where the reference throws"""
        _abytes(secretKey, 57, "secretKey")
        out = self.sign_batch([msg], secretKey, context, engine)[0]
        if out is None:
            raise ValueError("invalid scalar: expected 1 <= sc < curve.n")
        return out

    @staticmethod
    def shake256_batch(msgs, dkLen, engine=None):
        """shake256(msg, { dkLen }) for every message, on the device (`ncg_shake256_batch`): list of bytes"""
        ms = [_abytes(m, None, "message") for m in msgs]
        if not isinstance(dkLen, int) or isinstance(dkLen, bool) or not 1 <= dkLen <= 65535:
            raise ValueError("dkLen must be an integer in 1..65535")
        off = np.zeros(len(ms) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in ms], dtype=np.uint64)
        blob = np.frombuffer(b"".join(ms), np.uint8) if off[-1] else np.zeros(0, np.uint8)
        out = (engine or get_engine()).shake256_batch(blob, off, dkLen)
        return [out[i].tobytes() for i in range(len(ms))]


ed448 = _EdDSA(False)
ed448ph = _EdDSA(True)


class ed448_Point:
    """batch forms of the reference's ed448.Point on ENCODINGS (57 bytes); decoded points are affine (x, y) pairs"""

    ZERO = (0, 1)

    @staticmethod
    def fromBytes_batch(encodings, engine=None):
        """Point.fromBytes (strict) per row -> (list of (x, y) or None, list of bool)"""
        out, ok = (engine or get_engine()).ed448_decode_batch(_rows(encodings, 57, "point"))
        pts = [(int.from_bytes(out[i, :56].tobytes(), "little"), int.from_bytes(out[i, 56:].tobytes(), "little")) if ok[i] else None
               for i in range(len(ok))]
        return pts, [bool(x) for x in ok]

    @staticmethod
    def fromBytes(encoding, engine=None):
        pts, ok = ed448_Point.fromBytes_batch([encoding], engine)
        if not ok[0]:
            raise ValueError(_decode_error(bytes(encoding)))
        return pts[0]

    @staticmethod
    def toBytes_batch(points, engine=None):
        """Point.toBytes of affine (x, y) pairs"""
        A = np.zeros((len(points), 112), np.uint8)
        for i, (x, y) in enumerate(points):
            A[i] = np.frombuffer(int(x).to_bytes(56, "little") + int(y).to_bytes(56, "little"), np.uint8)
        out = (engine or get_engine()).ed448_encode_batch(A)
        return [out[i].tobytes() for i in range(len(points))]

    @staticmethod
    def _scalars(scalars, lo, what):
        K = np.zeros((len(scalars), 56), np.uint8)
        for i, k in enumerate(scalars):
            if not isinstance(k, int) or isinstance(k, bool) or not lo <= k < N:
                raise ValueError("invalid scalar: expected %s" % what)
            K[i] = np.frombuffer(k.to_bytes(56, "little"), np.uint8)
        return K

    @staticmethod
    def multiplyUnsafe_batch(encodings, scalars, engine=None):
        """fromBytes(enc).multiplyUnsafe(k).toBytes() per row; `scalars` a list, or ONE int for every row"""
        one = isinstance(scalars, int)
        if not one and len(scalars) != len(encodings):
            raise ValueError("arrays of points and scalars must have equal length")
        K = ed448_Point._scalars([scalars] if one else scalars, 0, "0 <= sc < curve.n")
        return _result(*(engine or get_engine()).ed448_mul_batch(_rows(encodings, 57, "point"), K, one_scalar=one))

    @staticmethod
    def multiply_batch(encodings, scalars, engine=None):
        """Point.multiply: the same products, the scalar range 1 <= sc < curve.n"""
        ed448_Point._scalars([scalars] if isinstance(scalars, int) else scalars, 1, "1 <= sc < curve.n")
        return ed448_Point.multiplyUnsafe_batch(encodings, scalars, engine)

    @staticmethod
    def multiplyBase_batch(scalars, engine=None):
        """BASE.multiply(k).toBytes() per row"""
        out = (engine or get_engine()).ed448_mul_base_batch(ed448_Point._scalars(scalars, 1, "1 <= sc < curve.n"))
        return [out[i].tobytes() for i in range(len(scalars))]

    @staticmethod
    def add_batch(a_encodings, b_encodings, subtract=False, engine=None):
        """fromBytes(a).add(fromBytes(b)).toBytes() per row (subtract: .subtract); None where either encoding is refused"""
        if len(a_encodings) != len(b_encodings):
            raise ValueError("arrays of points must have equal length")
        eng = engine or get_engine()
        pa, oka = eng.ed448_decode_batch(_rows(a_encodings, 57, "point"))
        pb, okb = eng.ed448_decode_batch(_rows(b_encodings, 57, "point"))
        pb[~np.asarray(okb, bool), 56] = 1        # a refused row becomes the identity (0, 1) so that the addition stays on the curve
        pa[~np.asarray(oka, bool), 56] = 1
        out = eng.ed448_encode_batch(eng.ed448_add_pairs_batch(pa, pb, subtract))
        return _result(out, np.asarray(oka, bool) & np.asarray(okb, bool))


def xof_oversize_dst(dst, k):
    """the oversize rule of expand_message_xof over SHAKE256 (hash-to-curve.ts:263-266), which the device leaves to its caller: a DST
    above 255 bytes is replaced by SHAKE256("H2C-OVERSIZE-DST-" || DST, ceil(2 k / 8)) - 56 bytes for k = 224, 64 for k = 256"""
    return _xof_compress(b"H2C-OVERSIZE-DST-" + dst, k) if len(dst) > 255 else dst


def _xof_compress(tagged, k):
    return hashlib.shake_256(tagged).digest((2 * k + 7) // 8)


class _Ed448Hasher(_h2c.H2CDeviceHasher):
    """createHasher(ed448_Point, map_to_curve_elligator2_edwards448, defaults) (hash-to-curve.ts:441-530; ed448.ts:408-417): m = 1,
    k = 224, expand = 'xof' over SHAKE256, everything from the message bytes on running on the device (`ncg_ed448_h2c_*`).  The
    `defaults` snapshot, the DST override and the single-call forms are H2CDeviceHasher's; points are affine (x, y) pairs."""

    def __init__(self, engine=None):
        self.Point, self._engine = ed448_Point, engine
        self._defaults = {"DST": "edwards448_XOF:SHAKE256_ELL2_RO_", "encodeDST": "edwards448_XOF:SHAKE256_ELL2_NU_", "p": P, "m": 1,
                          "k": 224, "expand": "xof", "hash": "shake256"}

    def _compress_dst(self, tagged):
        return _xof_compress(tagged, self._defaults["k"])

    @staticmethod
    def _pairs(out):
        return [(int.from_bytes(out[i, :56].tobytes(), "little"), int.from_bytes(out[i, 56:].tobytes(), "little")) for i in range(out.shape[0])]

    def _hash(self, msgs, dst, count):
        msgs = [_h2c._msg_bytes(m) for m in msgs]
        return self._pairs(self._eng().ed448_h2c_hash_batch(msgs, dst, count)) if msgs else []

    def hashToCurveBatch(self, msgs, options=None):
        return self._hash(msgs, self._dst(options, self._defaults["DST"]), 2)

    def encodeToCurveBatch(self, msgs, options=None):
        return self._hash(msgs, self._dst(options, self._defaults["encodeDST"]), 1)

    def mapToCurveBatch(self, scalars_list):
        raw = bytearray()
        for u in scalars_list:
            if not isinstance(u, int) or isinstance(u, bool):
                raise ValueError("expected bigint (m=1)")
            raw += (u % P).to_bytes(56, "little")
        if not raw:
            return []
        return self._pairs(self._eng().ed448_h2c_map_batch(np.frombuffer(bytes(raw), dtype=np.uint8).reshape(-1, 56), 1))

    def hashToScalarBatch(self, msgs, options=None):
        dst = self._dst(options, "HashToScalar-")                # _DST_scalar (hash-to-curve.ts:412, :523)
        msgs = [_h2c._msg_bytes(m) for m in msgs]
        if not msgs:
            return []
        out = self._eng().ed448_h2c_hash_to_scalar_batch(msgs, dst)
        return [int.from_bytes(out[i].tobytes(), "little") for i in range(len(msgs))]


ed448_hasher = _Ed448Hasher()
