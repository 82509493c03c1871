"""decaf448 host shim: the `Point` of the reference's `decaf448` and its `decaf448_hasher` (src/ed448.ts:462-701, RFC 9496
section 5) with batch forms.

An element is held as an Edwards representative - an Ed448 affine point x || y, 112 bytes - exactly as the reference wraps an
EdwardsPoint; decoding, encoding, equals, the Elligator map and every multiply run in HIP kernels (`ncg_decaf448_*`, and the
`ncg_ed448_*` entry points for the group law on representatives).  The shim does the argument checks of the reference and raises
its messages; for a row the device refused, the field's range error (s >= p), 'invalid decaf448 encoding 1' (s odd) and
'encoding 2' are told apart with host integers.  `expand_message_xof` over SHAKE256 runs on the host (hashlib) and the map on the
device by default; with `device_hash=True` the hash runs on the device too, and `hashToScalar_batch` always does.  Batch forms take and return encodings (56 bytes): only bytes cross.  Two elements are compared only through `equals` or
their encodings.

Not provided: an MSM, a fixed-base table (multiplyBase runs the variable-base kernel on the base point), `decaf448_oprf`, FROST.
"""
import hashlib

import numpy as np

from ._native import get_engine
from .ed448 import N, P, xof_oversize_dst

DEFAULT_DST = "decaf448_XOF:SHAKE256_D448MAP_RO_"
DST_SCALAR = "HashToScalar-"
ENC1, ENC2 = "invalid decaf448 encoding 1", "invalid decaf448 encoding 2"
RANGE = "invalid field element: outside of range 0..ORDER"
_EXPECTED = "DecafPoint expected"
_GX = 0xaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa955555555555555555555555555555555555555555555555555555555
_GY = 0xae05e9634ad7048db359d6205086c2b0036ed7a035884dd7b7e36d728ad8c4b80d6565833a2a3098bbbcb2bed1cda06bdaeafbcdea9386ed


def _abytes(b, length):
    """utils abytes(value, length) without a title"""
    if not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
        kind = "string" if isinstance(b, str) else "boolean" if isinstance(b, bool) else "number" if isinstance(b, (int, float)) else "object"
        raise TypeError("expected Uint8Array of length %d, got type=%s" % (length, kind))
    b = bytes(b)
    if len(b) != length:
        raise ValueError("expected Uint8Array of length %d, got length=%d" % (length, len(b)))
    return b


def _rows(items, length):
    out = np.zeros((len(items), length), np.uint8)
    for i, b in enumerate(items):
        out[i] = np.frombuffer(_abytes(b, length), np.uint8)
    return out


def _decode_error(enc):
    """the message of the error DecafPoint.fromBytes throws for an encoding the device refused (rare path: host integers)"""
    s = int.from_bytes(enc, "little")
    if s >= P:                     # Fp.fromBytes refuses a non-canonical s before the decoder's own check is reached
        return RANGE
    return ENC1 if s & 1 else ENC2


def _scalars(ks, lo):
    out = np.zeros((len(ks), 56), np.uint8)
    for i, k in enumerate(ks):
        if not isinstance(k, int) or isinstance(k, bool) or not lo <= k < N:
            raise ValueError("invalid scalar: expected %d <= sc < curve.n" % lo)
        out[i] = np.frombuffer(k.to_bytes(56, "little"), np.uint8)
    return out


class Point:
    """`decaf448.Point`: an element through one Edwards representative (x || y, an Ed448 affine point of include/ncg.h)"""
    __slots__ = ("_w",)

    def __init__(self, wire):
        self._w = np.ascontiguousarray(wire, dtype=np.uint8).reshape(112).copy()

    @staticmethod
    def fromBytes(b, engine=None):
        b = _abytes(b, 56)
        out, ok = (engine or get_engine()).decaf448_decode_batch(np.frombuffer(b, np.uint8).reshape(1, 56))
        if not ok[0]:
            raise ValueError(_decode_error(b))
        return Point(out[0])

    @staticmethod
    def fromHex(h, engine=None):
        if not isinstance(h, str):
            raise TypeError("hex string expected, got " + type(h).__name__)
        if len(h) % 2:
            raise ValueError("hex string expected, got unpadded hex of length %d" % len(h))
        try:
            b = bytes.fromhex(h)
        except ValueError:
            raise ValueError("hex string expected, got non-hex character") from None
        return Point.fromBytes(b, engine)

    @staticmethod
    def fromAffine(x, y):
        """wraps the Edwards point as it is (not a canonical decoding path), like the reference's fromAffine"""
        return Point(np.frombuffer((x % P).to_bytes(56, "little") + (y % P).to_bytes(56, "little"), np.uint8))

    def toAffine(self):
        b = self._w.tobytes()
        return int.from_bytes(b[:56], "little"), int.from_bytes(b[56:], "little")

    def toBytes(self, engine=None):
        return (engine or get_engine()).decaf448_encode_batch(self._w.reshape(1, 112))[0].tobytes()

    def toHex(self, engine=None):
        return self.toBytes(engine).hex()

    def equals(self, other, engine=None):
        if not isinstance(other, Point):
            raise TypeError(_EXPECTED)
        return bool((engine or get_engine()).decaf448_equals_batch(self._w.reshape(1, 112), other._w.reshape(1, 112))[0])

    def is0(self, engine=None):
        return self.equals(Point.ZERO, engine)

    def add(self, other, engine=None):
        if not isinstance(other, Point):
            raise TypeError(_EXPECTED)
        return Point((engine or get_engine()).ed448_add_pairs_batch(self._w.reshape(1, 112), other._w.reshape(1, 112))[0])

    def subtract(self, other, engine=None):
        if not isinstance(other, Point):
            raise TypeError(_EXPECTED)
        return Point((engine or get_engine()).ed448_add_pairs_batch(self._w.reshape(1, 112), other._w.reshape(1, 112), True)[0])

    def negate(self):
        x, y = self.toAffine()
        return Point.fromAffine(-x, y)

    def double(self, engine=None):
        return self.add(self, engine)

    def _mul(self, k, lo, engine):
        """the exact multiple of THIS representative, as the reference multiplies its EdwardsPoint: through the Ed448 encoding of
        the representative (encode, decode + multiply + encode, decode)"""
        ks = _scalars([k], lo)
        eng = engine or get_engine()
        out, _ = eng.ed448_mul_batch(eng.ed448_encode_batch(self._w.reshape(1, 112)), ks)
        return Point(eng.ed448_decode_batch(out)[0][0])

    def multiply(self, k, engine=None):
        """Point.multiply: 1 <= k < n"""
        return self._mul(k, 1, engine)

    def multiplyUnsafe(self, k, engine=None):
        """Point.multiplyUnsafe: 0 <= k < n"""
        return self._mul(k, 0, engine)


Point.BASE = Point.fromAffine(_GX, _GY)
Point.ZERO = Point.fromAffine(0, 1)


def fromBytes_batch(encodings, engine=None):
    """DecafPoint.fromBytes for every 56-byte row: (list of Point-or-None, list of bool), None where the reference throws"""
    E = _rows(encodings, 56)
    if not len(encodings):
        return [], []
    out, ok = (engine or get_engine()).decaf448_decode_batch(E)
    ok = [bool(x) for x in ok]
    return [Point(out[i]) if ok[i] else None for i in range(len(ok))], ok


def _wires(points):
    for p in points:
        if not isinstance(p, Point):
            raise TypeError(_EXPECTED)
    return np.stack([p._w for p in points]) if len(points) else np.zeros((0, 112), np.uint8)


def toBytes_batch(points, engine=None):
    if not len(points):
        return []
    return [r.tobytes() for r in (engine or get_engine()).decaf448_encode_batch(_wires(points))]


def equals_batch(a, b, engine=None):
    if len(a) != len(b):
        raise ValueError("arrays of points must have equal length")
    if not len(a):
        return []
    return [bool(x) for x in (engine or get_engine()).decaf448_equals_batch(_wires(a), _wires(b))]


def _encodings(items, eng):
    """a list of 56-byte encodings, or of Points (encoded on the device first)"""
    if len(items) and all(isinstance(p, Point) for p in items):
        return eng.decaf448_encode_batch(_wires(items))
    return _rows(items, 56)


def multiply_batch(points, scalars, engine=None):
    """fromBytes(points[i]).multiply(scalars[i]).toBytes() for every row: (list of 56 bytes or None, list of bool), None where the
    encoding does not decode.  `scalars` may be ONE int: that scalar against every row (NCG_DECAF448_ONE_SCALAR, an OPRF server's
    blindEvaluate).  Scalars obey Point.multiply's range 1 <= k < n."""
    one = isinstance(scalars, int)
    if not one and len(scalars) != len(points):
        raise ValueError("arrays of points and scalars must have equal length")
    K = _scalars([scalars] if one else scalars, 1)
    if not len(points):
        return [], []
    eng = engine or get_engine()
    out, ok = eng.decaf448_mul_batch(_encodings(points, eng), K, one_scalar=one)
    ok = [bool(x) for x in ok]
    return [out[i].tobytes() if ok[i] else None for i in range(len(ok))], ok


def multiplyBase_batch(scalars, engine=None):
    """BASE.multiply(k).toBytes() for every k (1 <= k < n)"""
    K = _scalars(scalars, 1)
    if not len(scalars):
        return []
    return [r.tobytes() for r in (engine or get_engine()).decaf448_mul_base_batch(K)]


def _dst(DST, default):
    if DST is None:
        DST = default
    if isinstance(DST, str):
        DST = DST.encode("ascii")
    elif not isinstance(DST, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError("DST must be Uint8Array or ascii string")
    DST = bytes(DST)
    if not DST:
        raise ValueError("DST must be non-empty")
    return DST


def expand_message_xof(msg, DST, lenInBytes, k):
    """hash-to-curve.ts:252-286 over SHAKE256: an oversize DST (> 255 bytes) is replaced by SHAKE256("H2C-OVERSIZE-DST-" || DST,
    ceil(2 k / 8))"""
    if not isinstance(msg, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError("expected Uint8Array, got type=%s" % type(msg).__name__)
    DST = xof_oversize_dst(DST, k)
    return hashlib.shake_256(bytes(msg) + lenInBytes.to_bytes(2, "big") + DST + bytes([len(DST)])).digest(lenInBytes)


def deriveToCurve_batch(rows112, engine=None):
    """decaf448_hasher.deriveToCurve(bytes112).toBytes() for every 112-byte row"""
    B = _rows(rows112, 112)
    if not len(rows112):
        return []
    return [r.tobytes() for r in (engine or get_engine()).decaf448_from_uniform_batch(B)]


def deriveToCurve(bytes112, engine=None):
    """the element as a Point: the map and the encoding on the device, then the decoding of that encoding (the canonical
    representative of the element, which may differ from the reference's R1 + R2 by a point of E[4]; equals and toBytes agree)"""
    eng = engine or get_engine()
    return Point(eng.decaf448_decode_batch(eng.decaf448_from_uniform_batch(_rows([bytes112], 112)))[0][0])


def _msgs(msgs):
    for m in msgs:
        if not isinstance(m, (bytes, bytearray, memoryview, np.ndarray)):
            raise TypeError("expected Uint8Array, got type=%s" % type(m).__name__)
    return [bytes(m) for m in msgs]


def hashToCurve_batch(msgs, DST=None, engine=None, device_hash=False):
    """decaf448_hasher.hashToCurve(msg, { DST }).toBytes() for every message: expand_message_xof over SHAKE256 (112 bytes, k = 224)
    here with hashlib and the map on the device, or with device_hash=True the hash on the device as well, one call for the batch
    (`ncg_decaf448_hash_to_group_batch`)"""
    dst = _dst(DST, DEFAULT_DST)
    if not device_hash:
        return deriveToCurve_batch([expand_message_xof(m, dst, 112, 224) for m in msgs], engine)
    msgs = _msgs(msgs)
    if not msgs:
        return []
    return [r.tobytes() for r in (engine or get_engine()).decaf448_hash_to_group_batch(msgs, xof_oversize_dst(dst, 224))]


def hashToCurve(msg, DST=None, engine=None, device_hash=False):
    if not device_hash:
        return deriveToCurve(expand_message_xof(msg, _dst(DST, DEFAULT_DST), 112, 224), engine)
    eng = engine or get_engine()
    enc = eng.decaf448_hash_to_group_batch(_msgs([msg]), xof_oversize_dst(_dst(DST, DEFAULT_DST), 224))
    return Point(eng.decaf448_decode_batch(enc)[0][0])


def hashToScalar_batch(msgs, DST=None, engine=None):
    """decaf448_hasher.hashToScalar for every message, on the device (`ncg_decaf448_hash_to_scalar_batch`): 64 bytes of
    expand_message_xof (k = 256, so an oversize DST is compressed to 64 bytes), little-endian, mod n"""
    dst = _dst(DST, DST_SCALAR)
    msgs = _msgs(msgs)
    if not msgs:
        return []
    out = (engine or get_engine()).decaf448_hash_to_scalar_batch(msgs, xof_oversize_dst(dst, 256))
    return [int.from_bytes(out[i].tobytes(), "little") for i in range(len(msgs))]


def hashToScalar(msg, DST=None, engine=None, device_hash=False):
    """decaf448_hasher.hashToScalar: 64 bytes of expand_message_xof (k = 256), little-endian, mod n.  On the host by default."""
    if device_hash:
        return hashToScalar_batch([msg], DST, engine)[0]
    return int.from_bytes(expand_message_xof(msg, _dst(DST, DST_SCALAR), 64, 256), "little") % N
