"""ristretto255 host shim: the `Point` of the reference's `ristretto255` and its `ristretto255_hasher` (src/ed25519.ts:443-668,
RFC 9496) with batch forms.

An element is held as an Edwards representative - an ed25519 wire point, 64 bytes - exactly as the reference wraps an
EdwardsPoint; decoding, encoding, equals, the Elligator map and every multiply run in HIP kernels (`ncg_ristretto_*`).  The shim
does the argument checks of the reference and raises its messages: 'invalid ristretto255 encoding 1' is decided here from
canonicity and parity, 'invalid ristretto255 encoding 2' covers every other row the device rejects.  `expand_message_xmd` over
SHA-512 runs on the host (`h2c.expand_message_xmd`) and the map on the device, or both on the device with `device_hash=True`;
`hashToScalar` hashes and reduces on the device; the OPRF built on these is `noble_curves_amd.oprf`.  Batch forms take and return encodings (32 bytes):
only bytes cross.  The representatives may be fed to the NCG_ED25519 entry points (MSM, resident sets, add pairs); two elements
are compared only through `equals` or their encodings.
"""
import hashlib

import numpy as np

from ._native import ED25519, get_engine
from .ed25519 import L, P
from .h2c import expand_message_xmd

DEFAULT_DST = "ristretto255_XMD:SHA-512_R255MAP_RO_"
ENC1, ENC2 = "invalid ristretto255 encoding 1", "invalid ristretto255 encoding 2"
_SCALAR = "invalid scalar: expected 1 <= sc < curve.n"
_GX = 15112221349535400772501151409588531511454012693041857206046113283949847762202
_GY = 46316835694926478169428394003475163141307993866256225615783033603165251855960


def _abytes(b, length):
    """utils abytes(value, length) without a title"""
    if not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError("expected Uint8Array of length %d, got type=%s" % (length, type(b).__name__))
    b = bytes(b)
    if len(b) != length:
        raise ValueError("expected Uint8Array of length %d, got length=%d" % (length, len(b)))
    return b


def _rows(items, length):
    out = np.zeros((len(items), length), np.uint8)
    for i, b in enumerate(items):
        out[i] = np.frombuffer(_abytes(b, length), np.uint8)
    return out


def _canonical_even(b):
    s = int.from_bytes(b, "little")
    return s < P and not s & 1


def _scalars(ks, lo=1):
    out = np.zeros((len(ks), 32), np.uint8)
    for i, k in enumerate(ks):
        if not isinstance(k, int) or isinstance(k, bool) or not lo <= k < L:
            raise ValueError(_SCALAR)
        out[i] = np.frombuffer(k.to_bytes(32, "little"), np.uint8)
    return out


class Point:
    """`ristretto255.Point`: an element through one Edwards representative (x || y, the wire point of include/ncg.h)"""
    __slots__ = ("_w",)

    def __init__(self, wire):
        self._w = np.ascontiguousarray(wire, dtype=np.uint8).reshape(64).copy()

    @staticmethod
    def fromBytes(b, engine=None):
        b = _abytes(b, 32)
        if not _canonical_even(b):
            raise ValueError(ENC1)
        out, ok = (engine or get_engine()).ristretto_decode_batch(np.frombuffer(b, np.uint8).reshape(1, 32))
        if not ok[0]:
            raise ValueError(ENC2)
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
        return Point(np.frombuffer((x % P).to_bytes(32, "little") + (y % P).to_bytes(32, "little"), np.uint8))

    def toAffine(self):
        b = self._w.tobytes()
        return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")

    def toBytes(self, engine=None):
        return (engine or get_engine()).ristretto_encode_batch(self._w.reshape(1, 64))[0].tobytes()

    def toHex(self, engine=None):
        return self.toBytes(engine).hex()

    def equals(self, other, engine=None):
        if not isinstance(other, Point):
            raise TypeError("RistrettoPoint expected")
        return bool((engine or get_engine()).ristretto_equals_batch(self._w.reshape(1, 64), other._w.reshape(1, 64))[0])

    def is0(self, engine=None):
        return self.equals(Point.ZERO, engine)

    def add(self, other, engine=None):
        if not isinstance(other, Point):
            raise TypeError("RistrettoPoint expected")
        return Point((engine or get_engine()).add_pairs_batch(ED25519, self._w.reshape(1, 64), other._w.reshape(1, 64))[0][0])

    def subtract(self, other, engine=None):
        if not isinstance(other, Point):
            raise TypeError("RistrettoPoint expected")
        return Point((engine or get_engine()).add_pairs_batch(ED25519, self._w.reshape(1, 64), other._w.reshape(1, 64), True)[0][0])

    def multiply(self, k, engine=None):
        """Point.multiply: 1 <= k < L.  Through the encoding: encode, then decode + multiply + encode in one call, then decode."""
        ks = _scalars([k])
        eng = engine or get_engine()
        out, _ = eng.ristretto_mul_batch(eng.ristretto_encode_batch(self._w.reshape(1, 64)), ks)
        return Point(eng.ristretto_decode_batch(out)[0][0])


Point.BASE = Point.fromAffine(_GX, _GY)
Point.ZERO = Point.fromAffine(0, 1)


def fromBytes_batch(encodings, engine=None):
    """RistrettoPoint.fromBytes for every 32-byte row: (list of Point-or-None, list of bool), None where the reference throws"""
    E = _rows(encodings, 32)
    if not len(encodings):
        return [], []
    out, ok = (engine or get_engine()).ristretto_decode_batch(E)
    ok = [bool(x) for x in ok]
    return [Point(out[i]) if ok[i] else None for i in range(len(ok))], ok


def _wires(points):
    for p in points:
        if not isinstance(p, Point):
            raise TypeError("RistrettoPoint expected")
    return np.stack([p._w for p in points]) if len(points) else np.zeros((0, 64), np.uint8)


def toBytes_batch(points, engine=None):
    if not len(points):
        return []
    return [r.tobytes() for r in (engine or get_engine()).ristretto_encode_batch(_wires(points))]


def equals_batch(a, b, engine=None):
    if len(a) != len(b):
        raise ValueError("arrays of points must have equal length")
    if not len(a):
        return []
    return [bool(x) for x in (engine or get_engine()).ristretto_equals_batch(_wires(a), _wires(b))]


def _encodings(items, eng):
    """a list of 32-byte encodings, or of Points (encoded on the device first)"""
    if len(items) and all(isinstance(p, Point) for p in items):
        return eng.ristretto_encode_batch(_wires(items))
    return _rows(items, 32)


def multiply_batch(points, scalars, engine=None):
    """fromBytes(points[i]).multiply(scalars[i]).toBytes() for every row: (list of 32 bytes or None, list of bool), None where the
    encoding does not decode.  `scalars` may be ONE int: that scalar against every row (NCG_RISTRETTO_ONE_SCALAR, an OPRF
    server's blindEvaluate).  Scalars obey Point.multiply's range 1 <= k < L."""
    one = isinstance(scalars, int)
    if not one and len(scalars) != len(points):
        raise ValueError("arrays of points and scalars must have equal length")
    K = _scalars([scalars] if one else scalars)
    if not len(points):
        return [], []
    eng = engine or get_engine()
    out, ok = eng.ristretto_mul_batch(_encodings(points, eng), K, one_scalar=one)
    ok = [bool(x) for x in ok]
    return [out[i].tobytes() if ok[i] else None for i in range(len(ok))], ok


def multiplyBase_batch(scalars, engine=None):
    """BASE.multiply(k).toBytes() for every k (1 <= k < L), on the fixed-base table"""
    K = _scalars(scalars)
    if not len(scalars):
        return []
    return [r.tobytes() for r in (engine or get_engine()).ristretto_mul_base_batch(K)]


def msm(points, scalars, engine=None):
    """toBytes(sum scalars[i] * fromBytes(points[i])): decode, MSM and encode on the device.  Scalars 0 <= k < L, as the
    reference's pippenger takes them.  An encoding that does not decode raises ValueError with the reference's message."""
    if len(points) != len(scalars):
        raise ValueError("arrays of points and scalars must have equal length")
    K = _scalars(scalars, lo=0)
    eng = engine or get_engine()
    E = _encodings(points, eng)
    for i in range(E.shape[0]):
        if not _canonical_even(E[i].tobytes()):
            raise ValueError(ENC1)
    try:
        return eng.ristretto_msm(E, K).tobytes()
    except RuntimeError as e:
        if getattr(e, "bad_index", -1) >= 0:
            raise ValueError(ENC2) from None
        raise


def _dst(DST):
    if DST is None:
        DST = DEFAULT_DST
    if isinstance(DST, str):
        DST = DST.encode("utf-8")
    DST = bytes(DST)
    if not DST:
        raise ValueError("DST must be non-empty")
    return DST


def deriveToCurve_batch(rows64, engine=None):
    """ristretto255_hasher.deriveToCurve(bytes64).toBytes() for every 64-byte row"""
    B = _rows(rows64, 64)
    if not len(rows64):
        return []
    return [r.tobytes() for r in (engine or get_engine()).ristretto_from_uniform_batch(B)[0]]


def deriveToCurve(bytes64, engine=None):
    _, aff = (engine or get_engine()).ristretto_from_uniform_batch(_rows([bytes64], 64), want_affine=True)
    return Point(aff[0])


def _device_dst(dst):
    """RFC 9380 section 5.3.3: a DST above 255 bytes is replaced by its hash, on the host (the device takes 1..255 bytes)"""
    return hashlib.sha512(b"H2C-OVERSIZE-DST-" + dst).digest() if len(dst) > 255 else dst


def hashToCurve_batch(msgs, DST=None, engine=None, device_hash=False):
    """ristretto255_hasher.hashToCurve(msg, { DST }).toBytes() for every message: expand_message_xmd over SHA-512 here and the map on
    the device, or - device_hash - both in one kernel (ncg_ristretto_hash_to_group_batch)"""
    dst = _dst(DST)
    if device_hash:
        msgs = [bytes(m) for m in msgs]
        if not msgs:
            return []
        return [r.tobytes() for r in (engine or get_engine()).ristretto_hash_to_group_batch(msgs, _device_dst(dst))[0]]
    return deriveToCurve_batch([expand_message_xmd(m, dst, 64, hashlib.sha512) for m in msgs], engine)


def hashToCurve(msg, DST=None, engine=None, device_hash=False):
    if device_hash:
        return Point((engine or get_engine()).ristretto_hash_to_group_batch([bytes(msg)], _device_dst(_dst(DST)), want_affine=True)[1][0])
    return deriveToCurve(expand_message_xmd(msg, _dst(DST), 64, hashlib.sha512), engine)


def hashToScalar_batch(msgs, DST=None, engine=None):
    """ristretto255_hasher.hashToScalar(msg, { DST }) for every message, as ints: expand_message_xmd and the reduction mod L on the
    device (ncg_ristretto_hash_to_scalar_batch)"""
    msgs = [bytes(m) for m in msgs]
    if not msgs:
        return []
    out = (engine or get_engine()).ristretto_hash_to_scalar_batch(msgs, _device_dst(_dst(DST)))
    return [int.from_bytes(r.tobytes(), "little") for r in out]


def hashToScalar(msg, DST=None, engine=None):
    return hashToScalar_batch([msg], DST, engine)[0]
