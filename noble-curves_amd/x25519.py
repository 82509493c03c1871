"""X25519 host shim: `scalarMult` / `getSharedSecret` / `getPublicKey` and their batch forms with the reference's semantics
(src/abstract/montgomery.ts:247-420, built at src/ed25519.ts:266-292).

The shim does the argument checks of the reference, in its order - the u coordinate (the peer's key) before the scalar
(montgomery.ts:324-326) - and hands the raw 32-byte rows to the library: clamping, the reduction of non-canonical u, the
low-order test and the ladder all run in HIP kernels (`ncg_x25519_batch`, `ncg_x25519_base_batch`).  Batch forms return
(list of bytes-or-None, list of bool): None where the reference throws 'invalid private or public key received'.
"""
import numpy as np

from ._native import get_engine
from .ed25519 import _abytes

P = 2**255 - 19
GuBytes = (9).to_bytes(32, "little")
INVALID = "invalid private or public key received"
# u coordinates whose order divides the cofactor, on the curve and on its twist (montgomery.ts:303-312)
LOW_ORDER_U = frozenset((
    0, 1, P - 1,
    325606250916557431795983626356110631294008115727848805560023387167927233504,
    39382357235489614581723060781553021112529911719440698176882885853963445705823,
))


def _rows(items, title):
    out = np.zeros((len(items), 32), np.uint8)
    for i, b in enumerate(items):
        out[i] = np.frombuffer(_abytes(b, 32, title), np.uint8)
    return out


def _result(out, ok):
    ok = [bool(x) for x in ok]
    return [out[i].tobytes() if ok[i] else None for i in range(len(ok))], ok


def _is_low_order(u):
    """decodeU (bit 255 masked, mod p) then the blocklist: what the device tests before the ladder"""
    return (int.from_bytes(u, "little") & ((1 << 255) - 1)) % P in LOW_ORDER_U


def scalarMult_batch(scalars, us, engine=None):
    """x25519.scalarMult for every (scalar, u) pair.  `scalars` may be ONE bytes value: that secret against every u (one upload,
    NCG_X25519_ONE_SCALAR)."""
    one = isinstance(scalars, (bytes, bytearray, memoryview))
    if not one and len(scalars) != len(us):
        raise ValueError("arrays of scalars and u coordinates must have equal length")
    U = np.zeros((len(us), 32), np.uint8)
    S = np.zeros((1 if one else len(us), 32), np.uint8)
    for i in range(len(us)):   # row by row, the u coordinate first (montgomery.ts:324-326)
        U[i] = np.frombuffer(_abytes(us[i], 32, "uCoordinate"), np.uint8)
        if not one:
            S[i] = np.frombuffer(_abytes(scalars[i], 32, "scalar"), np.uint8)
    if one:
        S[0] = np.frombuffer(_abytes(scalars, 32, "scalar"), np.uint8)
    return _result(*(engine or get_engine()).x25519_batch(S, U, one_scalar=one))


def getSharedSecret_batch(secretKeys, publicKeys, engine=None):
    """x25519.getSharedSecret for every pair, or one secret key (a bytes value) against many public keys"""
    return scalarMult_batch(secretKeys, publicKeys, engine)


def getPublicKey_batch(secretKeys, engine=None):
    """x25519.getPublicKey for every secret key"""
    return _result(*(engine or get_engine()).x25519_base_batch(_rows(secretKeys, "scalar")))


def scalarMult(scalar, u, engine=None):
    """x25519.scalarMult (montgomery.ts:314-331): a batch of one, with the reference's errors in the reference's order"""
    u = _abytes(u, 32, "uCoordinate")
    if _is_low_order(u):
        raise ValueError(INVALID)
    out, ok = scalarMult_batch([_abytes(scalar, 32, "scalar")], [u], engine)
    if not ok[0]:
        raise ValueError(INVALID)
    return out[0]


def getSharedSecret(secretKey, publicKey, engine=None):
    return scalarMult(secretKey, publicKey, engine)


def getPublicKey(secretKey, engine=None):
    """x25519.getPublicKey = scalarMultBase (montgomery.ts:335-342)"""
    out, ok = getPublicKey_batch([secretKey], engine)
    if not ok[0]:
        raise ValueError(INVALID)
    return out[0]
