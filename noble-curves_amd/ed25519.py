"""ed25519 host shim: `verify` / `verify_batch` with the reference's semantics
(src/abstract/edwards.ts:942-989, ZIP-215 default from src/ed25519.ts:162-172).

The shim does the argument checks of the reference and hands (sig, pk, msg) to the library: the
SHA-512 challenge k = SHA-512(R || A || M) mod L (edwards.ts:984, :900-906, :866-868; @noble/hashes in
the reference) and the curve arithmetic both run in HIP kernels (`ncg_ed25519_verify_batch_msgs`).
`hash_on_device=False` computes k with hashlib instead and uses the k32 entry point.

`toMontgomery` / `toMontgomery_batch` (ed25519.utils.toMontgomery: the X25519 key of an Ed25519 public key) run on the device
(`ncg_ed25519_to_montgomery_batch`); `toMontgomerySecret` is one SHA-512 on the host.
"""
import hashlib

import numpy as np

from ._native import get_engine

L = 0x1000000000000000000000000000000014DEF9DEA2F79CD65812631A5CF5D3ED


def _abytes(b, length, title):
    if not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError('"%s" expected Uint8Array, got type=%s' % (title, type(b).__name__))
    b = bytes(b)
    if length is not None and len(b) != length:
        raise ValueError('"%s" expected Uint8Array of length %d, got length=%d' % (title, length, len(b)))
    return b


def challenge(r_bytes, pk_bytes, msg):
    """hashDomainToScalar + modN_LE (edwards.ts:900-906, :866-868)."""
    return int.from_bytes(hashlib.sha512(bytes(r_bytes) + bytes(pk_bytes) + bytes(msg)).digest(), "little") % L


def verify_batch(sigs, msgs, publicKeys, zip215=True, engine=None, hash_on_device=True):
    """List of booleans, one per (signature, message, publicKey) triple."""
    n = len(sigs)
    if len(msgs) != n or len(publicKeys) != n:
        raise ValueError("arrays of signatures, messages and public keys must have equal length")
    if not isinstance(zip215, bool):
        raise TypeError('"zip215" expected boolean')
    S = np.zeros((n, 64), np.uint8)
    P = np.zeros((n, 32), np.uint8)
    K = np.zeros((n, 32), np.uint8)
    ms = []
    for i in range(n):
        sig = _abytes(sigs[i], 64, "signature")
        msg = _abytes(msgs[i], None, "message")
        pk = _abytes(publicKeys[i], 32, "publicKey")
        S[i] = np.frombuffer(sig, np.uint8)
        P[i] = np.frombuffer(pk, np.uint8)
        if hash_on_device:
            ms.append(msg)
        else:
            K[i] = np.frombuffer(challenge(sig[:32], pk, msg).to_bytes(32, "little"), np.uint8)
    eng = engine or get_engine()
    if hash_on_device:
        off = np.zeros((n + 1,), np.uint64)
        if n:
            off[1:] = np.cumsum([len(m) for m in ms], dtype=np.uint64)
        blob = np.frombuffer(b"".join(ms), np.uint8) if n and off[n] else np.zeros((0,), np.uint8)
        return [bool(x) for x in eng.ed25519_verify_batch_msgs(S, P, blob, off, zip215)]
    return [bool(x) for x in eng.ed25519_verify_batch(S, P, K, zip215)]


def verify(sig, msg, publicKey, zip215=True, engine=None):
    """eddsa.verify (edwards.ts:942): one signature = a batch of one."""
    return verify_batch([sig], [msg], [publicKey], zip215, engine)[0]


# ---- ed25519.utils.toMontgomery / toMontgomerySecret (src/ed25519.ts:128-143, edwards.ts:1022-1031)
P = 2**255 - 19
_D = -121665 * pow(121666, -1, P) % P


def toMontgomery_batch(publicKeys, engine=None):
    """u = (1 + y) / (1 - y) of Point.fromBytes(publicKey) (strict rules) for every key, on the device
    (`ncg_ed25519_to_montgomery_batch`): (list of bytes-or-None, list of bool), None where the reference throws."""
    K = np.zeros((len(publicKeys), 32), np.uint8)
    for i, pk in enumerate(publicKeys):
        K[i] = np.frombuffer(_abytes(pk, 32, "point"), np.uint8)
    out, ok = (engine or get_engine()).ed25519_to_montgomery_batch(K)
    ok = [bool(x) for x in ok]
    return [out[i].tobytes() if ok[i] else None for i in range(len(ok))], ok


def _to_montgomery_error(pk):
    """the message of the error the reference throws for a key the device refused (rare path: host integers)"""
    y = int.from_bytes(pk, "little") & ((1 << 255) - 1)
    if y >= P:
        return "expected valid point.y: 0 <= n < %d, got %d" % (P, y)
    x2 = (y * y - 1) * pow(_D * y * y + 1, -1, P) % P
    if x2 and pow(x2, (P - 1) // 2, P) != 1:
        return "bad point: invalid y coordinate"
    if x2 == 0 and pk[31] & 0x80:
        return "bad point: x=0 and x_0=1"
    return "invert: expected non-zero number"   # y = 1


def toMontgomery(publicKey, engine=None):
    """ed25519.utils.toMontgomery: a batch of one; raises ValueError with the reference's message where it throws"""
    out, ok = toMontgomery_batch([publicKey], engine)
    if not ok[0]:
        raise ValueError(_to_montgomery_error(_abytes(publicKey, 32, "point")))
    return out[0]


def toMontgomerySecret(secretKey):
    """ed25519.utils.toMontgomerySecret: the clamped first half of SHA-512(secretKey), on the host"""
    if not isinstance(secretKey, (bytes, bytearray, memoryview, np.ndarray)):   # abytes without a title (ed25519.ts:138)
        raise TypeError("expected Uint8Array of length 32, got type=%s" % type(secretKey).__name__)
    if len(bytes(secretKey)) != 32:
        raise ValueError("expected Uint8Array of length 32, got length=%d" % len(bytes(secretKey)))
    h = bytearray(hashlib.sha512(bytes(secretKey)).digest()[:32])
    h[0] &= 248
    h[31] = (h[31] & 127) | 64
    return bytes(h)
