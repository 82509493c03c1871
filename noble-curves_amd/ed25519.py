"""ed25519 host shim: `verify` / `verify_batch` with the reference's semantics
(src/abstract/edwards.ts:942-989, ZIP-215 default from src/ed25519.ts:162-172).

The shim does the argument checks of the reference and hands (sig, pk, msg) to the library: the
SHA-512 challenge k = SHA-512(R || A || M) mod L (edwards.ts:984, :900-906, :866-868; @noble/hashes in
the reference) and the curve arithmetic both run in HIP kernels (`ncg_ed25519_verify_batch_msgs`).
`hash_on_device=False` computes k with hashlib instead and uses the k32 entry point.

`toMontgomery` / `toMontgomery_batch` (ed25519.utils.toMontgomery: the X25519 key of an Ed25519 public key) run on the device
(`ncg_ed25519_to_montgomery_batch`); `toMontgomerySecret` is one SHA-512 on the host.

Signing (edwards.ts:870-930): `getPublicKey[_batch]`, `getExtendedPublicKey`, `expand_keys`, `sign`, `sign_batch` run on the device,
hashes included (`ncg_ed25519_public_key_batch`, `ncg_ed25519_expand_key_batch`, `ncg_ed25519_sign_batch`); the namespaces
`ed25519ctx` and `ed25519ph` (src/ed25519.ts:146-223) add the domain prefix and the prehash flag.  `verify` / `verify_batch` take
`context=` / `prehash=`: their domain-separated challenge is hashed here and goes through the k32 entry point.
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


def verify_batch(sigs, msgs, publicKeys, zip215=True, engine=None, hash_on_device=True, context=None, prehash=False):
    """List of booleans, one per (signature, message, publicKey) triple.  A non-empty `context` verifies as ed25519ctx and
    `prehash=True` as ed25519ph (the reference's plain `ed25519.verify` throws for a context; here the keywords select the variant,
    and an empty context is plain ed25519 as it is there): the domain-separated challenge is computed with hashlib and goes through
    the k32 entry point.  ed25519ctx with an EMPTY context is `ed25519ctx.verify_batch`."""
    return _verify_rows(sigs, msgs, publicKeys, zip215, engine, hash_on_device,
                        _dom(context, prehash, prehash or (context is not None and len(context) > 0)), prehash)


def _verify_rows(sigs, msgs, publicKeys, zip215, engine, hash_on_device, dom, prehash):
    n = len(sigs)
    if len(msgs) != n or len(publicKeys) != n:
        raise ValueError("arrays of signatures, messages and public keys must have equal length")
    if not isinstance(zip215, bool):
        raise TypeError('"zip215" expected boolean')
    if dom or prehash:
        hash_on_device = False
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
            if prehash:
                msg = hashlib.sha512(msg).digest()
            K[i] = np.frombuffer(challenge(dom + sig[:32], pk, msg).to_bytes(32, "little"), np.uint8)
    eng = engine or get_engine()
    if hash_on_device:
        blob, off = _blob(ms)
        return [bool(x) for x in eng.ed25519_verify_batch_msgs(S, P, blob, off, zip215)]
    return [bool(x) for x in eng.ed25519_verify_batch(S, P, K, zip215)]


def verify(sig, msg, publicKey, zip215=True, engine=None, context=None, prehash=False):
    """eddsa.verify (edwards.ts:942): one signature = a batch of one."""
    return verify_batch([sig], [msg], [publicKey], zip215, engine, context=context, prehash=prehash)[0]


def _blob(ms):
    """messages back to back + their n + 1 offsets (the layout of the message-taking entry points)"""
    n = len(ms)
    off = np.zeros((n + 1,), np.uint64)
    if n:
        off[1:] = np.cumsum([len(m) for m in ms], dtype=np.uint64)
    blob = np.frombuffer(b"".join(ms), np.uint8) if n and off[n] else np.zeros((0,), np.uint8)
    return blob, off


# ---- signing: eddsa.getPublicKey / getExtendedPublicKey / sign (edwards.ts:870-930), ed25519ctx / ed25519ph (ed25519.ts:146-223)
_DOM_PREFIX = b"SigEd25519 no Ed25519 collisions"


def _dom(context, prehash, domain):
    """the bytes in front of both hashes: empty for plain ed25519, ed25519_domain (ed25519.ts:148-160) for ctx / ph"""
    ctx = b"" if context is None else _abytes(context, None, "context")
    if not domain:
        if len(ctx) or prehash:
            raise ValueError("Contexts/pre-hash are not supported")
        return b""
    if len(ctx) > 255:
        raise ValueError("Context is too big")
    return _DOM_PREFIX + bytes([1 if prehash else 0, len(ctx)]) + ctx


def _seeds(secretKeys):
    K = np.zeros((len(secretKeys), 32), np.uint8)
    for i, sk in enumerate(secretKeys):
        K[i] = np.frombuffer(_abytes(sk, 32, "secretKey"), np.uint8)
    return K


def getPublicKey_batch(secretKeys, engine=None):
    """eddsa.getPublicKey for every 32-byte secret key, on the device (`ncg_ed25519_public_key_batch`): list of bytes"""
    K = _seeds(secretKeys)
    out = (engine or get_engine()).ed25519_public_key_batch(K)
    K[:] = 0
    return [out[i].tobytes() for i in range(out.shape[0])]


def getPublicKey(secretKey, engine=None):
    return getPublicKey_batch([secretKey], engine)[0]


def expand_keys(secretKeys, engine=None):
    """96-byte rows scalar || prefix || publicKey (uint8 [n, 96]) for repeated use with sign_batch(..., expanded=True)"""
    K = _seeds(secretKeys)
    out = (engine or get_engine()).ed25519_expand_key_batch(K)
    K[:] = 0
    return out


def getExtendedPublicKey(secretKey, engine=None):
    """head, prefix, scalar, pointBytes of the reference's getExtendedPublicKey; scalar and pointBytes come from the device,
    head is the clamped first half of SHA-512(secretKey) (the device keeps it only reduced mod L)"""
    row = expand_keys([secretKey], engine)[0].tobytes()
    return {"head": toMontgomerySecret(secretKey), "prefix": row[32:64], "scalar": int.from_bytes(row[:32], "little"),
            "pointBytes": row[64:]}


def sign_batch(msgs, secretKeys, context=None, engine=None, expanded=False):
    """ed25519.sign per message (plain ed25519: a non-empty context raises like the reference; ed25519ctx / ed25519ph are the
    namespaces below).  secretKeys: ONE key for every message (bytes, or one 96-byte row with expanded=True) or a list / array as
    long as msgs.  Returns a list of 64-byte signatures; None where the device refused the row (r = 0 mod L)."""
    return _sign_rows(msgs, secretKeys, _dom(context, False, False), False, engine, expanded)


def _sign_rows(msgs, secretKeys, dom, prehash, engine, expanded):
    ms = [_abytes(m, None, "message") for m in msgs]
    width = 96 if expanded else 32
    one = isinstance(secretKeys, (bytes, bytearray, memoryview)) or (isinstance(secretKeys, np.ndarray) and secretKeys.ndim == 1)
    rows = [secretKeys] if one else secretKeys
    if not one and len(rows) != len(ms):
        raise ValueError("arrays of messages and secret keys must have equal length")
    K = np.zeros((len(rows), width), np.uint8)
    for i, sk in enumerate(rows):
        K[i] = np.frombuffer(_abytes(sk, width, "secretKey"), np.uint8)
    blob, off = _blob(ms)
    sig, ok = (engine or get_engine()).ed25519_sign_batch(K, blob, off, dom, expanded=expanded, one_key=one, prehash=prehash)
    K[:] = 0
    return [sig[i].tobytes() if ok[i] else None for i in range(len(ms))]


def _sign_one(msg, secretKey, dom, prehash, engine):
    _abytes(secretKey, 32, "secretKey")
    out = _sign_rows([msg], secretKey, dom, prehash, engine, False)[0]
    if out is None:
        raise ValueError("invalid scalar: expected 1 <= sc < curve.n")
    return out


def sign(msg, secretKey, context=None, engine=None):
    """ed25519.sign (edwards.ts:909): a batch of one; raises where the reference throws"""
    _abytes(secretKey, 32, "secretKey")
    return _sign_one(msg, secretKey, _dom(context, False, False), False, engine)


class _Variant:
    """ed25519ctx / ed25519ph: the same functions with the domain of ed25519.ts:148-160 and, for ph, SHA-512 of the message"""

    def __init__(self, prehash):
        self._ph = prehash

    getPublicKey = staticmethod(getPublicKey)
    getPublicKey_batch = staticmethod(getPublicKey_batch)
    getExtendedPublicKey = staticmethod(getExtendedPublicKey)
    expand_keys = staticmethod(expand_keys)

    def sign(self, msg, secretKey, context=None, engine=None):
        _abytes(secretKey, 32, "secretKey")
        return _sign_one(msg, secretKey, _dom(context, self._ph, True), self._ph, engine)

    def sign_batch(self, msgs, secretKeys, context=None, engine=None, expanded=False):
        return _sign_rows(msgs, secretKeys, _dom(context, self._ph, True), self._ph, engine, expanded)

    def verify(self, sig, msg, publicKey, zip215=True, engine=None, context=None):
        return self.verify_batch([sig], [msg], [publicKey], zip215, engine, context)[0]

    def verify_batch(self, sigs, msgs, publicKeys, zip215=True, engine=None, context=None):
        return _verify_rows(sigs, msgs, publicKeys, zip215, engine, False, _dom(context, self._ph, True), self._ph)


ed25519ctx = _Variant(False)
ed25519ph = _Variant(True)


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
