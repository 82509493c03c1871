"""secp256k1 BIP-340 Schnorr host shim: `verify` / `verify_batch` with the reference's semantics
(src/secp256k1.ts:228-258), and `getPublicKey` / `sign` with their batch forms (:147-221), whose three tagged hashes, both
fixed-base multiplies and s = k + e d run in HIP kernels (`ncg_schnorr_sign_batch`, `ncg_secp256k1_public_key_batch`).  The shim checks the argument types and lengths like the reference (loudly), computes
the challenge e = int(taggedHash('BIP0340/challenge', r || pk || m)) mod n with hashlib (the reference hashes on
the host as well, :129-137, :176-178) and hands (sig, e, pk) to the library; the range checks on r and s, lift_x,
R = s G - e P and the three acceptance tests run in HIP kernels (`ncg_schnorr_verify_batch`).
"""
import hashlib
import os

import numpy as np

from ._native import SECP_PK_XONLY, get_engine

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
_TAG = hashlib.sha256(b"BIP0340/challenge").digest() * 2


def _abytes(b, length, title):
    if not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError('"%s" expected Uint8Array, got type=%s' % (title, type(b).__name__))
    b = bytes(b)
    if length is not None and len(b) != length:
        raise ValueError('"%s" expected Uint8Array of length %d, got length=%d' % (title, length, len(b)))
    return b


def challenge(r_bytes, pk_bytes, msg):
    return int.from_bytes(hashlib.sha256(_TAG + r_bytes + pk_bytes + msg).digest(), "big") % N


def verify_batch(signatures, messages, publicKeys, engine=None, hash_on_device=True):
    """[schnorr.verify(sig, msg, pk) for each triple] in one launch.  hash_on_device: the tagged challenge hash runs in
    a HIP kernel as well (ncg_schnorr_verify_batch_msgs); False computes it here with hashlib."""
    n = len(signatures)
    if len(messages) != n or len(publicKeys) != n:
        raise ValueError("arrays of signatures, messages and public keys must have equal length")
    if n == 0:
        return []
    S = np.zeros((n, 64), np.uint8)
    E = np.zeros((n, 32), np.uint8)
    K = np.zeros((n, 32), np.uint8)
    ms = []
    for i in range(n):
        sig = _abytes(signatures[i], 64, "signature")
        msg = _abytes(messages[i], None, "message")
        pk = _abytes(publicKeys[i], 32, "publicKey")
        S[i] = np.frombuffer(sig, np.uint8)
        K[i] = np.frombuffer(pk, np.uint8)
        # pointToBytes(lift_x(pk)) is pk itself whenever lift_x succeeds; where it fails the verdict is false anyway
        if hash_on_device:
            ms.append(msg)
        else:
            E[i] = np.frombuffer(challenge(sig[:32], pk, msg).to_bytes(32, "big"), np.uint8)
    eng = engine or get_engine()
    if hash_on_device:
        return [bool(x) for x in eng.schnorr_verify_batch_msgs(S, ms, K)]
    return [bool(x) for x in eng.schnorr_verify_batch(S, E, K)]


def verify(signature, message, publicKey, engine=None, hash_on_device=True):
    return verify_batch([signature], [message], [publicKey], engine, hash_on_device)[0]


# ---- signing.  The messages of the errors are the reference's own (tests/golden/secp256k1_sign_kat.json, "errors").
def _amsg(b):
    if not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError('"message" expected Uint8Array, got type=%s' % {str: "string", int: "number", float: "number"}.get(type(b), "object"))
    return bytes(b)


def _secret_rows(secretKeys):
    """(uint8 [k, 32], one_key): a single bytes-like key serves every row"""
    one = isinstance(secretKeys, (bytes, bytearray, memoryview))
    keys = [secretKeys] if one else list(secretKeys)
    rows = np.zeros((len(keys), 32), np.uint8)
    try:
        for i, sk in enumerate(keys):
            rows[i] = np.frombuffer(_abytes(sk, 32, "secretKey"), np.uint8)
    except (TypeError, ValueError):
        rows.fill(0)
        raise
    return rows, one


def _public_keys(eng, rows):
    """the x-only public keys of packed secret-key rows as bytes; a refused key raises the reference's message"""
    out, ok = eng.secp256k1_public_key_batch(rows, SECP_PK_XONLY)
    for i in range(rows.shape[0]):
        if not ok[i]:
            raise ValueError(_refused_key(rows[i]))
    return [bytes(r) for r in out]


def _refused_key(row):
    d = int.from_bytes(bytes(row), "big")
    if d == 0:
        return "invalid scalar: out of range"
    return "invalid field element: outside of range 0..ORDER" if d >= N else None


def getPublicKey_batch(secretKeys, engine=None):
    """[schnorr.getPublicKey(sk) for each key]: the 32-byte x-only keys"""
    rows, _ = _secret_rows(list(secretKeys))
    if rows.shape[0] == 0:
        return []
    try:
        return _public_keys(engine or get_engine(), rows)
    finally:
        rows.fill(0)                                                       # the packed copy of the keys, on every way out


def getPublicKey(secretKey, engine=None):
    return getPublicKey_batch([secretKey], engine)[0]


def sign_batch(messages, secretKeys, auxRand=None, engine=None, verify=True):
    """[schnorr.sign(msg, sk, aux) for each pair] in one launch.  secretKeys: one key per message, or a single bytes object that
    signs every message.  auxRand: None (32 fresh bytes from os.urandom per row, as the reference draws them), one 32-byte value
    for every row, or a list of them.  verify (the reference verifies every signature it makes): run verify_batch over the result."""
    n = len(messages)
    msgs = [_amsg(m) for m in messages]
    rows, one_key = _secret_rows(secretKeys)
    A = None
    try:                                                                   # the packed keys and aux rows are zeroed on every way out
        if not one_key and rows.shape[0] != n:
            raise ValueError("arrays of messages and secret keys must have equal length")
        if auxRand is None:
            A = np.frombuffer(os.urandom(32 * n), np.uint8).reshape(n, 32).copy()
        else:
            aux = [auxRand] * n if isinstance(auxRand, (bytes, bytearray, memoryview)) else list(auxRand)
            if len(aux) != n:
                raise ValueError("arrays of messages and auxRand must have equal length")
            A = np.frombuffer(b"".join(_abytes(a, 32, "auxRand") for a in aux), np.uint8).reshape(n, 32).copy()
        if n == 0:
            return []
        eng = engine or get_engine()
        sig, ok = eng.schnorr_sign_batch(rows, A, msgs, one_key=one_key)
        for i in range(n):
            if not ok[i]:
                raise ValueError(_refused_key(rows[0 if one_key else i]) or "sign failed: k is zero")
        out = [bytes(r) for r in sig]
        if verify:
            pub = _public_keys(eng, rows)
            if not all(verify_batch(out, msgs, pub * n if one_key else pub, engine=eng)):
                raise ValueError("sign: Invalid signature produced")
        return out
    finally:
        rows.fill(0)
        if A is not None:
            A.fill(0)


def sign(message, secretKey, auxRand=None, engine=None, verify=True):
    return sign_batch([message], [secretKey], None if auxRand is None else [auxRand], engine, verify)[0]
