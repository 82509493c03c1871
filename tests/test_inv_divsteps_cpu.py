"""f_inv of the two plain Fe9 primes (fe9_inv.hpp: Bernstein - Yang division steps in batches of 30 on signed 30-bit limbs)
on the CPU twin of the device code, against pow(x, -1, p) with 0 -> 0 (modular.ts:159-182 values): the special values of
each prime, every 2^k, 2^k - 1 and p - 2^k, inverses of small integers, 10^5 random residues, and raw limbs at the top of
what the bound types 1, 2 and 7 admit.  The Fermat chains that f_inv replaced stay in the source (f_inv_fermat: cross-check
and the way out of the loop cap) and must agree."""
import ctypes
import random

import numpy as np
import pytest

import hosttest
from helpers import MASK29, U, limbs, loose, val
from oracle.curves import ED25519_P, SECP256K1_P

PRIMES = [pytest.param(0, SECP256K1_P, id="secp256k1"), pytest.param(1, ED25519_P, id="ed25519")]


def _inv_batch(field, A, which, rows, raw=False):
    """ht_fe9_inv_batch on rows of 9 raw limbs: the canonical values as ints (and the limbs f_inv returned)"""
    lib = hosttest.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.ht_fe9_inv_batch.argtypes = [i32, i32, i32, vp, vp, vp, i32]
    a = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 9)
    n = a.shape[0]
    out = np.zeros((n, 8), dtype=np.uint32)
    rw = np.zeros((n, 9), dtype=np.uint32)
    assert lib.ht_fe9_inv_batch(field, A, which, a.ctypes.data, out.ctypes.data, rw.ctypes.data if raw else None, n) == 0
    b = out.tobytes()
    vals = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(n)]
    return (vals, rw) if raw else vals


def _limbs_many(xs):
    """tight 29-bit limbs of many values below 2^256, vectorised"""
    by = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint8).reshape(-1, 32)
    bits = np.unpackbits(by, axis=1, bitorder="little")
    bits = np.concatenate([bits, np.zeros((bits.shape[0], 5), dtype=np.uint8)], axis=1).reshape(-1, 9, 29)
    return (bits.astype(np.uint64) << np.arange(29, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def _expect(x, p):
    return pow(x, -1, p) if x % p else 0


def edge_values(p):
    """the issue's list: values below 2^261 (tight limbs), not all below p"""
    xs = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, p, 2 * p, (1 << 256) - 1]
    for k in range(256):
        xs += [1 << k, (1 << k) - 1, (p - (1 << k)) % p]
    xs += list(range(3, 64)) + [pow(s, -1, p) for s in range(2, 64)]
    return xs


def loose_rows(p, B, rng, count):
    """raw limbs below B * U as test_gpu_field.py builds them (all at the top, one at the top, random with some at the top),
    and special values written with every limb as high as the bound admits (helpers.loose)"""
    rows = [[B * U - 1] * 9, [0] * 8 + [B * U - 1], [B * U - 1] + [0] * 8]
    for x in (0, 1, 2, p - 1, p - 2, (p - 1) // 2, 3):
        rows.append(loose(x, B, p))
    while len(rows) < count:
        rows.append([rng.randrange(B * U) if rng.randrange(4) else B * U - 1 for _ in range(9)])
    return rows


@pytest.mark.parametrize("field,p", PRIMES)
def test_edge_values_and_fermat(field, p):
    xs = edge_values(p)
    rows = [limbs(x) for x in xs]
    assert all(l < (1 << 29) for r in rows for l in r)
    exp = [_expect(x, p) for x in xs]
    got, raw = _inv_batch(field, 1, 0, rows, raw=True)
    assert got == exp
    # the returned limbs are the canonical ones: 0 (and p, 2p) come back as literal zero
    assert [val(r) for r in raw] == exp and int(raw.max()) <= MASK29
    assert _inv_batch(field, 1, 1, rows) == exp                       # the kept Fermat chain
    for A in (2, 7):                                                  # the same tight limbs read at a looser bound type
        assert _inv_batch(field, A, 0, rows) == exp


@pytest.mark.parametrize("field,p", PRIMES)
def test_loose_limbs(field, p):
    rng = random.Random(0xD1F5 + field)
    for A in (1, 2, 7):
        rows = loose_rows(p, A, rng, 600)
        exp = [_expect(val(r), p) for r in rows]
        assert _inv_batch(field, A, 0, rows) == exp, A
        assert _inv_batch(field, A, 1, rows) == exp, A


@pytest.mark.parametrize("field,p", PRIMES)
def test_random_values(field, p):
    rng = random.Random(0x5AFE6CD + field)
    xs = [rng.randrange(p) for _ in range(100000)]
    rows = _limbs_many(xs)
    assert [val(r) for r in rows[:16]] == xs[:16]
    got = _inv_batch(field, 1, 0, rows)
    assert got == [_expect(x, p) for x in xs]
    assert _inv_batch(field, 1, 1, rows[:5000]) == got[:5000]         # Fermat agrees
