"""Shared by the bn254 scalar-field NTT tests (test_ntt_bn254_host.py on the host twin, test_gpu_ntt_bn254.py on the
device): the oracle, the host-twin entry points that take a field, the operands of fr29.hpp's ops at the bounds they admit
for THIS field (the pattern of test_host_logic._fr29_cases with bn254's r, fold bit and value bounds), and the residue
sampler for this r."""
import ctypes

import numpy as np

from oracle.curves import Field, makeRng
from oracle.fft import FFT, RootsOfUnity

BN254_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FIELD_BLS12_381_FR, FIELD_BN254_FR = 0, 5          # include/ncg.h
Fr_bn = Field(BN254_R)
M29 = (1 << 29) - 1
C254 = (1 << 254) - BN254_R                        # the fold constant: 2^254 = C254 (mod r)
# the largest value a pass can hold: below 2^256 in (8 words), + 3 r per stage, 10 stages (fr29.hpp)
PASS_MAX = (1 << 256) + 30 * BN254_R - 1


def oracle_fft(generator=7):
    roots = RootsOfUnity(Fr_bn, generator)
    return roots, FFT(roots, Fr_bn)


# ---- host twin (tests/_build/libncg_hosttest.so through tests/hosttest.py's loader)
def _lib():
    import hosttest
    lib = hosttest.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.ht_ntt_field.argtypes = [i32, i32, vp, vp, vp, i32, i32, i32]
    lib.ht_fr29_field_op.argtypes = [i32, i32, vp, vp, vp]
    return lib


def host_ntt(field, log2n, values, omega, flags, passes=None):
    """hosttest.ntt for a field of ncg_ntt: one polynomial of ints -> list of ints; passes = (t0max, tmax) shrinks the
    passes (None: the device's 10 / 8).  Asserts that fr29.hpp's host checks saw no column or limb overflow."""
    n = 1 << log2n
    a = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()
    om = np.frombuffer(int(omega).to_bytes(32, "little"), dtype=np.uint8).copy()
    out = np.zeros(n * 32, dtype=np.uint8)
    t0max, tmax = passes or (0, 0)
    ovf = _lib().ht_ntt_field(field, log2n, om.ctypes.data, a.ctypes.data, out.ctypes.data, flags, t0max, tmax)
    assert ovf == 0, ("overflows (or a refused call: -1)", ovf, field, log2n, flags, passes)
    b = out.tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(n)]


def host_fr29_op(variant, op, a_limbs, b_limbs=None):
    """fr29.hpp op of field `variant` (0 bls12-381 Fr, 1 bn254 Fr) on raw 9-limb operands -> (9 words, overflow count)"""
    A = np.array(list(a_limbs) + [0] * (9 - len(a_limbs)), dtype=np.uint32)
    B = np.array(b_limbs if b_limbs is not None else [0] * 9, dtype=np.uint32)
    out = np.zeros(9, dtype=np.uint32)
    ovf = _lib().ht_fr29_field_op(variant, op, A.ctypes.data, B.ctypes.data, out.ctypes.data)
    assert ovf >= 0, (variant, op)
    return [int(x) for x in out], ovf


# ---- fr29 raw-limb cases
def fr29_val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def fr29_limbs(x):
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def fr29_bias():
    """3 r with limbs 0..7 in [2^29, 2^30) (Fr29Bn254R::BIAS), derived here and not read from the generated header"""
    r = BN254_R
    rest = 3 * r - sum(1 << (29 * i + 29) for i in range(8))
    bias = [((rest >> (29 * i)) & M29) + (1 << 29) for i in range(8)] + [rest >> 232]
    assert fr29_val(bias) == 3 * r and all((1 << 29) <= b < (1 << 30) for b in bias[:8])
    return bias


def fold(v):
    return (v & ((1 << 254) - 1)) + (v >> 254) * C254


def fr29_cases_bn254():
    """{op: (a rows, b rows, check)} numbered as ht_fr29_field_op / ncg_field_check field 8 variant 1; check(a, b, out)
    asserts value and output limbs of one row against big-int arithmetic.  The bounds are those fr29.hpp states for bn254:
    op 0 Montgomery product, left operand at limb bound 6 with limb 8 all ones, right operand r - 1 / all-ones limbs;
    op 1 / 2 a + t and a + 3 r - t with t up to limb 8 = BIAS[8]; op 3 weak normalisation of what op 2 leaves;
    op 4 two folds from PASS_MAX down below 2^256; op 8 one fold, and the third fold of the canonical store: from what two
    folds can leave down below 2 r; op 5 the conditional subtraction up to 2 r - 1; ops 6 / 7 words <-> limbs.
    120 rows per op or more."""
    r = BN254_R
    rinv = pow(1 << 261, -1, r)
    bias = fr29_bias()
    rng = makeRng(0xB254F29)
    cases = {op: ([], []) for op in range(9)}

    def add(op, a, b=None):
        cases[op][0].append(list(a))
        cases[op][1].append(list(b) if b is not None else [0] * 9)

    top_a = [(6 << 29) - 1] * 8 + [(1 << 32) - 1]
    for trial in range(120):
        a = [rng.rndBelow(6 << 29) for _ in range(8)] + [rng.rndBelow(1 << 32)]
        w = fr29_limbs(rng.rndBelow(r))
        if trial == 0:
            a = top_a
        if trial < 2:
            w = fr29_limbs(r - 1)
        if trial == 2:
            a, w = top_a, [M29] * 8 + [(1 << 22) - 1]
        if trial == 3:
            a, w = fr29_limbs(PASS_MAX), fr29_limbs(r - 1)
        add(0, a, w)
    # what one and two folds leave at most, from the largest h each can meet
    f1max = (1 << 254) - 1 + (PASS_MAX >> 254) * C254
    f2max = (1 << 254) - 1 + (f1max >> 254) * C254
    f3max = (1 << 254) - 1 + (f2max >> 254) * C254
    assert f2max < (1 << 256) and f2max >= 2 * r and f3max < 2 * r
    for trial in range(120):
        v = rng.rndBelow(PASS_MAX + 1) if trial else PASS_MAX
        add(4, fr29_limbs(v))
        loose = [rng.rndBelow(7 << 29) for _ in range(8)] + [rng.rndBelow(26 << 22)]    # loose limbs, value below PASS_MAX
        assert fr29_val(loose) <= PASS_MAX
        add(4, loose)
        add(8, fr29_limbs(v))
        add(8, loose)
        add(8, fr29_limbs(f2max if trial == 0 else f1max if trial == 1 else rng.rndBelow(f2max + 1)))
    for trial in range(120):
        v = [0, r - 1, r, 2 * r - 1, f3max][trial] if trial < 5 else rng.rndBelow(2 * r)
        add(5, fr29_limbs(v))
        add(6, [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0])
        add(7, fr29_limbs(v))
    add(6, [0xFFFFFFFF] * 8 + [0])
    add(7, fr29_limbs((1 << 256) - 1))
    for trial in range(120):
        a = [rng.rndBelow(5 << 29) for _ in range(8)] + [rng.rndBelow(1 << 28)]
        t = fr29_limbs(rng.rndBelow(5 * r // 4) if trial else (bias[8] << 232) + (1 << 232) - 1)   # limb 8 at BIAS[8]
        add(2, a, t)
        add(1, a, t)
        add(3, [x + k - y for x, k, y in zip(a, bias, t)])       # the limbs a - t leaves (checked under op 2)

    def mont(a, w, out):
        assert fr29_val(out) % r == fr29_val(a) * fr29_val(w) * rinv % r
        assert all(x <= M29 for x in out[:8]) and fr29_val(out) < fr29_val(a) * fr29_val(w) // (1 << 261) + r + 1
        if fr29_val(a) <= PASS_MAX and fr29_val(w) < r:
            assert fr29_val(out) < 5 * r // 4 and out[8] <= bias[8]

    def reduce256(a, _, out):
        assert fr29_val(out) == fold(fold(fr29_val(a))) and fr29_val(out) % r == fr29_val(a) % r
        assert fr29_val(out) < (1 << 256) and all(x <= M29 for x in out[:8])

    def one_fold(a, _, out):
        assert fr29_val(out) == fold(fr29_val(a)) and all(x <= M29 for x in out[:8])
        if fr29_val(a) <= f2max:        # the third fold of the canonical store
            assert fr29_val(out) < 2 * r

    def cond_sub(a, _, out):
        assert fr29_val(out) == fr29_val(a) % r and all(x <= M29 for x in out[:8])

    def from_words(a, _, out):
        assert fr29_val(out) == sum(x << (32 * i) for i, x in enumerate(a[:8])) and all(x <= M29 for x in out[:8])

    def to_words(a, _, out):
        assert sum(x << (32 * i) for i, x in enumerate(out[:8])) == fr29_val(a) and out[8] == 0

    def sub(a, t, out):
        assert fr29_val(out) == fr29_val(a) + 3 * r - fr29_val(t)
        assert list(out) == [x + k - y for x, k, y in zip(a, bias, t)]

    def add_(a, t, out):
        assert fr29_val(out) == fr29_val(a) + fr29_val(t)

    def weak(d, _, out):
        assert fr29_val(out) == fr29_val(d) and all(x < (1 << 29) + 8 for x in out[:8])

    checks = (mont, add_, sub, weak, reduce256, cond_sub, from_words, to_words, one_fold)
    return {op: (cases[op][0], cases[op][1], checks[op]) for op in range(9)}


# ---- inputs of the device sweep
def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def below_r(c, r=BN254_R):
    """rows of uint8 [k, 32] (little-endian) that are below r"""
    w = c.view("<u8").reshape(-1, 4)
    lt, eq = np.zeros(len(w), dtype=bool), np.ones(len(w), dtype=bool)
    for i in (3, 2, 1, 0):
        ri = np.uint64((r >> (64 * i)) & ((1 << 64) - 1))
        lt |= eq & (w[:, i] < ri)
        eq &= w[:, i] == ri
    return lt


def input_a(bits, seed, r=BN254_R):
    """uniform canonical residues of r with 0, 1, r - 1 at the front and then r - 1 - j, j < 64.  Candidates are 254-bit
    numbers (r has 254 bits: top byte mask 0x3F) and every one that is not below r is rejected."""
    n = 1 << bits
    mask = (1 << (r.bit_length() - 248)) - 1
    gen = np.random.default_rng(seed)
    out, filled = np.empty((n, 32), dtype=np.uint8), 0
    while filled < n:
        c = gen.integers(0, 256, size=(n - filled + (n - filled) // 2 + 16, 32), dtype=np.uint8)
        c[:, 31] &= mask
        c = c[below_r(c, r)][:n - filled]
        out[filled:filled + len(c)] = c
        filled += len(c)
    for i, v in enumerate([0, 1, r - 1] + [r - 1 - j for j in range(64)][:n]):
        if i < n:
            out[i] = le32(v)
    assert below_r(out, r).all()
    return out


def sum_mod_r(arr, r=BN254_R):
    """sum of the residues of a uint8 [n, 32] array mod r (64-bit column sums of the 32-bit words)"""
    w = np.ascontiguousarray(arr).view("<u4").reshape(-1, 8)
    cols = w.sum(axis=0, dtype=np.uint64)
    return sum(int(c) << (32 * j) for j, c in enumerate(cols)) % r
