"""Field-level parity ON THE DEVICE: the field code of the kernels - fe9.hpp's
inline-asm multiply-add chains, interleaved fold, bound-typed lazy add / sub / normalise / zero test /
addition-chain inversion for secp256k1 and ed25519, and the radix-2^29 Montgomery code for bls12-381 -
against big-int arithmetic (modular.ts:940-982 values), with operands at the top of what each bound type
admits and at the special values of each prime; the Fr form of the NTT butterflies (fr29.hpp) on raw limbs."""
import numpy as np
import pytest

from noble_curves_amd import get_engine
from oracle.curves import BLS_P, ED25519_P, SECP256K1_P, makeRng

pytestmark = pytest.mark.gpu
U = (1 << 29) + (1 << 19)
M29 = (1 << 29) - 1


def _val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def _words(out_row):
    return sum(int(w) << (32 * i) for i, w in enumerate(out_row))


@pytest.mark.parametrize("fid,p", [(0, SECP256K1_P), (1, ED25519_P)])
def test_fe9_ops_on_device(fid, p):
    eng = get_engine()
    rng = makeRng(0xF1E1D + fid)

    def operand(B, kind):
        if kind == 0:
            return [B * U - 1] * 9
        if kind == 1:
            return [0] * 8 + [B * U - 1]
        if kind == 2:
            return [B * U - 1] + [0] * 8
        if kind == 3:                                   # a canonical special value spread over tight limbs
            x = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, p, 2 * p, (1 << 256) - 1][rng.rnd64() % 9]
            return [(x >> (29 * i)) & M29 for i in range(9)]
        return [rng.rndBelow(B * U) if rng.rnd64() % 4 else B * U - 1 for _ in range(9)]

    for variant in (11, 12, 17, 71, 23, 22, 33, 77):
        A, B = variant // 10, variant % 10
        a = np.array([operand(A, k % 6) for k in range(96)], dtype=np.uint32)
        b = np.array([operand(B, (k * 5 + 1) % 7) for k in range(96)], dtype=np.uint32)
        va, vb = [_val(r) for r in a], [_val(r) for r in b]
        got = eng.field_check(fid, 0, variant, a, b)
        assert [_words(r) for r in got] == [x * y % p for x, y in zip(va, vb)], variant
        assert int(eng.field_check(fid, 9, variant, a, b)[:, 0].max()) < U
        if A <= 2:
            assert [_words(r) for r in eng.field_check(fid, 1, variant, a, b)] == [x * x % p for x in va]
        if A + B <= 7:
            assert [_words(r) for r in eng.field_check(fid, 2, variant, a, b)] == [(x + y) % p for x, y in zip(va, vb)]
        if A + B + 1 <= 7:
            assert [_words(r) for r in eng.field_check(fid, 3, variant, a, b)] == [(x - y) % p for x, y in zip(va, vb)]
        if A + 1 <= 7:
            assert [_words(r) for r in eng.field_check(fid, 4, variant, a, b)] == [(-x) % p for x in va]
        assert [_words(r) for r in eng.field_check(fid, 6, variant, a, b)] == [x % p for x in va]
        assert [int(r[0]) for r in eng.field_check(fid, 7, variant, a, b)] == [1 if x % p == 0 else 0 for x in va]
    # exact multiples of p written with loose limbs must test as zero; inversion by the addition chains
    mult = []
    for j in (0, 1, 2, 5, 31, 33, 64, 100):
        x = j * p
        l = [(x >> (29 * i)) & M29 for i in range(8)] + [x >> (29 * 8)]
        if l[8] < 7 * U:
            mult.append(l)
    zl = np.array(mult, dtype=np.uint32)
    assert [int(r[0]) for r in eng.field_check(fid, 7, 71, zl, zl)] == [1] * len(mult)
    xs = [1, 2, 3, p - 1, p - 2, 0] + [rng.rndBelow(p) for _ in range(26)]
    xl = np.array([[(x >> (29 * i)) & M29 for i in range(9)] for x in xs], dtype=np.uint32)
    assert [_words(r) for r in eng.field_check(fid, 5, 11, xl, xl)] == [pow(x, -1, p) if x else 0 for x in xs]


def test_fe29_ops_on_device():
    eng = get_engine()
    rng = makeRng(0xB15)
    p = BLS_P
    xs = [0, 1, 2, p - 1, p - 2, (p - 1) // 2] + [rng.rndBelow(p) for _ in range(58)]
    ys = [xs[(i * 7 + 3) % len(xs)] for i in range(len(xs))]
    w = lambda v: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]  # noqa: E731
    a, b = np.array([w(x) for x in xs], dtype=np.uint32), np.array([w(y) for y in ys], dtype=np.uint32)
    for op, f in ((0, lambda x, y: x * y % p), (1, lambda x, y: x * x % p), (2, lambda x, y: (x + y) % p),
                  (3, lambda x, y: (x - y) % p), (4, lambda x, y: (-x) % p), (5, lambda x, y: pow(x, -1, p) if x else 0)):
        got = eng.field_check(2, op, 0, a, b)
        assert [_words(r) for r in got] == [f(x, y) for x, y in zip(xs, ys)], op


# ---- bls12-381: RAW radix-2^29 limbs at the top of the lazy value bounds:
# the fused products keep up to 56 product + 14 reduction terms per 64-bit column, which only fits because limb 13
# of a value below 2^12 p is at most 53256 (fe29.hpp) - generic values never come near that bound.
R406 = 1 << 406


def _max_limbs(bound):
    """largest value below bound * p whose 13 low limbs are all 2^29 - 1"""
    top = (bound * BLS_P - 1) >> 377
    v = (top << 377) | ((1 << 377) - 1)
    if v >= bound * BLS_P:
        v -= 1 << 377
    assert v < bound * BLS_P
    return v


def _limbs14(v):
    assert v < (1 << 406)
    return [(v >> (29 * i)) & M29 for i in range(13)] + [v >> 377]


def _operand29(bound, kind, rng):
    if kind == 0:
        return _max_limbs(bound)
    if kind == 1:
        return bound * BLS_P - 1                     # the largest value of the bound type
    if kind == 2:
        return [0, 1, BLS_P, BLS_P - 1, (bound - 1) * BLS_P + 1][rng.rnd64() % 5]
    return rng.rndBelow(bound * BLS_P)


def _unmont(v):
    return v * pow(R406, -2, BLS_P) % BLS_P          # product of two Montgomery-form operands, taken out of the form


@pytest.mark.parametrize("op", [0, 1, 6])
def test_fe29_raw_limbs_at_the_bounds(op):
    eng = get_engine()
    rng = makeRng(0x29F + op)
    ba, bb = 4096, (4096 if op == 0 else 2048)
    A, B, exp = [], [], []
    for it in range(96):
        ka, kb = (it % 4, (it // 4) % 4) if it < 16 else (3, 3)
        a, c = _operand29(ba, ka, rng), _operand29(ba, ka if it < 16 else 3, rng)
        b, d = _operand29(bb, kb, rng), _operand29(bb, kb if it < 16 else 3, rng)
        A.append(_limbs14(a) + _limbs14(c))
        B.append(_limbs14(b) + _limbs14(d))
        exp.append(_unmont(a * b if op == 0 else a * a if op == 1 else a * b - c * d))
    out = eng.field_check(3, op, 0, np.array(A, dtype=np.uint32), np.array(B, dtype=np.uint32))
    for i in range(len(exp)):
        assert _words(out[i]) == exp[i], (op, i)


@pytest.mark.parametrize("op", [0, 1, 6])
def test_lane_paired_fp2_raw_limbs_at_the_bounds(op):
    """Fe29x2P multiply / square / fused a*b - c*d (tower.ts:420-438 values) with every limb of every half at its maximum."""
    eng = get_engine()
    rng = makeRng(0x2F2 + op)
    ba = 2048 if op == 1 else 4096
    bb = 2048 if op == 0 else 1024
    A, B, exp = [], [], []

    def fp2mul(x, y):
        return (x[0] * y[0] - x[1] * y[1], x[0] * y[1] + x[1] * y[0])
    for it in range(96):
        ka, kb = (it % 4, (it // 4) % 4) if it < 16 else (3, 3)
        a = (_operand29(ba, ka, rng), _operand29(ba, ka, rng))
        c = (_operand29(ba, ka, rng), _operand29(ba, ka, rng))
        b = (_operand29(bb, kb, rng), _operand29(bb, kb, rng))
        d = (_operand29(bb, kb, rng), _operand29(bb, kb, rng))
        A.append(_limbs14(a[0]) + _limbs14(a[1]) + _limbs14(c[0]) + _limbs14(c[1]))
        B.append(_limbs14(b[0]) + _limbs14(b[1]) + _limbs14(d[0]) + _limbs14(d[1]))
        if op == 0:
            r = fp2mul(a, b)
        elif op == 1:
            r = fp2mul(a, a)
        else:
            ab, cd = fp2mul(a, b), fp2mul(c, d)
            r = (ab[0] - cd[0], ab[1] - cd[1])
        exp.append((_unmont(r[0]), _unmont(r[1])))
    out = eng.field_check(4, op, 0, np.array(A, dtype=np.uint32), np.array(B, dtype=np.uint32))
    for i in range(len(exp)):
        assert (_words(out[i][:12]), _words(out[i][12:])) == exp[i], (op, i)


@pytest.mark.parametrize("op", range(8))
def test_fr29_on_device_at_the_bounds(op):
    """fr29.hpp - the NTT butterflies' Fr form, whose Montgomery product is the generated asm of fr29_asm_gen.hpp on the
    device and plain C++ on the host twin - through ncg_field_check field 8 on the cases of the host test (operands at the
    bounds each op admits: the 64-bit columns of fr29_mont are tight only for a left operand at 6 * 2^29 with limb 8 all
    ones), the same value and output-limb assertions; 120 rows and more per launch, so a full wave and a partial one."""
    from test_host_logic import _fr29_cases
    rows_a, rows_b, check = _fr29_cases()[op]
    assert len(rows_a) >= 120
    out = get_engine().field_check(8, op, 0, np.array(rows_a, dtype=np.uint32), np.array(rows_b, dtype=np.uint32))
    for i, (a, b) in enumerate(zip(rows_a, rows_b)):
        try:
            check(a, b, [int(x) for x in out[i]])
        except AssertionError as e:
            raise AssertionError("op %d row %d: a %s b %s out %s" % (op, i, a, b, [int(x) for x in out[i]])) from e
