"""The NTT over the bn254 scalar field (NCG_FIELD_BN254_FR) without a device: the oracle against the reference's known
answers, fr29.hpp's bn254 form on the host twin at the bounds each op admits, the host twin's transform (the kernels'
pass schedule, index arithmetic and butterflies executed serially) in every ordering, and the Python mirror's checks."""
import pytest

from helpers import load_golden
from ntt_bn254_helpers import (BN254_R, FIELD_BN254_FR, fr29_cases_bn254, host_fr29_op, host_ntt, oracle_fft)
from oracle.curves import makeRng
from oracle.fft import bitReversalPermutation

R = BN254_R


def test_oracle_reproduces_the_reference_bn254_tables():
    """test/fft.test.ts 'cache and fixed vectors': rootsOfUnity(bn254.fields.Fr, 7n).roots(3) / .brp(3)"""
    kat = load_golden("fft_kat_bn254.json")
    roots, f = oracle_fft(int(kat["generator"]))
    r3, b3 = [int(x) for x in kat["roots3"]], [int(x) for x in kat["brp3"]]
    assert roots.roots(3) == r3 and roots.brp(3) == b3
    assert roots.omega(3) == r3[1] and pow(r3[1], 8, R) == 1 and pow(r3[1], 4, R) == R - 1
    assert f.direct([0, 1, 0, 0, 0, 0, 0, 0]) == r3
    assert roots.info["powerOfTwo"] == 28 and oracle_fft(None)[0].info["G"] == 5      # findGenerator
    with pytest.raises(ValueError):
        roots.roots(29)


def test_fr29_bn254_butterfly_arithmetic_at_the_bounds():
    """fr29.hpp for bn254 Fr on raw limbs against big-int arithmetic; the host twin counts every 64-bit column and 32-bit
    limb overflow (must be none).  The same rows run on the device in test_gpu_ntt_bn254.py."""
    for op, (rows_a, rows_b, check) in fr29_cases_bn254().items():
        assert len(rows_a) >= 120
        for a, b in zip(rows_a, rows_b):
            out, ovf = host_fr29_op(1, op, a, b)
            assert ovf == 0, (op, a, b)
            check(a, b, out)


def test_fr29_field_op_variant_0_is_the_bls12_381_form():
    """variant 0 of the new entry point is ht_fr29_op's field: the cases of test_host_logic give the same words"""
    import hosttest
    from test_host_logic import _fr29_cases
    for op, (rows_a, rows_b, _) in _fr29_cases().items():
        for a, b in list(zip(rows_a, rows_b))[:8]:
            assert host_fr29_op(0, op, a, b) == hosttest.fr29_op(op, a, b)


def _inputs(bits, rng):
    n = 1 << bits
    x = [rng.rndBelow(R) for _ in range(n)]
    for i, v in enumerate((0, 1, R - 1)[:n]):
        x[i] = v
    return [("random", x), ("all r - 1", [R - 1] * n), ("r - 1 / 0", [(R - 1) if i % 2 == 0 else 0 for i in range(n)])]


def _check_all_orderings(bits, x, y, passes, what):
    """x, y: natural-order pair with y = D(x) from ONE oracle transform; direct orderings map x or brp(x) to y or brp(y),
    inverse ones back"""
    roots, _ = oracle_fft()
    brp = (lambda v: bitReversalPermutation(v)) if bits else (lambda v: list(v))
    for flags in range(8):
        inv, bi, bo = bool(flags & 1), bool(flags & 2), bool(flags & 4)
        src, exp = (y, x) if inv else (x, y)
        got = host_ntt(FIELD_BN254_FR, bits, brp(src) if bi else src, roots.omega(bits), flags, passes)
        assert got == (brp(exp) if bo else exp), (what, bits, flags, passes)


@pytest.mark.parametrize("bits", range(13))
def test_host_twin_ntt_every_ordering_with_the_device_pass_limits(bits):
    """sizes 2^0 .. 2^12 (one pass up to 2^10, two above) in all 8 orderings on random residues with 0, 1, r - 1, on all
    r - 1 and on r - 1 / 0 alternating (the largest lazily reduced values) against the oracle; zero overflows"""
    _, f = oracle_fft()
    for what, x in _inputs(bits, makeRng(0xB2540 + bits)):
        y = f.direct(x)
        if bits <= 3:      # the pairing of orderings above rests on the oracle's own four forms agreeing
            assert f.inverse(y) == x and (bits == 0 or f.direct(x, False, True) == bitReversalPermutation(y))
        _check_all_orderings(bits, x, y, None, what)


@pytest.mark.parametrize("bits,passes", [(5, (2, 1)), (6, (2, 2)), (7, (3, 2)), (7, (4, 3)), (8, (2, 1)), (9, (3, 3)), (9, (4, 2))])
def test_host_twin_ntt_shrunken_passes(bits, passes):
    """the passes shrunk to t0max / tmax stages so that small sizes run three to eight passes: tiles with 4 columns, the
    bit reversal folded through the workspace, the 1/N scale and the third fold on the last pass"""
    _, f = oracle_fft()
    for what, x in _inputs(bits, makeRng(0x5B254 + 16 * bits + passes[0])):
        _check_all_orderings(bits, x, f.direct(x), passes, what)


def test_host_twin_refuses_other_fields_and_keeps_bls12_381():
    import numpy as np

    import hosttest
    from ntt_bn254_helpers import _lib
    from oracle.curves import Fr_bls
    from oracle.fft import RootsOfUnity
    out = np.zeros(8, dtype=np.uint32)
    one = np.array([1] + [0] * 7, dtype=np.uint32)
    for field in (1, 2, 3, 4, 6, -1):
        assert _lib().ht_ntt_field(field, 0, one.ctypes.data, one.ctypes.data, out.ctypes.data, 0, 0, 0) == -1
    rng = makeRng(0xB15)
    x = [rng.rndBelow(Fr_bls.ORDER) for _ in range(64)]
    om = RootsOfUnity(Fr_bls, 7).omega(6)
    for flags in range(8):
        assert host_ntt(0, 6, x, om, flags) == hosttest.ntt(6, x, om, flags)


def test_python_mirror_takes_bn254_without_a_device():
    from noble_curves_amd import _native
    from noble_curves_amd import fft as G
    kat = load_golden("fft_kat_bn254.json")
    assert _native.FIELD_BN254_FR == 5 and _native.FIELD_BLS12_381_FR == 0
    assert G.bn254_Fr.ORDER == R and G.bn254_Fr.BITS == 254 and G.bls12_381_Fr.BITS == 255
    roots = G.rootsOfUnity(G.bn254_Fr, 7)
    assert roots.omega(3) == int(kat["roots3"][1])
    assert roots.info["powerOfTwo"] == 28 and G.rootsOfUnity(G.bn254_Fr).info["G"] == 5
    assert roots.omega(28) == pow(7, (R - 1) >> 28, R)
    with pytest.raises(ValueError, match="rootsOfUnity: wrong bits 29 powerOfTwo=28"):
        roots.roots(29)
    with pytest.raises(ValueError, match="rootsOfUnity: wrong bits"):
        roots.omega(29)

    class Foreign:
        ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141

    with pytest.raises(ValueError, match="bls12-381 and bn254"):
        G.rootsOfUnity(Foreign())

    class NoEngine:
        def ntt(self, *a, **kw):
            raise AssertionError("the range check comes before the engine")

    f = G.FFT(roots, G.bn254_Fr, engine=NoEngine())
    with pytest.raises(ValueError, match="outside of range"):
        f.direct([R, 0])
    with pytest.raises(ValueError, match="outside of range"):
        f.inverse([0, G.BLS12_381_FR_ORDER - 1])
    with pytest.raises(ValueError, match="FFT: Polynomial size should be power of two"):
        f.direct([1, 2, 3])

    class Probe:
        def ntt(self, bits, data, omega, **kw):
            self.seen = (bits, omega, kw["field"])
            return data

    p = Probe()
    assert G.FFT(roots, G.bn254_Fr, engine=p).direct([R - 1, 0]) == [R - 1, 0] and p.seen == (1, R - 1, 5)
    assert G.FFT(G.rootsOfUnity(G.bls12_381_Fr, 7), engine=p).direct([1, 0]) == [1, 0] and p.seen[2] == 0
