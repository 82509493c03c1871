"""GPU parity for the NTT over the bn254 scalar field (NCG_FIELD_BN254_FR = 5) through the C ABI (`ncg_ntt`,
`ncg_ntt_dev`), the Python mirror and ncg_field_check.  The oracle is oracle.fft over Field(BN254_R) (oracle/c's fft_fr is
bls12-381 only), which reproduces the reference's bn254 roots(3) / brp(3) (test_ntt_bn254_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

from noble_curves_amd import fft as G
from noble_curves_amd import get_engine
from noble_curves_amd._native import FIELD_BLS12_381_FR, FIELD_BN254_FR, NativeError, ints_to_le, le_to_ints
from oracle import cport
from oracle.curves import Fr_bls, makeRng

from helpers import NTT_SWEEP_MAX_LOG2N, load_golden
from ntt_bn254_helpers import BN254_R, fr29_cases_bn254, input_a, le32, oracle_fft, sum_mod_r
from test_gpu_ntt import ORDERINGS, _brev_index, _Dev

pytestmark = pytest.mark.gpu
R = BN254_R
BN = dict(field=FIELD_BN254_FR)
ORACLE_MAX_LOG2N = 16           # oracle.fft (Python integers): 1.4 s at 2^16; above, identities and sampled outputs


def _oracle_np(bits, x_np):
    """one oracle transform y = D(x) of a uint8 [N, 32] array"""
    _, f = oracle_fft()
    y = f.direct(le_to_ints(x_np, 32)) if bits else le_to_ints(x_np, 32)
    return ints_to_le(y, 32)


def test_abi_takes_field_5_and_refuses_the_others():
    """ncg_ntt / ncg_ntt_dev with field 5 answer OK; every id other than 0 and 5 keeps the refusal and its message"""
    eng = get_engine()
    L, h = eng.lib, eng.h
    OK, UNSUPPORTED = 0, -4                                              # NCG_OK, NCG_ERR_UNSUPPORTED (include/ncg.h)
    assert FIELD_BN254_FR == 5

    def err():
        return (L.ncg_last_error(h) or b"").decode()
    om = np.frombuffer(int(G.rootsOfUnity(G.bn254_Fr, 7).omega(3)).to_bytes(32, "little"), dtype=np.uint8).copy()
    x = ints_to_le([1, 2, 3, 4, 5, 6, 7, R - 1], 32)
    out = np.zeros_like(x)
    assert L.ncg_ntt(h, 5, 3, 1, om.ctypes.data, x.ctypes.data, out.ctypes.data, 0) == OK, err()
    _, f = oracle_fft()
    assert le_to_ints(out, 32) == f.direct([1, 2, 3, 4, 5, 6, 7, R - 1])
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros_like(dx)
    assert L.ncg_ntt_dev(h, 5, 3, 1, om.ctypes.data, ctypes.c_void_p(dx.data_ptr()), ctypes.c_void_p(dy.data_ptr()), 0, None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(dy.cpu().numpy(), out)
    for field in (4, 6, -1, 1, 2, 3, 7):
        assert L.ncg_ntt(h, field, 3, 1, om.ctypes.data, x.ctypes.data, out.ctypes.data, 0) == UNSUPPORTED
        assert err().endswith("ntt: unsupported field %d" % field)
        assert L.ncg_ntt_dev(h, field, 3, 1, om.ctypes.data, ctypes.c_void_p(dx.data_ptr()), ctypes.c_void_p(dy.data_ptr()), 0,
                             None) == UNSUPPORTED
        assert err().endswith("ntt: unsupported field %d" % field)


def test_fft_known_answers_bn254_gpu():
    """test/fft.test.ts 'cache and fixed vectors' for bn254 through the mirror, and the assertions of
    test_fft_known_answers_gpu on this field (its expected vector from the oracle, whose tables the fixture pins)"""
    kat = load_golden("fft_kat_bn254.json")
    roots = G.rootsOfUnity(G.bn254_Fr, 7)
    assert roots.roots(3) == [int(x) for x in kat["roots3"]]
    assert roots.brp(3) == [int(x) for x in kat["brp3"]]
    fftFr = G.FFT(roots, G.bn254_Fr)
    _, of = oracle_fft()
    inp = [1, 2, 3, 4, 5, 6, 7, 8, R - 1, R - 2, 0, 12345, 1 << 253, 0x30644E72E131A029, 99, 1]
    exp = of.direct(inp)
    brp = G.bitReversalPermutation
    assert fftFr.direct(inp) == exp
    assert fftFr.direct(brp(inp), True) == exp
    assert brp(fftFr.direct(inp, False, True)) == exp
    assert brp(fftFr.direct(brp(inp), True, True)) == exp
    assert fftFr.inverse(fftFr.direct(inp)) == inp
    assert fftFr.inverse(fftFr.direct(inp, False, True), True) == inp
    assert brp(fftFr.inverse(fftFr.direct(inp), False, True)) == inp
    assert brp(fftFr.inverse(fftFr.direct(inp, False, True), True, True)) == inp
    assert fftFr.direct([5]) == [5] and fftFr.inverse([5]) == [5]
    with pytest.raises(ValueError, match="FFT: Polynomial size should be power of two"):
        fftFr.inverse([])
    with pytest.raises(ValueError, match="FFT: Polynomial size should be power of two"):
        fftFr.direct([1, 2, 3])
    with pytest.raises(ValueError, match="rootsOfUnity: wrong bits"):
        roots.roots(29)
    with pytest.raises(ValueError, match="outside of range"):
        fftFr.direct([R, 0])
    # the other generator the reference would pick for this field (findGenerator: 5)
    r5 = G.rootsOfUnity(G.bn254_Fr)
    assert r5.info["G"] == 5 and G.FFT(r5, G.bn254_Fr).direct(inp) == oracle_fft(5)[1].direct(inp)


@pytest.mark.parametrize("op", range(9))
def test_fr29_bn254_on_device_at_the_bounds(op):
    """fr29.hpp for bn254 Fr - the Montgomery product is the generated asm of fr29_asm_gen.hpp here - through
    ncg_field_check field 8 variant 1 on the rows of the host test, the same value and output-limb assertions"""
    rows_a, rows_b, check = fr29_cases_bn254()[op]
    assert len(rows_a) >= 120
    out = get_engine().field_check(8, op, 1, np.array(rows_a, dtype=np.uint32), np.array(rows_b, dtype=np.uint32))
    for i, (a, b) in enumerate(zip(rows_a, rows_b)):
        try:
            check(a, b, [int(x) for x in out[i]])
        except AssertionError as e:
            raise AssertionError("op %d row %d: a %s b %s out %s" % (op, i, a, b, [int(x) for x in out[i]])) from e


def test_field_check_fr29_unknown_variant_leaves_zero():
    rows_a, rows_b, _ = fr29_cases_bn254()[0]
    out = get_engine().field_check(8, 0, 2, np.array(rows_a[:4], dtype=np.uint32), np.array(rows_b[:4], dtype=np.uint32))
    assert not out.any()


@pytest.mark.parametrize("bits", range(NTT_SWEEP_MAX_LOG2N + 1))
def test_ntt_bn254_sweep_every_schedule(bits):
    """log2n = bits in all 8 (inverse, brpInput, brpOutput) orderings through ncg_ntt_dev (out of place, side stream, the
    input must come back unchanged) and ncg_ntt (host buffers, in place), which must agree byte for byte.  (a) uniform
    residues of THIS r with 0, 1, r - 1 and a run of r - 1 - j: against one oracle transform up to 2^16 (y = D(x); direct
    orderings map x or brp(x) to y or brp(y), inverse ones back), above it against the device's own natural-order
    transform (all orderings agree under bit reversal and round-trip) pinned by y[0] = sum x and sum y = N x[0] and by a
    sparse input checked at 1024 sampled outputs against the defining sum.  (b) all r - 1 and (c) r - 1, 0 alternating -
    the largest lazily reduced values - against their closed forms."""
    eng = get_engine()
    dev = torch.device("cuda", 0)
    run = _Dev(eng)
    n = 1 << bits
    om = G.rootsOfUnity(G.bn254_Fr, 7).omega(bits)
    rev = _brev_index(bits, dev)

    def check_all(x, y, what, host=False):
        """x, y: natural-order pair with y = D(x) (device tensors)"""
        for kw in ORDERINGS:
            src, exp = (y, x) if kw["inverse"] else (x, y)
            inp = src[rev] if kw["brp_input"] else src
            want = exp[rev] if kw["brp_output"] else exp
            got = run(bits, om, inp, **BN, **kw)
            if not torch.equal(got, want):
                bad = (got != want).any(dim=1).nonzero().flatten()
                raise AssertionError("2^%d %s %s: %d wrong elements, first at %s" % (bits, what, kw, len(bad), bad[:8].tolist()))
            if host:
                h = eng.ntt(bits, inp.cpu().numpy(), om, **BN, **kw)
                assert np.array_equal(h, got.cpu().numpy()), ("ncg_ntt != ncg_ntt_dev", bits, what, kw)

    # (a) random residues
    xa_np = input_a(bits, 0xB25EE9 + bits)
    xa = torch.from_numpy(xa_np).to(dev)
    if bits <= ORACLE_MAX_LOG2N:
        ya = torch.from_numpy(_oracle_np(bits, xa_np)).to(dev)
    else:
        ya = run(bits, om, xa, **BN)
        assert int.from_bytes(ya[0].cpu().numpy().tobytes(), "little") == sum_mod_r(xa_np)
        assert sum_mod_r(ya.cpu().numpy()) == n * int.from_bytes(xa_np[0].tobytes(), "little") % R
    check_all(xa, ya, "random", host=True)
    del xa, ya, xa_np

    # (b) all r - 1: D = N (r - 1) at 0; (c) r - 1 / 0 alternating: D = N/2 (r - 1) at 0 and N/2
    top = torch.from_numpy(le32(R - 1).copy()).to(dev)
    xb = top.repeat(n, 1)
    yb = torch.zeros_like(xb)
    yb[0] = torch.from_numpy(le32(n * (R - 1) % R).copy()).to(dev)
    check_all(xb, yb, "all r - 1")
    xc = xb.clone()
    xc[1::2] = 0
    yc = torch.zeros_like(xc)
    half = torch.from_numpy(le32(max(n // 2, 1) * (R - 1) % R).copy()).to(dev)
    yc[0] = half
    yc[n // 2] = half
    check_all(xc, yc, "r - 1, 0 alternating")
    del xb, yb, xc, yc

    if bits > ORACLE_MAX_LOG2N:   # sparse input: y[k] = sum c_t w^(j_t k), sampled at k = 0, 1, N/2, N - 1 and 1020 more
        rng = makeRng(0xB25A75E + bits)
        pos = [0, n - 1] + [rng.rndBelow(n) for _ in range(6)]
        cs = [R - 1 - rng.rndBelow(1 << 20) for _ in pos]
        xs = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        coef = {}
        for j, c in zip(pos, cs):
            coef[j] = (coef.get(j, 0) + c) % R
        for j, c in coef.items():
            xs[j] = torch.from_numpy(le32(c).copy()).to(dev)
        ks = [0, 1, n // 2, n - 1] + [rng.rndBelow(n) for _ in range(1020)]
        ninv = pow(n, -1, R)
        fwd = [sum(c * pow(om, j * k % n, R) for j, c in coef.items()) % R for k in ks]
        bwd = [sum(c * pow(om, -j * k % n, R) for j, c in coef.items()) * ninv % R for k in ks]
        kt = torch.tensor(ks, dtype=torch.int64, device=dev)
        for kw in ORDERINGS:
            got = run(bits, om, xs[rev] if kw["brp_input"] else xs, **BN, **kw)
            rows = got[rev[kt] if kw["brp_output"] else kt].cpu().numpy()
            vals = [int.from_bytes(r.tobytes(), "little") for r in rows]
            assert vals == (bwd if kw["inverse"] else fwd), ("sparse", bits, kw)


@pytest.mark.parametrize("bits", [9, 13, 19])
def test_ntt_bn254_batch_of_three_every_ordering(bits):
    """blockIdx.y carries the polynomial: batch 3 at one size per pass count (1, 2 and 3 passes) in every ordering ==
    each polynomial's own transform"""
    eng = get_engine()
    dev = torch.device("cuda", 0)
    run = _Dev(eng)
    n = 1 << bits
    om = G.rootsOfUnity(G.bn254_Fr, 7).omega(bits)
    x = torch.from_numpy(np.concatenate([input_a(bits, 0xB2BA7 + 7 * bits + i) for i in range(3)])).to(dev)
    for kw in ORDERINGS:
        out = run(bits, om, x, batch=3, **BN, **kw)
        for b in range(3):
            one = run(bits, om, x[b * n:(b + 1) * n].contiguous(), **BN, **kw)
            assert torch.equal(out[b * n:(b + 1) * n], one), (bits, b, kw)


def test_ntt_alternating_fields_on_one_fresh_context():
    """The twiddle cache is keyed by (field, log2n): bls12-381 2^12, bn254 2^12, bls12-381 2^12 with another root, bn254
    2^14 batch 2 on one fresh context, each against its oracle (cport.fft_fr resp. oracle.fft) - and then the first two
    again, which must be served from tables the other field did not disturb.  A root of the other field is refused."""
    from noble_curves_amd._native import Engine
    eng = Engine(0)
    try:
        bls_roots, bn_roots = G.rootsOfUnity(G.bls12_381_Fr, 7), G.rootsOfUnity(G.bn254_Fr, 7)
        from test_gpu_ntt import _input_a as bls_input
        xl, xn = bls_input(12, 0xA17E), input_a(12, 0xA17F)
        wl, wn = bls_roots.omega(12), bn_roots.omega(12)

        def bls(x, om, bits=12, **kw):
            assert np.array_equal(eng.ntt(bits, x, om, field=FIELD_BLS12_381_FR, **kw), cport.fft_fr(bits, x, om, **kw)), ("bls", kw)

        def bn(x, om, bits, flags):
            kw = ORDERINGS[flags]
            n = 1 << bits
            out = eng.ntt(bits, x, om, **BN, **kw)
            _, f = oracle_fft()
            for b in range(x.shape[0] // n):
                exp = (f.inverse if kw["inverse"] else f.direct)(le_to_ints(x[b * n:(b + 1) * n], 32), kw["brp_input"], kw["brp_output"])
                assert le_to_ints(out[b * n:(b + 1) * n], 32) == exp, ("bn254", bits, flags, b)

        bls(xl, wl)
        bn(xn, wn, 12, 0)
        bls(xl, pow(wl, 3, Fr_bls.ORDER), **ORDERINGS[5])
        bn(np.concatenate([input_a(14, 0xA180), input_a(14, 0xA181)]), bn_roots.omega(14), 14, 6)
        bn(xn, wn, 12, 3)                                  # still this field's table for 2^12
        bls(xl, pow(wl, 3, Fr_bls.ORDER), **ORDERINGS[2])
        bls(xl, wl, **ORDERINGS[7])
        with pytest.raises(NativeError, match="not a primitive 2\\^12-th root"):
            eng.ntt(12, xl, wn, field=FIELD_BLS12_381_FR)
        with pytest.raises(NativeError, match="not a primitive 2\\^12-th root"):
            eng.ntt(12, xn, wl % R, **BN)
        with pytest.raises(NativeError, match="not a primitive 2\\^12-th root"):
            eng.ntt(12, xn, bn_roots.omega(11), **BN)
        bn(xn, wn, 12, 5)                                  # a refused root leaves the cached tables usable
        bls(xl, wl)
    finally:
        eng.close()


def test_ntt_bn254_prover_shaped_product():
    """inverse(direct(a) .* direct(b)) of two 2^11-coefficient polynomials zero-padded to 2^12 == the schoolbook product
    mod r (the quotient-polynomial step of a Groth16 / PLONK prover)"""
    rng = makeRng(0xB254C0)
    h = 1 << 11
    a = [rng.rndBelow(R) for _ in range(h)]
    b = [rng.rndBelow(R) for _ in range(h)]
    a[0], a[1], b[0], b[h - 1] = R - 1, 0, 1, R - 1
    f = G.FFT(G.rootsOfUnity(G.bn254_Fr, 7), G.bn254_Fr)
    fa, fb = f.direct(a + [0] * h), f.direct(b + [0] * h)
    got = f.inverse([x * y % R for x, y in zip(fa, fb)])
    conv = [0] * (2 * h)
    for i, ai in enumerate(a):
        if ai:
            for j, bj in enumerate(b):
                conv[i + j] += ai * bj
    assert got == [c % R for c in conv]
    # the same through the bit-reversed middle, as a prover that skips the permutation runs it
    fa, fb = f.direct(a + [0] * h, False, True), f.direct(b + [0] * h, False, True)
    assert f.inverse([x * y % R for x, y in zip(fa, fb)], True) == got
