"""GPU parity for the NTT over bls12-381 Fr through the C ABI (`ncg_ntt`, `ncg_ntt_dev`)."""
import numpy as np
import pytest
import torch

from noble_curves_amd import fft as G
from noble_curves_amd import get_engine
from noble_curves_amd._native import ints_to_le, le_to_ints
from oracle import cport
from oracle.curves import Fr_bls, makeRng
from oracle.fft import FFT, RootsOfUnity, bitReversalPermutation

from helpers import NTT_SWEEP_MAX_LOG2N, load_golden

pytestmark = pytest.mark.gpu
R = Fr_bls.ORDER



def test_fft_known_answers_gpu():
    """test/fft.test.ts:155-183, :221-251 through the mirror (same calls as the reference's test)."""
    kat = load_golden("fft_kat.json")
    roots = G.rootsOfUnity(G.bls12_381_Fr, 7)
    assert roots.roots(3) == [int(x) for x in kat["roots3"]]
    assert roots.brp(3) == [int(x) for x in kat["brp3"]]
    fftFr = G.FFT(roots, G.bls12_381_Fr)
    inp, exp = [int(x) for x in kat["basic_input"]], [int(x) for x in kat["basic_exp"]]
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
        roots.roots(33)


@pytest.mark.parametrize("bits", [1, 2, 5, 9, 10, 11, 12, 14])
def test_ntt_matches_oracle_all_orderings(bits):
    """every (inverse, brpInput, brpOutput) combination; sizes straddle the 1-pass / 2-pass boundary"""
    rng = makeRng(0x4E77 + bits)
    oroots = RootsOfUnity(Fr_bls, 7)
    of = FFT(oroots, Fr_bls)
    f = G.FFT(G.rootsOfUnity(G.bls12_381_Fr, 7))
    x = [rng.rndBelow(R) for _ in range(1 << bits)]
    x[0], x[1] = 0, R - 1
    for flags in range(8):
        inv, bi, bo = bool(flags & 1), bool(flags & 2), bool(flags & 4)
        exp = (of.inverse if inv else of.direct)(x, bi, bo)
        got = (f.inverse if inv else f.direct)(x, bi, bo)
        assert got == exp, (bits, flags)


def test_ntt_three_pass_size_matches_oracle():
    """2^19 = 10 + 5 + 4 stages: three passes, both butterfly kinds, folded bit reversal through the workspace"""
    bits = 19
    rng = makeRng(0x4E7719)
    oroots = RootsOfUnity(Fr_bls, 7)
    f = G.FFT(G.rootsOfUnity(G.bls12_381_Fr, 7))
    x = [rng.rndBelow(R) for _ in range(1 << bits)]
    # oracle via the defining sum at a few output indices (an O(N) check per index)
    w = oroots.omega(bits)
    y = f.direct(x)
    for k in (0, 1, 2, 12345, (1 << bits) - 1, 1 << 18):
        wk = pow(w, k, R)
        acc, cur = 0, 1
        for xi in x:
            acc = (acc + xi * cur) % R
            cur = cur * wk % R
        assert y[k] == acc, k
    yb = f.direct(x, False, True)
    assert yb == bitReversalPermutation(y)
    assert f.inverse(yb, True) == x
    assert f.inverse(y) == x
    assert f.direct(bitReversalPermutation(x), True) == y


def test_ntt_extreme_values_at_the_bench_size():
    """2^22 (the bench's size: three passes of 8 + 7 + 7 stages in every ordering) on the inputs that build up the
    largest lazily reduced values the fr29 butterflies can meet - every coefficient r - 1, and r - 1 / 0 alternating - whose
    transforms are known in closed form: N (r - 1) at index 0 (and N/2 (r - 1) at 0 and N/2), zero elsewhere.  Raw arrays
    in and out; natural and bit-reversed output, inverse round trip."""
    eng = get_engine()
    bits = 22
    n = 1 << bits
    roots = G.rootsOfUnity(G.bls12_381_Fr, 7)
    om = roots.omega(bits)
    top = np.frombuffer((R - 1).to_bytes(32, "little"), dtype=np.uint8)
    x = np.tile(top, (n, 1))
    for flags_out in (False, True):
        y = eng.ntt(bits, x, om, brp_output=flags_out)
        assert int.from_bytes(y[0].tobytes(), "little") == n * (R - 1) % R
        assert not y[1:].any()
    x2 = x.copy()
    x2[1::2] = 0
    y = eng.ntt(bits, x2, om)
    half = (n // 2) * (R - 1) % R
    assert int.from_bytes(y[0].tobytes(), "little") == half and int.from_bytes(y[n // 2].tobytes(), "little") == half
    y[0] = 0
    y[n // 2] = 0
    assert not y.any()
    yb = eng.ntt(bits, x2, om, brp_output=True)            # bit-reversed: index N/2 lands at 1
    assert int.from_bytes(yb[0].tobytes(), "little") == half and int.from_bytes(yb[1].tobytes(), "little") == half
    back = eng.ntt(bits, yb, om, inverse=True, brp_input=True)
    assert (back == x2).all()


def test_ntt_batch_and_raw_arrays():
    """a batch of polynomials in one call == the transforms one by one; uint8 arrays pass through"""
    eng = get_engine()
    roots = G.rootsOfUnity(G.bls12_381_Fr, 7)
    rng = makeRng(0xBA7C4)
    bits, batch = 11, 5
    polys = [[rng.rndBelow(R) for _ in range(1 << bits)] for _ in range(batch)]
    data = ints_to_le([v for p in polys for v in p], 32)
    for flags in (0, 1, 4, 7):
        out = eng.ntt(bits, data, roots.omega(bits), inverse=bool(flags & 1), brp_input=bool(flags & 2),
                      brp_output=bool(flags & 4))
        for b in range(batch):
            one = eng.ntt(bits, data[b << bits:(b + 1) << bits], roots.omega(bits), inverse=bool(flags & 1),
                          brp_input=bool(flags & 2), brp_output=bool(flags & 4))
            assert (out[b << bits:(b + 1) << bits] == one).all()
    f = G.FFT(roots)
    raw = f.direct(data[:1 << bits])
    assert isinstance(raw, np.ndarray) and le_to_ints(raw, 32) == f.direct(polys[0])


def test_ntt_rejects_bad_root_and_range():
    eng = get_engine()
    from noble_curves_amd._native import NativeError
    data = ints_to_le([1, 2, 3, 4], 32)
    with pytest.raises(NativeError, match="primitive 2\\^2-th root"):
        eng.ntt(2, data, 5)
    f = G.FFT(G.rootsOfUnity(G.bls12_381_Fr, 7))
    with pytest.raises(ValueError, match="outside of range"):
        f.direct([R, 0])


def test_fft_algebra_properties_gpu():
    """test/fft.test.ts:544-640 'random and algebra properties' through the device transform: round trips,
    additivity, scalar multiples, constant / zero polynomials, the convolution theorem, eval(a*b) = eval(a) eval(b)."""
    rng = makeRng(0xA16EB7A)
    f = G.FFT(G.rootsOfUnity(G.bls12_381_Fr, 7))
    for n in (8, 256, 2048):
        a = [rng.rndBelow(R) for _ in range(n)]
        b = [rng.rndBelow(R) for _ in range(n)]
        c = rng.rndBelow(R - 1) + 1
        assert f.inverse(f.direct(a)) == a and f.direct(f.inverse(a)) == a
        fa, fb = f.direct(a), f.direct(b)
        assert f.direct([(x + y) % R for x, y in zip(a, b)]) == [(x + y) % R for x, y in zip(fa, fb)]
        assert f.direct([x * c % R for x in a]) == [x * c % R for x in fa]
        out = f.direct([c] * n)
        assert out[0] == c * n % R and not any(out[1:])
        assert not any(f.direct([0] * n))
        # convolution theorem on zero-padded halves: direct(a) .* direct(b) = direct(a (*) b)
        h = n // 2
        a0, b0 = a[:h] + [0] * h, b[:h] + [0] * h
        conv = [0] * n
        if n <= 256:
            for i in range(h):
                for j in range(h):
                    conv[i + j] = (conv[i + j] + a0[i] * b0[j]) % R
            assert f.inverse([x * y % R for x, y in zip(f.direct(a0), f.direct(b0))]) == conv
        # eval(a*b)(x) = eval(a)(x) eval(b)(x) through the transform-domain product
        prod = f.inverse([x * y % R for x, y in zip(f.direct(a0), f.direct(b0))])
        x = rng.rndBelow(R)

        def ev(p):
            acc = 0
            for coef in reversed(p):
                acc = (acc * x + coef) % R
            return acc
        assert ev(prod) == ev(a0) * ev(b0) % R


def test_fft_is_evaluation_at_roots_gpu():
    """test/fft.test.ts:642-648 'direct == eval at roots' (and the bit-reversed form)"""
    rng = makeRng(0xD0F7)
    roots = G.rootsOfUnity(G.bls12_381_Fr, 7)
    f = G.FFT(roots)
    for bits in (3, 6):
        n = 1 << bits
        a = [rng.rndBelow(R) for _ in range(n)]
        om = roots.roots(bits)

        def ev(p, x):
            acc = 0
            for coef in reversed(p):
                acc = (acc * x + coef) % R
            return acc
        exp = [ev(a, w) for w in om]
        assert f.direct(a) == exp
        assert f.direct(a, False, True) == G.bitReversalPermutation(exp)
        assert roots.inverse(bits)[1:] == om[1:][::-1] and roots.inverse(bits)[0] == 1


# ---- every pass shape of the schedule on the device.  ntt_schedule (ntt.hip) turns (log2n, flags) into passes that differ in
# what k_ntt_pass branches on (stages per tile, tile columns, DIT / DIF, inverse, bit-reversed store, 1/N scale, canonical
# store, src / ws / dst hand-over); every shape the planner can produce occurs at 2^NTT_SWEEP_MAX_LOG2N or below
# (test_host_logic.py checks that), so the sweep runs every size up to it in all 8 orderings, out of place on a side stream.
ORDERINGS = [dict(inverse=bool(f & 1), brp_input=bool(f & 2), brp_output=bool(f & 4)) for f in range(8)]
ORACLE_MAX_LOG2N = 22           # oracle/c transforms up to here (about 5 s at 2^22); above, identities and sampled outputs


def _le(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def _below_r(c):
    """rows of uint8 [k, 32] (little-endian) that are below r"""
    w = c.view("<u8").reshape(-1, 4)
    lt, eq = np.zeros(len(w), dtype=bool), np.ones(len(w), dtype=bool)
    for i in (3, 2, 1, 0):
        ri = np.uint64((R >> (64 * i)) & ((1 << 64) - 1))
        lt |= eq & (w[:, i] < ri)
        eq &= w[:, i] == ri
    return lt


def _input_a(bits, seed):
    """uniform canonical residues with 0, 1, r - 1 at the front and then r - 1 - j, j < 64"""
    n = 1 << bits
    gen = np.random.default_rng(seed)
    out, filled = np.empty((n, 32), dtype=np.uint8), 0
    while filled < n:
        c = gen.integers(0, 256, size=(n - filled + (n - filled) // 4 + 16, 32), dtype=np.uint8)
        c[:, 31] &= 0x7F
        c = c[_below_r(c)][:n - filled]
        out[filled:filled + len(c)] = c
        filled += len(c)
    for i, v in enumerate([0, 1, R - 1] + [R - 1 - j for j in range(64)][:n]):
        if i < n:
            out[i] = _le(v)
    return out


def _brev_index(bits, dev):
    i = torch.arange(1 << bits, device=dev, dtype=torch.int64)
    rev = torch.zeros_like(i)
    for b in range(bits):
        rev |= ((i >> b) & 1) << (bits - 1 - b)
    return rev


def _sum_mod_r(t):
    """sum of the residues of a uint8 [n, 32] tensor mod r (64-bit column sums of the 32-bit words)"""
    w = t.cpu().numpy().view("<u4").reshape(-1, 8)
    cols = w.sum(axis=0, dtype=np.uint64)
    return sum(int(c) << (32 * j) for j, c in enumerate(cols)) % R


class _Dev:
    """ncg_ntt_dev out of place on a non-default stream; the input must come back unchanged"""

    def __init__(self, eng):
        self.eng, self.dev = eng, torch.device("cuda", 0)
        self.stream = torch.cuda.Stream(device=self.dev)

    def __call__(self, bits, om, x, batch=1, **kw):
        y = torch.full_like(x, 0xFF)                # not a residue: an element the transform does not write shows
        keep = x.clone()
        torch.cuda.synchronize()
        self.eng.ntt_dev(bits, batch, om, x.data_ptr(), y.data_ptr(), self.stream.cuda_stream, **kw)
        self.stream.synchronize()
        assert torch.equal(x, keep), ("ncg_ntt_dev wrote its input", bits, kw)
        return y


@pytest.mark.parametrize("bits", range(NTT_SWEEP_MAX_LOG2N + 1))
def test_ntt_sweep_every_schedule(bits):
    """log2n = bits in all 8 (inverse, brpInput, brpOutput) orderings through ncg_ntt_dev (out of place, side stream) and
    ncg_ntt (host buffers, in place), which must agree byte for byte.  (a) uniform residues with 0, 1, r - 1 and a run of
    r - 1 - j: against oracle/c's FFT up to 2^22 (one oracle call: y = D(x); direct orderings map x or brp(x) to y or
    brp(y), inverse ones y or brp(y) back to x or brp(x)), above it against the device's own natural-order transform
    (all orderings agree under bit reversal and round-trip) pinned by y[0] = sum x and sum y = N x[0] and by a sparse
    input whose transform is checked at 1024 sampled outputs.  (b) all r - 1 and (c) r - 1, 0 alternating - the largest
    lazily reduced values - against their closed forms."""
    eng = get_engine()
    dev = torch.device("cuda", 0)
    run = _Dev(eng)
    n = 1 << bits
    om = G.rootsOfUnity(G.bls12_381_Fr, 7).omega(bits)
    rev = _brev_index(bits, dev)

    def check_all(x, y, what, host=False):
        """x, y: natural-order pair with y = D(x) (device tensors)"""
        for kw in ORDERINGS:
            src, exp = (y, x) if kw["inverse"] else (x, y)
            inp = src[rev] if kw["brp_input"] else src
            want = exp[rev] if kw["brp_output"] else exp
            got = run(bits, om, inp, **kw)
            if not torch.equal(got, want):
                bad = (got != want).any(dim=1).nonzero().flatten()
                raise AssertionError("2^%d %s %s: %d wrong elements, first at %s" % (bits, what, kw, len(bad), bad[:8].tolist()))
            if host:
                h = eng.ntt(bits, inp.cpu().numpy(), om, **kw)
                assert np.array_equal(h, got.cpu().numpy()), ("ncg_ntt != ncg_ntt_dev", bits, what, kw)

    # (a) random residues
    xa_np = _input_a(bits, 0x5EE9 + bits)
    xa = torch.from_numpy(xa_np).to(dev)
    if bits <= ORACLE_MAX_LOG2N:
        ya = torch.from_numpy(cport.fft_fr(bits, xa_np, om)).to(dev)
    else:
        ya = run(bits, om, xa)
        assert int.from_bytes(ya[0].cpu().numpy().tobytes(), "little") == _sum_mod_r(xa)
        assert _sum_mod_r(ya) == n * int.from_bytes(xa_np[0].tobytes(), "little") % R
    check_all(xa, ya, "random", host=True)
    del xa, ya, xa_np

    # (b) all r - 1: D = N (r - 1) at 0; (c) r - 1 / 0 alternating: D = N/2 (r - 1) at 0 and N/2
    top = torch.from_numpy(_le(R - 1).copy()).to(dev)
    xb = top.repeat(n, 1)
    yb = torch.zeros_like(xb)
    yb[0] = torch.from_numpy(_le(n * (R - 1) % R).copy()).to(dev)
    check_all(xb, yb, "all r - 1")
    xc = xb.clone()
    xc[1::2] = 0
    yc = torch.zeros_like(xc)
    half = torch.from_numpy(_le(max(n // 2, 1) * (R - 1) % R).copy()).to(dev)
    yc[0] = half
    yc[n // 2] = half
    check_all(xc, yc, "r - 1, 0 alternating")
    del xb, yb, xc, yc

    if bits > ORACLE_MAX_LOG2N:   # sparse input: y[k] = sum c_t w^(j_t k), sampled at k = 0, 1, N/2, N - 1 and 1020 more
        rng = makeRng(0x5A75E + bits)
        pos = [0, n - 1] + [rng.rndBelow(n) for _ in range(6)]
        cs = [R - 1 - rng.rndBelow(1 << 20) for _ in pos]
        xs = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        coef = {}
        for j, c in zip(pos, cs):
            coef[j] = (coef.get(j, 0) + c) % R
        for j, c in coef.items():
            xs[j] = torch.from_numpy(_le(c).copy()).to(dev)
        ks = [0, 1, n // 2, n - 1] + [rng.rndBelow(n) for _ in range(1020)]
        ninv = pow(n, -1, R)
        fwd = [sum(c * pow(om, j * k % n, R) for j, c in coef.items()) % R for k in ks]
        bwd = [sum(c * pow(om, -j * k % n, R) for j, c in coef.items()) * ninv % R for k in ks]
        kt = torch.tensor(ks, dtype=torch.int64, device=dev)
        for kw in ORDERINGS:
            got = run(bits, om, xs[rev] if kw["brp_input"] else xs, **kw)
            rows = got[rev[kt] if kw["brp_output"] else kt].cpu().numpy()
            vals = [int.from_bytes(r.tobytes(), "little") for r in rows]
            assert vals == (bwd if kw["inverse"] else fwd), ("sparse", bits, kw)


@pytest.mark.parametrize("bits", [9, 13, 19])
def test_ntt_batch_of_three_every_ordering(bits):
    """blockIdx.y carries the polynomial: batch 3 at one size per pass count (1, 2 and 3 passes) in every ordering ==
    each polynomial's own transform"""
    eng = get_engine()
    dev = torch.device("cuda", 0)
    run = _Dev(eng)
    n = 1 << bits
    om = G.rootsOfUnity(G.bls12_381_Fr, 7).omega(bits)
    x = torch.from_numpy(np.concatenate([_input_a(bits, 0xBA7 + 7 * bits + i) for i in range(3)])).to(dev)
    for kw in ORDERINGS:
        out = run(bits, om, x, batch=3, **kw)
        for b in range(3):
            one = run(bits, om, x[b * n:(b + 1) * n].contiguous(), **kw)
            assert torch.equal(out[b * n:(b + 1) * n], one), (bits, b, kw)


def test_ntt_workspace_regrow_and_twiddle_cache_on_one_context():
    """On a fresh context: a small folded multi-pass transform, then a larger batch that regrows the workspace
    (ncg_ntt_dev), then a smaller one that reuses it; and, at one size, the twiddle table alternating between three
    primitive roots of the same order (w, w^(N-1), w^3) - the table is cached per size and rebuilt when the root
    changes.  Every result against oracle/c with the root in use."""
    from noble_curves_amd._native import Engine
    eng = Engine(0)
    try:
        dev = torch.device("cuda", 0)
        run = _Dev(eng)
        roots = G.rootsOfUnity(G.bls12_381_Fr, 7)
        for bits, batch, flags in ((11, 1, 0), (13, 3, 0), (14, 2, 6), (12, 2, 7)):
            om = roots.omega(bits)
            kw = ORDERINGS[flags]
            xs = [_input_a(bits, 0x3E6 + 31 * bits + i) for i in range(batch)]
            out = run(bits, om, torch.from_numpy(np.concatenate(xs)).to(dev), batch=batch, **kw).cpu().numpy()
            for b, x in enumerate(xs):
                assert np.array_equal(out[b << bits:(b + 1) << bits], cport.fft_fr(bits, x, om, **kw)), (bits, batch, flags, b)
        bits = 12
        n = 1 << bits
        w = roots.omega(bits)
        x = _input_a(bits, 0x7C4C)
        for i, om in enumerate((w, pow(w, n - 1, R), w, pow(w, 3, R), pow(w, n - 1, R), pow(w, 3, R), w)):
            kw = ORDERINGS[(0, 1, 4, 3, 6, 5, 7)[i]]
            assert np.array_equal(eng.ntt(bits, x, om, **kw), cport.fft_fr(bits, x, om, **kw)), (i, om == w, kw)
    finally:
        eng.close()
