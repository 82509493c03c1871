"""GPU checks of the pair-sum path of the secp256k1 batch multiply (csrc/mulvar_pairsum.hpp: prepare, batched inverse, ladder,
affine step) through mul_var_batch_dev, at item counts around the threshold T from which the device takes it (exported by the
host twin): every row of every count bit-exact against the oracle's C restatement.

T is the crossover with the single-kernel path, 2^19 items, and the oracle takes a third of a millisecond per product: the batch
is therefore TILE distinct pairs repeated - the oracle multiplies each distinct pair once, and row i is compared with the
oracle's product of the pair in row i.  TILE is odd, so that a pair meets every position of the groups of 16 and of the waves."""
import numpy as np
import pytest
import torch

import ladder_exceptions as LE
import ladder_pairsum as PS
from helpers import SECP_LAMBDA as LAM
from noble_curves_amd import get_engine
from noble_curves_amd._native import SECP256K1
from oracle.curves import SECP256K1_N as N, SECP256K1_P as P, Secp256k1

pytestmark = pytest.mark.gpu

TILE = 2049
_REF = {}


def _small_x_point():
    """the point of the curve with the smallest x"""
    x = 1
    while True:
        v = (x ** 3 + 7) % P
        y = pow(v, (P + 1) // 4, P)
        if y * y % P == v:
            return Secp256k1.fromAffine((x, y))
        x += 1


def _tiled(a, n):
    return np.tile(a, (n // a.shape[0] + 1,) + (1,) * (a.ndim - 1))[:n]


def _reference():
    """T + 65 rows of TILE random pairs repeated, and their products, computed once; `planted` is the first T + 64 of them with
    P = O, k = 0, k = +-lambda and the small-x point put into ONE group of 16 of the last full wave (rows T + 2 .. T + 10 step 2:
    ordinary rows between them), with their own products."""
    if not _REF:
        T = PS.min_n()
        assert T % 64 == 0
        rng = LE.rng(0x14B0)
        pairs = LE.random_pairs(rng, TILE, nbase=16)
        pw, sw = LE.wires(pairs)
        out, inf = LE.expected(pairs)
        assert not inf.any()
        n = T + 65
        wire, out, inf = (_tiled(pw, n), _tiled(sw, n)), _tiled(out, n), _tiled(inf, n)
        q = pairs[T % TILE][1]
        rows = {T + 2: (12345, Secp256k1.ZERO), T + 4: (0, q), T + 6: (LAM, q), T + 8: (N - LAM, q),
                T + 10: (pairs[(T + 10) % TILE][0], _small_x_point())}
        assert len({r // 16 for r in rows}) == 1 and len({r // 64 for r in rows}) == 1
        order = sorted(rows)
        rw = LE.wires([rows[r] for r in order])
        rout, rinf = LE.expected([rows[r] for r in order])
        assert rinf.tolist() == [1, 1, 0, 0, 0]
        pwire = (wire[0][:T + 64].copy(), wire[1][:T + 64].copy())
        pout, pinf = out[:T + 64].copy(), inf[:T + 64].copy()
        pwire[0][order], pwire[1][order], pout[order], pinf[order] = rw[0], rw[1], rout, rinf
        _REF.update(T=T, wire=wire, out=out, inf=inf, rows=order, pwire=pwire, pout=pout, pinf=pinf)
    return _REF


def _run(wire, n):
    dev = torch.device("cuda", 0)
    pts = torch.from_numpy(np.ascontiguousarray(wire[0][:n])).to(dev)
    sc = torch.from_numpy(np.ascontiguousarray(wire[1][:n])).to(dev)
    out = torch.full((n, 64), 0xA5, dtype=torch.uint8, device=dev)
    inf = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    get_engine().mul_var_batch_dev(SECP256K1, n, pts.data_ptr(), sc.data_ptr(), out.data_ptr(), inf.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), inf.cpu().numpy()


@pytest.mark.parametrize("extra", [0, 1, 15, 17, 63, 65, -1])
def test_counts_around_the_threshold(extra):
    """n = T + extra: a partial last group of 16 (1, 15, 17), a partial last wave (1 .. 63), both (17, 65); T - 1 is the
    single-kernel path - the same bytes either side of the switch"""
    ref = _reference()
    n = ref["T"] + extra
    out, inf = _run(ref["wire"], n)
    assert np.array_equal(inf, ref["inf"][:n])
    bad = np.nonzero((out != ref["out"][:n]).any(axis=1))[0]
    assert bad.size == 0, (n, bad[:8].tolist())


def test_planted_rows_do_not_poison_their_group():
    """P = O, k = 0, k = +-lambda and the small-x point inside one group of 16 of the batched inverse and one wave: every row is
    the oracle's, and outside the planted rows the output is that of the batch without them."""
    ref = _reference()
    n = ref["T"] + 64
    out, inf = _run(ref["pwire"], n)
    assert np.array_equal(inf, ref["pinf"]) and np.array_equal(out, ref["pout"])
    keep = np.ones(n, dtype=bool)
    keep[ref["rows"]] = False
    assert np.array_equal(out[keep], ref["out"][:n][keep]) and not inf[keep].any()
