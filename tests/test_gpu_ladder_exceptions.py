"""GPU checks of the exception-free additions in k_mul_var_gtab<CurveSecpI, 4, 3, true>, through mul_var_batch_dev (the engine's
scratch, so the inlined kernel runs): lanes that meet an exceptional addition are flagged and redone by the complete ladder,
lanes whose result is known beforehand are not, and a flagged lane changes nothing in its neighbours."""
import numpy as np
import pytest
import torch

import ladder_exceptions as LE
from noble_curves_amd import get_engine
from noble_curves_amd._native import SECP256K1
from oracle.curves import Secp256k1

pytestmark = pytest.mark.gpu

_REF = {}


def _reference():
    """192 pairs, three waves: wave 0 the special pairs (flagged scalars, edge list, P = O) at its first lanes and random pairs
    behind them, wave 1 random pairs only, wave 2 P = O or k = 0 in every lane; `plain` has random pairs at the special lanes of
    wave 0.  Products by the oracle, computed once."""
    if not _REF:
        rng = LE.rng(0x10E6)
        special = LE.special_pairs(rng)
        assert len(special) < 60
        rnd = LE.random_pairs(rng, 128 + len(special))
        w2 = [(0, p) if i % 2 else (k, Secp256k1.ZERO) for i, (k, p) in enumerate(LE.random_pairs(rng, 64))]
        mixed = special + rnd[len(special):128] + w2
        plain = rnd[128:] + rnd[len(special):128] + w2
        assert len(mixed) == len(plain) == 192
        out, inf = LE.expected(mixed)
        assert inf[:len(special)].any() and not inf[len(special):128].any() and inf[128:].all()
        _REF.update(ns=len(special), mixed=LE.wires(mixed), plain=LE.wires(plain), out=out, inf=inf)
    return _REF


def _run(wire, n):
    dev = torch.device("cuda", 0)
    pts = torch.from_numpy(wire[0][:n].copy()).to(dev)
    sc = torch.from_numpy(wire[1][:n].copy()).to(dev)
    out = torch.full((n, 64), 0xA5, dtype=torch.uint8, device=dev)
    inf = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    get_engine().mul_var_batch_dev(SECP256K1, n, pts.data_ptr(), sc.data_ptr(), out.data_ptr(), inf.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), inf.cpu().numpy()


@pytest.mark.parametrize("n", [1, 65, 192])
def test_flagged_lanes_against_oracle(n):
    """n = 1: a flagged lane alone (k = lambda on G); 65: the special wave and one lane of the next; 192: all three waves"""
    ref = _reference()
    out, inf = _run(ref["mixed"], n)
    assert np.array_equal(inf, ref["inf"][:n])
    bad = np.nonzero((out != ref["out"][:n]).any(axis=1))[0]
    assert bad.size == 0, (n, bad[:8].tolist())


def test_flag_stays_in_its_lane():
    """The same 192 inputs with random pairs in place of the special ones: every other lane's output is identical."""
    ref = _reference()
    ns = ref["ns"]
    out_m, inf_m = _run(ref["mixed"], 192)
    out_p, inf_p = _run(ref["plain"], 192)
    assert np.array_equal(out_m[ns:], out_p[ns:]) and np.array_equal(inf_m[ns:], inf_p[ns:])
    assert not inf_p[:ns].any() and (out_m[:ns] != out_p[:ns]).any(axis=1).all()
