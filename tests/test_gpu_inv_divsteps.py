"""The division-step f_inv (fe9_inv.hpp) ON THE DEVICE: ncg_field_check op 5 for secp256k1 and ed25519 p on the edge values of
test_inv_divsteps_cpu.py, a few thousand random residues and loose limbs, against pow(x, -1, p) with 0 -> 0; and the kernel that
leans on it, the batched Jacobian -> affine step behind the secp256k1 batch multiply (k_jac_batch_affine<CurveSecpI, K, true>:
one inversion per K results), at the sizes where its groups are full, short by one, over by one and more than one block, with
results at infinity (Z = 0: skipped by the running product) first, last and alone in a group and filling a whole group."""
import random

import numpy as np
import pytest
import torch

from helpers import limbs, points_to_wire, scalars_to_wire, val
from noble_curves_amd import get_engine
from noble_curves_amd._native import SECP256K1
from oracle.curves import ED25519_P, SECP256K1_N, SECP256K1_P, Secp256k1
from test_inv_divsteps_cpu import _expect, _limbs_many, edge_values, loose_rows

pytestmark = pytest.mark.gpu
# Points per inversion of the shipped secp256k1 affine step: the last template argument of launch_mul_var_gtab<CurveSecpI, 4, 3, 16>
# in csrc/mulvar_inl.hip.  The native API does not expose it, so this constant has to follow that line by hand; with another K
# the cases below still check the results, but their zeros no longer sit on the group boundaries they are named after.
K = 16


def _words(out_row):
    return sum(int(w) << (32 * i) for i, w in enumerate(out_row))


@pytest.mark.parametrize("fid,p", [pytest.param(0, SECP256K1_P, id="secp256k1"), pytest.param(1, ED25519_P, id="ed25519")])
def test_f_inv_on_device(fid, p):
    eng = get_engine()
    rng = random.Random(0xD1F5D + fid)
    xs = edge_values(p) + [rng.randrange(p) for _ in range(4096)]
    a = np.concatenate([np.array([limbs(x) for x in xs[:-4096]], dtype=np.uint32), _limbs_many(xs[-4096:])])
    got = eng.field_check(fid, 5, 11, a, a)
    assert [_words(r) for r in got] == [_expect(x, p) for x in xs]
    for variant in (22, 77):                       # operand bound 2 and 7: limbs at the top of what the type admits
        A = variant // 10
        rows = loose_rows(p, A, rng, 256)
        a = np.array(rows, dtype=np.uint32)
        got = eng.field_check(fid, 5, variant, a, a)
        assert [_words(r) for r in got] == [_expect(val(r), p) for r in rows], variant


_REF = {}


def _reference():
    """1025 (point, scalar) pairs and their products by the oracle's C restatement, computed once"""
    if not _REF:
        from oracle import cport
        rng = random.Random(0xAFF1E)
        base = [Secp256k1.BASE.multiplyUnsafe(rng.randrange(1, SECP256K1_N)) for _ in range(8)]
        nmax = 64 * K + 1
        pw = np.ascontiguousarray(points_to_wire(SECP256K1, base)[np.arange(nmax) % 8])
        ks = [rng.randrange(1, SECP256K1_N) for _ in range(nmax)]
        out, inf = cport.multiply_unsafe("secp256k1", pw, scalars_to_wire(ks))
        assert not inf.any()
        zo, zi = cport.multiply_unsafe("secp256k1", pw[:1], scalars_to_wire([0]))   # k = 0: the all-zero row and the flag
        assert not zo.any() and zi[0] == 1
        _REF.update(pw=pw, ks=ks, out=out)
    return _REF


@pytest.mark.parametrize("n", [1, K - 1, K, K + 1, 64 * K - 1, 64 * K + 1, 1000])
def test_batch_affine_behind_secp256k1_multiply(n):
    ref = _reference()
    eng = get_engine()
    dev = torch.device("cuda", 0)
    # k = 0 -> Z = 0: first of a group (0), last of a full group (K - 1), last of all (n - 1: alone in its group when n = 1 mod K),
    # inside a group (K + 5), and the whole third group; for n = 1 the only result is at infinity and the product of its group is 1
    zero = {i for i in (0, K - 1, n - 1, K + 5) if i < n} | {i for i in range(2 * K, 3 * K) if i < n}
    ks = [0 if i in zero else ref["ks"][i] for i in range(n)]
    pts = torch.from_numpy(ref["pw"][:n].copy()).to(dev)
    sc = torch.from_numpy(scalars_to_wire(ks).copy()).to(dev)
    out = torch.full((n, 64), 0xA5, dtype=torch.uint8, device=dev)
    inf = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    eng.mul_var_batch_dev(SECP256K1, n, pts.data_ptr(), sc.data_ptr(), out.data_ptr(), inf.data_ptr())
    torch.cuda.synchronize()
    out_h, inf_h = out.cpu().numpy(), inf.cpu().numpy()
    exp = ref["out"][:n].copy()
    exp[sorted(zero)] = 0
    assert sorted(np.nonzero(inf_h)[0].tolist()) == sorted(zero) and set(inf_h.tolist()) <= {0, 1}
    bad = np.nonzero((out_h != exp).any(axis=1))[0]
    assert bad.size == 0, (n, bad[:8].tolist())
