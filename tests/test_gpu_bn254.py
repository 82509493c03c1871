"""bn254 G1 (src/bn254.ts, alt_bn128 / EIP-196) on the device: the Montgomery field form (ncg_field_check field 9), the batch
variable-base multiply, the pairwise add, normalize_batch and every MSM entry point against the bn254 oracle and the
reference's EIP-196 vectors (tests/golden/bn254_g1_eip196.json); the entry points without a bn254 form return UNSUPPORTED."""
import ctypes

import numpy as np
import pytest
import torch

from bn254_helpers import (BN254_G1, BN254_P, BN254_R, Bn254, OPS, VARIANTS, fe9m_cases, from_wire, rand_point,
                           scalars_wire, to_wire)
from helpers import load_golden
from noble_curves_amd import NativeError, get_engine
from oracle.curves import makeRng

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4


def _pt(xy):
    xy = tuple(int(t, 16) if isinstance(t, str) else t for t in xy)
    return Bn254.ZERO if xy == (0, 0) else Bn254.fromAffine(xy)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _aff(p):
    return p.toAffine()


@pytest.mark.parametrize("op", OPS)
def test_field_on_device_at_the_bounds(op):
    """fe9m.hpp through ncg_field_check field 9 (the generated asm columns on the device) on the host twin's cases"""
    eng = get_engine()
    cases = fe9m_cases()
    for variant in VARIANTS:
        rows_a, rows_b, check = cases[(op, variant)]
        out = eng.field_check(9, op, variant, np.array(rows_a, dtype=np.uint32), np.array(rows_b, dtype=np.uint32))
        for i, (a, b) in enumerate(zip(rows_a, rows_b)):
            try:
                check(a, b, [int(x) for x in out[i]])
            except AssertionError as e:
                raise AssertionError("op %d variant %d row %d: out %s" % (op, variant, i, list(out[i]))) from e


def test_mul_var_eip196_vectors_and_edges():
    g = load_golden("bn254_g1_eip196.json")
    pts = [_pt(v["p"]) for v in g["mul"]]
    ks = [int(v["k"], 16) % BN254_R for v in g["mul"]]
    exp = [tuple(int(t, 16) for t in v["out"]) for v in g["mul"]]
    rng = makeRng(0x254C)
    for k in (0, 1, 2, BN254_R - 1, BN254_R - 2, 15, 16, 17) + tuple(rng.rndBelow(BN254_R) for _ in range(60)):
        p = rand_point(rng)
        pts.append(p)
        ks.append(k)
        exp.append(_aff(p.multiplyUnsafe(k)))
    pts.append(Bn254.ZERO)
    ks.append(12345)
    exp.append((0, 0))
    out, inf = get_engine().mul_var_batch(BN254_G1, to_wire(pts), scalars_wire(ks))
    for i, e in enumerate(exp):
        assert from_wire(out[i]) == e, (i, hex(ks[i]))
        assert bool(inf[i]) == (e == (0, 0))
    # the oracle agrees with the vectors (the golden file is the reference's)
    for i in range(len(g["mul"])):
        assert _aff(pts[i].multiplyUnsafe(ks[i])) == exp[i]


def test_add_pairs_eip196_vectors_and_edges():
    g = load_golden("bn254_g1_eip196.json")
    A = [_pt(v["a"]) for v in g["add"]]
    B = [_pt(v["b"]) for v in g["add"]]
    rng = makeRng(0x254D)
    for _ in range(20):
        p, q = rand_point(rng), rand_point(rng)
        A += [p, p, Bn254.ZERO, p, p]
        B += [q, p, q, p.negate(), Bn254.ZERO]
    eng = get_engine()
    for sub in (False, True):
        out, inf = eng.add_pairs_batch(BN254_G1, to_wire(A), to_wire(B), subtract=sub)
        for i, (p, q) in enumerate(zip(A, B)):
            e = _aff(p.subtract(q) if sub else p.add(q))
            assert from_wire(out[i]) == e, (sub, i)
            assert bool(inf[i]) == (e == (0, 0))
    for i, v in enumerate(g["add"]):
        assert _aff(A[i].add(B[i])) == tuple(int(t, 16) for t in v["out"])


def test_normalize_batch():
    rng = makeRng(0x254E)
    rows, exp = [], []
    for i in range(70):
        p = rand_point(rng)
        x, y = p.toAffine()
        z = rng.rndBelow(BN254_P - 1) + 1
        if i == 3:
            x, y, z = 0, 1, 0                    # ZERO
        rows.append(b"".join(v.to_bytes(32, "little") for v in (x * z % BN254_P, y * z % BN254_P, z)))
        exp.append((x, y) if z else (0, 0))
    out, inf = get_engine().normalize_batch(BN254_G1, np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(70, 96))
    for i, e in enumerate(exp):
        assert from_wire(out[i]) == e and bool(inf[i]) == (e == (0, 0)), i


def _oracle_msm(pts, ks):
    acc = Bn254.ZERO
    for p, k in zip(pts, ks):
        acc = acc.add(p.multiplyUnsafe(k))
    return _aff(acc)


def _gpu_points(eng, a):
    """a_i G on the device (the batch multiply, checked against the oracle above)"""
    n = len(a)
    out, inf = eng.mul_var_batch(BN254_G1, np.tile(to_wire([Bn254.BASE]), (n, 1)), scalars_wire(a))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 100])
def test_msm_small_against_oracle(n):
    rng = makeRng(0x2540 + n)
    pts = [rand_point(rng) for _ in range(n)]
    ks = [rng.rndBelow(BN254_R) for _ in range(n)]
    if n >= 3:
        pts[1], ks[2] = Bn254.ZERO, 0
    out, inf = get_engine().msm(BN254_G1, to_wire(pts), scalars_wire(ks))
    e = _oracle_msm(pts, ks)
    assert from_wire(out) == e and inf == (e == (0, 0))


def test_msm_fuzz_families():
    """ZERO points, P / -P pairs, repeated points, zero scalars, r - 1"""
    rng = makeRng(0x254F)
    P = [rand_point(rng) for _ in range(6)]
    pts = [Bn254.ZERO, P[0], P[0].negate(), P[1], P[1], P[1], P[2], P[3], P[4], P[5]] * 5
    ks = [rng.rndBelow(BN254_R) for _ in pts]
    ks[1] = ks[2] = 777                                   # P + (-P) with equal scalars
    ks[6], ks[7] = 0, BN254_R - 1
    eng = get_engine()
    for pk, kk in ((pts, ks), (pts, [BN254_R - 1] * len(pts)), (pts, [0] * len(pts)), ([P[0], P[0].negate()], [5, 5])):
        out, inf = eng.msm(BN254_G1, to_wire(pk), scalars_wire(kk))
        e = _oracle_msm(pk, kk)
        assert from_wire(out) == e and inf == (e == (0, 0))


def test_msm_out_of_range_scalar_is_reported_with_its_index():
    rng = makeRng(0x2541)
    pts = [rand_point(rng) for _ in range(50)]
    ks = [rng.rndBelow(BN254_R) for _ in range(50)]
    ks[37] = BN254_R
    with pytest.raises(NativeError, match="index 37"):
        get_engine().msm(BN254_G1, to_wire(pts), scalars_wire(ks))


def _every_entry_point(eng, pw, sw, exp, tag):
    n = pw.shape[0]
    got, _ = eng.msm(BN254_G1, pw, sw)
    assert from_wire(got) == exp, (tag, "ncg_msm")
    dp, ds = _dev(pw), _dev(sw)
    got, _ = eng.msm_dev(BN254_G1, n, dp.data_ptr(), ds.data_ptr())
    assert from_wire(got) == exp, (tag, "ncg_msm_dev")
    for parts in (2, 5):
        got, _ = eng.msm_split_windows_dev(BN254_G1, n, parts, dp.data_ptr(), ds.data_ptr())
        assert from_wire(got) == exp, (tag, "windows", parts)
        got, _ = eng.msm_split_dev(BN254_G1, n, parts, dp.data_ptr(), ds.data_ptr())
        assert from_wire(got) == exp, (tag, "points", parts)
    for lane in (0, 1):
        eng.msm_async_submit(lane, BN254_G1, n, dp.data_ptr(), ds.data_ptr())
    for lane in (0, 1):
        got, _ = eng.msm_async_collect(lane, BN254_G1)
        assert from_wire(got) == exp, (tag, "async", lane)
    half = n // 2
    slots = [eng.msm_shard_local_dev(BN254_G1, half, dp.data_ptr(), ds.data_ptr(), n_max=n - half),
             eng.msm_shard_local_dev(BN254_G1, n - half, dp.data_ptr() + half * 64, ds.data_ptr() + half * 32, n_max=n - half)]
    got, _ = eng.msm_shard_combine(BN254_G1, n - half, np.stack(slots))
    assert from_wire(got) == exp, (tag, "shard combine")
    rs = eng.upload_points(BN254_G1, pw)
    for stage in ("generic", "precomputed"):
        if stage == "precomputed":
            assert rs.precompute() == (n >= 4096)
        got, _ = rs.msm(sw)
        assert from_wire(got) == exp, (tag, stage, "resident")
        got, _ = rs.msm_dev(ds.data_ptr())
        assert from_wire(got) == exp, (tag, stage, "resident_dev")
        got, _ = eng.msm_split_windows_dev(BN254_G1, n, 4, 0, ds.data_ptr(), resident=rs)
        assert from_wire(got) == exp, (tag, stage, "resident windows")
        eng.msm_async_submit(2, BN254_G1, n, 0, ds.data_ptr(), resident=rs)
        got, _ = eng.msm_async_collect(2, BN254_G1)
        assert from_wire(got) == exp, (tag, stage, "resident async")
    out, inf = rs.mul_var_batch(sw)                                            # ncg_mul_var_batch_resident
    for i in range(3):
        k = int.from_bytes(bytes(sw[i]), "little")
        assert from_wire(out[i]) == _aff(_pt(from_wire(pw[i])).multiplyUnsafe(k)), (tag, "resident mul_var", i)
    rs.free()


@pytest.mark.parametrize("lg", [12, 16])
def test_msm_every_entry_point(lg):
    """points a_i G from the device batch multiply: sum k_i a_i G = (sum k_i a_i mod r) G, one oracle multiply"""
    n = 1 << lg
    rng = makeRng(0x2542 + lg)
    eng = get_engine()
    a = [rng.rndBelow(BN254_R) for _ in range(n)]
    k = [rng.rndBelow(BN254_R) for _ in range(n)]
    a[0], k[1], a[2], a[3], k[2] = 0, 0, 5, BN254_R - 5, k[3]      # ZERO, a zero scalar, a P / -P pair with equal scalars
    pw = _gpu_points(eng, a)
    exp = _aff(Bn254.BASE.multiplyUnsafe(sum(x * y for x, y in zip(a, k)) % BN254_R))
    _every_entry_point(eng, pw, scalars_wire(k), exp, lg)


def test_msm_32768_identical_points():
    n = 32768
    P = Bn254.BASE.multiplyUnsafe(1 << 235)
    s = 1 << 241
    pw = np.tile(to_wire([P]), (n, 1))
    sw = np.tile(scalars_wire([s]), (n, 1))
    exp = _aff(P.multiplyUnsafe(n * s % BN254_R))
    _every_entry_point(get_engine(), pw, sw, exp, "identical")


def test_msm_2_20_and_its_halves():
    n = 1 << 20
    rng = np.random.default_rng(0x2543)
    eng = get_engine()
    a_small = [int(x) for x in rng.integers(1, 1 << 62, size=1024)]
    pts1024 = _gpu_points(eng, a_small)
    idx = rng.integers(0, 1024, size=n)
    pw = np.ascontiguousarray(pts1024[idx])
    kw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    kw[:, 31] &= 0x0F                                             # below 2^252 < r
    ks = [int.from_bytes(kw[i].tobytes(), "little") for i in range(0, n)]
    total = sum(a_small[idx[i]] * ks[i] for i in range(n)) % BN254_R
    exp = _aff(Bn254.BASE.multiplyUnsafe(total))
    got, _ = eng.msm(BN254_G1, pw, kw)
    assert from_wire(got) == exp
    h = n // 2
    g1, _ = eng.msm(BN254_G1, pw[:h], kw[:h])
    g2, _ = eng.msm(BN254_G1, pw[h:], kw[h:])
    parts = [_pt(from_wire(g1)), _pt(from_wire(g2))]
    assert _aff(parts[0].add(parts[1])) == from_wire(got)


def test_unsupported_entry_points():
    eng = get_engine()
    L, h = eng.lib, eng.h
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data
    err = lambda: (L.ncg_last_error(h) or b"").decode()
    assert L.ncg_decode_points_batch(h, 5, 1, p, 0, p, p, p) == UNSUPPORTED and "unsupported curve 5" in err()
    assert L.ncg_encode_points_batch(h, 5, 1, p, p, p) == UNSUPPORTED and "unsupported curve 5" in err()
    hnd = ctypes.c_void_p()
    assert L.ncg_points_from_encoded(h, 5, 1, p, 0, ctypes.byref(hnd), ctypes.byref(ctypes.c_int64(-1))) == UNSUPPORTED
    assert L.ncg_aggregate_encoded(h, 5, 1, p, 0, p, p, p) == UNSUPPORTED
    assert L.ncg_mul_base_batch(h, 5, 1, p, p, p) == UNSUPPORTED and "unsupported curve 5" in err()
    assert L.ncg_map_to_curve_batch(h, 5, 1, 1, p, p, p) == UNSUPPORTED
    assert L.ncg_ecdsa_verify_batch(h, 5, 1, p, p, p, 0, p) == UNSUPPORTED
    rs = eng.upload_points(BN254_G1, to_wire([Bn254.BASE]))
    with pytest.raises(NativeError):
        rs.verify_subgroup()
    rs.free()


def test_python_mirror():
    from noble_curves_amd import curve as G
    c = G.bn254_G1_Point
    rng = makeRng(0x2544)
    opts = [rand_point(rng) for _ in range(40)]
    ks = [rng.rndBelow(BN254_R) for _ in opts]
    pts = [c.fromAffine(p.toAffine()) for p in opts]
    assert G.pippenger(c, pts, ks).toAffine() == _oracle_msm(opts, ks)
    got = G.multiplyUnsafeBatch(c, pts, ks)
    assert [q.toAffine() for q in got] == [_aff(p.multiplyUnsafe(k)) for p, k in zip(opts, ks)]
    s = G.addBatch(c, pts[:10], pts[10:20])
    assert [q.toAffine() for q in s] == [_aff(p.add(q)) for p, q in zip(opts[:10], opts[10:20])]
    with pytest.raises(ValueError, match="no batch decoder"):
        G.fromBytesBatch(c, [b"\0" * 32])
    with pytest.raises(ValueError, match="no batch encoder"):
        G.toBytesBatch(c, pts[:1])
    # argument errors as for the other Weierstrass classes (the reference's pippenger / multiplyUnsafe checks)
    for cc, pp in ((c, pts[:2]), (G.secp256k1_Point, [G.secp256k1_Point.BASE] * 2)):
        errs = []
        for call in (lambda: G.pippenger(cc, pp, [1]), lambda: G.multiplyUnsafeBatch(cc, pp, [1, -1])):
            with pytest.raises(Exception) as ei:
                call()
            errs.append((type(ei.value), str(ei.value)))
        if cc is c:
            ref = errs
    assert errs == ref


# ---- batch multiply, pairwise add and normalize at the block and wave edges ------------------------------------------
# k_mul_var_gtab runs 64 lanes per block; the pairwise add and normalize_batch take K = 8 items per lane (one inversion per 8).
EDGE_SCALARS = [BN254_R, BN254_R + 1, 2 * BN254_R - 1, 1 << 255, (1 << 256) - 1, 5 * BN254_R + 3, BN254_R - 1, 0, 1, 2,
                1 << 254, (1 << 256) - BN254_R]


class _Comb:
    """k G for many k with the oracle's group law: 32 tables of j 2^(8 w) G (j < 256), 32 additions per multiple"""

    def __init__(self):
        self.tab = []
        Q = Bn254.BASE
        for _ in range(32):
            row = [Bn254.ZERO]
            for _ in range(255):
                row.append(row[-1].add(Q))
            self.tab.append(row)
            Q = row[-1].add(Q)

    def mul(self, k):
        k %= BN254_R
        acc = Bn254.ZERO
        for w in range(32):
            acc = acc.add(self.tab[w][(k >> (8 * w)) & 255])
        return acc


def _progression_points(a, b, n):
    """(a + i b) G for i < n, by additions, normalised together"""
    from oracle import curve as OC
    P, step, out = Bn254.BASE.multiplyUnsafe(a), Bn254.BASE.multiplyUnsafe(b), []
    for _ in range(n):
        out.append(P)
        P = P.add(step)
    return OC.normalizeZ(Bn254, out)


def _affine_all(pts):
    from oracle import curve as OC
    return [p.toAffine() for p in OC.normalizeZ(Bn254, pts)]


def test_batch_multiply_empty_and_block_edges():
    """n = 0 through the C ABI; n = 63, 64, 65 and 64 k +- 1 over several blocks, as slices of one pool at shifted offsets so
    that every edge scalar (r, r + 1, 2r - 1, 2^255, 2^256 - 1, ... : the C ABI takes any k < 2^256, the value is (k mod r) P)
    and ZERO point meets other lane positions; the first wave of the pool has only even scalars and the second every other one
    (the ladder's was_even fix-up at every lane position)."""
    eng = get_engine()
    L = eng.lib
    assert L.ncg_mul_var_batch(eng.h, BN254_G1, 0, None, None, None, None) == 0
    assert L.ncg_add_pairs_batch(eng.h, BN254_G1, 0, None, None, 0, None, None) == 0
    assert L.ncg_normalize_batch(eng.h, BN254_G1, 0, None, None, None) == 0
    out, inf = eng.mul_var_batch(BN254_G1, np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8))
    assert out.shape == (0, 64) and inf.shape == (0,)
    rng = makeRng(0x254B)
    npool = 700
    a0, b0 = rng.rndBelow(BN254_R - 1) + 1, rng.rndBelow(BN254_R - 1) + 1
    pts = _progression_points(a0, b0, npool)
    ks = []
    for i in range(npool):
        k = rng.rndBelow(1 << 256)
        if i < 64 or (i < 128 and i % 2 == 0) or i % 5 == 0:
            k &= ~1
        ks.append(k)
    for j, k in enumerate(EDGE_SCALARS):
        ks[3 + j] = k                                   # the first lanes of the pool
        ks[60 + j] = k                                  # across the first block boundary
        ks[npool - 1 - j] = k                           # the last lanes
    for i in (7, 64, 129, 400):
        pts[i] = Bn254.ZERO
    comb = _Comb()
    exp = _affine_all([Bn254.ZERO if p.is0() else comb.mul(k * (a0 + i * b0)) for i, (p, k) in enumerate(zip(pts, ks))])
    pw, sw = to_wire(pts), scalars_wire(ks)
    for n, off in ((63, 0), (64, 0), (65, 0), (64, 37), (127, 1), (129, 0), (191, 60), (193, 5), (575, 125), (577, 0),
                   (64 * 10 - 1, 0), (64 * 10 + 1, npool - 641)):
        out, inf = eng.mul_var_batch(BN254_G1, pw[off:off + n], sw[off:off + n])
        for i in range(n):
            e = exp[off + i]
            assert from_wire(out[i]) == e and bool(inf[i]) == (e == (0, 0)), (n, off, i, hex(ks[off + i]))


def test_batch_multiply_2_18_identity_and_sample():
    """2^18 pairs (the bench size): P_i = (a + i b) G from the device, k_i uniform below 2^256 with the edge scalars planted;
    sum_i c_i (k_i P_i) for random 62-bit c_i through the MSM equals (sum_i c_i k_i (a + i b) mod r) G, and 4096 items (the
    first and last waves among them) equal the oracle's (k_i (a + i b) mod r) G."""
    import bench
    eng = get_engine()
    dev = torch.device("cuda", 0)
    n = 1 << 18
    rng = makeRng(0x254C18)
    a, b = rng.rndBelow(BN254_R - 1) + 1, rng.rndBelow(BN254_R - 1) + 1
    pts, pks = bench.gen_points(eng, BN254_G1, Bn254, n, a, b, dev, None)
    sc = bench.gen_scalars(n, 256, 0x254, dev, edge_order=BN254_R)
    for j, k in enumerate(EDGE_SCALARS):
        for i in (100 + j, n // 2 + 64 * j, n - 1 - j):
            sc[i] = torch.from_numpy(scalars_wire([k])[0].copy()).to(dev)
    out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    inf = torch.empty((n,), dtype=torch.uint8, device=dev)
    eng.mul_var_batch_dev(BN254_G1, n, pts.data_ptr(), sc.data_ptr(), out.data_ptr(), inf.data_ptr())
    torch.cuda.synchronize()
    ks = bench.scalars_to_ints(sc)
    assert max(ks) == (1 << 256) - 1
    zero = [i for i, k in enumerate(ks) if k % BN254_R == 0]
    inf_h = inf.cpu().numpy()
    assert sorted(np.nonzero(inf_h)[0].tolist()) == zero
    cr = np.random.RandomState(0x254).randint(1, 1 << 62, size=n, dtype=np.int64)
    cw = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    cw[:, :8] = torch.from_numpy(cr.view(np.uint8).reshape(n, 8)).to(dev)
    tot, _ = eng.msm_dev(BN254_G1, n, out.data_ptr(), cw.data_ptr())
    expect = sum(int(c) * k * p for c, k, p in zip(cr, ks, pks)) % BN254_R
    assert from_wire(tot) == _aff(Bn254.BASE.multiplyUnsafe(expect))
    idx = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), np.random.RandomState(2).randint(0, n, 4096 - 128)]))
    comb = _Comb()
    want = _affine_all([comb.mul(ks[i] * pks[i]) for i in idx])
    out_h = out.cpu().numpy()
    for j, i in enumerate(idx):
        assert from_wire(out_h[i]) == want[j], (int(i), hex(ks[i]))


def test_add_pairs_and_normalize_over_waves():
    """K = 8 items per lane, 256 lanes per block: two full blocks, three full waves and a partial one (n = 2 * 2048 + 3 * 512 + 43);
    P + Q, P + P, P + (-P) and ZERO operands at scattered positions; normalize with Z = 0 (any X, Y) at every position of a group
    of 8, and a whole group of Z = 0."""
    eng = get_engine()
    n = 2 * 2048 + 3 * 512 + 43
    rng = makeRng(0x254A)
    A = _progression_points(rng.rndBelow(BN254_R - 1) + 1, rng.rndBelow(BN254_R - 1) + 1, n)
    B = _progression_points(rng.rndBelow(BN254_R - 1) + 1, rng.rndBelow(BN254_R - 1) + 1, n)
    for i in range(n):
        kind = (i * 7 + i // 8) % 11
        if kind == 1:
            B[i] = A[i]
        elif kind == 2:
            B[i] = A[i].negate()
        elif kind == 3:
            A[i] = Bn254.ZERO
        elif kind == 4:
            B[i] = Bn254.ZERO
    A[n - 1], B[n - 1] = Bn254.ZERO, Bn254.ZERO
    for sub in (False, True):
        out, inf = eng.add_pairs_batch(BN254_G1, to_wire(A), to_wire(B), subtract=sub)
        exp = _affine_all([p.subtract(q) if sub else p.add(q) for p, q in zip(A, B)])
        for i, e in enumerate(exp):
            assert from_wire(out[i]) == e and bool(inf[i]) == (e == (0, 0)), (sub, i)
    rows, exp = [], []
    for i in range(n):
        x, y = A[i].toAffine() if not A[i].is0() else B[i].toAffine()
        z = rng.rndBelow(BN254_P - 1) + 1
        g, j = divmod(i, 8)
        if (g % 300 < 8 and j == g % 300) or g == 100 or i == n - 1:   # Z = 0 at position g of group g (every block), group 100, the last item
            rows.append(b"".join(v.to_bytes(32, "little") for v in ((x * z % BN254_P, y * z % BN254_P, 0) if i % 2 else (0, 1, 0))))
            exp.append((0, 0))
        else:
            rows.append(b"".join(v.to_bytes(32, "little") for v in (x * z % BN254_P, y * z % BN254_P, z)))
            exp.append((x, y))
    out, inf = eng.normalize_batch(BN254_G1, np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(n, 96))
    for i, e in enumerate(exp):
        assert from_wire(out[i]) == e and bool(inf[i]) == (e == (0, 0)), i
