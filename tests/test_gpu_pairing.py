"""bls12-381 pairings on the device: ncg_fp12_batch and ncg_pairing_batch (host-pointer and _dev forms) against the plain-integer
restatement of tests/pairing_helpers.py - itself pinned to the reference's answers by tests/test_pairing_host.py - and the host mirror
noble_curves_amd.bls against the fixture.  The 130 pairs every pairing test draws from, and their Miller values, are computed once."""
import functools
import random

import numpy as np
import pytest
import torch

import pairing_helpers as H
from noble_curves_amd import _native, bls, get_engine
from noble_curves_amd._native import BLS12_381_G1, BLS12_381_G2, NativeError

pytestmark = pytest.mark.gpu
W = H.f12_wire
N_PAIRS = 130
GROUPS_130 = [1, 2, 0, 3, 7, 8, 9, 35, 65]          # with an empty group; 35 and 65 straddle a block of 32 lane pairs


def rows(arr, n, w):
    return [bytes(arr[i]) for i in range(n)] if arr.ndim == 2 else [bytes(arr[i * w:(i + 1) * w]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def pairs_and_miller():
    """([a_i] G1, [b_i] G2) with a_i = 7 + 3 i, b_i = 11 + 5 i by repeated addition, and each pair's Miller value"""
    s1, s2 = H.g1_mul(3), H.g2_mul(5)
    p, q = H.g1_mul(7), H.g2_mul(11)
    pairs = []
    for _ in range(N_PAIRS):
        pairs.append((p, q))
        p, q = H.C1.add(p, s1), H.C2.add(q, s2)
    return pairs, [H.miller_loop([pq]) for pq in pairs]


def want_groups(offsets):
    _, miller = pairs_and_miller()
    out = []
    for g in range(len(offsets) - 1):
        f = H.F12_ONE
        for i in range(offsets[g], offsets[g + 1]):
            f = H.f12_mul(f, miller[i])
        out.append(H.final_exponentiate(f) if offsets[g + 1] > offsets[g] else H.F12_ONE)
    return out


def wires(pairs):
    g1 = np.frombuffer(b"".join(H.g1_wire(p) for p, _ in pairs), dtype=np.uint8).reshape(-1, 96)
    g2 = np.frombuffer(b"".join(H.g2_wire(q) for _, q in pairs), dtype=np.uint8).reshape(-1, 192)
    return g1, g2


def run(pairs, offsets, want_gt=True):
    g1, g2 = wires(pairs)
    gt, one = get_engine(0).pairing_batch(g1, g2, offsets, want_gt)
    return ([H.f12_from_wire(gt[i]) for i in range(len(offsets) - 1)] if want_gt else None), [bool(v) for v in one]


def edge_elements():
    out = [H.f12_from_coeffs([v] * 12) for v in (0, 1, H.P - 1)] + [H.F12_ONE]
    for k in range(12):
        c = H.f12_coeffs(H.seeded_f12("edge", k))
        c[k] = (0, 1, H.P - 1)[k % 3]
        out.append(H.f12_from_coeffs(c))
    return out


def elements(n, tag):
    e = edge_elements()
    return [e[i] if i < len(e) else H.seeded_f12(tag, i) for i in range(n)]


PY_OPS = {_native.FP12_MUL: H.f12_mul, _native.FP12_SQR: H.f12_sqr, _native.FP12_INV: H.f12_inv, _native.FP12_CONJUGATE: H.f12_conj,
          _native.FP12_FROBENIUS1: lambda a: H.f12_frob(a, 1), _native.FP12_FROBENIUS2: lambda a: H.f12_frob(a, 2),
          _native.FP12_FROBENIUS3: lambda a: H.f12_frob(a, 3), _native.FP12_CYCLOTOMIC_SQR: H.f12_cyclotomic_sqr,
          _native.FP12_FINAL_EXP: H.final_exponentiate}


@pytest.mark.parametrize("n", [1, 33, 130])
def test_fp12_ops(n):
    eng = get_engine(0)
    a, b = elements(n, "gpu/a"), elements(n, "gpu/b")[::-1]
    aw = np.frombuffer(b"".join(W(x) for x in a), dtype=np.uint8)
    bw = np.frombuffer(b"".join(W(x) for x in b), dtype=np.uint8)
    for op, fn in PY_OPS.items():
        out = eng.fp12_batch(op, aw, bw if op == _native.FP12_MUL else None)
        want = [fn(x, y) if op == _native.FP12_MUL else fn(x) for x, y in zip(a, b)]
        assert [H.f12_from_wire(out[i]) for i in range(n)] == want, op
    lines = [tuple(H.seeded_f2("gpu/line/%d" % k, i) for k in range(3)) for i in range(n)]
    lines[0] = ((0, 0), (1, 0), (H.P - 1, H.P - 1))
    lw = np.frombuffer(b"".join(H.f2_wire(o) for r in lines for o in r), dtype=np.uint8)
    out = eng.fp12_batch(_native.FP12_MUL014, aw, lw)
    assert [H.f12_from_wire(out[i]) for i in range(n)] == [H.f12_mul014(x, *r) for x, r in zip(a, lines)]
    assert list(eng.fp12_batch(_native.FP12_IS_ONE, aw)) == [x == H.F12_ONE for x in a]
    # the cyclotomic square is the square on the cyclotomic subgroup
    cyc = [H.seeded_cyclotomic("gpu/cyc", i) for i in range(min(n, 8))]
    cw = np.frombuffer(b"".join(W(x) for x in cyc), dtype=np.uint8)
    out = eng.fp12_batch(_native.FP12_CYCLOTOMIC_SQR, cw)
    assert [H.f12_from_wire(out[i]) for i in range(len(cyc))] == [H.f12_sqr(x) for x in cyc]


def test_fp12_dev_form_agrees_and_arguments():
    eng = get_engine(0)
    a = elements(33, "gpu/a")
    aw = np.frombuffer(b"".join(W(x) for x in a), dtype=np.uint8).copy()
    host = eng.fp12_batch(_native.FP12_SQR, aw)
    da = torch.from_numpy(aw).cuda()
    do = torch.zeros(33 * 576, dtype=torch.uint8, device="cuda")
    eng.fp12_batch_dev(_native.FP12_SQR, 33, da.data_ptr(), None, do.data_ptr())
    eng.sync()
    assert np.array_equal(do.cpu().numpy().reshape(33, 576), host)
    with pytest.raises(NativeError, match="unknown op 11"):
        eng.fp12_batch(11, aw)
    with pytest.raises(NativeError, match="NULL buffer"):
        eng.fp12_batch_dev(_native.FP12_MUL, 33, da.data_ptr(), None, do.data_ptr())


def test_pairing_vector_rows():
    pairs = [(H.g1_mul(i + 1), H.g2_mul(i + 1)) for i in range(32)]
    gt, one = run(pairs, list(range(33)))
    assert gt == [H.f12_from_b64(v) for v in H.kat()["vectors"]] and not any(one)


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33])
def test_pairing_small_batches(n):
    pairs, _ = pairs_and_miller()
    gt, one = run(pairs[:n], list(range(n + 1)))             # groups of one
    assert gt == want_groups(list(range(n + 1))) and not any(one)
    gt, _ = run(pairs[:n], [0, n])                           # one group
    assert gt == want_groups([0, n])


def test_pairing_130_pairs_mixed_groups_both_forms_and_null_gt():
    pairs, _ = pairs_and_miller()
    off = [0] + list(np.cumsum(GROUPS_130))
    assert off[-1] == N_PAIRS
    want = want_groups(off)
    gt, one = run(pairs, off)
    assert gt == want and one == [w == H.F12_ONE for w in want] and one[2]
    _, one2 = run(pairs, off, want_gt=False)
    assert one2 == one
    eng = get_engine(0)
    g1, g2 = wires(pairs)
    d1, d2 = torch.from_numpy(g1.copy()).cuda(), torch.from_numpy(g2.copy()).cuda()
    dgt = torch.zeros(len(want) * 576, dtype=torch.uint8, device="cuda")
    done = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    eng.pairing_batch_dev(N_PAIRS, d1.data_ptr(), d2.data_ptr(), off, dgt.data_ptr(), done.data_ptr())
    assert [H.f12_from_wire(r) for r in rows(dgt.cpu().numpy(), len(want), 576)] == want
    assert [bool(v) for v in done.cpu().numpy()] == one


@pytest.mark.parametrize("n", [65, 257])
def test_cancelling_group(n):
    """sum a_i b_i = 0 (mod r) gives ONE; changing one scalar does not.  The points come from the fixed-base multiplies."""
    eng = get_engine(0)
    rng = random.Random(n)
    a = [rng.randrange(1, H.R) for _ in range(n)]
    b = [rng.randrange(1, H.R) for _ in range(n - 1)]
    b.append((-sum(x * y for x, y in zip(a, b)) * pow(a[-1], -1, H.R)) % H.R)
    assert sum(x * y for x, y in zip(a, b)) % H.R == 0 and b[-1] != 0
    sw = lambda ks: np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32)  # noqa: E731
    g1, _ = eng.mul_base_batch(BLS12_381_G1, sw(a))
    g2, _ = eng.mul_base_batch(BLS12_381_G2, sw(b))
    gt, one = eng.pairing_batch(g1, g2, [0, n])
    assert list(one) == [True] and H.f12_from_wire(gt[0]) == H.F12_ONE
    b[n // 2] = b[n // 2] % (H.R - 1) + 1
    g2, _ = eng.mul_base_batch(BLS12_381_G2, sw(b))
    gt, one = eng.pairing_batch(g1, g2, [0, n])
    assert list(one) == [False] and H.f12_from_wire(gt[0]) != H.F12_ONE
    # the same pairs as two groups: their values are inverse to each other
    gt, one = eng.pairing_batch(g1, g2, [0, n // 2, n])
    assert not any(one)


def test_refused_operands_leave_the_outputs_untouched():
    eng = get_engine(0)
    pairs, _ = pairs_and_miller()
    good = list(pairs[:40])
    P1, Q1 = good[0]
    cases = [(((0, 0), Q1), "pairing is not available for ZERO point"),
             ((P1, (H.F2_ZERO, H.F2_ZERO)), "pairing is not available for ZERO point"),
             (((P1[0], (P1[1] + 1) % H.P), Q1), "bad point: equation left != right"),
             ((P1, (Q1[0], ((Q1[1][0] + 1) % H.P, Q1[1][1]))), "bad point: equation left != right"),
             (((P1[0] + H.P, P1[1]), Q1), "bad point: equation left != right"),
             ((P1, ((Q1[0][0], Q1[0][1] + H.P), Q1[1])), "bad point: equation left != right")]
    for k, (bad, msg) in enumerate(cases):
        at = (5, 33, 39, 0, 34, 17)[k]
        rows_ = good[:at] + [bad] + good[at + 1:]
        rows_[min(at + 3, 39)] = bad                          # a second bad pair after it: the first one is reported
        g1, g2 = wires(rows_)
        gt = np.full((4, 576), 0xA5, dtype=np.uint8)
        one = np.full((4,), 0xA5, dtype=np.uint8)
        import ctypes
        off = np.array([0, 10, 20, 30, 40], dtype=np.uint32)
        badi = ctypes.c_int64(-7)
        rc = eng.lib.ncg_pairing_batch(eng.h, 40, g1.ctypes.data, g2.ctypes.data, 4, off.ctypes.data, 0, gt.ctypes.data, one.ctypes.data,
                                       ctypes.byref(badi))
        err = (eng.lib.ncg_last_error(eng.h) or b"").decode()
        assert rc == -1 and badi.value == at and msg in err and "index %d" % at in err, (k, err)
        with pytest.raises(ValueError) as ei:               # the mirror hands on the reference's text alone
            bls._run_pairing([(bls.G1Point(*p) if p != (0, 0) else bls.G1Point.ZERO, bls.G2Point(*q)) for p, q in rows_[:at + 1]][at:],
                             [0, 1], eng, check_subgroup=False)
        assert str(ei.value) == msg
        assert (gt == 0xA5).all() and (one == 0xA5).all()
    g1, g2 = wires(good)
    with pytest.raises(NativeError, match="group offsets must ascend"):
        eng.pairing_batch(g1, g2, [0, 30, 20, 40])
    with pytest.raises(NativeError, match="group offsets must ascend"):
        eng.pairing_batch(g1, g2, [0, 39])
    with pytest.raises(NativeError, match="unknown flag bits"):
        import ctypes
        one = np.zeros(1, dtype=np.uint8)
        off = np.array([0, 40], dtype=np.uint32)
        eng._check(eng.lib.ncg_pairing_batch(eng.h, 40, g1.ctypes.data, g2.ctypes.data, 1, off.ctypes.data, 2, None, one.ctypes.data, None))
    gt, one = eng.pairing_batch(g1[:0], g2[:0], [0, 0, 0])   # only empty groups
    assert list(one) == [True, True] and H.f12_from_wire(gt[1]) == H.F12_ONE


def test_subgroup_flag():
    """an operand on its curve and outside the subgroup: accepted without NCG_PAIRING_CHECK_SUBGROUP (the restatement's value), refused
    with it - right index and message, outputs untouched - and subgroup members pass under the flag"""
    import ctypes
    eng = get_engine(0)
    pairs, _ = pairs_and_miller()
    T1, T2 = H.torsion_points()
    P1, Q1 = pairs[0]
    gt, one = run([(T1, Q1), (P1, T2)], [0, 1, 2])
    assert gt == [H.pairing(T1, Q1), H.pairing(P1, T2)] and one == [g == H.F12_ONE for g in gt]   # (x = 0 on T1: its value is ONE)
    for rows_, at in (([pairs[k] for k in range(35)] + [(T1, Q1)] + [(P1, T2)], 35), ([(P1, T2)] + [pairs[k] for k in range(36)], 0)):
        g1, g2 = wires(rows_)
        gt = np.full((1, 576), 0xA5, dtype=np.uint8)
        one = np.full((1,), 0xA5, dtype=np.uint8)
        off = np.array([0, 37], dtype=np.uint32)
        badi = ctypes.c_int64(-7)
        rc = eng.lib.ncg_pairing_batch(eng.h, 37, g1.ctypes.data, g2.ctypes.data, 1, off.ctypes.data, _native.PAIRING_CHECK_SUBGROUP,
                                       gt.ctypes.data, one.ctypes.data, ctypes.byref(badi))
        err = (eng.lib.ncg_last_error(eng.h) or b"").decode()
        assert rc == -1 and badi.value == at and "bad point: not in prime-order subgroup" in err and "index %d" % at in err, err
        assert (gt == 0xA5).all() and (one == 0xA5).all()
    g1, g2 = wires(pairs[:33])
    gt, one = eng.pairing_batch(g1, g2, [0, 33], flags=_native.PAIRING_CHECK_SUBGROUP)
    assert [H.f12_from_wire(gt[0])] == want_groups([0, 33])


def _verify_inputs(scheme, count):
    """`count` rows (pk, sig, u) of the fixture's verify rows of one scheme, repeated cyclically, and the reference's booleans"""
    from noble_curves_amd import h2c
    items, want = H.verify_rows()[scheme], H.kat()["verify"][scheme]
    hasher = h2c.bls12_381_G2_hasher if scheme == "long" else h2c.bls12_381_G1_hasher
    o = hasher._opts(None)
    pk, sig, u, exp = b"", b"", b"", []
    for i in range(count):
        s_, m, k_ = items[i % len(items)]
        pk, sig = pk + bytes.fromhex(k_), sig + bytes.fromhex(s_)
        u += b"".join(int(c).to_bytes(48, "little") for e in h2c.hash_to_field(bytes.fromhex(m), 2, o) for c in e)
        exp.append(want[i % len(items)])
    return (np.frombuffer(pk, dtype=np.uint8).copy(), np.frombuffer(sig, dtype=np.uint8).copy(), np.frombuffer(u, dtype=np.uint8).copy(), exp)


@pytest.mark.parametrize("scheme", ["long", "short"])
@pytest.mark.parametrize("n", [1, 12, 33])
def test_bls_verify_batch(scheme, n):
    """ncg_bls_verify_batch: every fixture verify row - valid rows interleaved with the wrong message, wrong key, swapped signature,
    ZERO key, ZERO signature and a key outside the subgroup - from bytes in one call, against the reference's booleans"""
    eng = get_engine(0)
    sid = _native.BLS_LONG_SIGNATURES if scheme == "long" else _native.BLS_SHORT_SIGNATURES
    pk, sig, u, want = _verify_inputs(scheme, n)
    assert list(eng.bls_verify_batch(sid, pk, sig, u)) == want
    if n == 33:                                              # the _dev form, and the mirror's one-call form
        d = [torch.from_numpy(x).cuda() for x in (pk, sig, u)]
        ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        eng.bls_verify_batch_dev(sid, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), ok.data_ptr())
        assert [bool(v) for v in ok.cpu().numpy()] == want
        S = bls.longSignatures if scheme == "long" else bls.shortSignatures
        rows_ = H.verify_rows()[scheme]
        assert S.verifyMessagesBatch(rows_ + [("00", "00", "00")]) == H.kat()["verify"][scheme] + [False]
        pk2 = pk.copy()
        pk2[0] ^= 0x80                                      # the compression flag cleared: fromBytes throws
        assert not eng.bls_verify_batch(sid, pk2, sig, u)[0]
    with pytest.raises(NativeError, match="scheme must be 0"):
        eng.bls_verify_batch(2, pk, sig, u)


def test_fp12_in_place():
    eng = get_engine(0)
    a = elements(33, "gpu/a")
    aw = np.frombuffer(b"".join(W(x) for x in a), dtype=np.uint8).copy()
    d = torch.from_numpy(aw).cuda()
    eng.fp12_batch_dev(_native.FP12_MUL, 33, d.data_ptr(), d.data_ptr(), d.data_ptr())
    eng.sync()
    assert [H.f12_from_wire(r) for r in rows(d.cpu().numpy(), 33, 576)] == [H.f12_sqr(x) for x in a]


def test_mirror_pairing_and_fp12():
    k = H.kat()
    G1, G2 = bls.G1Point, bls.G2Point
    sc = [H.seeded_pair_scalars(i) for i in range(4)]
    ps = [(G1.fromAffine(H.g1_mul(a)), G2.fromAffine(H.g2_mul(b))) for a, b in sc]
    assert bls.pairingRows(ps) == [H.f12_from_b64(v) for v in k["pairing"][:4]]
    assert bls.pairing(*ps[0]) == H.f12_from_b64(k["pairing"][0])
    j = 4                                                   # five pairs
    grp = [{"g1": G1.fromAffine(H.g1_mul(a)), "g2": G2.fromAffine(H.g2_mul(b))} for a, b in H.seeded_batch(j)]
    want = H.f12_from_b64(k["batch"][j])
    assert bls.pairingBatch(grp) == want and bls.pairingBatch(grp + grp[:1], groups=[5, 0, 1])[:2] == [want, bls.Fp12.ONE]
    e = bls.pairing(G1.BASE, G2.BASE)
    F = bls.Fp12
    assert F.mul(e, F.inv(e)) == F.ONE and F.conjugate(e) == F.inv(e) and F._cyclotomicSquare(e) == F.sqr(e)
    assert F.frobeniusMap(F.frobeniusMap(e, 3), 3) == F.frobeniusMap(e, 6) and F.isOneBatch([e, F.ONE]) == [False, True]
    assert F.finalExponentiate(H.seeded_f12("fe", 0)) == H.f12_from_b64(k["final_exp"][0])
    torsion = G1.fromAffine((0, 2))                         # order 3: on the curve, outside the subgroup
    with pytest.raises(ValueError, match="not in prime-order subgroup"):
        bls.pairing(torsion, G2.BASE)
    with pytest.raises(ValueError, match="bad point: equation left != right"):
        bls.pairing(G1(1, 2), G2.BASE)


@pytest.mark.parametrize("scheme", ["long", "short"])
def test_mirror_verify_against_reference_booleans(scheme):
    k, rows_ = H.kat()["verify"], H.verify_rows()
    S = bls.longSignatures if scheme == "long" else bls.shortSignatures
    items = rows_[scheme]
    msgs = S.hashBatch([bytes.fromhex(m) for _, m, _ in items])
    triples = [(bytes.fromhex(s), msgs[i], bytes.fromhex(pk)) for i, (s, _, pk) in enumerate(items)]
    assert S.verifyRows(triples) == k[scheme]                # valid and invalid rows interleaved, one batch
    assert S.verify(*triples[0]) is True and S.verify(*triples[1]) is False
    for case, want in zip(rows_[scheme + "_batch"], k[scheme + "_batch"]):
        its = [{"message": S.hash(bytes.fromhex(m)), "publicKey": bytes.fromhex(pk)} for m, pk in case["items"]]
        assert S.verifyBatch(bytes.fromhex(case["sig"]), its) is want
    # keys grouped under one message object, and the aggregates
    m = S.hash(b"one message")
    assert S.verifyBatch(triples[0][0], [{"message": m, "publicKey": triples[0][2]}, {"message": m, "publicKey": triples[2][2]}]) is False
    agg = S.aggregateSignatures([t[0] for t in triples[0:6:2]])
    assert S.verifyBatch(agg, [{"message": t[1], "publicKey": t[2]} for t in triples[0:6:2]]) is True
