"""bls12-381 pairings without a GPU: the plain-integer restatement of tests/pairing_helpers.py against every row of the fixture
(the reference's own answers), then the ht_fp12_op / ht_pairing host twins - the lane templates of csrc/fp12.hpp and csrc/pairing.hpp
on the unpaired Fp2 - against the restatement; bilinearity; the generated Frobenius coefficients; the mirror's argument errors."""
import random

import pytest

import pairing_helpers as H

W = H.f12_wire
OPS = [("mul", H.OP_MUL), ("sqr", H.OP_SQR), ("inv", H.OP_INV), ("conjugate", H.OP_CONJ), ("frobenius1", H.OP_FROB1),
       ("frobenius2", H.OP_FROB2), ("frobenius3", H.OP_FROB3), ("cyclotomic_sqr", H.OP_CYC_SQR)]


def py_op(op, a, b=None):
    return {H.OP_MUL: lambda: H.f12_mul(a, b), H.OP_SQR: lambda: H.f12_sqr(a), H.OP_INV: lambda: H.f12_inv(a),
            H.OP_CONJ: lambda: H.f12_conj(a), H.OP_FROB1: lambda: H.f12_frob(a, 1), H.OP_FROB2: lambda: H.f12_frob(a, 2),
            H.OP_FROB3: lambda: H.f12_frob(a, 3), H.OP_CYC_SQR: lambda: H.f12_cyclotomic_sqr(a),
            H.OP_MUL014: lambda: H.f12_mul014(a, *b), H.OP_FINAL_EXP: lambda: H.final_exponentiate(a)}[op]()


def op_inputs(name):
    if name == "cyclotomic_sqr":
        return [H.seeded_cyclotomic("op/cyc", i) for i in range(8)], None
    return [H.seeded_f12("op/a", i) for i in range(8)], [H.seeded_f12("op/b", i) for i in range(8)]


def edge_elements():
    """coefficients 0, 1 and p - 1 in every mix, ONE, ZERO, and seeded elements with one coefficient at an edge"""
    rows = [H.f12_from_coeffs([v] * 12) for v in (0, 1, H.P - 1)]
    rows.append(H.F12_ONE)
    for k in range(12):
        c = H.f12_coeffs(H.seeded_f12("edge", k))
        c[k] = (0, 1, H.P - 1)[k % 3]
        rows.append(H.f12_from_coeffs(c))
    rows.append(H.f12_from_coeffs([(0, 1, H.P - 1)[i % 3] for i in range(12)]))
    return rows


# ---------------------------------------------------------------- the restatement against the reference's answers
def test_restatement_matches_go_vectors():
    for i, want in enumerate(H.kat()["vectors"]):
        assert H.pairing(H.g1_mul(i + 1), H.g2_mul(i + 1)) == H.f12_from_b64(want), i


def test_restatement_matches_reference_pairings():
    k = H.kat()
    for i, want in enumerate(k["pairing"]):
        a, b = H.seeded_pair_scalars(i)
        assert H.pairing(H.g1_mul(a), H.g2_mul(b)) == H.f12_from_b64(want), i
    for j, want in enumerate(k["batch"]):
        assert H.pairing_batch([(H.g1_mul(a), H.g2_mul(b)) for a, b in H.seeded_batch(j)]) == H.f12_from_b64(want), j


def test_restatement_matches_reference_fp12():
    k = H.kat()
    for name, op in OPS:
        a, b = op_inputs(name)
        for i, want in enumerate(k["ops"][name]):
            assert py_op(op, a[i], b[i] if b else None) == H.f12_from_b64(want), (name, i)
    for i, want in enumerate(k["final_exp"]):
        assert H.final_exponentiate(H.seeded_f12("fe", i)) == H.f12_from_b64(want), i
    for i, want in enumerate(k["ops"]["mul014"]):          # the reference's Fp12.mul by the sparse element
        assert H.f12_mul014(H.seeded_f12("op/a", i), *H.seeded_line(i)) == H.f12_from_b64(want), i
    a, _ = op_inputs("mul")
    assert [x == H.F12_ONE for x in a + [H.F12_ONE]] == k["ops"]["is_one"]
    x = a[0]                                                # the cyclotomic exponentiation is the plain power
    c = H.seeded_cyclotomic("op/cyc", 0)
    assert H.cyclotomic_exp_x(c) == H.f12_pow(c, H.BLS_X)
    assert H.f12_mul(x, H.f12_inv(x)) == H.F12_ONE
    assert len(H.ATE_NAF) == 64 and [63 - i for i, d in enumerate(H.ATE_NAF) if d] == [62, 60, 57, 48, 16] and H.ATE_NAF[1] == -1


# ---------------------------------------------------------------- the host twins against the restatement
def test_twin_fp12_ops_fixture_random_and_edges():
    rng = random.Random(0x12F)
    rand = [H.f12_from_coeffs([rng.randrange(H.P) for _ in range(12)]) for _ in range(16)]
    for name, op in OPS:
        a, b = op_inputs(name)
        if name != "cyclotomic_sqr":
            a = a + rand + edge_elements()
            b = (b + rand[::-1] + edge_elements()[::-1])
        got = H.ht_fp12_op(op, [W(x) for x in a], [W(y) for y in b] if op == H.OP_MUL else None)
        assert got == [py_op(op, x, b[i] if b else None) for i, x in enumerate(a)], name
    a = [H.seeded_f12("op/a", i) for i in range(8)] + edge_elements()
    lines = [H.seeded_line(i) for i in range(len(a))]
    lines[11] = ((0, 0), (1, 0), (H.P - 1, H.P - 1))
    got = H.ht_fp12_op(H.OP_MUL014, [W(x) for x in a], [b"".join(H.f2_wire(o) for o in r) for r in lines])
    assert got == [H.f12_mul014(x, *r) for x, r in zip(a, lines)]
    assert got[:8] == [H.f12_from_b64(v) for v in H.kat()["ops"]["mul014"]]
    fe = [H.seeded_f12("fe", i) for i in range(8)] + rand[:4]
    assert H.ht_fp12_op(H.OP_FINAL_EXP, [W(x) for x in fe]) == [H.final_exponentiate(x) for x in fe]
    ones = [H.F12_ONE, rand[0], H.f12_from_coeffs([1] + [0] * 10 + [1]), H.f12_from_coeffs([0] * 12)]
    assert H.ht_fp12_op(H.OP_IS_ONE, [W(x) for x in ones]) == [True, False, False, False]


def test_twin_raw_limbs_at_the_top_of_the_storage_bound():
    """operands as stored words: the largest value of the bound type (256 p - 1), every limb at 2^29 - 1 below the top limb, 0 and p"""
    top = 256 * H.P - 1
    full = (top >> (29 * 13) << (29 * 13)) - 1              # limbs 0..12 all ones, top limb one below the maximum
    raws = [top, full, 0, H.P, 255 * H.P + 1]
    rng = random.Random(0x7A)
    rows = [[raws[(i + k) % len(raws)] if (i * 5 + k) % 3 else rng.randrange(256 * H.P) for k in range(12)] for i in range(6)]
    elems = [H.f12_from_coeffs([H.stored_to_int(v) for v in r]) for r in rows]
    a = [b"".join(H.stored_limbs(v) for v in r) for r in rows]
    other = [H.seeded_f12("raw", i) for i in range(len(rows))]
    for op in (H.OP_MUL, H.OP_SQR, H.OP_INV, H.OP_CONJ, H.OP_FROB1, H.OP_FROB2, H.OP_FROB3, H.OP_CYC_SQR, H.OP_FINAL_EXP):
        got = H.ht_fp12_op(op, a, [W(y) for y in other] if op == H.OP_MUL else None, raw=True)
        assert got == [py_op(op, x, other[i]) for i, x in enumerate(elems)], op


def test_twin_pairing_fixture_rows_and_groups():
    k = H.kat()
    pairs = [(H.g1_mul(i + 1), H.g2_mul(i + 1)) for i in range(32)]
    gt, one = H.ht_pairing(pairs, list(range(33)))
    assert gt == [H.f12_from_b64(v) for v in k["vectors"]] and not any(one)
    rows, off = [], [0]
    for j in range(8):
        rows += [(H.g1_mul(a), H.g2_mul(b)) for a, b in H.seeded_batch(j)]
        off.append(len(rows))
    off.insert(3, off[3])                                    # an empty group
    gt, one = H.ht_pairing(rows, off)
    want = [H.f12_from_b64(v) for v in k["batch"]]
    want.insert(3, H.F12_ONE)
    assert gt == want and one == [w == H.F12_ONE for w in want]


def test_twin_pairing_random_pairs_and_bilinearity():
    rng = random.Random(0xB11)
    sc = [(rng.randrange(1, H.R), rng.randrange(1, H.R)) for _ in range(16)]
    pairs = [(H.g1_mul(a), H.g2_mul(b)) for a, b in sc]
    gt, _ = H.ht_pairing(pairs, list(range(17)))
    assert gt == [H.pairing(p, q) for p, q in pairs]
    base = H.ht_pairing([(H.G1, H.G2)], [0, 1])[0][0]
    for (a, b), e in list(zip(sc, gt))[:4]:                  # e([a] P, [b] Q) = e(P, Q)^(a b)
        assert e == H.f12_pow(base, a * b % H.R)
    # a cancelling group: sum a_i b_i = 0 mod r
    a3 = [3, 5, 7]
    b3 = [11, 13, (-(3 * 11 + 5 * 13) * pow(7, -1, H.R)) % H.R]
    grp = [(H.g1_mul(a), H.g2_mul(b)) for a, b in zip(a3, b3)]
    gt, one = H.ht_pairing(grp + grp[:2] + [(H.g1_mul(7), H.g2_mul(b3[2] + 1))], [0, 3, 6])
    assert one == [True, False] and gt[0] == H.F12_ONE


def test_twin_refuses_what_the_reference_refuses():
    P1, Q1 = H.g1_mul(5), H.g2_mul(9)
    off_g1, off_g2 = (P1[0], (P1[1] + 1) % H.P), (Q1[0], ((Q1[1][0] + 1) % H.P, Q1[1][1]))
    big = (P1[0] + H.P, P1[1])
    assert H.ht_pairing([(P1, Q1), ((0, 0), Q1)], [0, 2]) == (1, H.BAD_ZERO)
    assert H.ht_pairing([(P1, (H.F2_ZERO, H.F2_ZERO))], [0, 1]) == (0, H.BAD_ZERO)
    assert H.ht_pairing([(P1, Q1), (P1, Q1), (off_g1, Q1)], [0, 1, 3]) == (2, H.BAD_G1)
    assert H.ht_pairing([(P1, off_g2)], [0, 1]) == (0, H.BAD_G2)
    assert H.ht_pairing([(big, Q1)], [0, 1]) == (0, H.BAD_G1)
    with pytest.raises(ValueError, match=H.ZERO_MSG):
        H.pairing_batch([((0, 0), Q1)])


def test_twin_subgroup_flag():
    """points on the curves and outside the subgroups: accepted without NCG_PAIRING_CHECK_SUBGROUP (the value is the restatement's),
    refused with it - G1 before G2, as g1.assertValidity runs first - and members pass under the flag"""
    T1, T2 = H.torsion_points()
    assert H.on_curve_g1(T1) and H.on_curve_g2(T2)
    P1, Q1 = H.g1_mul(5), H.g2_mul(9)
    gt, _ = H.ht_pairing([(T1, Q1), (P1, T2)], [0, 1, 2])
    assert gt == [H.pairing(T1, Q1), H.pairing(P1, T2)]
    assert H.ht_pairing([(P1, Q1), (T1, Q1)], [0, 2], H.CHECK_SUBGROUP) == (1, H.BAD_G1_SUBGROUP)
    assert H.ht_pairing([(P1, T2)], [0, 1], H.CHECK_SUBGROUP) == (0, H.BAD_G2_SUBGROUP)
    assert H.ht_pairing([(T1, T2)], [0, 1], H.CHECK_SUBGROUP) == (0, H.BAD_G1_SUBGROUP)
    gt, _ = H.ht_pairing([(P1, Q1)], [0, 1], H.CHECK_SUBGROUP)
    assert gt == [H.pairing(P1, Q1)]


def test_generated_frobenius_coefficients():
    """consts_gen.hpp BlsTower against pow(u + 1, (p^k - 1) / 6) and its kin recomputed here"""
    got = H.ht_tower_consts()
    for k in range(4):
        assert got[0][k] == H.f2_pow((1, 1), (H.P ** k - 1) // 3)
        assert got[1][k] == H.f2_pow((1, 1), (2 * H.P ** k - 2) // 3)
        assert got[2][k] == H.f2_pow((1, 1), (H.P ** k - 1) // 6)


def test_mirror_argument_errors():
    from noble_curves_amd import bls
    g1, g2 = bls.G1Point.BASE, bls.G2Point.BASE
    with pytest.raises(TypeError, match='"Q" expected G1 point'):
        bls.pairing(g2, g2)
    with pytest.raises(TypeError, match='"P" expected G2 point'):
        bls.pairing(g1, g1)
    with pytest.raises(TypeError, match=r'"pairs\[1\].g2" expected G2 point'):
        bls.pairingBatch([(g1, g2), (g1, g1)])
    with pytest.raises(TypeError, match='"pairs" expected Array'):
        bls.pairingBatch(5)
    with pytest.raises(ValueError, match=bls.ZERO_MSG):
        bls.pairing(bls.G1Point.ZERO, g2)
    with pytest.raises(ValueError, match=bls.ZERO_MSG):
        bls.pairingBatch([{"g1": g1, "g2": bls.G2Point.ZERO}])
    with pytest.raises(ValueError, match="group sizes"):
        bls.pairingBatch([(g1, g2)], groups=[2])
    assert bls.pairingBatch([]) == bls.Fp12.ONE and bls.pairingBatch([], groups=[]) == []
    with pytest.raises(ValueError, match="expected non-empty array"):
        bls.longSignatures.verifyBatch(b"\x00" * 96, [])
    with pytest.raises(ValueError, match="expected valid message hashed to G2 curve"):
        bls.longSignatures.verifyRows([(b"\x00" * 96, g1, b"\x00" * 48)])
    with pytest.raises(ValueError, match="expected valid message hashed to G1 curve"):
        bls.shortSignatures.verifyRows([(b"\x00" * 48, g2, b"\x00" * 96)])
    with pytest.raises(ValueError, match="fromBytes invalid length=3"):
        bls.Fp12.fromBytes(b"abc")
    one = bls.Fp12.fromBytes(bls.Fp12.toBytes(bls.Fp12.ONE))
    assert one == bls.Fp12.ONE and bls.Fp12.eql(one, bls.Fp12.ONE) and bls.Fp12.frobeniusMapBatch([one], 12) == [one]
    with pytest.raises(ValueError, match="coefficients in"):
        bls.Fp12.toBytes((((bls._P, 0), (0, 0), (0, 0)), ((0, 0),) * 3))
