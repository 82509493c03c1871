"""The ristretto255 OPRF ON THE DEVICE: ncg_xmd_sha512_batch, ncg_ristretto_hash_to_{group,scalar}_batch, ncg_oprf_{blind,mul,
finalize,evaluate,composite_scalars}_batch (host and _dev forms), ncg_oprf_{generate,verify}_proof and ncg_oprf_check, against the CPU
twins of the same lane code (oprf_helpers.ht_*), the reference's recorded answers (tests/golden/ristretto255_oprf_kat.json) and the
mirror noble_curves_amd.oprf - bit for bit, no tolerances.  The twin's answers for the 129 seeded rows are computed once and every
batch size is a prefix of them."""
import functools

import numpy as np
import pytest
import torch

import oprf_helpers as oh
import ristretto_helpers as rh
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -4
L = oh.L
H = bytes.fromhex
SIZES = [1, 2, 63, 64, 65, 129]
NMAX = 129
INFO = b"public info"


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _fill(shape, v):
    return torch.full(shape, v, dtype=torch.uint8, device="cuda")


def _rows32(items):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, 32).copy()


def _blob_dev(msgs):
    blob, off = oh.blob(msgs)
    return _dev(np.frombuffer(blob + b"\0", np.uint8)), _dev(off)


# ---------------------------------------------------------------- the seeded rows and the twin's answers, once
@functools.lru_cache(None)
def seeded():
    """129 rows: inputs of mixed lengths, blinds and keys with a zero, L and 2^256 - 1 in mid-wave, and elements of which some do
    not decode, one is the identity and the rest are valid - rejected rows sit between accepted ones inside the first wave"""
    rng = np.random.RandomState(94970)
    inputs = [oh.seeded_bytes("gpu-in", i, (7 * i) % 90) for i in range(NMAX)]
    scalars = [int.from_bytes(rng.bytes(32), "little") % (L - 1) + 1 for _ in range(NMAX)]
    scalars[5], scalars[37], scalars[70] = 0, L, 2**256 - 1
    base = rh.base_multiples(64)
    elements = [rh.encode(base[(11 * i) % 64]) for i in range(NMAX)]
    elements[3], elements[20], elements[41], elements[100] = b"\x01" + bytes(31), bytes(32), oh.le32(rh.P - 1), bytes(32)
    return inputs, [oh.le32(k) for k in scalars], elements


@functools.lru_cache(None)
def want_blind(mode):
    inputs, scalars, _ = seeded()
    return [oh.ht_blind(mode, i, k) for i, k in zip(inputs, scalars)]


@functools.lru_cache(None)
def want_mul(flags):
    _, scalars, elements = seeded()
    one = flags & oh.ONE_SCALAR
    return [oh.ht_mul(e, scalars[1] if one else k, flags & oh.INVERT) for e, k in zip(elements, scalars)]


@functools.lru_cache(None)
def want_finalize(mode):
    inputs, scalars, elements = seeded()
    return [oh.ht_finalize(mode, i, k, e, INFO if mode == 2 else None) for i, k, e in zip(inputs, scalars, elements)]


@functools.lru_cache(None)
def want_evaluate(mode, flags):
    inputs, scalars, _ = seeded()
    return [oh.ht_evaluate(mode, i, scalars[2], flags & oh.INVERT, INFO if mode == 2 else None) for i in inputs]


def _check(got_out, got_st, want, n, width):
    assert list(got_st) == [w[0] for w in want[:n]]
    assert [bytes(r) for r in got_out] == [w[1] for w in want[:n]]
    assert all(w[1] == bytes(width) for w in want[:n] if w[0])


# ---------------------------------------------------------------- the fused rows: every size, both forms
@pytest.mark.parametrize("n", SIZES)
def test_blind_batch_sizes(n):
    eng = get_engine()
    inputs, scalars, _ = seeded()
    mode = n % 3
    out, st = eng.oprf_blind_batch(mode, inputs[:n], _rows32(scalars[:n]))
    _check(out, st, want_blind(mode), n, 32)
    blob, off = _blob_dev(inputs[:n])
    dk, do, ds = _dev(_rows32(scalars[:n])), _fill((n, 32), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_oprf_blind_batch_dev(eng.h, 0, mode, n, blob.data_ptr(), off.data_ptr(), dk.data_ptr(), do.data_ptr(), ds.data_ptr(), None) == OK
    torch.cuda.synchronize()
    _check(do.cpu().numpy(), ds.cpu().numpy(), want_blind(mode), n, 32)
    if n >= 63:
        assert sorted(set(st)) == [0, 3] and st[5] == st[37] == 3 and st[4] == st[6] == 0


@pytest.mark.parametrize("flags", [0, oh.INVERT, oh.ONE_SCALAR, oh.ONE_SCALAR | oh.INVERT])
@pytest.mark.parametrize("n", SIZES)
def test_mul_batch_sizes_and_flags(n, flags):
    eng = get_engine()
    _, scalars, elements = seeded()
    ks = _rows32([scalars[1]] if flags & oh.ONE_SCALAR else scalars[:n])
    out, st = eng.oprf_mul_batch(_rows32(elements[:n]), ks, one_scalar=bool(flags & oh.ONE_SCALAR), invert=bool(flags & oh.INVERT))
    _check(out, st, want_mul(flags), n, 32)
    de, dk, do, ds = _dev(_rows32(elements[:n])), _dev(ks), _fill((n, 32), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_oprf_mul_batch_dev(eng.h, 0, n, de.data_ptr(), dk.data_ptr(), flags, do.data_ptr(), ds.data_ptr(), None) == OK
    torch.cuda.synchronize()
    _check(do.cpu().numpy(), ds.cpu().numpy(), want_mul(flags), n, 32)
    if n >= 63:      # undecodable, identity, valid and (with a scalar per row) a refused scalar in one wave, refused rows between accepted ones
        assert (st[3], st[20], st[41], st[4], st[19], st[21]) == (1, 2, 1, 0, 0, 0)
        assert (st[5] == 3 and st[37] == 3) != bool(flags & oh.ONE_SCALAR)


def test_mul_one_scalar_refused_scalar():
    eng = get_engine()
    _, _, elements = seeded()
    for bad in (0, L):
        for inv in (False, True):
            out, st = eng.oprf_mul_batch(_rows32(elements[:8]), _rows32([oh.le32(bad)]), one_scalar=True, invert=inv)
            assert list(st) == [3, 3, 3, 1, 3, 3, 3, 3] and not out.any()


@pytest.mark.parametrize("n", SIZES)
def test_finalize_and_evaluate_batch_sizes(n):
    eng = get_engine()
    inputs, scalars, elements = seeded()
    mode = (n + 1) % 3
    info = INFO if mode == 2 else None
    out, st = eng.oprf_finalize_batch(mode, inputs[:n], _rows32(scalars[:n]), _rows32(elements[:n]), info)
    _check(out, st, want_finalize(mode), n, 64)
    blob, off = _blob_dev(inputs[:n])
    dk, de, do, ds = _dev(_rows32(scalars[:n])), _dev(_rows32(elements[:n])), _fill((n, 64), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_oprf_finalize_batch_dev(eng.h, 0, mode, n, blob.data_ptr(), off.data_ptr(), info, len(info or b""), dk.data_ptr(),
                                               de.data_ptr(), do.data_ptr(), ds.data_ptr(), None) == OK
    torch.cuda.synchronize()
    _check(do.cpu().numpy(), ds.cpu().numpy(), want_finalize(mode), n, 64)
    for flags in (oh.ONE_SCALAR, oh.ONE_SCALAR | oh.INVERT):
        out, st = eng.oprf_evaluate_batch(mode, inputs[:n], _rows32([scalars[2]]), bool(flags & oh.INVERT), info)
        _check(out, st, want_evaluate(mode, flags), n, 64)
        k1, do, ds = _dev(_rows32([scalars[2]])), _fill((n, 64), 0xAA), _fill((n,), 7)
        assert eng.lib.ncg_oprf_evaluate_batch_dev(eng.h, 0, mode, n, blob.data_ptr(), off.data_ptr(), info, len(info or b""), k1.data_ptr(),
                                                   flags, do.data_ptr(), ds.data_ptr(), None) == OK
        torch.cuda.synchronize()
        _check(do.cpu().numpy(), ds.cpu().numpy(), want_evaluate(mode, flags), n, 64)


def test_evaluate_with_a_scalar_per_row():
    eng = get_engine()
    inputs, scalars, _ = seeded()
    n = 9
    blob, off = _blob_dev(inputs[:n])
    dk, do, ds = _dev(_rows32(scalars[:n])), _fill((n, 64), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_oprf_evaluate_batch_dev(eng.h, 0, 1, n, blob.data_ptr(), off.data_ptr(), None, 0, dk.data_ptr(), oh.INVERT, do.data_ptr(),
                                               ds.data_ptr(), None) == OK
    torch.cuda.synchronize()
    want = [oh.ht_evaluate(1, i, k, oh.INVERT) for i, k in zip(inputs[:n], scalars[:n])]
    _check(do.cpu().numpy(), ds.cpu().numpy(), want, n, 64)
    assert ds.cpu().numpy()[5] == 3


def test_inputs_of_length_0_and_65535():
    eng = get_engine()
    inputs = [b"", oh.seeded_bytes("long", 0, 65535), b"z"]
    ks = [oh.le32(k) for k in (3, L - 2, 2**252 + 1)]
    for mode in (0, 2):
        info = b"" if mode == 2 else None
        out, st = eng.oprf_blind_batch(mode, inputs, _rows32(ks))
        assert [(s, bytes(o)) for s, o in zip(st, out)] == [oh.ht_blind(mode, i, k) for i, k in zip(inputs, ks)]
        out, st = eng.oprf_evaluate_batch(mode, inputs, _rows32(ks[1:2]), False, info)
        assert [(s, bytes(o)) for s, o in zip(st, out)] == [oh.ht_evaluate(mode, i, ks[1], 0, info) for i in inputs]
    assert bytes(out[1]) == oh.evaluate(2, inputs[1], ks[1], False, b"")[1]
    blob, off = oh.blob([bytes(65536)])
    o, s = np.zeros(32, np.uint8), np.zeros(1, np.uint8)
    k = np.frombuffer(ks[0], np.uint8)
    assert eng.lib.ncg_oprf_blind_batch(eng.h, 0, 0, 1, blob, off.ctypes.data, k.ctypes.data, o.ctypes.data, s.ctypes.data) == INVALID


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_blind_evaluate_finalize_equals_evaluate(mode):
    eng = get_engine()
    inputs, scalars, _ = seeded()
    n, info = 66, INFO if mode == 2 else None
    good = [i for i in range(n) if i not in (5, 37)]
    ins, blinds = [inputs[i] for i in good], _rows32([scalars[i] for i in good])
    sk = _rows32([scalars[1]])
    blinded, st = eng.oprf_blind_batch(mode, ins, blinds)
    assert not st.any()
    evaluated, st = eng.oprf_mul_batch(blinded, sk, one_scalar=True, invert=mode == 2)
    assert not st.any()
    out, st = eng.oprf_finalize_batch(mode, ins, blinds, evaluated, info)
    direct, st2 = eng.oprf_evaluate_batch(mode, ins, sk, mode == 2, info)
    assert not st.any() and not st2.any() and np.array_equal(out, direct) and len({bytes(r) for r in out}) == len(good)
    assert bytes(out[0]) == oh.evaluate(mode, ins[0], scalars[1], mode == 2, info)[1]


# ---------------------------------------------------------------- the reference's recorded answers
def _block_key(block):
    mode, info = block["mode"], H(block["info"])
    sk = int.from_bytes(H(block["skS"]), "little")
    return ((sk + oh.poprf_m(info)) % L, True, info) if mode == 2 else (sk, False, None)


def test_fixture_rows_through_the_c_abi():
    eng = get_engine()
    all_inputs = oh.seeded_inputs()
    for block in oh.kat()["modes"]:
        mode = block["mode"]
        scalar, invert, info = _block_key(block)
        for b in block["batches"]:
            ins = [all_inputs[i] for i in b["idx"]]
            blinds = _rows32([H(x) for x in b["blind"]])
            out, st = eng.oprf_blind_batch(mode, ins, blinds)
            assert not st.any() and [bytes(r).hex() for r in out] == b["blinded"]
            ev, st = eng.oprf_mul_batch(out, _rows32([oh.le32(scalar)]), one_scalar=True, invert=invert)
            assert not st.any() and [bytes(r).hex() for r in ev] == b["evaluated"]
            fin, st = eng.oprf_finalize_batch(mode, ins, blinds, ev, info)
            assert not st.any() and [bytes(r).hex() for r in fin] == b["output"]
            fin, st = eng.oprf_evaluate_batch(mode, ins, _rows32([oh.le32(scalar)]), invert, info)
            assert not st.any() and [bytes(r).hex() for r in fin] == b["evaluate"]


def test_hashes_against_fixture_and_twin():
    eng = get_engine()
    k = oh.kat()["seeded"]
    h2s = "".join(k["hash_to_scalar"])
    for mode in (0, 1, 2):
        idx = [i for i in range(64) if i % 3 == mode]
        out = eng.ristretto_hash_to_scalar_batch([oh.seeded_scalar_msg(i) for i in idx], b"HashToScalar-" + oh.ctx_of(mode))
        assert [bytes(r).hex() for r in out] == [h2s[64 * i:64 * i + 64] for i in idx]
    for i in range(64):      # one DST per call: 64 calls of one row, then batches per DST length below
        msg, dst, n = oh.seeded_xmd_row(i)
        assert bytes(eng.xmd_sha512_batch([msg], dst, n)[0]).hex() == k["xmd"][i]
    rng = np.random.RandomState(5)
    for dl, n, out_len in ((1, 65, 1), (40, 129, 65), (255, 64, 256), (17, 2, 128)):
        dst = rng.bytes(dl)
        msgs = [rng.bytes((13 * i) % 300) for i in range(n)]
        want = [oh.ht_xmd(m, dst, out_len) for m in msgs]
        assert [bytes(r) for r in eng.xmd_sha512_batch(msgs, dst, out_len)] == want
        blob, off = _blob_dev(msgs)
        do = _fill((n, out_len), 0xAA)
        assert eng.lib.ncg_xmd_sha512_batch_dev(eng.h, n, blob.data_ptr(), off.data_ptr(), dst, dl, out_len, do.data_ptr(), None) == OK
        torch.cuda.synchronize()
        assert [bytes(r) for r in do.cpu().numpy()] == want
    rows = [c for c in rh.kat()["hash"] if c["dst"] is None][:70]
    out, aff = eng.ristretto_hash_to_group_batch([H(c["msg"]) for c in rows], rh.DEFAULT_DST, want_affine=True)
    assert [bytes(r).hex() for r in out] == [c["out"] for c in rows]
    assert [rh.encode(rh.unwire(a)) for a in aff[:8]] == [bytes(r) for r in out[:8]]
    assert bytes(aff[0]) == oh.ht_hash_to_group(H(rows[0]["msg"]), rh.DEFAULT_DST, affine=True)[1]


def test_device_hash_forms_of_the_ristretto_mirror():
    from noble_curves_amd import ristretto255 as rc
    rows = [c for c in rh.kat()["hash"] if c["dst"] is None][:9]
    msgs = [H(c["msg"]) for c in rows]
    assert [b.hex() for b in rc.hashToCurve_batch(msgs, device_hash=True)] == [c["out"] for c in rows]
    assert rc.hashToCurve(msgs[1], device_hash=True).toBytes().hex() == rows[1]["out"]
    big = b"x" * 300
    assert rc.hashToCurve_batch(msgs[:2], DST=big, device_hash=True) == rc.hashToCurve_batch(msgs[:2], DST=big)
    dst = b"HashToScalar-" + oh.ctx_of(1)
    assert rc.hashToScalar_batch(msgs, DST=dst) == [oh.hash_to_scalar(m, dst) for m in msgs]
    assert rc.hashToScalar(msgs[0], DST=dst) == oh.hash_to_scalar(msgs[0], dst)


# ---------------------------------------------------------------- composites and proofs
@functools.lru_cache(None)
def proof_case(n, mode):
    """n blinded elements C, their evaluations D = k C, the key k and its public key B"""
    rng = np.random.RandomState(1000 + n)
    k = int.from_bytes(rng.bytes(32), "little") % (L - 1) + 1
    base = rh.base_multiples(64)
    C = [rh.encode(base[(5 * i + 1) % 64]) for i in range(n)]
    D = [oh.ht_mul(c, oh.le32(k))[1] for c in C]
    B = oh.ht_mul(rh.encode(rh.BASE), oh.le32(k))[1]
    r = int.from_bytes(rng.bytes(32), "little") % (L - 1) + 1
    return k, B, C, D, r


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_composite_scalars(n):
    eng = get_engine()
    mode = 1 + n % 2
    k, B, C, D, r = proof_case(n, mode)
    want, wst = oh.ht_composite(mode, B, C, D)
    out, st = eng.oprf_composite_scalars_batch(mode, B, _rows32(C), _rows32(D))
    assert [bytes(x) for x in out] == want and list(st) == list(wst) == [0] * n
    if n <= 3:
        assert [int.from_bytes(x, "little") for x in want] == oh.composite_scalars(mode, B, C, D)
    C2, D2 = list(C), list(D)
    C2[0], D2[-1] = bytes(32), b"\x01" + bytes(31)
    want, wst = oh.ht_composite(mode, B, C2, D2)
    dc, dd, do, ds = _dev(_rows32(C2)), _dev(_rows32(D2)), _fill((n, 32), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_oprf_composite_scalars_batch_dev(eng.h, 0, mode, n, B, dc.data_ptr(), dd.data_ptr(), do.data_ptr(), ds.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert [bytes(x) for x in do.cpu().numpy()] == want and list(ds.cpu().numpy()) == list(wst) and wst[0] == 2 and (n == 1 or wst[-1] == 1)


def _flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_generate_then_verify_and_rejections(n):
    eng = get_engine()
    mode = 1 + n % 2
    k, B, C, D, r = proof_case(n, mode)
    proof = eng.oprf_generate_proof(mode, oh.le32(k), B, _rows32(C), _rows32(D), oh.le32(r))
    d, _ = oh.ht_composite(mode, B, C, D)
    M = bytes(eng.ristretto_msm(_rows32(C), _rows32(d)))
    assert oh.ht_proof(mode, oh.le32(k), B, M, oh.le32(r)) == (0, proof)
    if n <= 3:
        assert proof == oh.generate_proof(mode, k, B, C, D, r)
    assert eng.oprf_verify_proof(mode, B, _rows32(C), _rows32(D), proof)
    dc, dd = _dev(_rows32(C)), _dev(_rows32(D))
    out, ok = np.zeros(64, np.uint8), np.zeros(1, np.uint8)
    assert eng.lib.ncg_oprf_generate_proof_dev(eng.h, 0, mode, n, oh.le32(k), B, dc.data_ptr(), dd.data_ptr(), oh.le32(r), out.ctypes.data, None) == OK
    assert out.tobytes() == proof
    assert eng.lib.ncg_oprf_verify_proof_dev(eng.h, 0, mode, n, B, dc.data_ptr(), dd.data_ptr(), proof, ok.ctypes.data, None) == OK and ok[0] == 1
    other = oh.ht_mul(rh.encode(rh.BASE), oh.le32(k + 1 if k + 1 < L else 1))[1]
    bad_c, bad_d = list(C), list(D)
    bad_c[n // 2], bad_d[n // 2] = oh.ht_mul(C[n // 2], oh.le32(2))[1], oh.ht_mul(D[n // 2], oh.le32(3))[1]    # other valid elements
    s_over = proof[:32] + oh.le32(int.from_bytes(proof[32:], "little") + L)
    rejected = [(B, C, D, _flip(proof, 3)), (B, C, D, _flip(proof, 256 + 77)), (B, bad_c, D, proof), (B, C, bad_d, proof), (other, C, D, proof),
                (B, C, D, bytes(64)), (B, C, D, s_over)]
    if n > 1:
        rejected.append((B, C[1:] + C[:1], D, proof))
        rejected.append((B, [C[1], C[0]] + C[2:], [D[1], D[0]] + D[2:], proof))      # two rows swapped together: the index is hashed
    verdicts = set()
    for which in (0, 1):      # one bit of one C_i, then of one D_i: another valid element (rejected) or an undecodable row (the call fails)
        for bit in (1, 9, 100, 200, 255):
            rows = [list(C), list(D)]
            rows[which][n // 2] = _flip(rows[which][n // 2], bit)
            decodes = not isinstance(rh.decode(rows[which][n // 2]), str)
            ca, da = _rows32(rows[0]), _rows32(rows[1])      # named: the arrays must outlive the call that takes their addresses
            rc = eng.lib.ncg_oprf_verify_proof(eng.h, 0, mode, n, B, ca.ctypes.data, da.ctypes.data, proof, ok.ctypes.data)
            assert (rc, ok[0]) == ((OK, 0) if decodes else (INVALID, 0)), (which, bit, decodes)
            verdicts.add(decodes)
    assert False in verdicts      # bit 255 makes s >= p, which never decodes; the other bits decide by the curve
    for b, c, dd_, p in rejected:
        assert int.from_bytes(s_over[32:], "little") >= L
        assert not eng.oprf_verify_proof(mode, b, _rows32(c), _rows32(dd_), p)
    # a flipped bit that leaves an undecodable row fails the call, as ncg_ristretto_msm does
    broken = [b"\x01" + bytes(31)] + C[1:]
    ca, da, cc = _rows32(broken), _rows32(D), _rows32(C)
    assert eng.lib.ncg_oprf_verify_proof(eng.h, 0, mode, n, B, ca.ctypes.data, da.ctypes.data, proof, ok.ctypes.data) == INVALID
    assert b"row 0" in eng.lib.ncg_last_error(eng.h)
    assert eng.lib.ncg_oprf_generate_proof(eng.h, 0, mode, n, oh.le32(0), B, cc.ctypes.data, da.ctypes.data, oh.le32(r),
                                           out.ctypes.data) == INVALID


def test_recorded_proofs():
    eng = get_engine()
    count = 0
    for block in oh.kat()["modes"]:
        if block["mode"] == 0:
            continue
        for b in block["batches"][:4]:
            mode, n = block["mode"], len(b["idx"])
            scalar, _, _ = _block_key(block)
            B = H(block["pkS"]) if mode == 1 else H(b["tweakedKey"])
            C, D = [H(x) for x in b["blinded"]], [H(x) for x in b["evaluated"]]
            if mode == 2:
                C, D = D, C
            r = oh.random_scalar(H(b["rng"])[48 * n:48 * n + 48])
            assert eng.oprf_generate_proof(mode, oh.le32(scalar), B, _rows32(C), _rows32(D), oh.le32(r)).hex() == b["proof"]
            assert eng.oprf_verify_proof(mode, B, _rows32(C), _rows32(D), H(b["proof"]))
            assert not eng.oprf_verify_proof(3 - mode, B, _rows32(C), _rows32(D), H(b["proof"]))
            count += 1
    assert count == 16


# ---------------------------------------------------------------- the pieces, the mirror, the arguments
def test_oprf_check_against_twin():
    eng = get_engine()
    rng = np.random.RandomState(77)
    ks = [1, 2, L - 1, L - 2, 2**252] + [int.from_bytes(rng.bytes(32), "little") % (L - 1) + 1 for _ in range(124)]
    a, b = rh.scalars_le(ks), rh.scalars_le(ks[7:] + ks[:7])
    for op in (0, 1, 4, 5):
        assert np.array_equal(eng.oprf_check(op, 0, a, b), oh.ht_check(op, 0, a, b)), op
    pts = rh.wire([rh.add(rh.base_multiples(64)[i % 64], rh.TORSION4[i % 4]) for i in range(129)])
    assert np.array_equal(eng.oprf_check(2, 0, pts, a), oh.ht_check(2, 0, pts, a))
    msgs = np.frombuffer(rng.bytes(32 * 65), np.uint8).reshape(65, 32)
    dstp = np.zeros((65, 32), np.uint8)
    dstp[:, :20] = np.frombuffer(b"oprf-check-DST-test" + bytes([19]), np.uint8)
    got = eng.oprf_check(3, 20, msgs, dstp)
    assert np.array_equal(got, oh.ht_check(3, 20, msgs, dstp))
    assert bytes(got[0]) == rh.expand_message_xmd(bytes(msgs[0]), b"oprf-check-DST-test", 64)
    with pytest.raises(RuntimeError):
        eng.oprf_check(3, 1, msgs, dstp)
    assert not eng.oprf_check(9, 0, a, b).any()


def _replay(data):
    at = [0]

    def rng(n):
        out = data[at[0]:at[0] + n]
        at[0] += n
        assert len(out) == n
        return out
    return rng


def test_mirror_reproduces_the_reference():
    from noble_curves_amd.oprf import ristretto255_oprf as O
    k = oh.kat()
    all_inputs = oh.seeded_inputs()
    for block in k["modes"]:
        mode = block["mode"]
        S = O.oprf if mode == 0 else O.voprf if mode == 1 else O.poprf(H(block["info"]))
        keys = S.deriveKeyPair(H(k["seed"]), H(k["key_info"]))
        assert (keys["secretKey"].hex(), keys["publicKey"].hex()) == (block["skS"], block["pkS"])
        sk, pk = keys["secretKey"], keys["publicKey"]
        for b in block["batches"][:5]:
            ins, rng = [all_inputs[i] for i in b["idx"]], _replay(H(b["rng"]))
            if mode == 2:
                blinds, blinded, tw = S.blind_batch(ins, pk, rng)
                assert tw.hex() == b["tweakedKey"]
            else:
                blinds, blinded = S.blind_batch(ins, rng)
            assert [x.hex() for x in blinds] == b["blind"] and [x.hex() for x in blinded] == b["blinded"]
            items = [{"input": i, "blind": bl, "blinded": bd} for i, bl, bd in zip(ins, blinds, blinded)]
            if mode == 0:
                ev = S.blindEvaluate_batch(sk, blinded)
                assert S.finalize_batch(ins, blinds, ev) == [H(x) for x in b["output"]]
            else:
                res = S.blindEvaluateBatch(sk, pk, blinded, rng) if mode == 1 else S.blindEvaluateBatch(sk, blinded, rng)
                ev = res["evaluated"]
                assert res["proof"].hex() == b["proof"]
                for it, e in zip(items, ev):
                    it["evaluated"] = e
                out = S.finalizeBatch(items, pk, res["proof"]) if mode == 1 else S.finalizeBatch(items, res["proof"], tw)
                assert out == [H(x) for x in b["output"]]
                with pytest.raises(ValueError, match="proof verification failed"):
                    S.finalizeBatch(items, pk, bytes(64)) if mode == 1 else S.finalizeBatch(items, bytes(64), tw)
            assert [x.hex() for x in ev] == b["evaluated"]
            assert S.evaluate_batch(sk, ins) == [H(x) for x in b["evaluate"]]
        b = block["batches"][0]
        i0 = all_inputs[b["idx"][0]]
        assert S.evaluate(sk, i0).hex() == b["evaluate"][0]


def test_mirror_generate_key_pair_and_round_trip():
    from noble_curves_amd.oprf import ristretto255_oprf as O
    for S, mode in ((O.oprf, 0), (O.voprf, 1), (O.poprf(b"info"), 2)):
        keys = S.generateKeyPair()
        sk = int.from_bytes(keys["secretKey"], "little")
        assert 0 < sk < L and keys["publicKey"] == rh.encode(rh.mul(rh.BASE, sk))
    keys = O.voprf.generateKeyPair()
    assert keys["secretKey"] != O.voprf.generateKeyPair()["secretKey"]
    inputs = [b"", b"round trip", bytes(range(70))]
    blinds, blinded = O.voprf.blind_batch(inputs)
    res = O.voprf.blindEvaluateBatch(keys["secretKey"], keys["publicKey"], blinded)
    items = [{"input": i, "blind": bl, "blinded": bd, "evaluated": e} for i, bl, bd, e in zip(inputs, blinds, blinded, res["evaluated"])]
    out = O.voprf.finalizeBatch(items, keys["publicKey"], res["proof"])
    assert out == O.voprf.evaluate_batch(keys["secretKey"], inputs) and out[1] == oh.evaluate(1, inputs[1], keys["secretKey"])[1]
    other = O.voprf.generateKeyPair()
    with pytest.raises(ValueError, match="proof verification failed"):
        O.voprf.finalizeBatch(items, other["publicKey"], res["proof"])


def test_mirror_reports_the_first_refused_row():
    from noble_curves_amd.oprf import ristretto255_oprf as O
    good, bad = rh.encode(rh.BASE), b"\x01" + bytes(31)
    with pytest.raises(ValueError, match="invalid ristretto255 encoding 1"):      # the undecodable row comes before the zero blind
        O.oprf.finalize_batch([b"a", b"b", b"c"], [oh.le32(5), oh.le32(5), oh.le32(0)], [good, bad, good])
    with pytest.raises(ValueError, match="invert: expected non-zero number"):
        O.oprf.finalize_batch([b"a", b"b", b"c"], [oh.le32(5), oh.le32(0), oh.le32(5)], [good, good, bad])


def test_mirror_messages():
    from noble_curves_amd.oprf import ristretto255_oprf as O
    k = oh.kat()
    err, ei = k["errors"], {n: H(v) for n, v in k["error_inputs"].items()}
    V, P2 = O.voprf, O.poprf(bytes(3))
    zero, bad = bytes(32), b"\x01" * 32
    cases = [("blind_zero", lambda: O.oprf.finalize(b"\x00", zero, ei["blinded"])),
             ("blind_order", lambda: O.oprf.finalize(b"\x00", oh.le32(L), ei["blinded"])),
             ("secret_zero", lambda: O.oprf.blindEvaluate(zero, ei["blinded"])),
             ("bad_encoding", lambda: O.oprf.blindEvaluate(ei["skS"], bad)),
             ("identity_blinded", lambda: O.oprf.blindEvaluate(ei["skS"], zero)),
             ("identity_evaluated", lambda: O.oprf.finalize(b"\x00", ei["blind"], zero)),
             ("identity_public_key", lambda: V.blindEvaluate(ei["skS"], zero, ei["blinded"])),
             ("identity_tweaked_key", lambda: P2.finalize(b"\x00", ei["blind"], ei["evaluated"], ei["blinded"], ei["proof"], zero)),
             ("proof_length", lambda: V.finalize(b"\x00", ei["blind"], ei["evaluated"], ei["blinded"], ei["pkS"], bytes(63))),
             ("proof_ff", lambda: V.finalize(b"\x00", ei["blind"], ei["evaluated"], ei["blinded"], ei["pkS"], b"\xff" * 64)),
             ("proof_zero", lambda: V.finalize(b"\x00", ei["blind"], ei["evaluated"], ei["blinded"], ei["pkS"], bytes(64))),
             ("expected_array", lambda: V.blindEvaluateBatch(ei["skS"], ei["pkS"], ei["blinded"]))]
    for name, f in cases:
        with pytest.raises(ValueError) as e:
            f()
        assert str(e.value) == err[name], name
    assert V.finalize(b"\x00", ei["blind"], ei["evaluated"], ei["blinded"], ei["pkS"], ei["proof"]) == \
        oh.finalize(1, b"\x00", ei["blind"], ei["evaluated"])[1]


def test_argument_table():
    """n = 1 and every non-NULL pointer a zeroed 4 KB buffer (device buffers for the _dev forms), so that a check that went missing
    runs on valid memory and fails the test instead of faulting; the rows with an oversize count or length pass every pointer as
    NULL (dst, at most 255 bytes, excepted), since they are refused before any buffer is looked at"""
    eng = get_engine()
    lib, h = eng.lib, eng.h
    hb = np.zeros(4096, np.uint8)
    db = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    Hp, Dp = hb.ctypes.data, db.data_ptr()
    BIG = 0x7fffffff - 254          # one above the largest batch

    def err():
        return lib.ncg_last_error(h) or b""

    for X, dev in ((Hp, False), (Dp, True)):
        tail = (None,) if dev else ()
        sfx = "_dev" if dev else ""
        f = lambda name: getattr(lib, name + sfx)  # noqa: E731
        rows = [
            ("suite", UNSUPPORTED, b"unsupported suite", lambda: f("ncg_oprf_blind_batch")(h, 1, 0, 1, X, X, X, X, X, *tail)),
            ("suite", UNSUPPORTED, b"unsupported suite", lambda: f("ncg_oprf_mul_batch")(h, 7, 1, X, X, 0, X, X, *tail)),
            ("suite", UNSUPPORTED, b"unsupported suite", lambda: f("ncg_oprf_finalize_batch")(h, -1, 0, 1, X, X, None, 0, X, X, X, X, *tail)),
            ("suite", UNSUPPORTED, b"unsupported suite", lambda: f("ncg_oprf_evaluate_batch")(h, 1, 0, 1, X, X, None, 0, X, 1, X, X, *tail)),
            ("suite", UNSUPPORTED, b"unsupported suite", lambda: f("ncg_oprf_composite_scalars_batch")(h, 1, 1, 1, Hp, X, X, X, X, *tail)),
            ("suite", UNSUPPORTED, b"unsupported suite", lambda: f("ncg_oprf_generate_proof")(h, 1, 1, 1, Hp, Hp, X, X, Hp, Hp, *tail)),
            ("suite", UNSUPPORTED, b"unsupported suite", lambda: f("ncg_oprf_verify_proof")(h, 1, 1, 1, Hp, X, X, Hp, Hp, *tail)),
            ("mode", INVALID, b"mode 3", lambda: f("ncg_oprf_blind_batch")(h, 0, 3, 1, X, X, X, X, X, *tail)),
            ("mode", INVALID, b"mode -1", lambda: f("ncg_oprf_evaluate_batch")(h, 0, -1, 1, X, X, None, 0, X, 1, X, X, *tail)),
            ("flags", INVALID, b"unknown flag bits 0x4", lambda: f("ncg_oprf_mul_batch")(h, 0, 1, X, X, 4, X, X, *tail)),
            ("flags", INVALID, b"unknown flag bits 0x8", lambda: f("ncg_oprf_evaluate_batch")(h, 0, 0, 1, X, X, None, 0, X, 8, X, X, *tail)),
            ("info", INVALID, b"info is read only in mode 2", lambda: f("ncg_oprf_finalize_batch")(h, 0, 1, 1, X, X, Hp, 0, X, X, X, X, *tail)),
            ("info", INVALID, b"info is read only in mode 2", lambda: f("ncg_oprf_evaluate_batch")(h, 0, 0, 1, X, X, None, 3, X, 1, X, X, *tail)),
            ("info", INVALID, b"NULL buffer (info)", lambda: f("ncg_oprf_finalize_batch")(h, 0, 2, 1, X, X, None, 3, X, X, X, X, *tail)),
            ("info", INVALID, b"above 65535", lambda: f("ncg_oprf_finalize_batch")(h, 0, 2, 1, None, None, None, 65536, None, None, None, None, *tail)),
            ("rows", INVALID, b"must fit 16 bits", lambda: f("ncg_oprf_composite_scalars_batch")(h, 0, 1, 65536, None, None, None, None, None, *tail)),
            ("rows", INVALID, b"must fit 16 bits", lambda: f("ncg_oprf_generate_proof")(h, 0, 1, 65536, None, None, None, None, None, None, *tail)),
            ("rows", INVALID, b"must fit 16 bits", lambda: f("ncg_oprf_verify_proof")(h, 0, 1, 65536, None, None, None, None, None, *tail)),
            # an oversize count is refused before any buffer is looked at: every pointer NULL
            ("large", INVALID, b"batch too large", lambda: f("ncg_oprf_mul_batch")(h, 0, BIG, None, None, 0, None, None, *tail)),
            ("large", INVALID, b"batch too large", lambda: f("ncg_oprf_blind_batch")(h, 0, 0, BIG, None, None, None, None, None, *tail)),
            ("large", INVALID, b"batch too large", lambda: f("ncg_xmd_sha512_batch")(h, BIG, None, None, Hp, 4, 64, None, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_blind_batch")(h, 0, 0, 1, X, X, None, X, X, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_blind_batch")(h, 0, 0, 1, X, X, X, X, None, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_mul_batch")(h, 0, 1, None, X, 0, X, X, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_mul_batch")(h, 0, 1, X, X, 0, None, X, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_finalize_batch")(h, 0, 0, 1, X, X, None, 0, X, None, X, X, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_evaluate_batch")(h, 0, 0, 1, X, X, None, 0, None, 1, X, X, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_composite_scalars_batch")(h, 0, 1, 1, None, X, X, X, X, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_generate_proof")(h, 0, 1, 1, None, Hp, X, X, Hp, Hp, *tail)),
            ("null", INVALID, b"NULL buffer", lambda: f("ncg_oprf_verify_proof")(h, 0, 1, 1, Hp, X, X, Hp, None, *tail)),
            ("dst", INVALID, b"dst_len 0 outside", lambda: f("ncg_xmd_sha512_batch")(h, 1, X, X, Hp, 0, 64, X, *tail)),
            ("dst", INVALID, b"dst_len 256 outside", lambda: f("ncg_ristretto_hash_to_group_batch")(h, 1, X, X, Hp, 256, X, None, *tail)),
            ("dst", INVALID, b"NULL buffer (dst)", lambda: f("ncg_ristretto_hash_to_scalar_batch")(h, 1, X, X, None, 5, X, *tail)),
            ("out_len", INVALID, b"out_len 0 outside", lambda: f("ncg_xmd_sha512_batch")(h, 1, X, X, Hp, 4, 0, X, *tail)),
            ("out_len", INVALID, b"out_len 257 outside", lambda: f("ncg_xmd_sha512_batch")(h, 1, X, X, Hp, 4, 257, X, *tail)),
            ("ctx", INVALID, b"ctx is NULL", lambda: f("ncg_oprf_mul_batch")(None, 0, 1, X, X, 0, X, X, *tail)),
            # zero rows: an identity element, a zero scalar, a zero public key - refused row by row or as a whole, never faulting
            ("zero key", INVALID, b"public key is the identity", lambda: f("ncg_oprf_verify_proof")(h, 0, 1, 1, Hp, X, X, Hp, Hp, *tail)),
            ("zero k", INVALID, b"must be below L and not zero", lambda: f("ncg_oprf_generate_proof")(h, 0, 1, 1, Hp, Hp, X, X, Hp, Hp, *tail)),
        ]
        if dev:
            rows.append(("align", INVALID, b"4-byte aligned", lambda: lib.ncg_oprf_mul_batch_dev(h, 0, 1, Dp, Dp + 2, 0, Dp, Dp, None)))
            rows.append(("align", INVALID, b"4-byte aligned", lambda: lib.ncg_oprf_blind_batch_dev(h, 0, 0, 1, Dp, Dp, Dp + 1, Dp, Dp, None)))
        for label, status, sub, call in rows:
            hb[:] = 0
            db.zero_()
            rc = call()
            assert rc == status and sub in (lib.ncg_last_error(None) if label == "ctx" else err()), (label, dev, rc, err())
        # what passes every check on zeroed rows: status bytes, not an error
        hb[:] = 0
        db.zero_()
        assert f("ncg_oprf_mul_batch")(h, 0, 1, X, X + 64, 0, X + 128, X + 256, *tail) == OK
        torch.cuda.synchronize()
        assert (db.cpu().numpy() if dev else hb)[256] == 2
        assert f("ncg_oprf_mul_batch")(h, 0, 0, None, None, 0, None, None, *tail) == OK           # n = 0 touches nothing
    assert lib.ncg_oprf_check(h, 0, 0, (1 << 24) + 1, None, None, None) == INVALID and b"too large" in err()
