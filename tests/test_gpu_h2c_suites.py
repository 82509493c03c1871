"""RFC 9380 for secp256k1 and edwards25519 ON THE DEVICE: ncg_h2c_{hash,map,hash_to_field,hash_to_scalar}_batch, ncg_xmd_sha256_batch
(host and _dev forms on the same bytes) and ncg_h2c_check, against the reference's recorded answers
(tests/golden/h2c_suites_kat.json), hashlib and the CPU twin of the same lane code - bit for bit, no tolerances.  The hashed points
then go unchanged into ncg_mul_var_batch and ncg_msm of the same curve."""
import hashlib

import numpy as np
import pytest
import torch

import h2c_suites_helpers as hh
from helpers import points_to_wire, scalars_to_wire, wire_to_affine
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -4
SUITE_NAMES = sorted(hh.SUITES)
SIZES = [1, 63, 64, 65, 257]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _fill(shape, v):
    return torch.full(shape, v, dtype=torch.uint8, device="cuda")


def _blob_dev(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return _dev(np.frombuffer(b"".join(msgs) + b"\0", np.uint8)), _dev(off)


def _pts(out, inf):
    return [(int.from_bytes(bytes(r[:32]), "little"), int.from_bytes(bytes(r[32:]), "little"), int(f)) for r, f in zip(out, inf)]


def _want(row):
    return int(row["x"], 16), int(row["y"], 16), row["inf"]


def _hash_both(suite, msgs, dst, count):
    """ncg_h2c_hash_batch and ncg_h2c_hash_batch_dev on the same bytes; the rows of the host form"""
    eng, sid, n = get_engine(), hh.SUITES[suite]["id"], len(msgs)
    out, inf = eng.h2c_hash_batch(sid, msgs, dst, count)
    blob, off = _blob_dev(msgs)
    do, df = _fill((n, 64), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_h2c_hash_batch_dev(eng.h, sid, n, count, blob.data_ptr(), off.data_ptr(), dst, len(dst), do.data_ptr(), df.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(do.cpu().numpy(), out) and np.array_equal(df.cpu().numpy(), inf)
    return _pts(out, inf)


def _map_both(suite, us, count):
    eng, sid = get_engine(), hh.SUITES[suite]["id"]
    u48 = np.frombuffer(b"".join(int(u).to_bytes(48, "little") for u in us), np.uint8).reshape(-1, 48 * count).copy()
    n = u48.shape[0]
    out, inf = eng.h2c_map_batch(sid, u48, count)
    du, do, df = _dev(u48), _fill((n, 64), 0xAA), _fill((n,), 7)
    assert eng.lib.ncg_h2c_map_batch_dev(eng.h, sid, n, count, du.data_ptr(), do.data_ptr(), df.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(do.cpu().numpy(), out) and np.array_equal(df.cpu().numpy(), inf)
    return _pts(out, inf)


def _groups(rows):
    """listed rows grouped by (dst, count): one call each"""
    g = {}
    for i, (_, msg, dst, count) in enumerate(rows):
        g.setdefault((dst, count), []).append(i)
    return g


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_fixture_rows_hash_and_hash_to_field(suite):
    eng, sid = get_engine(), hh.SUITES[suite]["id"]
    listed, rows = hh.listed_rows(suite), hh.kat()[suite]["hash"]
    groups = _groups(listed)
    # the default hashToCurve group mixes an empty message, the block-boundary lengths and the 1000-byte message in one batch
    lens = {len(listed[i][1]) for i in groups[(hh.SUITES[suite]["ro"], 2)]}
    assert {0, 3, 1000} <= lens and set(hh.boundary_lengths(suite)) <= lens
    for (dst, count), idx in groups.items():
        msgs, d = [listed[i][1] for i in idx], hh.effective_dst(suite, dst)
        assert _hash_both(suite, msgs, d, count) == [_want(rows[i]) for i in idx], (dst, count)
        u = eng.h2c_hash_to_field_batch(sid, msgs, d, count)
        assert [[int.from_bytes(bytes(r[32 * j:32 * j + 32]), "little") for j in range(count)] for r in u] == \
            [[int(v, 16) for v in rows[i]["u"]] for i in idx], (dst, count)
        blob, off = _blob_dev(msgs)
        du = _fill((len(msgs), 32 * count), 0xAA)
        assert eng.lib.ncg_h2c_hash_to_field_batch_dev(eng.h, sid, len(msgs), count, blob.data_ptr(), off.data_ptr(), d, len(d), du.data_ptr(), None) == OK
        torch.cuda.synchronize()
        assert np.array_equal(du.cpu().numpy(), u)
        # the map half on its own: the fixture's u through ncg_h2c_map_batch
        us = [int(v, 16) for i in idx for v in rows[i]["u"]]
        assert _map_both(suite, us, count) == [_want(rows[i]) for i in idx], (dst, count)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_seeded_rows_in_batches(suite, n):
    """partial waves (1, 63, 65) and a second block of every kernel (257: blocks of 64 and of 256); rows repeat beyond the family"""
    want = hh.seeded_answers(suite)
    by_kind = {}
    for i in range(hh.SEEDED):
        row = hh.seeded_row(suite, i)
        if i % 4 != 2:
            by_kind.setdefault(i % 4, []).append((row, want[i]))
    for kind, rows in by_kind.items():
        take = [rows[(7 * j) % len(rows)] for j in range(n)]
        if kind == 3:
            got = _map_both(suite, [u for r, _ in take for u in (r[1], r[2])], 2)
        else:
            got = _hash_both(suite, [r[1] for r, _ in take], take[0][0][2], take[0][0][3])
        assert got == [w for _, w in take], (kind, n)


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_seeded_rows_with_their_own_dst(suite):
    want = hh.seeded_answers(suite)
    eng, sid = get_engine(), hh.SUITES[suite]["id"]
    dst_lens = set()
    for i in range(2, hh.SEEDED, 4):
        _, msg, dst, count = hh.seeded_row(suite, i)
        dst_lens.add(len(dst))
        assert _pts(*eng.h2c_hash_batch(sid, [msg], dst, count)) == [want[i]], i
    assert min(dst_lens) < 16 and max(dst_lens) > 200


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_map_edges_exceptions_and_pairs(suite):
    k, s = hh.kat()[suite], hh.SUITES[suite]
    rows = k["map"] + k["exceptions"]
    got = _map_both(suite, [int(r["u"]) for r in rows], 1)
    assert got == [_want(r) for r in rows]
    zero = [g for g in got if g[2]]
    assert all(g[:2] == s["zero"] for g in zero) and (len(zero) == 2) == (suite == "ed25519")     # ZERO in the curve's wire form
    pairs = k["pairs"]
    got = _map_both(suite, [int(v) for r in pairs for v in (r["u0"], r["u1"])], 2)
    assert got == [_want(r) for r in pairs]
    if suite == "secp256k1":      # (u, -u) cancels: ZERO, flagged, as (0, 0); (u, u) is a doubling
        assert len(k["exceptions"]) == 2 and got[1] == got[3] == (0, 0, 1) and got[0][2] == 0


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_hash_to_scalar(suite):
    eng, sid = get_engine(), hh.SUITES[suite]["id"]
    rows, answers = hh.scalar_rows(suite), hh.kat()[suite]["scalar"]
    default = [i for i, r in enumerate(rows) if r[2] is None]
    msgs = [rows[i][1] for i in default]
    out = eng.h2c_hash_to_scalar_batch(sid, msgs, hh.SCALAR_DST)
    assert [bytes(r)[::-1].hex() for r in out] == [answers[i]["out"] for i in default]
    blob, off = _blob_dev(msgs)
    do = _fill((len(msgs), 32), 0xAA)
    assert eng.lib.ncg_h2c_hash_to_scalar_batch_dev(eng.h, sid, len(msgs), blob.data_ptr(), off.data_ptr(), hh.SCALAR_DST, len(hh.SCALAR_DST),
                                                    do.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(do.cpu().numpy(), out)
    for i, (name, msg, dst) in enumerate(rows):
        if dst is not None:
            assert bytes(eng.h2c_hash_to_scalar_batch(sid, [msg], dst)[0])[::-1].hex() == answers[i]["out"], name
    # a batch across two blocks against hashlib
    many = [hh.seeded_bytes("scalar-" + suite, i, 5 * i % 140) for i in range(257)]
    out = eng.h2c_hash_to_scalar_batch(sid, many, b"many")
    assert [int.from_bytes(bytes(r), "little") for r in out] == [hh.hash_to_field(suite, m, b"many", 1, modulus=hh.SUITES[suite]["n"])[0] for m in many]


@pytest.mark.parametrize("out_len", [1, 32, 33, 48, 96, 256])
def test_xmd_sha256_against_hashlib(out_len):
    eng = get_engine()
    msgs = [b"", b"abc", b"q" * 133, hh.seeded_bytes("xmd", 0, 1000)] + [hh.seeded_bytes("xmd", n, n % 120) for n in range(257)]
    for dst in (b"D", b"QUUX-V01-CS02-with-expander-SHA256-128", b"y" * 255):
        out = eng.xmd_sha256_batch(msgs, dst, out_len)
        assert [bytes(r) for r in out] == [hh.xmd(m, dst, out_len, hashlib.sha256) for m in msgs], len(dst)
    blob, off = _blob_dev(msgs)
    do = _fill((len(msgs), out_len), 0xAA)
    assert eng.lib.ncg_xmd_sha256_batch_dev(eng.h, len(msgs), blob.data_ptr(), off.data_ptr(), b"y" * 255, 255, out_len, do.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(do.cpu().numpy(), out)


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_hashed_points_feed_the_multiply_and_the_msm(suite):
    from oracle import curve as OC
    from oracle.curves import Ed25519, Secp256k1
    eng, s = get_engine(), hh.SUITES[suite]
    C, curve, sid = (Secp256k1 if suite == "secp256k1" else Ed25519), s["curve"], s["id"]
    want = hh.seeded_answers(suite)
    idx = [i for i in range(hh.SEEDED) if i % 4 == 0] * 2                       # 64 rows of hashToCurve under the default DST
    msgs = [hh.seeded_row(suite, i)[1] for i in idx]
    ks = [int.from_bytes(hh.seeded_bytes("k-" + suite, j, 32), "big") % s["n"] for j in range(64)]
    ks[3] = 0
    blob, off = _blob_dev(msgs)
    dp, df = _fill((64, 64), 0xAA), _fill((64,), 7)
    assert eng.lib.ncg_h2c_hash_batch_dev(eng.h, sid, 64, 2, blob.data_ptr(), off.data_ptr(), s["ro"], len(s["ro"]), dp.data_ptr(), df.data_ptr(), None) == OK
    dk, do, dinf = _dev(scalars_to_wire(ks)), _fill((64, 64), 0), _fill((64,), 0)
    eng.mul_var_batch_dev(curve, 64, dp.data_ptr(), dk.data_ptr(), do.data_ptr(), dinf.data_ptr())      # the hash's output, unchanged
    torch.cuda.synchronize()
    pts = [C.fromAffine(want[i][:2]) for i in idx]
    prod = [p.multiplyUnsafe(k) for p, k in zip(pts, ks)]
    assert np.array_equal(do.cpu().numpy(), points_to_wire(curve, prod))
    assert list(dinf.cpu().numpy()) == [1 if k == 0 else 0 for k in ks]
    got, got_inf = eng.msm_dev(curve, 64, dp.data_ptr(), dk.data_ptr())
    assert wire_to_affine(curve, got) == OC.pippenger(C, pts, ks).toAffine() and not got_inf
    # and through the host forms and the encoder
    out, inf = eng.h2c_hash_batch(sid, msgs, s["ro"], 2)
    assert np.array_equal(out, dp.cpu().numpy()) and not inf.any()
    assert np.array_equal(eng.mul_var_batch(curve, out, scalars_to_wire(ks))[0], points_to_wire(curve, prod))


@pytest.mark.parametrize("op", range(7))
def test_check_pieces_match_the_twin(op):
    eng = get_engine()
    rng = np.random.RandomState(9380 + op)
    vals = [0, 1, hh.SECP_P - 1, hh.SECP_P, hh.ED_P, 2**256 - 1, 2**384 - 1] + list(hh.exception_us("secp256k1").values())
    rows = [hh.check_row([(v, 12)]) for v in vals] + [np.frombuffer(rng.bytes(96), np.uint32) for _ in range(70 - len(vals))]
    if op == 5:      # two canonical coordinates
        rows = [hh.check_row([(int.from_bytes(r.tobytes()[:32], "little") % hh.SECP_P, 8), (int.from_bytes(r.tobytes()[32:64], "little") % hh.SECP_P, 8)])
                for r in rows]
    a = np.stack(rows)
    got = eng.h2c_check(op, a)
    for i in range(a.shape[0]):
        rc, want = hh.ht_check(op, a[i])
        assert rc == 0 and hh.words_to_ints(got[i]) == want, (op, i)
    assert not eng.h2c_check(7, a).any() and not eng.h2c_check(-1, a).any()      # an op nobody defines leaves out zero


def test_argument_checks_leave_the_context_usable():
    eng = get_engine()
    L, h = eng.lib, eng.h
    H = np.zeros(4096, np.uint8)
    off = np.array([0, 3], np.uint64)
    hp, op_ = H.ctypes.data, off.ctypes.data
    fl = hp + 2048
    D = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    doff = _dev(off)
    dp = D.data_ptr()
    dfl = dp + 2048

    def err():
        return (L.ncg_last_error(h) or b"").decode()
    for suite in (2, -1, 7):
        assert L.ncg_h2c_hash_batch(h, suite, 1, 2, hp, op_, b"D", 1, hp, fl) == UNSUPPORTED and "unsupported suite %d" % suite in err()
        assert L.ncg_h2c_map_batch(h, suite, 1, 1, hp, hp, fl) == UNSUPPORTED
        assert L.ncg_h2c_hash_to_scalar_batch(h, suite, 1, hp, op_, b"D", 1, hp) == UNSUPPORTED
        assert L.ncg_h2c_hash_to_field_batch_dev(h, suite, 1, 1, dp, doff.data_ptr(), b"D", 1, dp, None) == UNSUPPORTED
    for sid in (0, 1):
        for count in (0, 3, -1):
            assert L.ncg_h2c_hash_batch(h, sid, 1, count, hp, op_, b"D", 1, hp, fl) == INVALID and "count must be 1 or 2" in err()
            assert L.ncg_h2c_map_batch_dev(h, sid, 1, count, dp, dp, dfl, None) == INVALID and "count must be 1 or 2" in err()
            assert L.ncg_h2c_hash_to_field_batch(h, sid, 1, count, hp, op_, b"D", 1, hp) == INVALID
        for dl in (0, 256):
            assert L.ncg_h2c_hash_batch(h, sid, 1, 2, hp, op_, b"D" * 256, dl, hp, fl) == INVALID and "dst_len %d outside 1..255" % dl in err()
            assert L.ncg_h2c_hash_to_scalar_batch_dev(h, sid, 1, dp, doff.data_ptr(), b"D" * 256, dl, dp, None) == INVALID
            assert L.ncg_xmd_sha256_batch(h, 1, hp, op_, b"D" * 256, dl, 32, hp) == INVALID
        assert L.ncg_h2c_hash_batch(h, sid, 1, 2, hp, op_, None, 1, hp, fl) == INVALID and "NULL buffer" in err()
        assert L.ncg_h2c_hash_batch(h, sid, 1, 2, hp, op_, b"D", 1, None, fl) == INVALID and "NULL buffer" in err()
        assert L.ncg_h2c_hash_batch(h, sid, 1, 2, hp, op_, b"D", 1, hp, None) == INVALID
        assert L.ncg_h2c_hash_batch(h, sid, 1, 2, hp, None, b"D", 1, hp, fl) == INVALID
        assert L.ncg_h2c_hash_batch(h, sid, 1, 2, None, op_, b"D", 1, hp, fl) == INVALID and "NULL message buffer" in err()
        assert L.ncg_h2c_map_batch(h, sid, 1, 1, None, hp, fl) == INVALID and L.ncg_h2c_map_batch(h, sid, 1, 1, hp, None, fl) == INVALID
        assert L.ncg_h2c_map_batch_dev(h, sid, 1, 1, dp, dp, None, None) == INVALID
        assert L.ncg_h2c_hash_to_scalar_batch(h, sid, 1, hp, op_, b"D", 1, None) == INVALID
        assert L.ncg_h2c_hash_to_field_batch_dev(h, sid, 1, 2, dp, doff.data_ptr(), b"D", 1, None, None) == INVALID
        assert L.ncg_h2c_map_batch_dev(h, sid, 1, 1, dp + 1, dp, dfl, None) == INVALID and "4-byte aligned" in err()
        big = (1 << 31) - 255
        assert L.ncg_h2c_hash_batch_dev(h, sid, big, 2, dp, doff.data_ptr(), b"D", 1, dp, dfl, None) == INVALID and "batch too large" in err()
        assert L.ncg_h2c_map_batch_dev(h, sid, big, 1, dp, dp, dfl, None) == INVALID and "batch too large" in err()
        # n = 0 succeeds and touches nothing, whatever else is passed
        assert L.ncg_h2c_hash_batch(h, sid, 0, 2, None, None, b"D", 1, None, None) == OK
        assert L.ncg_h2c_map_batch_dev(h, sid, 0, 1, None, None, None, None) == OK
        assert L.ncg_h2c_hash_to_scalar_batch(h, sid, 0, None, None, b"D", 1, None) == OK
    assert L.ncg_xmd_sha256_batch(h, 1, hp, op_, b"D", 1, 0, hp) == INVALID and L.ncg_xmd_sha256_batch(h, 1, hp, op_, b"D", 1, 257, hp) == INVALID
    assert L.ncg_xmd_sha256_batch(h, 0, None, None, b"D", 1, 32, None) == OK
    assert L.ncg_h2c_check(h, 0, (1 << 24) + 1, hp, hp) == INVALID and L.ncg_h2c_check(h, 0, 1, None, hp) == INVALID
    assert L.ncg_h2c_hash_batch(None, 0, 1, 2, hp, op_, b"D", 1, hp, fl) == INVALID
    assert not H.any() and not D.cpu().numpy().any()                           # no refused call wrote anything
    # the context still works
    k = hh.kat()["secp256k1"]["hash"]
    row = {r["name"]: r for r in k}["abc/rfc/ro"]
    assert _pts(*eng.h2c_hash_batch(0, [b"abc"], b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_", 2)) == [_want(row)]


@pytest.mark.parametrize("suite", SUITE_NAMES)
def test_python_hashers_on_the_device(suite):
    from noble_curves_amd import h2c as GH
    h = GH.secp256k1_hasher if suite == "secp256k1" else GH.ed25519_hasher
    k = hh.kat()[suite]
    rows = {r["name"]: r for r in k["hash"]}
    assert h.hashToCurve(b"abc").toAffine() == _want(rows["abc/default/ro"])[:2]
    assert h.encodeToCurve(b"abc").toAffine() == _want(rows["abc/default/nu"])[:2]
    assert h.hashToCurve(b"abc", {"DST": b"x" * 300}).toAffine() == _want(rows["dst300"])[:2]
    assert [p.toAffine() for p in h.hashToCurveBatch([m for _, m in hh.MESSAGES])] == [_want(rows[n + "/default/ro"])[:2] for n, _ in hh.MESSAGES]
    assert h.hashToScalar(b"abc") == int(k["scalar"][1]["out"], 16)
    assert [p.toAffine() for p in h.mapToCurveBatch([int(r["u"]) for r in k["map"]])] == [_want(r)[:2] for r in k["map"]]
    assert h.mapToCurve(0).equals(h.Point.ZERO) == bool(k["map"][0]["inf"])
