"""RFC 9380 for edwards448 and the hash side of decaf448 ON THE DEVICE: ncg_xof_shake256_batch, the ncg_ed448_h2c_* entry points,
ncg_decaf448_hash_to_group_batch / _hash_to_scalar_batch (host and _dev forms) and ncg_h2c448_check, against the reference's own
answers (tests/golden/h2c448_kat.json), the Python restatement of h2c448_helpers and the CPU twin, bit for bit.  Every case runs at n
in {1, 64, 65, 299}: rows are built once and cycled to n, and a cycled row must give the same answer in every lane."""
import numpy as np
import pytest
import torch

import h2c448_helpers as hh
from noble_curves_amd import decaf448 as GD
from noble_curves_amd import ed448 as GE
from noble_curves_amd import get_engine

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
SIZES = [1, 64, 65, 299]
P, N = hh.P, hh.N
_cache = {}


def once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def err():
    eng = get_engine()
    return (eng.lib.ncg_last_error(eng.h) or b"").decode()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _odd(a):
    """the same bytes at an odd host address"""
    raw = np.empty(a.nbytes + 1, np.uint8)
    raw[1:] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return raw[1:]


def _blob(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) + b"\0", np.uint8)[:-1].copy(), off


def both_msgs(fn, msgs, dst, pre, post, width):
    """fn (host form, the message blob at an odd address) and fn_dev on the same rows: (ctx, n, *pre, msgs, off, dst, dst_len, *post,
    out[, stream]).  Both forms must agree bit for bit; returns uint8 [n, width]."""
    eng = get_engine()
    L, h, n = eng.lib, eng.h, len(msgs)
    blob, off = _blob(msgs)
    hblob = _odd(blob) if blob.size else None
    hout = np.full((n, width), 0xA5, np.uint8)
    rc = getattr(L, fn)(h, n, *pre, hblob.ctypes.data if blob.size else None, off.ctypes.data, dst, len(dst), *post, hout.ctypes.data)
    assert rc == OK, err()
    dblob, doff = _dev(blob if blob.size else np.zeros(1, np.uint8)), _dev(off.view(np.int64))
    dout = torch.full((n, width), 0x5A, dtype=torch.uint8, device="cuda")
    rc = getattr(L, fn + "_dev")(h, n, *pre, dblob.data_ptr(), doff.data_ptr(), dst, len(dst), *post, dout.data_ptr(), None)
    assert rc == OK, err()
    torch.cuda.synchronize()
    assert np.array_equal(hout, dout.cpu().numpy()), fn + ": the host form and the _dev form differ"
    return hout


def both_map(u56, count):
    eng = get_engine()
    L, h, n = eng.lib, eng.h, u56.shape[0]
    hin, hout = _odd(u56), np.full((n, 112), 0xA5, np.uint8)
    assert L.ncg_ed448_h2c_map_batch(h, n, count, hin.ctypes.data, hout.ctypes.data) == OK, err()
    din, dout = _dev(u56), torch.full((n, 112), 0x5A, dtype=torch.uint8, device="cuda")
    assert L.ncg_ed448_h2c_map_batch_dev(h, n, count, din.data_ptr(), dout.data_ptr(), None) == OK, err()
    torch.cuda.synchronize()
    assert np.array_equal(hout, dout.cpu().numpy()), "the host form and the _dev form differ"
    return hout


def cyc(items, n):
    return [items[i % len(items)] for i in range(n)]


def ints(row, k):
    b = bytes(row)
    return [int.from_bytes(b[56 * j:56 * j + 56], "little") for j in range(k)]


def same_in_every_lane(out, m):
    assert np.array_equal(out, hh.cycle(out[:m], out.shape[0]))


# ---------------------------------------------------------------- expand_message_xof
XOF_DSTS = {"ro": hh.RO, "dst1": b"D", "dst255": b"y" * 255}


def xof_msgs(dst):
    """messages that put len(msg) + 2 + len(DST) + 1 on 135, 136 and 137 mod 136, the empty one and 1000 bytes"""
    msgs = [hh.seeded_bytes("xof-gpu-%d" % r, len(dst), n) for r, n in zip((135, 136, 137), hh.boundary_lengths(dst))]
    assert [(len(m) + 2 + len(dst) + 1) % 136 for m in msgs] == [135, 0, 1]
    return msgs + [b"", hh.seeded_bytes("xof-gpu-long", 0, 1000)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("out_len", [1, 135, 136, 137, 272, 273])
@pytest.mark.parametrize("dst_name", sorted(XOF_DSTS))
def test_xof(dst_name, out_len, n):
    dst = XOF_DSTS[dst_name]
    msgs0 = xof_msgs(dst)
    want = once(("xof", dst_name, out_len), lambda: [hh.xof(m, dst, out_len) for m in msgs0])
    out = both_msgs("ncg_xof_shake256_batch", cyc(msgs0, n), dst, [], [out_len], out_len)
    assert [bytes(r) for r in out] == cyc(want, n)


def test_xof_fixture_rows_and_empty_messages():
    for (name, msg, dst, out_len), row in zip(hh.xof_rows(), hh.kat()["xof"]):
        assert bytes(both_msgs("ncg_xof_shake256_batch", [msg], dst, [], [out_len], out_len)[0]).hex() == row["out"], name
    eng = get_engine()
    out, off = np.zeros((3, 64), np.uint8), np.zeros(4, np.uint64)                 # every message empty: msgs may be NULL
    assert eng.lib.ncg_xof_shake256_batch(eng.h, 3, None, off.ctypes.data, hh.RO, len(hh.RO), 64, out.ctypes.data) == OK, err()
    assert [bytes(r) for r in out] == [hh.xof(b"", hh.RO, 64)] * 3
    assert eng.xof_shake256_batch([b"abc"], hh.RO, 65535)[0].tobytes() == hh.xof(b"abc", hh.RO, 65535)


# ---------------------------------------------------------------- hash_to_field / hash_to_scalar
FIELD_GROUPS = [("default/ro", hh.RO, 2), ("default/nu", hh.NU, 1), ("rfc/ro", hh.QUUX + hh.RO, 2), ("rfc/nu", hh.QUUX + hh.NU, 1)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group", range(len(FIELD_GROUPS)))
def test_hash_to_field(group, n):
    tag, dst, count = FIELD_GROUPS[group]
    msgs0 = [m for _, m in hh.MESSAGES]
    want = once(("field", group), lambda: [hh.hash_to_field(m, dst, count) for m in msgs0])
    by_name = {r["name"]: [int(u, 16) for u in r["u"]] for r in hh.kat()["hash"]}
    assert want == [by_name["%s/%s" % (name, tag)] for name, _ in hh.MESSAGES]                 # the reference's own hash_to_field
    out = both_msgs("ncg_ed448_h2c_hash_to_field_batch", cyc(msgs0, n), dst, [count], [], 56 * count)
    assert [ints(r, count) for r in out] == cyc(want, n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dst", [hh.SCALAR_DST, hh.QUUX + hh.RO], ids=["default", "quux"])
def test_hash_to_scalar(dst, n):
    msgs0 = [m for _, m in hh.MESSAGES]
    k = hh.kat()
    if dst == hh.SCALAR_DST:
        assert [hh.hash_to_scalar(m) for m in msgs0] == [int(r["out"], 16) for r in k["scalar"][:5]]
        assert [hh.decaf_hash_to_scalar(m) for m in msgs0] == [int(r["out"], 16) for r in k["decaf_scalar"][:5]]
    else:
        assert hh.hash_to_scalar(b"abc", dst) == int(k["scalar"][5]["out"], 16)
        assert hh.decaf_hash_to_scalar(b"abc", dst) == int(k["decaf_scalar"][5]["out"], 16)
    want = once(("scalar", dst), lambda: [hh.hash_to_scalar(m, dst) for m in msgs0])
    dwant = once(("dscalar", dst), lambda: [hh.decaf_hash_to_scalar(m, dst) for m in msgs0])
    out = both_msgs("ncg_ed448_h2c_hash_to_scalar_batch", cyc(msgs0, n), dst, [], [], 56)
    assert [ints(r, 1)[0] for r in out] == cyc(want, n)
    out = both_msgs("ncg_decaf448_hash_to_scalar_batch", cyc(msgs0, n), dst, [], [], 56)
    assert [ints(r, 1)[0] for r in out] == cyc(dwant, n)


def test_oversize_dst_through_the_python_layer():
    """a 300-byte DST is compressed by the caller: to 56 bytes for the k = 224 calls, to 64 for decaf448's hashToScalar (k = 256)"""
    k = hh.kat()
    hrow = {r["name"]: r for r in k["hash"]}["dst300"]
    assert GE.ed448_hasher.hashToCurve(b"abc", {"DST": b"x" * 300}) == (int(hrow["x"], 16), int(hrow["y"], 16))
    srow = {r["name"]: r for r in k["scalar"]}["abc/dst300"]
    assert GE.ed448_hasher.hashToScalar(b"abc", {"DST": b"z" * 300}) == int(srow["out"], 16) == hh.hash_to_scalar(b"abc", b"z" * 300)
    drow = {r["name"]: r for r in k["decaf_scalar"]}["abc/dst300"]
    assert GD.hashToScalar_batch([b"abc"], DST=b"z" * 300) == [int(drow["out"], 16)] == [hh.decaf_hash_to_scalar(b"abc", b"z" * 300)]
    assert GD.hashToScalar(b"abc", DST=b"z" * 300, device_hash=True) == int(drow["out"], 16)
    assert int(drow["out"], 16) != int.from_bytes(hh.xof(b"abc", b"z" * 300, 64, 224), "little") % N      # the 56-byte compression differs
    grow = {r["name"]: r for r in k["decaf"]}["abc/dst300"]
    assert GD.hashToCurve_batch([b"abc"], DST=b"w" * 300, device_hash=True) == [bytes.fromhex(grow["out"])]
    assert GD.hashToCurve(b"abc", DST=b"w" * 300, device_hash=True).toBytes() == bytes.fromhex(grow["out"])


# ---------------------------------------------------------------- the map
def _u56(us_rows):
    return np.frombuffer(b"".join(int(u).to_bytes(56, "little") for row in us_rows for u in row), np.uint8).reshape(len(us_rows), -1).copy()


def single_rows():
    """(u, fixture answer) of the count = 1 map: the edge values, every exceptional u, 128 seeded u"""
    k = hh.kat()
    exc = hh.exception_us()
    assert len(exc) >= 3 and [r["name"] for r in k["exceptions"]] == list(exc)
    us = hh.edge_us() + list(exc.values()) + hh.seeded_us()
    want = [(int(r["x"], 16), int(r["y"], 16)) for r in k["map"] + k["exceptions"]] + [(int(h[:112], 16), int(h[112:], 16)) for h in k["seeded_map"]]
    assert all(w == (0, 1) for w in want[6:6 + len(exc)])                                   # xEd yEd = 0: the identity, written (0, 1)
    return us, want


@pytest.mark.parametrize("n", SIZES)
def test_map_single(n):
    us, want = once("single", single_rows)
    out = both_map(_u56([[u] for u in cyc(us, n)]), 1)
    assert [tuple(ints(r, 2)) for r in out] == cyc(want, n)
    if n == 1:
        assert tuple(ints(out[0], 2)) == hh.map_to_curve([0])


def pair_rows():
    k = hh.kat()
    rows = list(hh.pair_rows())
    want = [(int(r["x"], 16), int(r["y"], 16)) for r in k["pairs"]]
    rows += hh.seeded_pairs()
    want += hh.seeded_pair_answers()
    return rows, want


@pytest.mark.parametrize("n", SIZES)
def test_map_pairs(n):
    rows, want = once("pairs", pair_rows)
    assert rows[0][1] == P - rows[0][0]                                                     # (u, p - u): the same image twice, a doubling
    out = both_map(_u56(cyc(rows, n)), 2)
    assert [tuple(ints(r, 2)) for r in out] == cyc(want, n)
    if n == 1:
        assert tuple(ints(out[0], 2)) == hh.map_to_curve(list(rows[0]))


def test_map_through_the_hasher():
    us, want = once("single", single_rows)
    assert GE.ed448_hasher.mapToCurveBatch(us[:12]) == want[:12] and GE.ed448_hasher.mapToCurve(0) == GE.ed448_Point.ZERO


# ---------------------------------------------------------------- hashToCurve / encodeToCurve from messages
def hash_groups():
    """the listed rows grouped by (DST, count) - one call takes one DST: [(dst given to the device, count, msgs, fixture answers)]"""
    groups = {}
    for (name, msg, dst, count), row in zip(hh.listed_rows(), hh.kat()["hash"]):
        g = groups.setdefault((dst, count), ([], []))
        g[0].append(msg)
        g[1].append((int(row["x"], 16), int(row["y"], 16)))
    return [(hh.effective_dst(dst), count, msgs, want) for (dst, count), (msgs, want) in groups.items()]


@pytest.mark.parametrize("n", SIZES)
def test_hash_listed_rows(n):
    groups = once("hash_groups", hash_groups)
    assert len(groups) == 7 and sum(len(g[2]) for g in groups) == len(hh.listed_rows())
    for dst, count, msgs, want in groups:
        out = both_msgs("ncg_ed448_h2c_hash_batch", cyc(msgs, n), dst, [count], [], 112)
        assert [tuple(ints(r, 2)) for r in out] == cyc(want, n), (dst, count)
    if n == 1:
        dst, count, msgs, want = groups[0]
        assert hh.hash_to_curve(msgs[0], dst, count) == want[0]


SEEDED_CALLS = {"ro": ("ncg_ed448_h2c_hash_batch", [2], 112), "nu": ("ncg_ed448_h2c_hash_batch", [1], 112),
                "decaf": ("ncg_decaf448_hash_to_group_batch", [], 56)}


@pytest.mark.parametrize("suite", hh.SEEDED_SUITES)
def test_hash_seeded_batches(suite):
    """128 seeded rows per suite (hashToCurve, encodeToCurve, decaf448 hashToCurve) in 8 batches of 16, each batch with its own DST
    and one call per form, against the reference's answers"""
    fn, pre, width = SEEDED_CALLS[suite]
    ans = hh.seeded_answers(suite)
    rows = [hh.seeded_row(suite, i) for i in range(hh.SEEDED)]
    dsts = set()
    for b in range(0, hh.SEEDED, hh.SEEDED_BATCH):
        batch = rows[b:b + hh.SEEDED_BATCH]
        dst = batch[0][1]
        assert len(batch) == hh.SEEDED_BATCH and all(d == dst for _, d in batch)
        dsts.add(dst)
        out = both_msgs(fn, [m for m, _ in batch], dst, pre, [], width)
        got = [bytes(r) for r in out] if suite == "decaf" else [tuple(ints(r, 2)) for r in out]
        assert got == ans[b:b + hh.SEEDED_BATCH], (suite, b)
    assert len(dsts) == hh.SEEDED // hh.SEEDED_BATCH == 8 and len(ans) == 128
    msg, dst = rows[0]
    if suite == "ro":
        assert GE.ed448_hasher.hashToCurve(msg, {"DST": dst}) == ans[0]
    elif suite == "nu":
        assert GE.ed448_hasher.encodeToCurve(msg, {"DST": dst}) == ans[0]
    else:
        assert GD.hashToCurve_batch([msg], DST=dst, device_hash=True) == [ans[0]] == GD.hashToCurve_batch([msg], DST=dst)


@pytest.mark.parametrize("n", SIZES)
def test_decaf_hash_to_group(n):
    """the device hash against today's host-hash path (device_hash=False) and the fixture"""
    rows = hh.decaf_rows()
    fixture = {r["name"]: bytes.fromhex(r["out"]) for r in hh.kat()["decaf"]}
    default = [(name, msg) for name, msg, dst in rows if dst == hh.DECAF_DST]
    msgs = cyc([m for _, m in default], n)
    host_path = once(("decaf_host", n), lambda: GD.hashToCurve_batch(msgs, device_hash=False))
    assert host_path[:len(default)] == [fixture[name] for name, _ in default][:n]
    out = both_msgs("ncg_decaf448_hash_to_group_batch", msgs, hh.DECAF_DST, [], [], 56)
    assert [bytes(r) for r in out] == host_path
    assert GD.hashToCurve_batch(msgs, device_hash=True) == host_path
    if n == 1:
        for name, msg, dst in rows:
            assert GD.hashToCurve_batch([msg], DST=dst, device_hash=True) == [fixture[name]] == GD.hashToCurve_batch([msg], DST=dst), name
        assert GD.hashToCurve(b"abc", device_hash=True).toBytes() == fixture["abc"] == GD.hashToCurve(b"abc").toBytes()


# ---------------------------------------------------------------- ncg_h2c448_check
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", range(hh.CHECK_OPS))
def test_check_device_against_restatement_and_twin(op, n):
    vals, rows0 = once(("check", op), lambda: hh.check_rows(op))
    want = once(("check_want", op), lambda: [hh.check_expected(op, v) for v in vals])
    out = get_engine().h2c448_check(op, hh.cycle(rows0, n))
    m = min(n, len(vals))
    assert [hh.check_out_ints(op, r) for r in out[:m]] == want[:m]
    assert not out[:, 14 * hh.CHECK_OUT_ELEMS[op]:].any()
    same_in_every_lane(out, m)
    for i in range(min(n, 24)):                                                # the (slow) CPU twin on the first rows
        rc, tw = hh.ht_check(op, rows0[i % len(vals)])
        assert rc == 0 and np.array_equal(tw, out[i])


def test_check_unknown_op_and_batch_limit():
    eng = get_engine()
    z = np.ones((3, 42), np.uint32)
    for op in (-1, hh.CHECK_OPS, 11):
        assert eng.h2c448_check(op, z).shape == (3, 42) and not eng.h2c448_check(op, z).any()
    assert eng.lib.ncg_h2c448_check(eng.h, 0, (1 << 24) + 1, None, None) == INVALID and "too large" in err()
    assert eng.lib.ncg_h2c448_check(None, 0, 1, z.ctypes.data, z.ctypes.data) == INVALID
    assert eng.lib.ncg_h2c448_check(eng.h, 0, 0, None, None) == OK
    assert eng.lib.ncg_h2c448_check(eng.h, 0, 1, None, z.ctypes.data) == INVALID and "NULL buffer" in err()


# ---------------------------------------------------------------- the argument table
# (entry point, has count, has out_len, the word-row arguments among the pointers): the call is
# (ctx, n, [count], msgs, off, dst, dst_len, [out_len], out[, stream])
MSG_CALLS = [("ncg_xof_shake256_batch", False, True, False), ("ncg_ed448_h2c_hash_batch", True, False, True),
             ("ncg_ed448_h2c_hash_to_field_batch", True, False, True), ("ncg_ed448_h2c_hash_to_scalar_batch", False, False, True),
             ("ncg_decaf448_hash_to_group_batch", False, False, True), ("ncg_decaf448_hash_to_scalar_batch", False, False, True)]


def test_argument_table():
    """NULL ctx, count = 3, dst_len 0 and 256, decreasing offsets, NULL messages with a non-empty range, a misaligned device row
    pointer, n = 0 and n = 2^31 with NULL buffers, for every new entry point.  Safe whatever the library does: every non-NULL pointer
    is a zeroed 4 KB buffer (device memory for the _dev forms) and n = 1, so a missing check runs on valid memory and fails the test
    instead of faulting."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    hbuf = np.zeros(4096, np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    hoff, dec = np.array([0, 3], np.uint64), np.array([3, 0], np.uint64)
    doff = _dev(hoff.view(np.int64))
    dst = b"QUUX"
    for fn, has_count, has_len, word_out in MSG_CALLS:
        for dev in (False, True):
            f = getattr(L, fn + ("_dev" if dev else ""))
            buf = dbuf.data_ptr() if dev else hbuf.ctypes.data
            off = doff.data_ptr() if dev else hoff.ctypes.data

            def call(ctx=h, n=1, count=2, msgs=buf, off=off, dst=dst, dst_len=len(dst), out_len=64, out=buf):
                a = [ctx, n] + ([count] if has_count else []) + [msgs, off, dst, dst_len] + ([out_len] if has_len else []) + [out]
                return f(*(a + [None] if dev else a))
            name = (fn, dev)
            assert call() == OK, (name, err())
            assert call(ctx=None) == INVALID, name
            if has_count:
                for bad in (0, 3, -1):
                    assert call(count=bad) == INVALID and "count must be 1 or 2" in err(), (name, bad)
                assert call(count=1) == OK, name
            for bad in (0, 256):
                assert call(dst_len=bad) == INVALID and "dst_len" in err(), (name, bad)
            assert call(dst=None) == INVALID and "NULL buffer" in err(), name
            if has_len:
                for bad in (0, 65536):
                    assert call(out_len=bad) == INVALID and "out_len" in err(), (name, bad)
            assert call(out=None) == INVALID and "NULL buffer" in err(), name
            assert call(off=None) == INVALID and "NULL buffer" in err(), name
            if not dev:                                                         # the host forms read the offsets
                assert call(off=dec.ctypes.data) == INVALID and "must not decrease" in err(), name
                assert call(msgs=None) == INVALID and "NULL message buffer" in err(), name
            if dev and word_out:
                for o in (1, 2, 3):
                    assert call(out=buf + o) == INVALID and "4-byte aligned" in err(), (name, o)
            assert call(n=0, msgs=None, off=None, out=None) == OK, name          # n = 0 touches nothing
            assert call(n=0, dst_len=0) == INVALID, name                          # the rule comes before the empty batch
            assert call(n=1 << 31, msgs=None, off=None, out=None) == INVALID and "too large" in err(), name
    for dev in (False, True):
        f = getattr(L, "ncg_ed448_h2c_map_batch" + ("_dev" if dev else ""))
        buf = dbuf.data_ptr() if dev else hbuf.ctypes.data

        def call(ctx=h, n=1, count=2, u=buf, out=buf + 1024):
            a = [ctx, n, count, u, out]
            return f(*(a + [None] if dev else a))
        assert call() == OK and call(count=1) == OK, err()
        assert call(ctx=None) == INVALID
        for bad in (0, 3):
            assert call(count=bad) == INVALID and "count must be 1 or 2" in err()
        assert call(u=None) == INVALID and "NULL buffer" in err() and call(out=None) == INVALID and "NULL buffer" in err()
        if dev:
            for o in (1, 2, 3):
                assert call(u=buf + o) == INVALID and "4-byte aligned" in err()
                assert call(out=buf + 1024 + o) == INVALID and "4-byte aligned" in err()
        assert call(n=0, u=None, out=None) == OK
        assert call(n=1 << 31, u=None, out=None) == INVALID and "too large" in err()
    assert L.ncg_sync(h) == OK
    torch.cuda.synchronize()
    # the context still answers a known multiplication: 1 * the decaf448 base is the base
    assert GD.multiplyBase_batch([1, 2]) == [GD.Point.BASE.toBytes(), GD.Point.BASE.multiply(2).toBytes()]
