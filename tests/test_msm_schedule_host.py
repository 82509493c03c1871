"""The launch schedule of the MSM device phase (csrc/msm_schedule.hpp), read on the CPU through the host twin.

msm.hip's driver computes one MsmSchedule per MSM and only executes it, so what an MSM launches - which sort, every grid, the
pinned accumulate placement, the fix-up merge, the fold levels and the tail - is integer arithmetic on the plan that these tests
can check without a GPU:
  * tests/golden/msm_launch_schedule.json holds the launches that the driver made BEFORE the schedule existed, recorded from a
    kernel trace on MI355X for a matrix of plans that reaches every branch; the schedule must expand to exactly those;
  * the workspace regions never overlap, and the parts of one host-pointer MSM address the same buckets;
  * the accumulate grid's LDS reservation and the placement that msm_seg prices follow one rule (MSM_ACC_PIN);
  * the stand-alone fold levels hand k_msm_tail a state it accepts."""
import hosttest as H
import pytest
from helpers import load_golden

SECP, ED, G1, G2, BN = 0, 1, 2, 3, 5
DEVICE_CURVE = {SECP: "CurveSecp", ED: "CurveEd", G1: "CurveG1", G2: "CurveG2P", BN: "CurveBn254"}
SORT_SMALL, SORT_TWO_LEVEL, SORT_ONE_LEVEL = 0, 1, 2
MERGE_PLAIN, MERGE_UNITS, MERGE_TREE = 0, 1, 2
SORT2_FALLBACK_BLOCKS = 128          # msm.hip: the fixed grid of the two slice kernels


def window_range(nwin, part, nparts):
    """csrc/msm_shard.hpp msm_shard_window_range"""
    base, rem = divmod(nwin, nparts)
    return part * base + min(part, rem), base + (1 if part < rem else 0)


def split_windows(curve, n, parts, c):
    nwin = H.msm_schedule(curve, n, c)["nwin"]
    return [dict(curve=curve, n=n, c_override=c, w0=w0, wcnt=cnt) for w0, cnt in (window_range(nwin, p, parts) for p in range(parts))]


def host_parts(curve, n):
    """api.hip ncg_msm: the points cross PCIe in parts that share the layout (and the window width) of the whole MSM"""
    parts = 4 if n >= 1 << 19 else 2 if n >= 1 << 17 else 1
    per = (((n + parts - 1) // parts) + 255) & ~255
    c = H.msm_schedule(curve, n)["c"]
    out = []
    for p in range(parts):
        lo = min(n, per * p)
        cnt = min(n, lo + per) - lo
        last = p == parts - 1 or lo + cnt >= n
        out.append(dict(curve=curve, n=max(cnt, 1), c_override=c, n_layout=min(n, per), pts_stored=True,
                        part_flags=(1 if p == 0 else 0) | (2 if last else 0)))
        if last:
            break
    return out


# the rows of the golden file: the plans of every MSM device phase the row ran, in order
ROWS = {
    "1 G1 n=300": [dict(curve=G1, n=300)],
    "2 G1 n=3000 c=16": [dict(curve=G1, n=3000, c_override=16)],
    "3 G1 n=40000 c=9": [dict(curve=G1, n=40000, c_override=9)],
    "4 G1 n=2^16 seg=4 then seg=16": [dict(curve=G1, n=1 << 16, seg=4), dict(curve=G1, n=1 << 16, seg=16)],
    "5 G2 n=2^14": [dict(curve=G2, n=1 << 14)],
    "6 secp256k1 n=3000": [dict(curve=SECP, n=3000)],
    "6b secp256k1 n=3000 c=11": [dict(curve=SECP, n=3000, c_override=11)],
    "6 ed25519 n=3000": [dict(curve=ED, n=3000)],
    "6b ed25519 n=3000 c=11": [dict(curve=ED, n=3000, c_override=11)],
    "6 bn254 G1 n=3000": [dict(curve=BN, n=3000)],
    "6b bn254 G1 n=3000 c=11": [dict(curve=BN, n=3000, c_override=11)],
    "7 G1 resident precomputed n=2^12": [dict(curve=G1, n=1 << 12, c_override=16, shared=True)],      # ncg_points_precompute: c = 16
    "8 G1 resident endomorphism n=2^12": [dict(curve=G1, n=1 << 12, endo=True)],
    "9 G1 split_windows parts=8 n=2^18 c=10": split_windows(G1, 1 << 18, 8, 10),
    "10 G1 host pointers n=2^17": host_parts(G1, 1 << 17),
    "11 G1 n=2^16 equal scalars": [dict(curve=G1, n=1 << 16)],
}


def expand(kw):
    """the main-stream launches of one device phase: [kernel, "x.y" workgroups, workgroup size]"""
    S = H.msm_schedule(**kw)
    D = DEVICE_CURVE[kw["curve"]]
    coop = "true" if S["coop"] else "false"
    out = []

    def launch(name, x, y, wg):
        out.append([name, "%d.%d" % (x, y), wg])

    sort_grid = (S["sort_grid_x"], S["sort_grid_y"])
    if kw.get("endo"):
        launch("k_msm_digits_endo<2>", (kw["n"] + 255) // 256, 1, 256)
    elif S["sort"] != SORT_SMALL:
        launch("k_msm_digits", S["digits_grid"], 1, 256)
    if S["sort"] == SORT_SMALL:
        launch("k_msm_sort_small", S["nwin"], 1, 1024)
    elif S["sort"] == SORT_TWO_LEVEL:
        R = 1 << S["s2_lgr"]
        launch("k_sort2_count", *sort_grid, 1024)
        launch("k_sort2_scan", S["nwin"], 1, R)
        launch("k_sort2_scatter", *sort_grid, 1024)
        launch("k_sort2_fine_staged", R, S["nwin"], 1024)
        launch("k_sort2_fine_count", SORT2_FALLBACK_BLOCKS, 1, 512)
        launch("k_sort2_fine_place", SORT2_FALLBACK_BLOCKS, 1, 512)
    else:
        launch("k_msm_hist", *sort_grid, 1024)
        launch("k_msm_bucket_totals_split" if S["split_totals"] else "k_msm_bucket_totals", S["totals_grid_x"], S["totals_grid_y"], 256)
        if kw.get("shared"):
            launch("k_msm_shared_totals", S["shared_grid"], 1, 256)
            launch("k_msm_scan", 1, 1, 1024)
            launch("k_msm_shared_starts", S["shared_grid"], 1, 256)
        else:
            launch("k_msm_scan", S["nwin"], 1, 1024)
        for _ in range(S["scatter_n"]):
            launch("k_msm_scatter", *sort_grid, 1024)
    launch("k_msm_accum<%s, %s>" % (D, "true" if S["acc_sparse"] else "false"), S["acc_grid_x"], S["acc_grid_y"], 256)
    merge = {MERGE_TREE: "k_msm_fixup_merge_tree<%s, %s>" % (D, coop), MERGE_UNITS: "k_msm_fixup_merge_units<%s, %s>" % (D, coop),
             MERGE_PLAIN: "k_msm_fixup_merge<%s>" % D}[S["merge"]]
    launch(merge, S["merge_grid_x"], S["merge_grid_y"], 256)
    launch("k_msm_fixup_long<%s, %s>" % (D, coop), S["long_blocks"], 1, S["tail_threads"])
    if S["part_last"]:
        for tasks, lv_coop, grid in S["fold"]:
            launch("k_msm_reduce_level%s<%s>" % ("_coop" if lv_coop else "", D), grid, 1, 256)
        launch("k_msm_tail<%s, %s>" % (D, coop), S["av_nwin"], 1, S["tail_threads"])
    return out


GOLDEN = load_golden("msm_launch_schedule.json")


def test_golden_covers_the_rows():
    assert set(GOLDEN["rows"]) == set(ROWS)


@pytest.mark.parametrize("row", list(ROWS))
def test_schedule_expands_to_the_recorded_launches(row):
    got = [ln for kw in ROWS[row] for ln in expand(kw)]
    assert got == GOLDEN["rows"][row]


def test_rows_reach_the_branches_they_are_there_for():
    s = {row: [H.msm_schedule(**kw) for kw in plans] for row, plans in ROWS.items()}
    one = lambda row: s[row][0]
    assert one("1 G1 n=300")["sort"] == SORT_SMALL and one("1 G1 n=300")["acc_reserve"] == 96 * 1024
    r2 = one("2 G1 n=3000 c=16")
    assert r2["sort"] == SORT_TWO_LEVEL and r2["nb"] > 8192
    assert [lv[1] for lv in r2["fold"]] == sorted(lv[1] for lv in r2["fold"]) and {lv[1] for lv in r2["fold"]} == {0, 1}
    r3 = one("3 G1 n=40000 c=9")
    assert r3["sort"] == SORT_ONE_LEVEL and not r3["split_totals"] and r3["scatter_n"] == 1
    a, b = s["4 G1 n=2^16 seg=4 then seg=16"]
    assert a["acc_grid_x"] * a["acc_grid_y"] > 512 and a["acc_reserve"] == 0
    assert 256 < b["acc_grid_x"] * b["acc_grid_y"] <= 512 and b["acc_reserve"] == 56 * 1024
    r5 = one("5 G2 n=2^14")
    assert r5["ls"] == 1 and r5["acc_sparse"] and r5["top_tb"] > 0 and r5["top_w"] == r5["nwin"] - 1
    for nm in ("secp256k1", "ed25519", "bn254 G1"):
        assert one("6 %s n=3000" % nm)["merge"] == MERGE_PLAIN and not one("6 %s n=3000" % nm)["coop"]
        f = one("6b %s n=3000 c=11" % nm)["fold"]
        assert f and not any(lv[1] for lv in f)          # stand-alone fold levels, none of them cooperative
    r7 = one("7 G1 resident precomputed n=2^12")
    assert r7["sort"] == SORT_ONE_LEVEL and r7["scatter_n"] == 4 and r7["acc_grid_y"] == r7["av_nwin"] == 1 and r7["pts_in_place"]
    r8 = one("8 G1 resident endomorphism n=2^12")
    assert r8["pts_in_place"] and r8["av_n"] == 2 << 12
    r9 = s["9 G1 split_windows parts=8 n=2^18 c=10"]
    assert len(r9) == 8 and all(p["split_totals"] and p["Q"] >= 64 for p in r9) and sum(p["nwin"] for p in r9) == H.msm_schedule(G1, 1 << 18, 10)["nwin"]
    r10 = s["10 G1 host pointers n=2^17"]
    assert [(p["part_first"], p["part_last"]) for p in r10] == [(1, 0), (0, 1)]


# plans for the structural checks: every curve, sizes either side of each threshold, the special plan kinds
def _plans():
    out = []
    for curve in (SECP, ED, G1, G2, BN):
        for n in (1, 37, 300, 3000, 1 << 12, (1 << 15), (1 << 15) + 1, 40000, 1 << 16, 100003, 1 << 18, 1 << 20):
            out.append(dict(curve=curve, n=n))
        for c in (9, 11, 13, 16):
            out.append(dict(curve=curve, n=3000, c_override=c))
        for seg in (4, 16, 64):
            out.append(dict(curve=curve, n=1 << 16, seg=seg))
    for curve in (G1, G2):
        out += [dict(curve=curve, n=1 << 12, endo=True), dict(curve=curve, n=1 << 17, endo=True),
                dict(curve=curve, n=1 << 12, c_override=16, shared=True), dict(curve=curve, n=1 << 16, c_override=16, shared=True)]
    out += split_windows(G1, 1 << 18, 8, 10) + split_windows(G2, 1 << 16, 3, 0) + host_parts(G1, 1 << 17) + host_parts(G2, 1 << 19)
    return out


PLANS = _plans()


def _acc_words(curve):
    return H.msm_plan(curve, 64)["acc_words"]


def test_layout_regions_do_not_overlap():
    """Every region starts 256-byte aligned, in the order of MsmLayout, and is at least as large as what the kernels address in
    it (sizes restated here from the kernels' indexing); `total` is the end of the last one."""
    for kw in PLANS:
        S = H.msm_schedule(**kw)
        xw = _acc_words(kw["curve"])
        n_entries = S["av_n"] // (S["nwin"] if kw.get("shared") else 1)          # entries per window of this launch
        lanes = S["av_nwin"] * S["nseg"]
        need = {
            "digits": S["nwin"] * n_entries * 2, "bucket_start": S["nwin"] * (S["nb"] + 1) * 4, "sorted": S["nwin"] * n_entries * 4,
            "sort_tmp": S["nwin"] * n_entries * 4 if S["sort"] == SORT_TWO_LEVEL else 0, "shared_start": (S["nb"] + 1) * 4,
            "counts": S["nwin"] * S["Q"] * S["nb"] * 4 if S["sort"] == SORT_ONE_LEVEL else 0,
            "buckets": S["av_nwin"] * S["nb"] * xw * 4, "part_pts": lanes * 2 * xw * 4, "part_meta": lanes * 16,
            "long_runs": 16 + S["av_nwin"] * (S["nseg"] + 1) * 16, "bad": 4, "red0": S["av_nwin"] * (S["nb"] // 2) * 2 * xw * 4,
            "red1": S["av_nwin"] * (S["nb"] // 4) * 3 * xw * 4, "tail0": S["av_nwin"] * (2 * S["tail_threads"] + 64) * xw * 4,
            "tail1": S["av_nwin"] * (2 * S["tail_threads"] + 64) * xw * 4, "fin": S["ngroups"] * S["av_nwin"] * xw * 4, "pts_mont": 0,
        }
        offs = [S[r] for r in H.MSM_LAYOUT_REGIONS] + [S["total"]]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs), kw
        for r, lo, hi in zip(H.MSM_LAYOUT_REGIONS, offs, offs[1:]):
            assert hi - lo >= need[r], (kw, r)
        assert S["total"] == S["fin"] + ((need["fin"] + 255) & ~255), kw


@pytest.mark.parametrize("curve,n", [(G1, 1 << 17), (G1, (1 << 19) + 12345), (G2, 1 << 19), (SECP, 1 << 18)])
def test_parts_of_one_msm_share_the_layout(curve, n):
    """the parts of a host-pointer MSM accumulate into ONE bucket array: every part's schedule places every region where the
    layout plan (the largest part, api.hip) places it, and runs the layout plan's lane segment"""
    parts = host_parts(curve, n)
    layout = H.msm_schedule(**dict(parts[0], part_flags=3))
    assert len(parts) > 1
    for kw in parts:
        S = H.msm_schedule(**kw)
        assert [S[r] for r in H.MSM_LAYOUT_REGIONS + ("total",)] == [layout[r] for r in H.MSM_LAYOUT_REGIONS + ("total",)], kw
        assert S["seg"] == layout["seg"] and S["nseg"] == (kw["n"] + S["seg"] - 1) // S["seg"]
        assert S["sort"] != SORT_SMALL          # the one-launch sort clears the buckets: whole MSMs only


def test_pinned_grid_rule():
    """The accumulate launch reserves 96 KB of LDS iff its grid has at most 256 workgroups (one per CU), 56 KB iff 257..512 (two
    per CU), nothing above; msm_seg prices the same grid at k = 1 / 2 / ceil(lanes / 65536) waves per SIMD: seg_pin is the
    placement msm_seg reads (csrc/msm_plan.hpp msm_acc_pinned), 0 = unpinned."""
    seen = set()
    for kw in PLANS:
        S = H.msm_schedule(**kw)
        wgs = S["acc_grid_x"] * S["acc_grid_y"]
        assert S["acc_grid_x"] == ((S["nseg"] << S["ls"]) + 255) // 256 and S["acc_grid_y"] == S["av_nwin"]
        want = (96 * 1024, 1) if wgs <= 256 else (56 * 1024, 2) if wgs <= 512 else (0, 0)
        assert (S["acc_reserve"], S["seg_pin"]) == want, kw
        seen.add(want)
    assert len(seen) == 3


def test_fold_levels_leave_the_tail_what_it_accepts():
    """k_msm_tail runs the levels whose (narr + 1) * (n_in / 2) additions and copies fit its units in one round; every wider
    level is a launch of its own, cooperative where the curve has cooperative units and the level fits the resident lanes."""
    for kw in PLANS:
        S = H.msm_schedule(**kw)
        units = S["tail_threads"] >> (S["ls"] + (2 if S["coop"] else 0))
        assert S["tail_units"] == units
        narr, n_in = 1, S["nb"]
        for tasks, coop, grid in S["fold"]:
            assert (narr + 1) * (n_in // 2) > units and tasks == (narr + 1) * S["av_nwin"] * (n_in // 2), kw
            assert coop == (1 if S["coop"] and tasks <= (131072 >> (S["ls"] + 2)) else 0), kw
            assert grid == ((tasks << (S["ls"] + 2 * coop)) + 255) // 256, kw
            narr, n_in = narr + 1, n_in // 2
        assert (narr, n_in) == (S["narr"], S["n_in"]) and (narr + 1) * (n_in // 2) <= units, kw
        assert narr + (n_in.bit_length() - 1) == S["c"], kw          # the tail ends with c arrays of one point per window


@pytest.mark.parametrize("rs", [0, 1, 5, 40])
def test_run_serial_override_is_what_the_merge_runs_with(rs):
    for kw in (dict(curve=G1, n=300), dict(curve=G1, n=1 << 16), dict(curve=G2, n=1 << 14), dict(curve=SECP, n=3000),
               dict(curve=G1, n=1 << 12, c_override=16, shared=True)):
        assert H.msm_schedule(run_serial=rs, **kw)["run_serial"] == rs
        assert H.msm_schedule(**kw)["run_serial"] >= 2


def test_dynamic_lds_sizes():
    """The kernel trace reports static LDS only, so the dynamic sizes are pinned here, worked out by hand from the expressions of
    the driver before the schedule existed: a unit's LDS is 10 exchange slots of one field element (cooperative curves only:
    14 words on G1, 28 on G2) plus one accumulator (56 / 112 words; 36 on the 256-bit curves); a 256-thread workgroup holds
    256 >> unit_shift units, a 512-thread one 512 >> unit_shift (unit_shift 2 on G1, 3 on G2, 0 elsewhere)."""
    g1, g2, k1 = H.msm_schedule(G1, 1 << 14), H.msm_schedule(G2, 1 << 14), H.msm_schedule(SECP, 1 << 15, 11)
    assert g1["merge"] == MERGE_TREE and (g1["merge_lds"], g1["long_lds"], g1["tail_lds"], g1["fold_coop_lds"]) == (64 * 196 * 4, 128 * 196 * 4, 128 * 196 * 4, 64 * 140 * 4)
    assert g2["merge"] == MERGE_TREE and (g2["merge_lds"], g2["long_lds"], g2["tail_lds"], g2["fold_coop_lds"]) == (32 * 392 * 4, 64 * 392 * 4, 64 * 392 * 4, 32 * 280 * 4)
    assert k1["merge"] == MERGE_PLAIN and (k1["merge_lds"], k1["long_lds"], k1["tail_lds"]) == (0, 512 * 36 * 4, 512 * 36 * 4)
    assert H.msm_schedule(G1, 1 << 16, seg=16)["merge"] == MERGE_UNITS and H.msm_schedule(G1, 1 << 16, seg=16)["merge_lds"] == 64 * 196 * 4
    # sorts: nb counters (+ n int16 digits, n rounded up to even, in the one-launch sort); the scan keeps nb + nb / 32 + 1 words
    assert g1["sort"] == SORT_SMALL and g1["small_lds"] == g1["nb"] * 4 + (1 << 14) * 2
    assert H.msm_schedule(G1, 301)["small_lds"] == H.msm_schedule(G1, 301)["nb"] * 4 + 302 * 2
    one = H.msm_schedule(G1, 40000, 9)
    assert (one["hist_lds"], one["scan_lds"]) == (256 * 4, (256 + 8 + 1) * 4) and H.msm_schedule(G1, 3000, 16)["sort2_stage_lds"] == 20 * 1024 * 4
