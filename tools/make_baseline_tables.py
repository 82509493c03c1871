#!/usr/bin/env python3
"""Rewrites section 5 of BASELINE.md from the committed round profiles (profiles/r05_*, r04 beside them), so the tables are
transcriptions of measured files, not hand-typed numbers.  python tools/make_baseline_tables.py"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda *a: os.path.join(ROOT, "profiles", *a)  # noqa: E731


def load(name):
    with open(P(name)) as f:
        return json.load(f)


def main():
    b = load("r06_bench_full.json")          # the FULL result object of the driver's command (bench.py --out); stdout carries the compact line
    b1 = load("r05_bench_full.json")
    ex, ex1 = load("r05_bench_extra.json"), load("r04_bench_extra.json")
    e = b["extra"]
    host = b.get("host", {})
    out = []
    out.append("## 5. Results table (round 6, one MI355X, the driver's command `python3 bench.py --gpus 1 --steps 20 --warmup 5` on a fresh box: `profiles/r06_bench_line.json` (the compact line the driver parses), `profiles/r06_bench_full.json` (the full object this table is made from), `profiles/r06_bench_kernel_stats.csv` (rocprofv3 --stats around the same command), `profiles/r06_pmc.json`)\n")
    out.append("Throughput with inputs resident in HBM, one run of the driver's command on a fresh box (per-step event / wall distributions "
               "are in the full object: `step_times`; the pool's boxes differ by up to 5 %% on these kernels, DESIGN.md section 7).  Every result is verified "
               "bit-exactly before it is printed (sample vs the CPU oracle's C restatement, full-size checksum / progression identity, "
               "ed25519 verdicts by construction + the reference's 196 zip215.json cases).  `hbm_frac` = algorithmic bytes ÷ 8 TB/s (the "
               "contract's figure; the path is VALU-bound, §2 caveat); `mad_frac` = executed `v_mad_u64_u32` FROM THE SQ_INSTS_VALU_INT64 COUNTER "
               "(round 6, DESIGN.md section 7; the static operation-sequence counts of rounds 2-5 read 4-19 %% high) ÷ the measured multiplier ceiling "
               "3.08×10¹³/s; `plain` = the other VALU instructions (SQ_INSTS_VALU minus the multiply-adds) ÷ the plain-instruction ceiling; `traffic` = HBM "
               "bytes per launch of the dominant kernel "
               "(FETCH_SIZE/WRITE_SIZE with the per-pattern calibration of `tools/pmc_calib`, in `profiles/r06_pmc.json`).  **The first time of each row is "
               "the DRIVER's own record of the previous round (BENCH_r05.json, the driver's box), the second this round's driver-command run on whatever box the pool "
               "handed out; the boxes differ by up to 5 %% (8.7 %% seen on the secp256k1 ladder), so the pair is not an A/B.**  CPU baseline = the "
               "REFERENCE's own TypeScript code on the GPU box's host (%s, %s logical cores; Node %s running the type-stripped sources of "
               "`oracle/_ref/refjs.bundle`, one thread), each result compared bit-exactly with the GPU's; the C port of round 1-3 beside it.\n"
               % (host.get("cpu_model"), host.get("logical_cores"), host.get("node_version")))
    out.append("| config | N | time (BENCH_r05 → r06) | throughput | hbm_frac | mad_frac | plain | traffic / algorithmic | CPU: reference (1 thread) | CPU: C port 1 thread / all threads | bit-exact |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|")

    def row(name, n, t1, t2, unit, entry, alg_bytes):
        rf = entry["roofline"]
        v = rf["valu"]
        cb = entry.get("cpu_baseline", {})
        ref = cb if cb.get("kind") == "reference" else {}
        cb = cb.get("port", cb)
        at = cb.get("all_threads", {})
        tr = rf.get("traffic")
        out.append("| %s | %s | %s → **%.2f ms** | **%.3g %s** | %.2f %% | %s | %s | %s | %s | %s / %s | yes |" % (
            name, n, ("%.2f ms" % t1) if t1 else "—", t2, entry["value"], unit, 100 * rf["frac"],
            ("%.0f %%" % (100 * v["mad_frac"])) if "mad_frac" in v else "—",
            ("%.0f %%" % (100 * v["plain_frac"])) if "plain_frac" in v else "—",
            ("%.2f GB / %.0f MB = %.0f×" % (tr / 1e9, alg_bytes / 1e6, tr / alg_bytes)) if tr else "—",
            ("**%.3g /s**" % ref["value"]) if ref else "—",
            ("%.3g /s" % cb["value"]) if cb else "—", ("%.3g /s (%d thr)" % (at["value"], at["cores"])) if at else "—"))

    e1 = b1["extra"]
    drv = {"secp": 9.234, "ed": 2.807, "g1": 3.491, "g2": 3.428, "ntt": 0.486}   # BENCH_r05.json (the driver's record, VERDICT r05 headline)
    row("secp256k1 `multiplyUnsafe` batch (GLV)", "2²⁰", drv["secp"], b["ms_per_step"], "scalar-mults/s", b, 160.0 * (1 << 20))
    row("ed25519 verify batch (ZIP-215, SHA-512 on the device)", "2¹⁸", drv["ed"], e["ed25519_verify"]["ms_per_batch"],
        "verifies/s", e["ed25519_verify"], 161.0 * (1 << 18))
    row("bls12-381 G1 MSM", "2²⁰", drv["g1"], e["msm_g1"]["ms_per_msm"], "points/s", e["msm_g1"], 128.0 * (1 << 20))
    row("bls12-381 G2 MSM", "2¹⁸", drv["g2"], e["msm_g2"]["ms_per_msm"], "points/s", e["msm_g2"], 224.0 * (1 << 18))
    row("bls12-381 Fr NTT (natural→natural)", "2²²", drv["ntt"], e["ntt_fr"]["ms_per_transform"], "elements/s", e["ntt_fr"],
        64.0 * (1 << 22))
    try:
        sb = load("r06_bench_full_slow_box.json")
        se = sb["extra"]
        out.append("\n**The same final build on a box of the slow kind** (`profiles/r06_bench_full_slow_box.json`, `r06_bench_kernel_stats_slow_box.csv`; kernel by kernel "
                   "against the table's box: `profiles/r06_box_to_box.md` - the ladder +7 %%, the NTT passes +5-6 %%, the accumulate kernels +2-3 %%, and ≈ 0.1 ms more per MSM "
                   "outside the kernels): secp256k1 %.2f ms, ed25519 %.2f, G1 MSM %.2f, G2 MSM %.2f, NTT %.3f - the driver's round-5 record above was taken on a box "
                   "of this kind." % (sb["ms_per_step"], se["ed25519_verify"]["ms_per_batch"], se["msm_g1"]["ms_per_msm"], se["msm_g2"]["ms_per_msm"], se["ntt_fr"]["ms_per_transform"]))
    except (OSError, KeyError, ValueError):
        pass
    # runs of the final build that carry bench.py's power_state legs (third session of round 6): what clock and package power the box held
    ps_rows = []
    for name, label in (("r06_bench_full_with_power_state.json", "a typical box"), ("r06_bench_full_low_clock_box.json", "a low-clock box")):
        try:
            pb = load(name)
            pe = pb["extra"]
            ps = pb["power_state"]
            g1, ed = pe["msm_g1"].get("power_state", {}), pe["ed25519_verify"].get("power_state", {})
            ps_rows.append("| %s (`profiles/%s`) | %.3f ms at %.0f MHz, %.0f W (%.2f k cycles per step) | %.3f ms at %.0f MHz, %.0f W | %.3f ms at %.0f MHz, %.0f W | %.3f ms | %.4f ms |" % (
                label, name, pb["ms_per_step"], ps["sclk_mhz"][1], ps["power_w"][1], ps["ms_per_step_x_sclk"] / 1e3,
                pe["msm_g1"]["ms_per_msm"], g1.get("sclk_mhz", [0, 0])[1], (g1.get("power_w") or [0, 0])[1],
                pe["ed25519_verify"]["ms_per_batch"], ed.get("sclk_mhz", [0, 0])[1], (ed.get("power_w") or [0, 0])[1],
                pe["msm_g2"]["ms_per_msm"], pe["ntt_fr"]["ms_per_transform"]))
        except (OSError, KeyError, ValueError, TypeError):
            pass
    if ps_rows:
        out.append("\n**What the boxes hold under these workloads** (`bench.py` `power_state`: the visible GPU's `hwmon` shader clock and package power, medians over 0.9-1.2 s of back-to-back "
                   "steps after the timed ones; DESIGN.md section 7, `profiles/r06_clock_probe.txt`).  The secp256k1 ladder and the ed25519 verifier run at the package power limit "
                   "(≈ 1.3 kW of a 1.4 kW cap) on every box, and the clock a box sustains there (2.18 ... 2.34 GHz seen) is what its time is made of: ms × MHz is constant within 1 % "
                   "across nine typical boxes.\n")
        out.append("| run | secp256k1 2²⁰ | G1 MSM 2²⁰ | ed25519 2¹⁸ | G2 MSM 2¹⁸ | NTT 2²² |")
        out.append("|---|---|---|---|---|---|")
        out.extend(ps_rows)
    out.append("\nThe builder's own round-5 run on another box (`profiles/r05_bench_full.json`): secp256k1 %.2f ms, ed25519 %.2f, G1 MSM %.2f, G2 MSM %.2f, NTT %.3f." % (
        b1["ms_per_step"], e1["ed25519_verify"]["ms_per_batch"], e1["msm_g1"]["ms_per_msm"], e1["msm_g2"]["ms_per_msm"], e1["ntt_fr"]["ms_per_transform"]))
    ko = e["ed25519_verify"]["kernel_only"]
    out.append("\ned25519 kernel-only (pre-hashed challenges): %.2f ms → **%.2f ms** (%.3g verifies/s); the device hash adds "
               "%.2f ms per 2¹⁸ signatures.  Multi-GPU (2/4/8): measured by the driver's scaling run - `bench.py --gpus N` reports weak "
               "scaling per line, `extra.msm_g1_strong` / `msm_g2_strong` = one 2²⁰ / 2¹⁸-point MSM split over the N GPUs through "
               "`ncg_msm_sharded_windows_dev` (every rank holds the set and runs a range of the windows; RCCL all-gather of one fixed-size slot per rank), synchronously and with three in flight; `python bench.py --gpus N` launches its own ranks; strong-scaling budget measured on one GPU: below and DESIGN.md section 6.\n"
               % (e1["ed25519_verify"]["ms_per_batch"], ko["ms_per_batch"], ko["value"], e["ed25519_verify"]["ms_per_batch"] - ko["ms_per_batch"]))
    # round 4: MSMs in flight, per-rank window shares, end to end
    for key, nm in (("msm_g1", "G1 2²⁰"), ("msm_g2", "G2 2¹⁸")):
        m = e[key]
        if "pipelined" in m:
            pp = m["pipelined"]
            out.append("%s MSM with several in flight (`ncg_msm_async_submit` / `_collect`, DESIGN §5): **%.2f ms** per MSM at depth 2, %.2f at depth 3 "
                       "(one at a time: %.2f ms); through the host-pointer entry point on buffers pinned once (`end_to_end`, PCIe-inclusive): **%.2f ms**.\n"
                       % (nm, pp["depth2"]["ms_per_msm"], pp["depth3"]["ms_per_msm"], m["ms_per_msm"], m["end_to_end"]["ms_per_msm"]))
        if "window_share" in m:
            ws = m["window_share"]
            out.append("| %s: one rank's share, window-sharded over G ranks (emulated on one GPU, resident set; DESIGN §6) | G = 2 | G = 4 | G = 8 |" % nm)
            out.append("|---|---|---|---|")
            out.append("| latency of one MSM: local phase of part 0 + combine / finish on the G slots | " + " | ".join(
                "%.2f ms (%.1f×)" % (ws["G%d" % g]["latency_ms"], ws["G%d" % g]["speedup_latency"]) for g in (2, 4, 8)) + " |")
            out.append("| sustained, parts of successive MSMs in flight on three lanes | " + " | ".join(
                "%.2f ms (%.1f×)" % (ws["G%d" % g]["pipelined_part_ms"], ws["G%d" % g]["speedup_pipelined"]) for g in (2, 4, 8)) + " |\n")
    if "end_to_end" in b:
        out.append("secp256k1 2²⁰ batch multiply through the host-pointer entry point (pinned once, chunks pipelined over three streams): **%.2f ms** "
                   "(96 MB in, 65 MB out).\n" % b["end_to_end"]["ms_per_batch"])
    r1, r2 = e["msm_g1"].get("resident_subgroup_set"), e["msm_g2"].get("resident_subgroup_set")
    p1, p2 = (r1 or {}).get("precomputed"), (r2 or {}).get("precomputed")
    if r1 and r2:
        out.append("MSM on a RESIDENT point set verified once to lie in the prime-order subgroup (`ncg_points_verify_subgroup`, %.0f ms for "
                   "2²⁰ G1 points / %.0f ms for 2¹⁸ G2 points; sets decoded by `ncg_points_from_encoded` qualify without it) - the scalars "
                   "are split along the curve endomorphism (DESIGN.md §5), the result is compared bit-exactly with the generic MSM in the "
                   "same run: G1 2²⁰ **%.2f ms** (%.3g points/s), G2 2¹⁸ **%.2f ms** (%.3g points/s).  The rows above are the generic "
                   "`pippenger` (arbitrary curve points, like the reference).\n"
                   % (r1["verify_once_ms"], r2["verify_once_ms"], r1["ms_per_msm"], r1["value"], r2["ms_per_msm"], r2["value"]))
    if p1 and p2:
        out.append("The same verified sets with `ncg_points_precompute` (interleavedMSMUnsafe's per-point tables in device form: window-"
                   "shifted copies, built once in %.0f / %.0f ms; one shared bucket set, no combine across windows): G1 2²⁰ **%.2f ms**, "
                   "G2 2¹⁸ **%.2f ms**; per size and path: `profiles/r06_msm_timing.json` (generic path, 2¹⁰ .. 2²⁰), `profiles/r05_msm_timing.json` (every path).\n"
                   % (p1["precompute_once_ms"], p2["precompute_once_ms"], p1["ms_per_msm"], p2["ms_per_msm"]))
    c0 = e.get("configs0_point_multiply")
    if c0:
        rj = c0.get("reference")
        out.append("BASELINE configs[0] (`benchmark/point.ts:20-32`, CPU plumbing; 1 core of the box's %s): %sC port: `Point.multiply` "
                   "%.0f ops/s (%.0f µs), `Point.multiplyUnsafe` %.0f ops/s (%.0f µs).\n"
                   % (c0.get("cpu_model"),
                      ("the REFERENCE's own code (Node 12, BASE precomputed with W = 6 as the benchmark does): `Point.multiply` **%.0f ops/s**, "
                       "`Point.multiplyUnsafe` **%.0f ops/s** (1 000 random scalars: %.0f / %.0f ops/s); " % (
                           rj["Point_mul"], rj["Point_mulUns"], rj["Point_mul_random_scalars"], rj["Point_mulUns_random_scalars"])) if rj else "",
                      c0["Point_multiply"]["value"], c0["Point_multiply"]["us_per_op"],
                      c0["Point_multiplyUnsafe"]["value"], c0["Point_multiplyUnsafe"]["us_per_op"]))
    out.append("Targets: ≥10⁷ secp256k1 scalar-mults/s per MI355X — met (%.1f×); \"≥40 %% HBM roofline\" for the 2²⁰ G1 MSM is not physically "
               "meaningful (§2 caveat): its dominant kernel runs at %.0f %% of the measured multiplier ceiling in EXECUTED multiplies.\n"
               % (b["value"] / 1e7, 100 * e["msm_g1"]["roofline"]["valu"]["mad_frac"]))
    out.append("### Other entry points (one MI355X, `tools/bench_extra.py`, `profiles/r05_bench_extra.json`; r04 beside it)\n")
    out.append("The r04 → r05 differences of this table (G2 hashToCurve +13 %, ed25519 variable-base +5 %, G1 GLV ladder +6 %, ECDSA verify +3 %; VERDICT r05 weak #7) "
               "were the BOX, not the code: `tools/ab_trees.sh` ran `bench_extra.py` of both trees (each with its own `libncg.so` and Python side) alternately, "
               "r04, r05, r04, r05, on ONE box - no row differs by more than its own run-to-run spread (`profiles/r06_side_table_ab.json`).\n")
    out.append("| entry point | N | r04 | r05 | throughput |")
    out.append("|---|---|---|---|---|")
    for k, v in ex.items():
        o = ex1.get(k)
        out.append("| %s | 2^%d | %s | %.2f ms | %.3g %s/s |" % (k, v["n"].bit_length() - 1, ("%.2f ms" % o["ms"]) if o else "—", v["ms"], v["per_s"], v["unit"]))
    ex7 = load("r07_bench_extra.json")
    rows = ["bn254 G1 MSM 2^16", "bn254 G1 MSM", "bls12-381 G1 MSM", "bn254 G1 variable-base multiply",
            "bls12-381 G1 variable-base multiply (10 steps)", "bn254 G1 pairwise point add", "bn254 G1 normalizeZ batch"]
    out.append("\nbn254 G1 beside bls12-381 G1, one run on one box (`profiles/r07_bench_extra.json`; the compared rows timed over 10 steps).  The\n"
               "bn254 2^20 MSM takes %.2f of the bls12-381 G1 one and the 2^18 batch multiply %.2f of G1's: the same pipelines, each bn254 product\n"
               "about 0.44 of the multiply-adds (DESIGN §3).\n"
               % (ex7["bn254 G1 MSM"]["ms"] / ex7["bls12-381 G1 MSM"]["ms"],
                  ex7["bn254 G1 variable-base multiply"]["ms"] / ex7["bls12-381 G1 variable-base multiply (10 steps)"]["ms"]))
    out.append("| entry point | N | r07 | throughput |")
    out.append("|---|---|---|---|")
    for k in rows:
        v = ex7[k]
        out.append("| %s | 2^%d | %.2f ms | %.3g %s/s |" % (k, v["n"].bit_length() - 1, v["ms"], v["per_s"], v["unit"]))
    out.append("\n### End to end from JavaScript (`addon/bench_js.js`, Node 12 on the GPU box, secp256k1, `profiles/r05_js_bench.jsonl`)\n")
    out.append("BigInt marshalling + N-API + H2D/D2H + kernels.  Every BigInt that crosses N-API costs ~100 ns (`napi_get_element` + "
               "`napi_get_value_bigint_words`), and a reference-shaped `pippenger(c, points, scalars)` call on `Point` objects spends its time in "
               "`toAffine()` + packing.  Round 5: the shim keeps the device copy of an array of FROZEN points (the reference's instances are; "
               "identity sweep per call, INTEGRATION.md), so only the first call on an array pays that; scalars as `BigUint64Array` / packed bytes "
               "skip the per-BigInt cost.  `resident` = an explicit `uploadPoints` set; `pinned` = `native.hostRegister(buffer)` once.\n")
    out.append("| N | `pippenger(c, Point[], bigint[])` first call | same array again, bigint[] scalars | same array again, **BigUint64Array scalars** | packed columns, pinned | resident set, packed scalars | native call alone, pinned | `multiplyUnsafeBatch` from JS | native, pinned |")
    out.append("|---|---|---|---|---|---|---|---|---|")
    for line in open(P("r05_js_bench.jsonl")):
        line = line.strip()
        if not line.startswith("{"):
            continue
        j = json.loads(line)
        out.append("| 2^%d | %.1f ms | %.1f ms | **%.2f ms** | %.2f ms | %.2f ms | %.2f ms | %.1f ms | %.2f ms |" % (
            j["n"].bit_length() - 1, j["pippenger_js_first_call_ms"], j["pippenger_js_cached_points_bigint_scalars_ms"],
            j["pippenger_js_cached_points_typed_scalars_ms"], j.get("pippenger_packed_columns_pinned_ms", float("nan")),
            j["pippenger_resident_bytes_ms"], j.get("pippenger_native_pinned_ms", float("nan")), j["multiplyUnsafeBatch_js_ms"],
            j.get("multiplyUnsafeBatch_native_pinned_ms", float("nan"))))
    text = "\n".join(out) + "\n"
    path = os.path.join(ROOT, "BASELINE.md")
    s = open(path).read()
    i = s.index("## 5. Results table")
    j = s.index("### NTT over bls12-381 Fr")
    k = s.index("### End to end from JavaScript")
    # keep the r01 NTT and host-buffer sub-sections (unchanged kernels), replace the rest
    s2 = s[:i] + text.split("### End to end from JavaScript")[0] + s[j:k] + "### End to end from JavaScript" + text.split("### End to end from JavaScript")[1]
    open(path, "w").write(s2)
    print("BASELINE.md section 5 rewritten")


if __name__ == "__main__":
    main()
