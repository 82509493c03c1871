#!/usr/bin/env python3
"""Per-kernel timeline of the LAST MSM of each (curve, shape) in a rocprofv3 --kernel-trace CSV:
    python tools/msm_timeline.py <dir with *kernel_trace.csv> [--seq]
(--seq: every launch in order with its start offset, duration, grid in workgroups x.y, workgroup size and LDS bytes instead of the
per-kernel sums.)  An MSM is the kernel sequence from k_msm_digits* to k_msm_tail*.
    python tools/msm_timeline.py <dir> --launches [rows.json]
prints no times at all, so that two builds can be compared with diff: every launch of the MSM driver (k_msm_*, k_sort2_*) in stream order
as "kernel  grid x.y  workgroup size  LDS", and k_points_to_mont (it runs on a side stream, anywhere in timestamp order) as a sorted list
beside them.  rows.json = [[name, number of k_msm_tail launches], ...] cuts the trace into the rows of a job that ran them in that order."""
import csv, glob, json, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))


def short_name(nm):
    return nm.split("(")[0].replace("void ", "").replace("ncg::", "").replace("(anonymous namespace)::", "")


def shape(r):
    """grid in workgroups (the trace has it in work-items), workgroup size, LDS bytes"""
    wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
    g = [int(r["Grid_Size_" + a]) // max(1, w) for a, w in zip("XYZ", wg)]
    return "%d.%d" % (g[0], g[1] * g[2]), wg[0] * wg[1] * wg[2], int(next((v for k, v in r.items() if k.lower() == "lds_block_size"), 0) or 0)


if "--launches" in sys.argv:
    arg = sys.argv[sys.argv.index("--launches") + 1:]
    cuts = json.load(open(arg[0])) if arg else [["all", 1 << 30]]
    ci, tails, main, side = 0, 0, [], []

    def flush():
        print("== %s" % cuts[ci][0])
        for ln in main + sorted(side):
            print("   " + ln)

    for r in rows:
        nm = short_name(r["Kernel_Name"])
        if not any(k in nm for k in ("k_msm_", "k_sort2_", "k_points_to_mont")):
            continue
        ln = "%-64s %10s %5d %7d" % ((nm,) + shape(r))
        (side if "k_points_to_mont" in nm else main).append(ln)
        if "k_msm_tail" in nm:
            tails += 1
            if tails == cuts[ci][1] and ci + 1 < len(cuts):
                flush()
                ci, tails, main, side = ci + 1, 0, [], []
    flush()
    sys.exit(0)
seq = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) + shape(r) for r in rows]
msms, cur = [], None
for nm, t0, t1, grid, wg, lds in seq:
    short = nm.split("(")[0].replace("void ncg::", "").replace("ncg::", "")
    if "k_msm_digits" in nm or ("k_points_to_mont" in nm and cur is None):
        if cur is None:
            cur = {"t0": t0, "k": []}
    if cur is not None:
        cur["k"].append((short, t0, t1, grid, wg, lds))
        if "k_msm_tail" in nm:
            cur["t1"] = t1
            msms.append(cur)
            cur = None
last = {}
for m in msms:
    tag = next((k[0] for k in m["k"] if "k_msm_accum" in k[0]), "?")
    grid = tuple(sorted(set(k[0] for k in m["k"])))
    last[(tag, len(m["k"]), round((m["t1"] - m["t0"]) / 2e4))] = m
for (tag, nk, _), m in last.items():
    print("%s  %d launches  span %.1f us" % (tag, nk, (m["t1"] - m["t0"]) / 1e3))
    if "--seq" in sys.argv:
        for nm, t0, t1, grid, wg, lds in m["k"]:
            print("   +%8.1f us  %-58s %9.1f us  %10s %5d %7d" % ((t0 - m["t0"]) / 1e3, nm[:58], (t1 - t0) / 1e3, grid, wg, lds))
        continue
    agg = {}
    for nm, t0, t1 in (k[:3] for k in m["k"]):
        a = agg.setdefault(nm, [0, 0.0]); a[0] += 1; a[1] += (t1 - t0) / 1e3
    busy = sum(v[1] for v in agg.values())
    for nm, (c, t) in agg.items():
        print("   %-58s x%-3d %9.1f us" % (nm[:58], c, t))
    print("   %-58s      %9.1f us" % ("(gaps between kernels)", (m["t1"] - m["t0"]) / 1e3 - busy))
