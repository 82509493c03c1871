#!/usr/bin/env python3
"""Batch X25519 (ncg_x25519_batch_dev) at 2^18 and 2^20 rows beside its yardstick, the ed25519 variable-base multiply
(ncg_mul_var_batch_dev on NCG_ED25519) at the same n: device-resident inputs, HIP-event timing on one explicit stream, the
candidates timed alternating over the same buffers in this process (--reps repetitions of --steps calls each, best of the
repetitions reported, all of them kept).  Also the two routes to a public key - ncg_x25519_base_batch_dev (the fixed-base Edwards
table) against the ladder at u = 9 - the one-scalar form and ncg_ed25519_to_montgomery_batch_dev.  Every operation is checked once
before it is timed (the two routes against each other, the one-scalar form against the per-row one).  The clock and package power
the box holds under the ladder are recorded with bench.py's power_state.  The ratio DESIGN.md section 8 quotes: x25519 / mul_var."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from noble_curves_amd import _native  # noqa: E402
from noble_curves_amd import get_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", default="18,20")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    eng = get_engine(0)
    L, h = eng.lib, eng.h
    gen = torch.Generator(device=dev)
    gen.manual_seed(25519)
    res = {"steps": args.steps, "reps": args.reps}

    def ok(rc):
        eng._check(rc)

    def timed(fns):
        times = {k: [] for k in fns}
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.steps)
        return times

    for bits in [int(b) for b in args.log2n.split(",")]:
        n = 1 << bits
        sc = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        u = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        nine = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        nine[:, 0] = 9
        out, out2 = torch.empty_like(u), torch.empty_like(u)
        flag, flag2 = torch.empty((n,), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.uint8, device=dev)
        # the yardstick's operands: n ed25519 points (multiples of the base point) and scalars below 2^252
        ks = sc.clone()
        ks[:, 31] &= 0x0F
        pts, pout = torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, 64), dtype=torch.uint8, device=dev)
        eng.mul_base_batch_dev(_native.ED25519, n, ks.data_ptr(), pts.data_ptr(), flag.data_ptr(), s)
        keys = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        ok(L.ncg_encode_points_batch_dev(h, _native.ED25519, n, pts.data_ptr(), keys.data_ptr(), flag.data_ptr(), s))

        fns = {
            "mul_var_ed25519": lambda: ok(L.ncg_mul_var_batch_dev(h, _native.ED25519, n, pts.data_ptr(), ks.data_ptr(), pout.data_ptr(),
                                                                  flag2.data_ptr(), s)),
            "x25519": lambda: ok(L.ncg_x25519_batch_dev(h, n, sc.data_ptr(), u.data_ptr(), 0, out.data_ptr(), flag.data_ptr(), s)),
            "x25519_one_scalar": lambda: ok(L.ncg_x25519_batch_dev(h, n, sc.data_ptr(), u.data_ptr(), 1, out.data_ptr(), flag.data_ptr(), s)),
            "base_table": lambda: ok(L.ncg_x25519_base_batch_dev(h, n, sc.data_ptr(), out2.data_ptr(), flag2.data_ptr(), s)),
            "base_ladder_u9": lambda: ok(L.ncg_x25519_batch_dev(h, n, sc.data_ptr(), nine.data_ptr(), 0, out.data_ptr(), flag.data_ptr(), s)),
            "to_montgomery": lambda: ok(L.ncg_ed25519_to_montgomery_batch_dev(h, n, keys.data_ptr(), out2.data_ptr(), flag2.data_ptr(), s)),
        }
        # checks before timing
        fns["base_table"]()
        fns["base_ladder_u9"]()
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and bool(flag.all().item()) and bool(flag2.all().item()), "table and ladder public keys differ"
        rows = min(n, 4096)
        fns["x25519_one_scalar"]()
        first = out[:rows].clone()
        ok(L.ncg_x25519_batch_dev(h, rows, sc[:1].expand(rows, 32).contiguous().data_ptr(), u.data_ptr(), 0, out2.data_ptr(), flag2.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(first, out2[:rows]), "one-scalar form differs from the per-row form"
        fns["to_montgomery"]()
        torch.cuda.synchronize()
        assert bool(flag2.all().item()), "toMontgomery refused a valid key"

        t = timed(fns)
        best = {k: min(v) for k, v in t.items()}
        entry = {
            "ms": {k: round(v, 4) for k, v in best.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in best.items()},
            "ratios": {
                "x25519_to_mul_var": round(best["x25519"] / best["mul_var_ed25519"], 3),
                "base_table_to_base_ladder": round(best["base_table"] / best["base_ladder_u9"], 3),
            },
        }
        try:   # the clock and package power held under the ladder (untimed leg; hwmon of the visible GPU)
            import bench
            entry["power_state_x25519"] = bench.power_state(fns["x25519"], 0)
            entry["power_state_mul_var"] = bench.power_state(fns["mul_var_ed25519"], 0)
        except Exception as e:  # noqa: BLE001 - a measurement beside the result
            entry["power_state_error"] = repr(e)
        res["2^%d" % bits] = entry
        for k in t:
            print("2^%-3d %-18s %9.4f ms  %8.2f ns/item  reps %s" % (bits, k, best[k], entry["ns_per_item"][k], entry["ms_reps"][k]), flush=True)
        print("2^%-3d ratios %s" % (bits, entry["ratios"]), flush=True)
        del sc, u, nine, out, out2, pts, pout, ks, keys
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict)}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
