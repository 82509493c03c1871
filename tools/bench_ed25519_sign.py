#!/usr/bin/env python3
"""Batch Ed25519 signing at 2^18 and 2^20 rows of 32-byte messages, each form beside its yardstick on the same rows:
  (a) ncg_ed25519_sign_batch_dev, expanded keys, ONE_KEY      against ncg_ed25519_verify_batch_msgs_dev of those signatures
  (b) ncg_ed25519_sign_batch_dev from per-row seeds            against the same verification
  (c) ncg_ed25519_public_key_batch_dev                         against ncg_mul_base_batch_dev + ncg_encode_points_batch_dev (the
      indexed-table route to the same bytes, from the already expanded scalars: it has no hash in it)
Device-resident inputs, HIP-event timing on one explicit stream, the candidates timed alternating over the same buffers in this
process (--reps repetitions of --steps calls each after one warm-up call each; median, minimum and maximum of the repetitions are
reported, all of them kept).  Every result is checked once before it is timed: the signatures verify, (a) and (b) agree on row 0's
key, and the two routes to a public key give the same bytes.  The clock and package power the box holds under (a) and under the
verification are recorded with bench.py's power_state.  `expected` holds the ratios counted from the multiply-add and select
counts of DESIGN.md section 8 "Ed25519 signing" before anything was measured.  The walk alone against k_ed_mul_base alone is NOT timed
here: the scan kernel ends with the per-lane inversion and the compression and no entry point stops before them; the kernel durations
of a trace of this script (a run of its own) are set against each other in DESIGN.md instead."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from noble_curves_amd import _native  # noqa: E402
from noble_curves_amd import get_engine  # noqa: E402

EXPECTED = {"sign_expanded_one_key_to_verify": 0.3, "sign_seeds_to_verify": 0.55, "public_key_to_indexed_route": 2.2}


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
    gen.manual_seed(8032)
    res = {"steps": args.steps, "reps": args.reps, "expected": EXPECTED}

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
        seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * 32).contiguous()
        rows = torch.empty((n, 96), dtype=torch.uint8, device=dev)
        ok(L.ncg_ed25519_expand_key_batch_dev(h, n, seeds.data_ptr(), rows.data_ptr(), s))
        torch.cuda.synchronize()
        pk_rows = rows[:, 64:].contiguous()
        pk_one = rows[:1, 64:].expand(n, 32).contiguous()
        scalars = rows[:, :32].contiguous()
        sig_a, sig_b = torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, 64), dtype=torch.uint8, device=dev)
        flag, verdict = torch.empty((n,), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.uint8, device=dev)
        pk_scan, pk_idx = torch.empty((n, 32), dtype=torch.uint8, device=dev), torch.empty((n, 32), dtype=torch.uint8, device=dev)
        pts = torch.empty((n, 64), dtype=torch.uint8, device=dev)

        def sign_a():
            ok(L.ncg_ed25519_sign_batch_dev(h, n, rows.data_ptr(), _native.ED25519_SIGN_EXPANDED | _native.ED25519_SIGN_ONE_KEY, None, 0,
                                            msgs.data_ptr(), off.data_ptr(), sig_a.data_ptr(), flag.data_ptr(), s))

        def sign_b():
            ok(L.ncg_ed25519_sign_batch_dev(h, n, seeds.data_ptr(), 0, None, 0, msgs.data_ptr(), off.data_ptr(), sig_b.data_ptr(),
                                            flag.data_ptr(), s))

        def verify(sig, pk):
            ok(L.ncg_ed25519_verify_batch_msgs_dev(h, n, sig.data_ptr(), pk.data_ptr(), msgs.data_ptr(), off.data_ptr(), 0,
                                                   verdict.data_ptr(), s))

        def indexed_route():
            eng.mul_base_batch_dev(_native.ED25519, n, scalars.data_ptr(), pts.data_ptr(), flag.data_ptr(), s)
            ok(L.ncg_encode_points_batch_dev(h, _native.ED25519, n, pts.data_ptr(), pk_idx.data_ptr(), flag.data_ptr(), s))

        fns = {
            "sign_expanded_one_key": sign_a,
            "verify_of_a": lambda: verify(sig_a, pk_one),
            "sign_seeds": sign_b,
            "verify_of_b": lambda: verify(sig_b, pk_rows),
            "public_key": lambda: ok(L.ncg_ed25519_public_key_batch_dev(h, n, seeds.data_ptr(), pk_scan.data_ptr(), s)),
            "mul_base_plus_encode": indexed_route,
        }
        # checks before timing
        for name, key in (("sign_expanded_one_key", "verify_of_a"), ("sign_seeds", "verify_of_b")):
            fns[name]()
            torch.cuda.synchronize()
            assert bool(flag.all().item()), name + " refused a row"
            fns[key]()
            torch.cuda.synchronize()
            assert bool(verdict.all().item()), name + ": a signature does not verify"
        assert torch.equal(sig_a[0], sig_b[0]), "expanded and seed forms differ on the shared key"
        fns["public_key"]()
        fns["mul_base_plus_encode"]()
        torch.cuda.synchronize()
        assert torch.equal(pk_scan, pk_idx) and torch.equal(pk_scan, pk_rows), "the two routes to a public key differ"

        t = timed(fns)
        med = {k: statistics.median(v) for k, v in t.items()}
        ratios = {
            "sign_expanded_one_key_to_verify": round(med["sign_expanded_one_key"] / med["verify_of_a"], 3),
            "sign_seeds_to_verify": round(med["sign_seeds"] / med["verify_of_b"], 3),
            "public_key_to_indexed_route": round(med["public_key"] / med["mul_base_plus_encode"], 3),
        }
        entry = {
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in med.items()},
            "per_second": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            "ratios": ratios,
        }
        try:   # the clock and package power held under the two kernels mixes (untimed leg; hwmon of the visible GPU)
            import bench
            entry["power_state_sign"] = bench.power_state(sign_a, 0)
            entry["power_state_verify"] = bench.power_state(fns["verify_of_a"], 0)
        except Exception as e:  # noqa: BLE001 - a measurement beside the result
            entry["power_state_error"] = repr(e)
        res["2^%d" % bits] = entry
        for k in t:
            print("2^%-3d %-24s median %9.4f ms  [%9.4f, %9.4f]  %8.2f ns/item" % (bits, k, med[k], min(t[k]), max(t[k]),
                                                                                    entry["ns_per_item"][k]), flush=True)
        print("2^%-3d ratios %s expected %s" % (bits, ratios, EXPECTED), flush=True)
        del seeds, msgs, off, rows, pk_rows, pk_one, scalars, sig_a, sig_b, flag, verdict, pk_scan, pk_idx, pts
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict) and "ratios" in v}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
