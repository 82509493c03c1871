#!/usr/bin/env python3
"""Batch decaf448 at 2^18 rows, each new path timed alternating with its Ed448 yardstick over device-resident buffers in this
process (HIP events on one explicit stream, --reps repetitions of --steps calls each, best of the repetitions reported, all of them
kept):
    decode        ncg_decaf448_decode_batch_dev        against  ncg_ed448_decode_batch_dev       counted: near 1 (one power chain each)
    encode        ncg_decaf448_encode_batch_dev        against  ncg_decaf448_decode_batch_dev    counted: near 1
    from_uniform  ncg_decaf448_from_uniform_batch_dev  against  ncg_decaf448_decode_batch_dev    counted: 3 (three chains)
    mul           ncg_decaf448_mul_batch_dev           against  ncg_ed448_mul_batch_dev          counted: near 1 (a chain for an inversion)
    mul_base      ncg_decaf448_mul_base_batch_dev      against  ncg_ed448_mul_base_batch_dev     counted: near 1
The counted expectations are written beside the measured ratios; nothing gates on them.  The encodings are valid elements
([k]BASE from the device).  Every path is checked once before it is timed: encode of decode gives the input back, [k]BASE by
mul_batch on the base encoding and by mul_base_batch agree, and from_uniform gives encodings that decode."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from noble_curves_amd import get_engine  # noqa: E402

# power chains (445 squarings + 13 products each) per item, counted from csrc/decaf448.hpp and csrc/ed448.hpp
COUNTED = {"decode_to_ed448_decode": 1.0, "encode_to_decode": 1.0, "from_uniform_to_decode": 3.0, "mul_to_ed448_mul": 1.0,
           "mul_base_to_ed448_mul_base": 1.0}
BASE_ENC = "66" * 28 + "33" * 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", default="18")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    eng = get_engine(0)
    L, h = eng.lib, eng.h
    gen = torch.Generator(device=dev)
    gen.manual_seed(448)
    res = {"steps": args.steps, "reps": args.reps, "counted_expectation": COUNTED}

    def ok(rc):
        eng._check(rc)

    def rnd(n, w):
        return torch.randint(0, 256, (n, w), dtype=torch.uint8, device=dev, generator=gen)

    def buf(n, w):
        return torch.empty((n, w), dtype=torch.uint8, device=dev)

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
        flag = buf(n, 1)
        k = rnd(n, 56)
        k[:, 55] &= 0x3F
        uni = rnd(n, 112)
        enc, enc2, out56, aff = buf(n, 56), buf(n, 56), buf(n, 56), buf(n, 112)
        pk57, out57, aff57 = buf(n, 57), buf(n, 57), buf(n, 112)
        ok(L.ncg_decaf448_mul_base_batch_dev(h, n, k.data_ptr(), enc.data_ptr(), s))
        ok(L.ncg_ed448_mul_base_batch_dev(h, n, k.data_ptr(), pk57.data_ptr(), s))
        # checks before timing
        ok(L.ncg_decaf448_decode_batch_dev(h, n, enc.data_ptr(), aff.data_ptr(), flag.data_ptr(), s))
        ok(L.ncg_decaf448_encode_batch_dev(h, n, aff.data_ptr(), enc2.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(enc, enc2) and bool(flag.all().item()), "encode(decode(e)) differs from e"
        base = torch.from_numpy(np.frombuffer(bytes.fromhex(BASE_ENC), dtype=np.uint8).copy()).to(dev).expand(n, 56).contiguous()
        ok(L.ncg_decaf448_mul_batch_dev(h, n, base.data_ptr(), k.data_ptr(), 0, enc2.data_ptr(), flag.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(enc, enc2) and bool(flag.all().item()), "[k]BASE by mul_batch and by mul_base_batch differ"
        ok(L.ncg_decaf448_from_uniform_batch_dev(h, n, uni.data_ptr(), enc2.data_ptr(), s))
        ok(L.ncg_decaf448_decode_batch_dev(h, n, enc2.data_ptr(), aff.data_ptr(), flag.data_ptr(), s))
        torch.cuda.synchronize()
        assert bool(flag.all().item()), "an element derived from uniform bytes does not decode"
        ok(L.ncg_decaf448_decode_batch_dev(h, n, enc.data_ptr(), aff.data_ptr(), flag.data_ptr(), s))

        fns = {
            "ed448_decode": lambda: ok(L.ncg_ed448_decode_batch_dev(h, n, pk57.data_ptr(), aff57.data_ptr(), flag.data_ptr(), s)),
            "decode": lambda: ok(L.ncg_decaf448_decode_batch_dev(h, n, enc.data_ptr(), aff.data_ptr(), flag.data_ptr(), s)),
            "encode": lambda: ok(L.ncg_decaf448_encode_batch_dev(h, n, aff.data_ptr(), out56.data_ptr(), s)),
            "from_uniform": lambda: ok(L.ncg_decaf448_from_uniform_batch_dev(h, n, uni.data_ptr(), out56.data_ptr(), s)),
            "ed448_mul": lambda: ok(L.ncg_ed448_mul_batch_dev(h, n, pk57.data_ptr(), k.data_ptr(), 0, out57.data_ptr(), flag.data_ptr(), s)),
            "mul": lambda: ok(L.ncg_decaf448_mul_batch_dev(h, n, enc.data_ptr(), k.data_ptr(), 0, out56.data_ptr(), flag.data_ptr(), s)),
            "ed448_mul_base": lambda: ok(L.ncg_ed448_mul_base_batch_dev(h, n, k.data_ptr(), out57.data_ptr(), s)),
            "mul_base": lambda: ok(L.ncg_decaf448_mul_base_batch_dev(h, n, k.data_ptr(), out56.data_ptr(), s)),
        }
        t = timed(fns)
        best = {key: min(v) for key, v in t.items()}
        entry = {
            "ms": {key: round(v, 4) for key, v in best.items()},
            "ms_reps": {key: [round(x, 4) for x in v] for key, v in t.items()},
            "ns_per_item": {key: round(v * 1e6 / n, 2) for key, v in best.items()},
            "ratios": {
                "decode_to_ed448_decode": round(best["decode"] / best["ed448_decode"], 3),
                "encode_to_decode": round(best["encode"] / best["decode"], 3),
                "from_uniform_to_decode": round(best["from_uniform"] / best["decode"], 3),
                "mul_to_ed448_mul": round(best["mul"] / best["ed448_mul"], 3),
                "mul_base_to_ed448_mul_base": round(best["mul_base"] / best["ed448_mul_base"], 3),
            },
        }
        res["2^%d" % bits] = entry
        for key in t:
            print("2^%-3d %-16s %9.4f ms  %9.2f ns/item  reps %s" % (bits, key, best[key], entry["ns_per_item"][key], entry["ms_reps"][key]),
                  flush=True)
        print("2^%-3d ratios %s (counted %s)" % (bits, entry["ratios"], COUNTED), flush=True)
    print(json.dumps({key: v["ratios"] for key, v in res.items() if isinstance(v, dict) and "ratios" in v}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
