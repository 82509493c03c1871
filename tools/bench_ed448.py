#!/usr/bin/env python3
"""Batch X448 / Ed448 at 2^14 and 2^18 rows, each path timed alternating with its 255-bit yardstick over device-resident buffers in
this process (HIP events on one explicit stream, --reps repetitions of --steps calls each, best of the repetitions reported, all
of them kept):
    x448              ncg_x448_batch_dev              against  ncg_x25519_batch_dev
    ed448_decode      ncg_ed448_decode_batch_dev      against  ncg_decode_points_batch_dev (NCG_ED25519, strict)
    ed448_mul         ncg_ed448_mul_batch_dev         against  ncg_mul_var_batch_dev (NCG_ED25519)
    ed448_verify      ncg_ed448_verify_batch_dev      against  ncg_ed25519_verify_batch_dev (the k-taking form, strict)
and the wall time of the host SHAKE256 challenge (hashlib, 32-byte messages) for the same number of rows.  The keys and R of the
verification rows are valid points ([k]B from the device), s and the challenge are random: the rows are refused, and both kernels
do the same work for a refused row as for an accepted one.  Every path is checked once before it is timed (the X448 ladder at
u = 5 against ncg_x448_base_batch, decode of encode, [k]B by both multiplies).  The counted multiply-add ratios beside the
measured ones: DESIGN.md section 8."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from noble_curves_amd import _native  # noqa: E402
from noble_curves_amd import get_engine  # noqa: E402

# multiply-adds counted from the code (csrc/x25519.hpp, csrc/ed448.hpp): per ladder step, and the steps
COUNTED = {"x448_to_x25519": round(448 * 1840 / (255 * 702), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", default="14,18")
    ap.add_argument("--steps", type=int, default=5)
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
    res = {"steps": args.steps, "reps": args.reps, "counted_multiply_add_ratio": COUNTED}
    ED = _native.ED25519

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
        flag, flag2 = buf(n, 1), buf(n, 1)
        # ---- 448 side
        sc4, u4, o4, o4b = rnd(n, 56), rnd(n, 56), buf(n, 56), buf(n, 56)
        k4 = rnd(n, 56)
        k4[:, 55] &= 0x3F
        pk4, r4, enc_out4, aff4 = buf(n, 57), buf(n, 57), buf(n, 57), buf(n, 112)
        ok(L.ncg_ed448_mul_base_batch_dev(h, n, k4.data_ptr(), pk4.data_ptr(), s))
        ok(L.ncg_ed448_mul_base_batch_dev(h, n, sc4.data_ptr(), r4.data_ptr(), s))
        sig4 = torch.cat([r4, k4, torch.zeros((n, 1), dtype=torch.uint8, device=dev)], dim=1).contiguous()
        # ---- 255 side
        sc2, u2, o2 = rnd(n, 32), rnd(n, 32), buf(n, 32)
        k2 = sc2.clone()
        k2[:, 31] &= 0x0F
        pts2, pout2, enc2, r2 = buf(n, 64), buf(n, 64), buf(n, 32), buf(n, 32)
        eng.mul_base_batch_dev(ED, n, k2.data_ptr(), pts2.data_ptr(), flag.data_ptr(), s)
        ok(L.ncg_encode_points_batch_dev(h, ED, n, pts2.data_ptr(), enc2.data_ptr(), flag.data_ptr(), s))
        r2.copy_(enc2.roll(1, 0))
        sig2 = torch.cat([r2, k2], dim=1).contiguous()

        fns = {
            "x25519": lambda: ok(L.ncg_x25519_batch_dev(h, n, sc2.data_ptr(), u2.data_ptr(), 0, o2.data_ptr(), flag.data_ptr(), s)),
            "x448": lambda: ok(L.ncg_x448_batch_dev(h, n, sc4.data_ptr(), u4.data_ptr(), 0, o4.data_ptr(), flag.data_ptr(), s)),
            "ed25519_decode": lambda: ok(L.ncg_decode_points_batch_dev(h, ED, n, enc2.data_ptr(), 0, pout2.data_ptr(), flag.data_ptr(),
                                                                      flag2.data_ptr(), s)),
            "ed448_decode": lambda: ok(L.ncg_ed448_decode_batch_dev(h, n, pk4.data_ptr(), aff4.data_ptr(), flag.data_ptr(), s)),
            "ed25519_mul": lambda: ok(L.ncg_mul_var_batch_dev(h, ED, n, pts2.data_ptr(), k2.data_ptr(), pout2.data_ptr(), flag2.data_ptr(), s)),
            "ed448_mul": lambda: ok(L.ncg_ed448_mul_batch_dev(h, n, pk4.data_ptr(), k4.data_ptr(), 0, enc_out4.data_ptr(), flag.data_ptr(), s)),
            "ed25519_verify": lambda: ok(L.ncg_ed25519_verify_batch_dev(h, n, sig2.data_ptr(), enc2.data_ptr(), k2.data_ptr(), 0,
                                                                        flag2.data_ptr(), s)),
            "ed448_verify": lambda: ok(L.ncg_ed448_verify_batch_dev(h, n, sig4.data_ptr(), pk4.data_ptr(), k4.data_ptr(), flag.data_ptr(), s)),
        }
        # checks before timing
        five = torch.zeros((n, 56), dtype=torch.uint8, device=dev)
        five[:, 0] = 5
        ok(L.ncg_x448_batch_dev(h, n, sc4.data_ptr(), five.data_ptr(), 0, o4.data_ptr(), flag.data_ptr(), s))
        ok(L.ncg_x448_base_batch_dev(h, n, sc4.data_ptr(), o4b.data_ptr(), flag2.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(o4, o4b) and bool(flag.all().item()), "the ladder at u = 5 and x448_base_batch differ"
        fns["ed448_decode"]()
        ok(L.ncg_ed448_encode_batch_dev(h, n, aff4.data_ptr(), enc_out4.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(enc_out4, pk4) and bool(flag.all().item()), "encode(decode(e)) differs from e"
        base = torch.from_numpy(np.frombuffer(bytes.fromhex(
            "14fa30f25b790898adc8d74e2c13bdfdc4397ce61cffd33ad7c2a0051e9c78874098a36c7373ea4b62c7c9563720768824bcb66e71463f6900"),
            dtype=np.uint8).copy()).to(dev).expand(n, 57).contiguous()
        ok(L.ncg_ed448_mul_batch_dev(h, n, base.data_ptr(), k4.data_ptr(), 0, enc_out4.data_ptr(), flag.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(enc_out4, pk4), "[k]B by mul_batch and by mul_base_batch differ"

        t = timed(fns)
        best = {k: min(v) for k, v in t.items()}
        m = min(n, 1 << 18)
        rows = [(bytes(57), bytes(57), b"m" * 32)] * m
        t0 = time.perf_counter()
        for r, a, msg in rows:
            int.from_bytes(hashlib.shake_256(b"SigEd448\0\0" + r + a + msg).digest(114), "little")
        host_ms = (time.perf_counter() - t0) * 1e3
        entry = {
            "ms": {k: round(v, 4) for k, v in best.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in best.items()},
            "ratios": {
                "x448_to_x25519": round(best["x448"] / best["x25519"], 3),
                "decode_448_to_255": round(best["ed448_decode"] / best["ed25519_decode"], 3),
                "mul_448_to_255": round(best["ed448_mul"] / best["ed25519_mul"], 3),
                "verify_448_to_255": round(best["ed448_verify"] / best["ed25519_verify"], 3),
            },
            "host_shake256_challenge_ms": round(host_ms, 2),
            "host_hash_share_of_verify_call": round(host_ms / (host_ms + best["ed448_verify"]), 3),
        }
        res["2^%d" % bits] = entry
        for k in t:
            print("2^%-3d %-16s %9.4f ms  %9.2f ns/item  reps %s" % (bits, k, best[k], entry["ns_per_item"][k], entry["ms_reps"][k]), flush=True)
        print("2^%-3d ratios %s host shake256 %.1f ms" % (bits, entry["ratios"], host_ms), flush=True)
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict) and "ratios" in v}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
