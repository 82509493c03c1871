#!/usr/bin/env python3
"""Batch ristretto255 (ncg_ristretto_*_dev) at 2^18 and 2^20 rows, each path beside its yardstick at the same n: device-resident
inputs, HIP-event timing on one explicit stream, the compared paths timed alternating over the same buffers in this process
(--reps repetitions of --steps calls each, best of the repetitions reported, all of them kept).
    decode        against ncg_decode_points_batch_dev(NCG_ED25519, strict)
    encode        against ncg_encode_points_batch_dev(NCG_ED25519)
    from_uniform  against the ristretto decode
    mul_batch     against ncg_mul_var_batch_dev(NCG_ED25519) alone (and the one-scalar form)
    mul_base      against ncg_mul_base_batch_dev(NCG_ED25519)
    msm           from bytes against ncg_msm_dev on points already decoded (2^18 only; one call per step, synchronous)
Every path is checked once before it is timed (decode then encode gives the bytes back; mul_base against mul of the encoded base
point on the first rows)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from noble_curves_amd import _native  # noqa: E402
from noble_curves_amd import get_engine  # noqa: E402

ED = _native.ED25519


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
    gen.manual_seed(9496)
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

    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    for bits in [int(b) for b in args.log2n.split(",")]:
        n = 1 << bits
        ks = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        ks[:, 31] &= 0x0F                                       # below 2^252: valid for the MSM as well
        uni = torch.randint(0, 256, (n, 64), dtype=torch.uint8, device=dev, generator=gen)
        enc, enc2, out32 = u8(n, 32), u8(n, 32), u8(n, 32)
        pts, pts2 = u8(n, 64), u8(n, 64)
        flag, flag2 = u8(n), u8(n)
        # n valid elements: hashed points; their representatives; their ed25519 encodings for the yardstick decoder
        ok(L.ncg_ristretto_from_uniform_batch_dev(h, n, uni.data_ptr(), enc.data_ptr(), None, s))
        ok(L.ncg_ristretto_decode_batch_dev(h, n, enc.data_ptr(), pts.data_ptr(), flag.data_ptr(), s))
        ed_enc = u8(n, 32)
        ok(L.ncg_encode_points_batch_dev(h, ED, n, pts.data_ptr(), ed_enc.data_ptr(), flag2.data_ptr(), s))
        ok(L.ncg_ristretto_encode_batch_dev(h, n, pts.data_ptr(), enc2.data_ptr(), s))
        torch.cuda.synchronize()
        assert bool(flag.all().item()) and bool(flag2.all().item()) and torch.equal(enc, enc2), "decode then encode changed the bytes"
        rows = min(n, 4096)
        base = torch.from_numpy(np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), np.uint8).copy())
        base = base.to(dev).expand(rows, 32).contiguous()
        ok(L.ncg_ristretto_mul_batch_dev(h, rows, base.data_ptr(), ks.data_ptr(), 0, out32.data_ptr(), flag.data_ptr(), s))
        ok(L.ncg_ristretto_mul_base_batch_dev(h, rows, ks.data_ptr(), enc2.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(out32[:rows], enc2[:rows]), "mul_base differs from mul of the encoded base point"

        fns = {
            "ed25519_decode_strict": lambda: ok(L.ncg_decode_points_batch_dev(h, ED, n, ed_enc.data_ptr(), 0, pts2.data_ptr(), flag.data_ptr(),
                                                                              flag2.data_ptr(), s)),
            "ristretto_decode": lambda: ok(L.ncg_ristretto_decode_batch_dev(h, n, enc.data_ptr(), pts2.data_ptr(), flag.data_ptr(), s)),
            "ed25519_encode": lambda: ok(L.ncg_encode_points_batch_dev(h, ED, n, pts.data_ptr(), enc2.data_ptr(), flag.data_ptr(), s)),
            "ristretto_encode": lambda: ok(L.ncg_ristretto_encode_batch_dev(h, n, pts.data_ptr(), enc2.data_ptr(), s)),
            "ristretto_from_uniform": lambda: ok(L.ncg_ristretto_from_uniform_batch_dev(h, n, uni.data_ptr(), out32.data_ptr(), None, s)),
            "ed25519_mul_var": lambda: ok(L.ncg_mul_var_batch_dev(h, ED, n, pts.data_ptr(), ks.data_ptr(), pts2.data_ptr(), flag2.data_ptr(), s)),
            "ristretto_mul": lambda: ok(L.ncg_ristretto_mul_batch_dev(h, n, enc.data_ptr(), ks.data_ptr(), 0, out32.data_ptr(), flag.data_ptr(), s)),
            "ristretto_mul_one_scalar": lambda: ok(L.ncg_ristretto_mul_batch_dev(h, n, enc.data_ptr(), ks.data_ptr(), 1, out32.data_ptr(),
                                                                                 flag.data_ptr(), s)),
            "ed25519_mul_base": lambda: ok(L.ncg_mul_base_batch_dev(h, ED, n, ks.data_ptr(), pts2.data_ptr(), flag2.data_ptr(), s)),
            "ristretto_mul_base": lambda: ok(L.ncg_ristretto_mul_base_batch_dev(h, n, ks.data_ptr(), out32.data_ptr(), s)),
        }
        if bits <= 18:
            host_pt, host32 = np.zeros(64, np.uint8), np.zeros(32, np.uint8)
            inf, bad = ctypes.c_uint8(0), ctypes.c_int64(-1)
            fns["ed25519_msm_decoded"] = lambda: ok(L.ncg_msm_dev(h, ED, n, pts.data_ptr(), ks.data_ptr(), host_pt.ctypes.data, ctypes.byref(inf), s))
            fns["ristretto_msm_from_bytes"] = lambda: ok(L.ncg_ristretto_msm_dev(h, n, enc.data_ptr(), ks.data_ptr(), host32.ctypes.data,
                                                                                ctypes.byref(bad), s))
        t = timed(fns)
        best = {k: min(v) for k, v in t.items()}
        ratios = {
            "decode_to_ed25519_decode": best["ristretto_decode"] / best["ed25519_decode_strict"],
            "encode_to_ed25519_encode": best["ristretto_encode"] / best["ed25519_encode"],
            "from_uniform_to_decode": best["ristretto_from_uniform"] / best["ristretto_decode"],
            "mul_to_ed25519_mul_var": best["ristretto_mul"] / best["ed25519_mul_var"],
            "mul_one_scalar_to_ed25519_mul_var": best["ristretto_mul_one_scalar"] / best["ed25519_mul_var"],
            "mul_base_to_ed25519_mul_base": best["ristretto_mul_base"] / best["ed25519_mul_base"],
        }
        if "ristretto_msm_from_bytes" in best:
            ratios["msm_from_bytes_to_msm_decoded"] = best["ristretto_msm_from_bytes"] / best["ed25519_msm_decoded"]
        entry = {
            "ms": {k: round(v, 4) for k, v in best.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in best.items()},
            "ratios": {k: round(v, 3) for k, v in ratios.items()},
        }
        res["2^%d" % bits] = entry
        for k in t:
            print("2^%-3d %-26s %9.4f ms  %8.2f ns/item  reps %s" % (bits, k, best[k], entry["ns_per_item"][k], entry["ms_reps"][k]), flush=True)
        print("2^%-3d ratios %s" % (bits, entry["ratios"]), flush=True)
        del ks, uni, enc, enc2, out32, pts, pts2, flag, flag2, ed_enc
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict)}))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in res.items()) + "\n}\n")   # one size per line


if __name__ == "__main__":
    main()
