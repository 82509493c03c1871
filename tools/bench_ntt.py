#!/usr/bin/env python3
"""NTT over bls12-381 Fr or bn254 Fr: time per transform for several sizes / orderings with device-resident
data, HIP-event timing on an explicit stream.  Reports elements/s and the effective HBM rate
N * 64 B / t (one read + one write of the data is the algorithmic traffic).  Every size is checked
by inverse(direct(x)) == x on the device before it is timed.
--field bls12_381|bn254 picks the field; --field bls12_381,bn254 times the two alternating at every size and ordering
(--reps repetitions of --steps transforms each) and adds the ratio of the second field's best time to the first's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from noble_curves_amd import _native  # noqa: E402
from noble_curves_amd import fft as G  # noqa: E402
from noble_curves_amd import get_engine  # noqa: E402

# field -> (mirror field, ncg field id, mask of the top byte that keeps random bytes below r: 2^254 < r resp. 2^253 < r)
FIELDS = {"bls12_381": (G.bls12_381_Fr, _native.FIELD_BLS12_381_FR, 0x3F), "bn254": (G.bn254_Fr, _native.FIELD_BN254_FR, 0x1F)}
ORDERINGS = (("natural->natural", {}), ("natural->bitrev", {"brp_output": True}),
             ("bitrev->natural inverse", {"inverse": True, "brp_input": True}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="12,16,20,22,24")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--field", default="bls12_381", help="bls12_381, bn254 or both separated by a comma (timed alternating)")
    ap.add_argument("--reps", type=int, default=1, help="repetitions of the timed loop per field, size and ordering")
    args = ap.parse_args()
    fields = args.field.split(",")
    for f in fields:
        if f not in FIELDS:
            ap.error("--field: %s is not one of %s" % (f, ", ".join(FIELDS)))
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    eng = get_engine(0)
    res = {}
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for bits in [int(x) for x in args.sizes.split(",")]:
        n = 1 << bits
        batch = max(1, (1 << 22) >> bits) if bits < 22 else 1
        x = torch.randint(0, 256, (batch * n, 32), dtype=torch.uint8, device=dev, generator=gen)
        x[:, 31] &= min(FIELDS[f][2] for f in fields)      # canonical residues of every field timed
        y = torch.empty_like(x)
        z = torch.empty_like(x)
        run = {}
        for f in fields:
            fld, fid, _ = FIELDS[f]
            om = G.rootsOfUnity(fld, 7).omega(bits)
            run[f] = lambda src, dst, om=om, fid=fid, **kw: eng.ntt_dev(bits, batch, om, src.data_ptr(), dst.data_ptr(), s, field=fid, **kw)
            run[f](x, y)
            run[f](y, z, inverse=True)
            torch.cuda.synchronize()
            assert bool((z == x).all().item()), "%s: inverse(direct(x)) != x at 2^%d" % (f, bits)
            run[f](x, y, brp_output=True)
            run[f](y, z, inverse=True, brp_input=True)
            torch.cuda.synchronize()
            assert bool((z == x).all().item()), "%s: brp round trip failed at 2^%d" % (f, bits)
        for name, kw in ORDERINGS:
            times = {f: [] for f in fields}
            for _ in range(args.reps):
                for f in fields:                           # alternating: field A, field B, field A, ...
                    run[f](x, y, **kw)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        run[f](x, y, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    times[f].append(e0.elapsed_time(e1) / args.steps)
            for f in fields:
                ms = min(times[f])
                key = "2^%d x%d %s" % (bits, batch, name) if fields == ["bls12_381"] else "%s 2^%d x%d %s" % (f, bits, batch, name)
                res[key] = {"field": f, "log2n": bits, "batch": batch, "ms": round(ms, 4), "ms_reps": [round(t, 4) for t in times[f]],
                            "elements_per_s": batch * n / (ms * 1e-3), "butterflies_per_s": batch * n / 2 * bits / (ms * 1e-3),
                            "algorithmic_GBps": batch * n * 64 / (ms * 1e-3) / 1e9}
                print("%-52s %9.4f ms  %.3e elem/s  %.3e bfly/s  %7.1f GB/s (N*64B/t)  reps %s" % (
                    key, ms, res[key]["elements_per_s"], res[key]["butterflies_per_s"], res[key]["algorithmic_GBps"],
                    res[key]["ms_reps"]), flush=True)
            if len(fields) == 2:
                a, b = fields
                key = "ratio %s/%s 2^%d x%d %s" % (b, a, bits, batch, name)
                res[key] = {"log2n": bits, "batch": batch, "ratio": round(min(times[b]) / min(times[a]), 4),
                            "spread": {f: round(max(times[f]) / min(times[f]) - 1, 4) for f in fields}}
                print("%-52s %9.4f  run-to-run spread %s" % (key, res[key]["ratio"], res[key]["spread"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
