#!/usr/bin/env python3
"""Polynomial layer (ncg_poly_*_dev) over bls12-381 Fr and bn254 Fr at 2^--log2n elements: device-resident data, HIP-event timing
on one explicit stream, every candidate of a comparison timed alternating with its yardstick over the same buffers in this
process (--reps repetitions of --steps calls each, best of the repetitions reported, all of them kept):
  * pointwise add and dot beside a device-to-device copy of the same 96 bytes per element (two reads, one write);
  * ncg_poly_mul_dev beside two direct (natural -> bit-reversed) and one inverse (bit-reversed -> natural) ncg_ntt_dev;
  * the dot-sum, the monomial evaluation at 1 and at 8 points, the Lagrange basis.
Every operation is checked once before it is timed (against the other route to the same values).  The ratios the README and
DESIGN section 8 quote: add / copy, dot / copy, mul / three transforms, evaluation at 8 / at 1."""
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

FIELDS = {"bls12_381": (G.bls12_381_Fr, _native.FIELD_BLS12_381_FR, 0x3F), "bn254": (G.bn254_Fr, _native.FIELD_BN254_FR, 0x1F)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--field", default="bls12_381,bn254")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    eng = get_engine(0)
    bits, n = args.log2n, 1 << args.log2n
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    res = {"log2n": bits, "steps": args.steps, "reps": args.reps}

    def timed(fns):
        """{name: callable} timed alternating; returns {name: [ms per call of each repetition]}"""
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

    for f in args.field.split(","):
        fld, fid, mask = FIELDS[f]
        r = fld.ORDER
        om = G.rootsOfUnity(fld, 7).omega(bits)
        a = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        b = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        a[:, 31] &= mask
        b[:, 31] &= mask
        ab = torch.cat([a, b])                          # the copy's source
        out = torch.empty_like(a)
        cp = torch.empty((n + n // 2, 32), dtype=torch.uint8, device=dev)
        t1, t2 = torch.empty_like(a), torch.empty_like(a)
        small = torch.zeros((16, 32), dtype=torch.uint8, device=dev)
        xs = [pow(3, 1000 + 7 * k, r) for k in range(8)]
        P = dict(field=fid)

        def three_ntts():
            eng.ntt_dev(bits, 1, om, a.data_ptr(), t1.data_ptr(), s, brp_output=True, **P)
            eng.ntt_dev(bits, 1, om, b.data_ptr(), t2.data_ptr(), s, brp_output=True, **P)
            eng.ntt_dev(bits, 1, om, t1.data_ptr(), t1.data_ptr(), s, inverse=True, brp_input=True, **P)

        def copy96():                                   # 48 bytes in and 48 out per element: the 96 bytes add and dot move
            cp.copy_(ab[:n + n // 2])

        # checks before timing: dot through the transforms == mul; eval of the product at a point == product of the evals
        eng.poly_mul_dev(bits, om, n // 2, a.data_ptr(), n // 2, b.data_ptr(), out.data_ptr(), s, **P)
        eng.poly_eval_monomial_dev(n, out.data_ptr(), xs[:1], small.data_ptr(), s, **P)
        eng.poly_eval_monomial_dev(n // 2, a.data_ptr(), xs[:1], small.data_ptr() + 32, s, **P)
        eng.poly_eval_monomial_dev(n // 2, b.data_ptr(), xs[:1], small.data_ptr() + 64, s, **P)
        torch.cuda.synchronize()
        v = _native.le_to_ints(small[:3].cpu().numpy(), 32)
        assert v[0] == v[1] * v[2] % r, "%s: eval(a b, x) != eval(a, x) eval(b, x)" % f
        eng.poly_eval_monomial_dev(n, a.data_ptr(), xs, small.data_ptr(), s, **P)
        eng.poly_eval_monomial_dev(n, a.data_ptr(), xs[7:], small.data_ptr() + 256, s, **P)
        eng.poly_scale_dev(n, b.data_ptr(), xs[7], True, out.data_ptr(), s, **P)       # b[i] x^i
        eng.poly_pointwise_dev(_native.POLY_SUB, n, out.data_ptr(), out.data_ptr(), t1.data_ptr(), s, **P)
        eng.poly_lagrange_basis_dev(bits, om, xs[0], False, out.data_ptr(), s, **P)
        eng.poly_pointwise_dev(_native.POLY_ADD, n, out.data_ptr(), t1.data_ptr(), t2.data_ptr(), s, **P)
        eng.poly_eval_dev(n, t2.data_ptr(), a.data_ptr(), small.data_ptr() + 288, s, **P)
        eng.poly_eval_dev(n, out.data_ptr(), a.data_ptr(), small.data_ptr() + 320, s, **P)
        torch.cuda.synchronize()
        v = _native.le_to_ints(small[:11].cpu().numpy(), 32)
        assert v[7] == v[8], "%s: evaluation at 8 points != at 1" % f
        assert v[9] == v[10] and not bool(t1.any().item()), "%s: sub / add / eval disagree" % f

        t = timed({
            "copy_96B": copy96,
            "add": lambda: eng.poly_pointwise_dev(_native.POLY_ADD, n, a.data_ptr(), b.data_ptr(), out.data_ptr(), s, **P),
            "dot": lambda: eng.poly_pointwise_dev(_native.POLY_DOT, n, a.data_ptr(), b.data_ptr(), out.data_ptr(), s, **P),
        })
        t.update(timed({
            "three_ntts": three_ntts,
            "mul": lambda: eng.poly_mul_dev(bits, om, n, a.data_ptr(), n, b.data_ptr(), out.data_ptr(), s, **P),
        }))
        t.update(timed({
            "eval_monomial_1": lambda: eng.poly_eval_monomial_dev(n, a.data_ptr(), xs[:1], small.data_ptr(), s, **P),
            "eval_monomial_8": lambda: eng.poly_eval_monomial_dev(n, a.data_ptr(), xs, small.data_ptr(), s, **P),
            "dot_sum": lambda: eng.poly_eval_dev(n, a.data_ptr(), b.data_ptr(), small.data_ptr(), s, **P),
            "shift": lambda: eng.poly_scale_dev(n, a.data_ptr(), xs[0], True, out.data_ptr(), s, **P),
            "lagrange_basis": lambda: eng.poly_lagrange_basis_dev(bits, om, xs[0], False, out.data_ptr(), s, **P),
        }))
        best = {k: min(v) for k, v in t.items()}
        res[f] = {
            "ms": {k: round(v, 4) for k, v in best.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "GBps_96B_per_element": {k: round(n * 96 / (best[k] * 1e-3) / 1e9, 1) for k in ("copy_96B", "add", "dot")},
            "ratios": {
                "add_to_copy": round(best["add"] / best["copy_96B"], 3),
                "dot_to_copy": round(best["dot"] / best["copy_96B"], 3),
                "mul_to_three_ntts": round(best["mul"] / best["three_ntts"], 3),
                "eval8_to_eval1": round(best["eval_monomial_8"] / best["eval_monomial_1"], 3),
            },
        }
        for k in t:
            print("%-10s %-18s %9.4f ms  reps %s" % (f, k, best[k], res[f]["ms_reps"][k]), flush=True)
        print("%-10s ratios %s" % (f, res[f]["ratios"]), flush=True)
        del a, b, ab, out, cp, t1, t2
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict)}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
