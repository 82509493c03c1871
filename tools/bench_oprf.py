#!/usr/bin/env python3
"""The ristretto255 OPRF (ncg_oprf_*_dev) at 2^16 and 2^18 rows of 32-byte inputs, each path beside its yardstick at the same n:
device-resident inputs, HIP-event timing on one explicit stream, the compared paths timed alternating over the same buffers in this
process (--reps repetitions of --steps calls each, the MEDIAN of the repetitions reported, all of them kept).
    mul                against ncg_ristretto_mul_batch_dev, the scalar-indexed multiply (and the INVERT and ONE_SCALAR forms)
    blind              against ncg_ristretto_from_uniform_batch_dev followed by ncg_ristretto_mul_batch_dev
    finalize           against ncg_oprf_mul_batch_dev with INVERT
    composite_scalars  against ncg_ristretto_hash_to_scalar_batch_dev on messages of the length a composite transcript has (145 bytes)
    generate_proof, verify_proof  against one and two ncg_ristretto_msm_dev of the same n; the row index of a proof must fit 16 bits,
                       so these run at n = 65535 only (they synchronise: one call per step)
Every path is checked once before it is timed: blind, multiply by a key, finalize gives what evaluate gives, and the generated
proof verifies."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from noble_curves_amd import get_engine  # noqa: E402

ONE_SCALAR, INVERT = 1, 2
TRANSCRIPT_BYTES = 2 + 64 + 2 + 2 + 32 + 2 + 32 + 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", default="16,18")
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
    gen.manual_seed(9497)
    res = {"steps": args.steps, "reps": args.reps, "input_bytes": 32}

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
    offsets = lambda n, width: torch.from_numpy(np.arange(n + 1, dtype=np.int64) * width).to(dev)  # noqa: E731  (uint64 offsets, same bits)
    for bits in [int(b) for b in args.log2n.split(",")]:
        n = 1 << bits
        ks = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        ks[:, 31] &= 0x0F                                       # below 2^252 < L
        inputs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        uni = torch.randint(0, 256, (n, 64), dtype=torch.uint8, device=dev, generator=gen)
        msgs = torch.randint(0, 256, (n, TRANSCRIPT_BYTES), dtype=torch.uint8, device=dev, generator=gen)
        off32, offm = offsets(n, 32), offsets(n, TRANSCRIPT_BYTES)
        blinded, evaluated, out32, out64, out64b = u8(n, 32), u8(n, 32), u8(n, 32), u8(n, 64), u8(n, 64)
        status, flag = u8(n), u8(n)
        key = ks[7:8].clone()
        # check: blind -> multiply by the key -> finalize equals evaluate
        ok(L.ncg_oprf_blind_batch_dev(h, 0, 0, n, inputs.data_ptr(), off32.data_ptr(), ks.data_ptr(), blinded.data_ptr(), status.data_ptr(), s))
        ok(L.ncg_oprf_mul_batch_dev(h, 0, n, blinded.data_ptr(), key.data_ptr(), ONE_SCALAR, evaluated.data_ptr(), flag.data_ptr(), s))
        ok(L.ncg_oprf_finalize_batch_dev(h, 0, 0, n, inputs.data_ptr(), off32.data_ptr(), None, 0, ks.data_ptr(), evaluated.data_ptr(),
                                         out64.data_ptr(), status.data_ptr(), s))
        ok(L.ncg_oprf_evaluate_batch_dev(h, 0, 0, n, inputs.data_ptr(), off32.data_ptr(), None, 0, key.data_ptr(), ONE_SCALAR, out64b.data_ptr(),
                                         flag.data_ptr(), s))
        torch.cuda.synchronize()
        assert not bool(status.any().item()) and not bool(flag.any().item()) and torch.equal(out64, out64b), "finalize differs from evaluate"
        B = eng.oprf_mul_batch(np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), np.uint8),
                               key.cpu().numpy(), one_scalar=True)[0][0].tobytes()

        fns = {
            "ristretto_mul": lambda: ok(L.ncg_ristretto_mul_batch_dev(h, n, blinded.data_ptr(), ks.data_ptr(), 0, out32.data_ptr(), flag.data_ptr(), s)),
            "oprf_mul": lambda: ok(L.ncg_oprf_mul_batch_dev(h, 0, n, blinded.data_ptr(), ks.data_ptr(), 0, out32.data_ptr(), flag.data_ptr(), s)),
            "oprf_mul_invert": lambda: ok(L.ncg_oprf_mul_batch_dev(h, 0, n, blinded.data_ptr(), ks.data_ptr(), INVERT, out32.data_ptr(),
                                                                   flag.data_ptr(), s)),
            "oprf_mul_one_scalar": lambda: ok(L.ncg_oprf_mul_batch_dev(h, 0, n, blinded.data_ptr(), key.data_ptr(), ONE_SCALAR, out32.data_ptr(),
                                                                       flag.data_ptr(), s)),
            "from_uniform_then_ristretto_mul": lambda: (
                ok(L.ncg_ristretto_from_uniform_batch_dev(h, n, uni.data_ptr(), evaluated.data_ptr(), None, s)),
                ok(L.ncg_ristretto_mul_batch_dev(h, n, evaluated.data_ptr(), ks.data_ptr(), 0, out32.data_ptr(), flag.data_ptr(), s))),
            "oprf_blind": lambda: ok(L.ncg_oprf_blind_batch_dev(h, 0, 0, n, inputs.data_ptr(), off32.data_ptr(), ks.data_ptr(), out32.data_ptr(),
                                                                status.data_ptr(), s)),
            "oprf_finalize": lambda: ok(L.ncg_oprf_finalize_batch_dev(h, 0, 0, n, inputs.data_ptr(), off32.data_ptr(), None, 0, ks.data_ptr(),
                                                                      blinded.data_ptr(), out64.data_ptr(), status.data_ptr(), s)),
            "oprf_evaluate": lambda: ok(L.ncg_oprf_evaluate_batch_dev(h, 0, 0, n, inputs.data_ptr(), off32.data_ptr(), None, 0, key.data_ptr(),
                                                                      ONE_SCALAR, out64.data_ptr(), status.data_ptr(), s)),
            "hash_to_scalar_145": lambda: ok(L.ncg_ristretto_hash_to_scalar_batch_dev(h, n, msgs.data_ptr(), offm.data_ptr(), b"HashToScalar-bench", 18,
                                                                                      out32.data_ptr(), s)),
        }
        np_ = 65535
        if bits == 16:
            proof, okb = np.zeros(64, np.uint8), np.zeros(1, np.uint8)
            host32, bad = np.zeros(32, np.uint8), ctypes.c_int64(-1)
            kb, rb = key.cpu().numpy().tobytes(), ks[9].cpu().numpy().tobytes()
            C, D = blinded, evaluated       # D = key * C from the check above
            ok(L.ncg_oprf_blind_batch_dev(h, 0, 0, n, inputs.data_ptr(), off32.data_ptr(), ks.data_ptr(), blinded.data_ptr(), status.data_ptr(), s))
            ok(L.ncg_oprf_mul_batch_dev(h, 0, n, blinded.data_ptr(), key.data_ptr(), ONE_SCALAR, evaluated.data_ptr(), flag.data_ptr(), s))
            Cp, Dp = C.clone(), D.clone()
            ok(L.ncg_oprf_generate_proof_dev(h, 0, 1, np_, kb, B, Cp.data_ptr(), Dp.data_ptr(), rb, proof.ctypes.data, s))
            ok(L.ncg_oprf_verify_proof_dev(h, 0, 1, np_, B, Cp.data_ptr(), Dp.data_ptr(), proof.tobytes(), okb.ctypes.data, s))
            assert okb[0] == 1, "the generated proof does not verify"
            fns["composite_scalars"] = lambda: ok(L.ncg_oprf_composite_scalars_batch_dev(h, 0, 1, np_, B, Cp.data_ptr(), Dp.data_ptr(), out32.data_ptr(),
                                                                                         status.data_ptr(), s))
            fns["hash_to_scalar_145_65535"] = lambda: ok(L.ncg_ristretto_hash_to_scalar_batch_dev(h, np_, msgs.data_ptr(), offm.data_ptr(),
                                                                                                  b"HashToScalar-bench", 18, out32.data_ptr(), s))
            fns["ristretto_msm"] = lambda: ok(L.ncg_ristretto_msm_dev(h, np_, Cp.data_ptr(), ks.data_ptr(), host32.ctypes.data, ctypes.byref(bad), s))
            fns["generate_proof"] = lambda: ok(L.ncg_oprf_generate_proof_dev(h, 0, 1, np_, kb, B, Cp.data_ptr(), Dp.data_ptr(), rb, proof.ctypes.data, s))
            fns["verify_proof"] = lambda: ok(L.ncg_oprf_verify_proof_dev(h, 0, 1, np_, B, Cp.data_ptr(), Dp.data_ptr(), proof.tobytes(),
                                                                         okb.ctypes.data, s))
        t = timed(fns)
        med = {k: statistics.median(v) for k, v in t.items()}
        ratios = {
            "mul_to_ristretto_mul": med["oprf_mul"] / med["ristretto_mul"],
            "mul_one_scalar_to_ristretto_mul": med["oprf_mul_one_scalar"] / med["ristretto_mul"],
            "blind_to_from_uniform_then_mul": med["oprf_blind"] / med["from_uniform_then_ristretto_mul"],
            "finalize_to_mul_invert": med["oprf_finalize"] / med["oprf_mul_invert"],
            "mul_invert_to_mul": med["oprf_mul_invert"] / med["oprf_mul"],
            "evaluate_to_blind": med["oprf_evaluate"] / med["oprf_blind"],
        }
        if "generate_proof" in med:
            ratios["composite_to_hash_to_scalar"] = med["composite_scalars"] / med["hash_to_scalar_145_65535"]
            ratios["generate_proof_to_one_msm"] = med["generate_proof"] / med["ristretto_msm"]
            ratios["verify_proof_to_two_msm"] = med["verify_proof"] / (2 * med["ristretto_msm"])
        entry = {
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in med.items()},
            "ratios": {k: round(v, 3) for k, v in ratios.items()},
        }
        res["2^%d" % bits] = entry
        for k in t:
            print("2^%-3d %-32s %9.4f ms  reps %s" % (bits, k, med[k], entry["ms_reps"][k]), flush=True)
        print("2^%-3d ratios %s" % (bits, entry["ratios"]), flush=True)
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict)}))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in res.items()) + "\n}\n")   # one size per line


if __name__ == "__main__":
    main()
