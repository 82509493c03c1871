#!/usr/bin/env python3
"""Times the bls12-381 pairing path on one GPU, each shape alternating with its yardstick - the G2 variable-base batch multiply
(ncg_mul_var_batch_dev, curve 3) at the same n - and writes profiles/r11_pairing.json.
    python tools/bench_pairing.py [--out profiles/r11_pairing.json] [--reps 7]
ncg_pairing_batch_dev at 2^12 / 2^16 pairs as groups of one, groups of two and one group; the latency of one group of two pairs;
ncg_bls_verify_batch_dev of both schemes at the same n; ncg_fp12_batch_dev final exponentiation and product at the same n - the
final-exponentiation kernel's work timed alone; the Miller kernel and the product passes are DERIVED from them (Miller = groups of
one minus the final exponentiations; product passes plus the one final exponentiation of the group = one group minus Miller), not timed by themselves; and, where Node and the
oracle/_ref bundle are present, the reference's own pairingBatch on one host core.  Times are wall times of the synchronous call,
minimum and median over the repetitions."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from noble_curves_amd import _native, get_engine  # noqa: E402
from noble_curves_amd._native import BLS12_381_G1, BLS12_381_G2  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x3F                                       # below 2^254 < r
    raw[:, 0] |= 1
    return raw


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


REF_DRIVER = r"""
import './polyfill.mjs';
import { bls12_381 as bls } from './bls12-381.mjs';
const G1 = bls.G1.Point, G2 = bls.G2.Point;
const pairs = [];
for (let i = 1; i <= 8; i++) pairs.push({ g1: G1.BASE.multiply(BigInt(1000 + i)), g2: G2.BASE.multiply(BigInt(2000 + i)) });
bls.pairingBatch(pairs.slice(0, 2));
const t = [];
for (let r = 0; r < 3; r++) { const a = process.hrtime.bigint(); bls.pairingBatch(pairs); t.push(Number(process.hrtime.bigint() - a) / 1e6); }
const s = [];
for (let r = 0; r < 3; r++) { const a = process.hrtime.bigint(); for (const p of pairs.slice(0, 4)) bls.pairing(p.g1, p.g2); s.push(Number(process.hrtime.bigint() - a) / 1e6); }
console.log(JSON.stringify({ pairingBatch_8_pairs_ms: Math.min(...t), ms_per_pair_in_batch: Math.min(...t) / 8, pairing_ms_each: Math.min(...s) / 4 }));
"""


def reference_cpu():
    """the reference's own code from the oracle/_ref bundle on one host core; None where Node or the bundle is missing"""
    try:
        import subprocess
        from oracle import refjs
        if not (refjs.node() and refjs.available()):
            return None
        drv = os.path.join(refjs.ref_dir(), "bench_pairing.mjs")
        with open(drv, "w") as f:
            f.write(REF_DRIVER)
        r = subprocess.run([refjs.node(), drv], capture_output=True, text=True, timeout=600)
        return json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None
    except Exception:  # noqa: BLE001 - a missing baseline must not lose the device figures
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_pairing.json"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    eng = get_engine(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "unit": "ms", "rows": []}
    for log2n in (12, 16):
        n = 1 << log2n
        g1, _ = eng.mul_base_batch(BLS12_381_G1, scalars(n, 1))
        g2, _ = eng.mul_base_batch(BLS12_381_G2, scalars(n, 2))
        d1, d2 = torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()
        dsc = torch.from_numpy(scalars(n, 3)).cuda()
        dout = torch.zeros(n * 192, dtype=torch.uint8, device="cuda")
        dinf = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dgt = torch.zeros(n * 576, dtype=torch.uint8, device="cuda")
        dgt2 = torch.zeros(n * 576, dtype=torch.uint8, device="cuda")
        done = torch.zeros(n, dtype=torch.uint8, device="cuda")

        def yard():
            eng.mul_var_batch_dev(BLS12_381_G2, n, d2.data_ptr(), dsc.data_ptr(), dout.data_ptr(), dinf.data_ptr())
            eng.sync()
        shapes = {"groups_of_one": np.arange(n + 1, dtype=np.uint32), "groups_of_two": np.arange(0, n + 1, 2, dtype=np.uint32),
                  "one_group": np.array([0, n], dtype=np.uint32)}
        paths = {k: (lambda off=off: eng.pairing_batch_dev(n, d1.data_ptr(), d2.data_ptr(), off, dgt.data_ptr(), done.data_ptr()))
                 for k, off in shapes.items()}

        def fe():
            eng.fp12_batch_dev(_native.FP12_FINAL_EXP, n, dgt.data_ptr(), None, dgt2.data_ptr())
            eng.sync()

        def mul():
            eng.fp12_batch_dev(_native.FP12_MUL, n, dgt.data_ptr(), dgt.data_ptr(), dgt2.data_ptr())
            eng.sync()
        paths["groups_of_one"]()                             # dgt now holds n GT elements for the two Fp12 rows
        paths["fp12_final_exp"], paths["fp12_mul"] = fe, mul
        # verification rows: any bytes exercise the whole path (decode with subgroup tests, map, two pairs per row, is_one); valid
        # encodings of the points above with random messages, so every row runs its pairings and verifies false
        for scheme, pkc, sgc, pts_pk, pts_sg in ((0, BLS12_381_G1, BLS12_381_G2, g1, g2), (1, BLS12_381_G2, BLS12_381_G1, g2, g1)):
            pk_enc, _ = eng.encode_points_batch(pkc, pts_pk)
            sg_enc, _ = eng.encode_points_batch(sgc, pts_sg)
            uw = 192 if scheme == 0 else 96
            u = scalars(n * uw // 32, 5 + scheme).reshape(n, uw).copy()
            u[:, 47::48] &= 0x0F                             # every 48-byte coefficient below p
            dv = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pk_enc, sg_enc, u)]
            paths["bls_verify_%s" % ("long" if scheme == 0 else "short")] = (
                lambda scheme=scheme, dv=dv: eng.bls_verify_batch_dev(scheme, n, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), done.data_ptr()))
        for name, fn in paths.items():
            fn()
            yard()
            tp, ty = [], []
            for _ in range(a.reps):                          # alternate path and yardstick
                tp += timed(fn, 1)
                ty += timed(yard, 1)
            row = {"path": name, "log2n": log2n, "ms_min": round(min(tp), 4), "ms_med": round(statistics.median(tp), 4),
                   "yardstick_g2_mul_var_ms_min": round(min(ty), 4), "yardstick_g2_mul_var_ms_med": round(statistics.median(ty), 4),
                   "ratio_med": round(statistics.median(tp) / statistics.median(ty), 3)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    by = {(r["path"], r["log2n"]): r["ms_med"] for r in res["rows"]}
    res["derived_ms_med"] = [{"log2n": k, "miller_kernel": round(by[("groups_of_one", k)] - by[("fp12_final_exp", k)], 4),
                              "product_passes_plus_one_final_exp_one_group": round(by[("one_group", k)] - (by[("groups_of_one", k)] - by[("fp12_final_exp", k)]), 4),
                              "final_exp_kernel": by[("fp12_final_exp", k)]} for k in (12, 16)]
    print(json.dumps(res["derived_ms_med"]))
    res["reference_pairingBatch_one_core"] = reference_cpu()
    print(json.dumps(res["reference_pairingBatch_one_core"]))
    off2 = np.array([0, 2], dtype=np.uint32)
    lat = timed(lambda: eng.pairing_batch_dev(2, d1.data_ptr(), d2.data_ptr(), off2, dgt.data_ptr(), done.data_ptr()), 3 * a.reps)[a.reps:]
    res["latency_one_group_of_two_ms"] = {"min": round(min(lat), 4), "med": round(statistics.median(lat), 4)}
    print(json.dumps(res["latency_one_group_of_two_ms"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
