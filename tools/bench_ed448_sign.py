#!/usr/bin/env python3
"""Batch Ed448 signing, verification from messages and SHAKE256 at 2^14 and 2^18 rows of 32-byte messages, each form beside its
yardstick on the same rows:
  (a) ncg_ed448_verify_batch_msgs_dev                        against ncg_ed448_verify_batch_dev with the challenges given
  (b) ncg_ed448_sign_batch_dev, expanded keys, ONE_KEY        against ncg_ed448_mul_base_batch_dev (one base multiply per signature)
  (c) ncg_ed448_sign_batch_dev from per-row seeds             against the same multiply (two per signature)
  (d) ncg_ed448_public_key_batch_dev                          against the same multiply (one)
  (e) ncg_shake256_batch_dev, 64 bytes out of 32-byte and of 1000-byte messages: ns per 136-byte block (no yardstick in the project)
Device-resident inputs, HIP-event timing on one explicit stream, the candidates timed alternating over the same buffers in this
process (--reps repetitions of --steps calls each after one warm-up call each; median, minimum and maximum of the repetitions are
reported, all of them kept).  Every result is checked once before it is timed: the signatures verify by both routes, (b) and (c)
agree on row 0's key, and the public keys equal the multiples of the expanded scalars.  `expected` holds the ratios counted before
anything was measured (a Keccak-f permutation is 7-8 k VALU instructions, a verification 448 x 4 024 multiply-adds: the hashing
should be below 1 % of a row).  --python-rows N also times the Python mirror's verify_batch with device_hash=True against its default
(hashlib on one core) on N rows, one call each."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from noble_curves_amd import _native  # noqa: E402
from noble_curves_amd import get_engine  # noqa: E402

EXPECTED = {"verify_msgs_to_verify": 1.0, "sign_expanded_one_key_to_mul_base": 1.0, "sign_seeds_to_mul_base": 2.0,
            "public_key_to_mul_base": 1.0}
DOM = b"SigEd448\x00\x00"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", default="14,18")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--python-rows", type=int, default=0)
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
        seeds = torch.randint(0, 256, (n, 57), dtype=torch.uint8, device=dev, generator=gen)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        long_msgs = torch.randint(0, 256, (n, 1000), dtype=torch.uint8, device=dev, generator=gen)
        off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * 32).contiguous()
        long_off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * 1000).contiguous()
        rows = torch.empty((n, 172), dtype=torch.uint8, device=dev)
        ok(L.ncg_ed448_expand_key_batch_dev(h, n, seeds.data_ptr(), rows.data_ptr(), s))
        torch.cuda.synchronize()
        pk_rows = rows[:, 113:170].contiguous()
        pk_one = rows[:1, 113:170].expand(n, 57).contiguous()
        scalars = rows[:, :56].contiguous()
        sig_b, sig_c = torch.empty((n, 114), dtype=torch.uint8, device=dev), torch.empty((n, 114), dtype=torch.uint8, device=dev)
        flag, verdict = torch.empty((n,), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.uint8, device=dev)
        pk_new, pk_mul = torch.empty((n, 57), dtype=torch.uint8, device=dev), torch.empty((n, 57), dtype=torch.uint8, device=dev)
        ks = torch.empty((n, 56), dtype=torch.uint8, device=dev)
        digest = torch.empty((n, 64), dtype=torch.uint8, device=dev)

        def sign_b():
            ok(L.ncg_ed448_sign_batch_dev(h, n, rows.data_ptr(), _native.ED448_SIGN_EXPANDED | _native.ED448_SIGN_ONE_KEY, DOM, len(DOM),
                                          msgs.data_ptr(), off.data_ptr(), sig_b.data_ptr(), flag.data_ptr(), s))

        def sign_c():
            ok(L.ncg_ed448_sign_batch_dev(h, n, seeds.data_ptr(), 0, DOM, len(DOM), msgs.data_ptr(), off.data_ptr(), sig_c.data_ptr(),
                                          flag.data_ptr(), s))

        def verify_msgs(sig, pk):
            ok(L.ncg_ed448_verify_batch_msgs_dev(h, n, sig.data_ptr(), pk.data_ptr(), 0, DOM, len(DOM), msgs.data_ptr(), off.data_ptr(),
                                                 verdict.data_ptr(), s))

        def verify_given():
            ok(L.ncg_ed448_verify_batch_dev(h, n, sig_c.data_ptr(), pk_rows.data_ptr(), ks.data_ptr(), verdict.data_ptr(), s))

        def mul_base():
            ok(L.ncg_ed448_mul_base_batch_dev(h, n, scalars.data_ptr(), pk_mul.data_ptr(), s))

        # checks before timing
        sign_b()
        torch.cuda.synchronize()
        assert bool(flag.all().item()), "sign (expanded, one key) refused a row"
        verify_msgs(sig_b, pk_one)
        torch.cuda.synchronize()
        assert bool(verdict.all().item()), "sign (expanded, one key): a signature does not verify"
        sign_c()
        torch.cuda.synchronize()
        assert bool(flag.all().item()), "sign (seeds) refused a row"
        verify_msgs(sig_c, pk_rows)
        torch.cuda.synchronize()
        assert bool(verdict.all().item()), "sign (seeds): a signature does not verify"
        assert torch.equal(sig_b[0], sig_c[0]), "expanded and seed forms differ on the shared key"
        ok(L.ncg_ed448_challenge_batch_dev(h, n, sig_c.data_ptr(), pk_rows.data_ptr(), 0, DOM, len(DOM), msgs.data_ptr(), off.data_ptr(),
                                           ks.data_ptr(), s))
        verdict.zero_()
        verify_given()
        torch.cuda.synchronize()
        assert bool(verdict.all().item()), "the challenges of the device do not verify through the existing entry point"
        ok(L.ncg_ed448_public_key_batch_dev(h, n, seeds.data_ptr(), pk_new.data_ptr(), s))
        mul_base()
        torch.cuda.synchronize()
        assert torch.equal(pk_new, pk_mul) and torch.equal(pk_new, pk_rows), "the routes to a public key differ"

        fns = {
            "verify_msgs": lambda: verify_msgs(sig_c, pk_rows),
            "verify_given_k": verify_given,
            "sign_expanded_one_key": sign_b,
            "sign_seeds": sign_c,
            "public_key": lambda: ok(L.ncg_ed448_public_key_batch_dev(h, n, seeds.data_ptr(), pk_new.data_ptr(), s)),
            "mul_base": mul_base,
            "shake256_32B": lambda: ok(L.ncg_shake256_batch_dev(h, n, msgs.data_ptr(), off.data_ptr(), 64, digest.data_ptr(), s)),
            "shake256_1000B": lambda: ok(L.ncg_shake256_batch_dev(h, n, long_msgs.data_ptr(), long_off.data_ptr(), 64, digest.data_ptr(), s)),
        }
        t = timed(fns)
        med = {k: statistics.median(v) for k, v in t.items()}
        ratios = {
            "verify_msgs_to_verify": round(med["verify_msgs"] / med["verify_given_k"], 3),
            "sign_expanded_one_key_to_mul_base": round(med["sign_expanded_one_key"] / med["mul_base"], 3),
            "sign_seeds_to_mul_base": round(med["sign_seeds"] / med["mul_base"], 3),
            "public_key_to_mul_base": round(med["public_key"] / med["mul_base"], 3),
        }
        entry = {
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in med.items()},
            "per_second": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            # 32 bytes: one absorbed block; 1000 bytes: 1000 // 136 + 1 = 8
            "shake256_ns_per_block": {"32B": round(med["shake256_32B"] * 1e6 / n, 2), "1000B": round(med["shake256_1000B"] * 1e6 / n / 8, 2)},
            "ratios": ratios,
        }
        res["2^%d" % bits] = entry
        for k in t:
            print("2^%-3d %-24s median %9.4f ms  [%9.4f, %9.4f]  %8.2f ns/item" % (bits, k, med[k], min(t[k]), max(t[k]),
                                                                                    entry["ns_per_item"][k]), flush=True)
        print("2^%-3d ratios %s expected %s" % (bits, ratios, EXPECTED), flush=True)
        if args.python_rows and n >= args.python_rows:
            from noble_curves_amd import ed448 as m
            k = args.python_rows
            sigs = [bytes(x) for x in sig_c[:k].cpu().numpy()]
            pks = [bytes(x) for x in pk_rows[:k].cpu().numpy()]
            ms = [bytes(x) for x in msgs[:k].cpu().numpy()]
            py = {}
            for name, dh in (("default_host_hash", False), ("device_hash", True)):
                t0 = time.perf_counter()
                out = m.ed448.verify_batch(sigs, ms, pks, engine=eng, device_hash=dh)
                py[name + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                assert all(out), "the Python mirror refused a valid row"
            entry["python_verify_batch"] = dict(py, rows=k)
            print("2^%-3d python verify_batch on %d rows: %s" % (bits, k, py), flush=True)
            args.python_rows = 0
        del seeds, msgs, long_msgs, off, long_off, rows, pk_rows, pk_one, scalars, sig_b, sig_c, flag, verdict, pk_new, pk_mul, ks, digest
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict) and "ratios" in v}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
