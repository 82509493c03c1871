#!/usr/bin/env python3
"""RFC 9380 for secp256k1 and edwards25519 (ncg_h2c_*_dev) at 2^16 and 2^18 rows of 32-byte messages, each path beside its yardstick
at the same n: device-resident inputs, HIP-event timing on one explicit stream, the compared paths timed alternating over the same
buffers in this process (--reps repetitions of --steps calls each, the MEDIAN of the repetitions reported, all of them kept).
    secp256k1 hash_batch, count 2   against ncg_decode_points_batch_dev of compressed secp256k1 points (one square-root chain per row)
    ed25519 hash_batch, count 2     against ncg_ristretto_hash_to_group_batch_dev (two maps, their sum, one encode)
    hash_to_field, count 2          against ncg_xmd_sha512_batch_dev at equal output length (96 bytes); the secp256k1 suite hashes
                                    with SHA-256, so its xmd over SHA-256 is timed as well
The map halves (ncg_h2c_map_batch_dev, count 2 and 1) are timed too.  Every path is checked once before it is timed: hash_batch equals
hash_to_field followed by map_batch, and the first rows equal the CPU's hashlib / the recorded RFC 9380 vector."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from noble_curves_amd import get_engine  # noqa: E402

SECP, ED = 0, 1
DST = {SECP: b"secp256k1_XMD:SHA-256_SSWU_RO_", ED: b"edwards25519_XMD:SHA-512_ELL2_RO_"}


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
    gen.manual_seed(9380)
    res = {"steps": args.steps, "reps": args.reps, "message_bytes": 32}

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
    # the vector of RFC 9380 J.8.1 through the path that is timed
    x = eng.h2c_hash_batch(SECP, [b"abc"], b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_", 2)[0][0]
    assert bytes(x[:32])[::-1].hex() == "3377e01eab42db296b512293120c6cee72b6ecf9f9205760bd9ff11fb3cb2c4b"
    for bits in [int(b) for b in args.log2n.split(",")]:
        n = 1 << bits
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        off = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * 32).to(dev)
        pts, pts2, inf, inf2 = u8(n, 64), u8(n, 64), u8(n), u8(n)
        u, u48, enc, okb, out96, out32 = u8(n, 64), torch.zeros((n, 96), dtype=torch.uint8, device=dev), u8(n, 33), u8(n), u8(n, 96), u8(n, 32)
        fns = {}
        for suite, name in ((SECP, "secp256k1"), (ED, "ed25519")):
            d = DST[suite]
            ok(L.ncg_h2c_hash_batch_dev(h, suite, n, 2, msgs.data_ptr(), off.data_ptr(), d, len(d), pts.data_ptr(), inf.data_ptr(), s))
            ok(L.ncg_h2c_hash_to_field_batch_dev(h, suite, n, 2, msgs.data_ptr(), off.data_ptr(), d, len(d), u.data_ptr(), s))
            u48.view(n, 2, 48)[:, :, :32] = u.view(n, 2, 32)
            ok(L.ncg_h2c_map_batch_dev(h, suite, n, 2, u48.data_ptr(), pts2.data_ptr(), inf2.data_ptr(), s))
            torch.cuda.synchronize()
            assert torch.equal(pts, pts2) and torch.equal(inf, inf2), "%s: hash_batch differs from hash_to_field + map_batch" % name
            if suite == SECP:       # compressed encodings of the hashed points: the decoder's input
                ok(L.ncg_encode_points_batch_dev(h, 0, n, pts.data_ptr(), enc.data_ptr(), okb.data_ptr(), s))
                torch.cuda.synchronize()
                assert bool(okb.all().item())

            def mk(suite=suite, d=d):
                return {
                    "hash_batch_ro": lambda: ok(L.ncg_h2c_hash_batch_dev(h, suite, n, 2, msgs.data_ptr(), off.data_ptr(), d, len(d), pts.data_ptr(),
                                                                         inf.data_ptr(), s)),
                    "hash_batch_nu": lambda: ok(L.ncg_h2c_hash_batch_dev(h, suite, n, 1, msgs.data_ptr(), off.data_ptr(), d, len(d), pts.data_ptr(),
                                                                         inf.data_ptr(), s)),
                    "hash_to_field_2": lambda: ok(L.ncg_h2c_hash_to_field_batch_dev(h, suite, n, 2, msgs.data_ptr(), off.data_ptr(), d, len(d),
                                                                                    u.data_ptr(), s)),
                    "map_batch_2": lambda: ok(L.ncg_h2c_map_batch_dev(h, suite, n, 2, u48.data_ptr(), pts2.data_ptr(), inf2.data_ptr(), s)),
                    "map_batch_1": lambda: ok(L.ncg_h2c_map_batch_dev(h, suite, n, 1, u48.data_ptr(), pts2.data_ptr(), inf2.data_ptr(), s)),
                    "hash_to_scalar": lambda: ok(L.ncg_h2c_hash_to_scalar_batch_dev(h, suite, n, msgs.data_ptr(), off.data_ptr(), b"HashToScalar-", 13,
                                                                                    out32.data_ptr(), s)),
                }
            for k, f in mk().items():
                fns[name + "_" + k] = f
        fns["secp256k1_decode_compressed"] = lambda: ok(L.ncg_decode_points_batch_dev(h, 0, n, enc.data_ptr(), 0, pts2.data_ptr(), okb.data_ptr(),
                                                                                     inf2.data_ptr(), s))
        fns["ristretto_hash_to_group"] = lambda: ok(L.ncg_ristretto_hash_to_group_batch_dev(h, n, msgs.data_ptr(), off.data_ptr(), DST[ED], len(DST[ED]),
                                                                                            out32.data_ptr(), None, s))
        fns["xmd_sha512_96"] = lambda: ok(L.ncg_xmd_sha512_batch_dev(h, n, msgs.data_ptr(), off.data_ptr(), DST[ED], len(DST[ED]), 96, out96.data_ptr(), s))
        fns["xmd_sha256_96"] = lambda: ok(L.ncg_xmd_sha256_batch_dev(h, n, msgs.data_ptr(), off.data_ptr(), DST[SECP], len(DST[SECP]), 96, out96.data_ptr(), s))
        t = timed(fns)
        med = {k: statistics.median(v) for k, v in t.items()}
        ratios = {
            "secp256k1_hash_ro_to_decode_compressed": med["secp256k1_hash_batch_ro"] / med["secp256k1_decode_compressed"],
            "ed25519_hash_ro_to_ristretto_hash_to_group": med["ed25519_hash_batch_ro"] / med["ristretto_hash_to_group"],
            "ed25519_hash_to_field_to_xmd_sha512_96": med["ed25519_hash_to_field_2"] / med["xmd_sha512_96"],
            "secp256k1_hash_to_field_to_xmd_sha512_96": med["secp256k1_hash_to_field_2"] / med["xmd_sha512_96"],
            "secp256k1_hash_to_field_to_xmd_sha256_96": med["secp256k1_hash_to_field_2"] / med["xmd_sha256_96"],
            "secp256k1_map_2_to_decode_compressed": med["secp256k1_map_batch_2"] / med["secp256k1_decode_compressed"],
        }
        entry = {
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in med.items()},
            "ratios": {k: round(v, 3) for k, v in ratios.items()},
        }
        res["2^%d" % bits] = entry
        for k in t:
            print("2^%-3d %-36s %9.4f ms  reps %s" % (bits, k, med[k], entry["ms_reps"][k]), flush=True)
        print("2^%-3d ratios %s" % (bits, entry["ratios"]), flush=True)
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict)}))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in res.items()) + "\n}\n")   # one size per line


if __name__ == "__main__":
    main()
