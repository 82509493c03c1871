#!/usr/bin/env python3
"""Batch secp256k1 signing at 2^18 and 2^20 rows of 32-byte messages, each form beside its yardstick on the same rows:
  (a) ncg_ecdsa_sign_batch_msgs_dev, per-row keys          against ncg_ecdsa_verify_batch_msgs_dev of those signatures
  (b) ncg_ecdsa_sign_batch_msgs_dev, ONE_KEY               against the same verification (the one public key repeated)
  (c) ncg_schnorr_sign_batch_dev, per-row keys             against ncg_schnorr_verify_batch_msgs_dev
  (d) ncg_secp256k1_public_key_batch_dev (compressed)      against ncg_mul_base_batch_dev + ncg_encode_points_batch_dev (the
      indexed-table route to the same bytes)
Device-resident inputs, HIP-event timing on one explicit stream, the candidates timed alternating over the same buffers in this
process (--reps repetitions of --steps calls each after one warm-up call each; median, minimum and maximum of the repetitions are
reported, all of them kept).  Every result is checked once before it is timed: no row is refused, the signatures verify, and the two
routes to a public key give the same bytes.  `expected` holds the ratios counted from the multiply-add, select and compression counts
of DESIGN.md section 8 "secp256k1 signing" before anything was measured."""
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

EXPECTED = {"ecdsa_sign_to_verify": 0.65, "ecdsa_sign_one_key_to_verify": 0.65, "schnorr_sign_to_verify": 0.78, "public_key_to_indexed_route": 2.1}
SECP = _native.SECP256K1


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
    gen.manual_seed(6979)
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
        sk = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        sk[:, 0] &= 0x7F                                           # below 2^255 < n; zero has probability 2^-255
        aux = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * 32).contiguous()
        u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        pub, xonly, pub_idx, pts = u8(n, 33), u8(n, 32), u8(n, 33), u8(n, 64)
        sig_a, sig_b, sig_c, rec, flag, verdict = u8(n, 64), u8(n, 64), u8(n, 64), u8(n), u8(n), u8(n)
        scalars = torch.flip(sk, dims=[1]).contiguous()            # the multiply's wire scalars are little-endian
        ok(L.ncg_secp256k1_public_key_batch_dev(h, n, sk.data_ptr(), _native.SECP_PK_COMPRESSED, pub.data_ptr(), flag.data_ptr(), s))
        ok(L.ncg_secp256k1_public_key_batch_dev(h, n, sk.data_ptr(), _native.SECP_PK_XONLY, xonly.data_ptr(), flag.data_ptr(), s))
        torch.cuda.synchronize()
        assert bool(flag.all().item()), "a key was refused"
        pub_one = pub[:1].expand(n, 33).contiguous()

        def ecdsa_sign(out, flags):
            ok(L.ncg_ecdsa_sign_batch_msgs_dev(h, SECP, n, sk.data_ptr(), msgs.data_ptr(), off.data_ptr(), None, flags, out.data_ptr(),
                                               rec.data_ptr(), flag.data_ptr(), s))

        def ecdsa_verify(sig, keys):
            ok(L.ncg_ecdsa_verify_batch_msgs_dev(h, SECP, n, sig.data_ptr(), msgs.data_ptr(), off.data_ptr(), keys.data_ptr(),
                                                 _native.ECDSA_LOW_S, verdict.data_ptr(), s))

        def indexed_route():
            eng.mul_base_batch_dev(SECP, n, scalars.data_ptr(), pts.data_ptr(), flag.data_ptr(), s)
            ok(L.ncg_encode_points_batch_dev(h, SECP, n, pts.data_ptr(), pub_idx.data_ptr(), flag.data_ptr(), s))

        fns = {
            "ecdsa_sign": lambda: ecdsa_sign(sig_a, _native.ECDSA_LOW_S),
            "ecdsa_verify_of_a": lambda: ecdsa_verify(sig_a, pub),
            "ecdsa_sign_one_key": lambda: ecdsa_sign(sig_b, _native.ECDSA_LOW_S | _native.SECP_SIGN_ONE_KEY),
            "ecdsa_verify_of_b": lambda: ecdsa_verify(sig_b, pub_one),
            "schnorr_sign": lambda: ok(L.ncg_schnorr_sign_batch_dev(h, n, sk.data_ptr(), aux.data_ptr(), msgs.data_ptr(), off.data_ptr(), 0,
                                                                    sig_c.data_ptr(), flag.data_ptr(), s)),
            "schnorr_verify": lambda: ok(L.ncg_schnorr_verify_batch_msgs_dev(h, n, sig_c.data_ptr(), msgs.data_ptr(), off.data_ptr(),
                                                                             xonly.data_ptr(), verdict.data_ptr(), s)),
            "public_key": lambda: ok(L.ncg_secp256k1_public_key_batch_dev(h, n, sk.data_ptr(), _native.SECP_PK_COMPRESSED, pub.data_ptr(),
                                                                          flag.data_ptr(), s)),
            "mul_base_plus_encode": indexed_route,
        }
        # checks before timing
        for name, key in (("ecdsa_sign", "ecdsa_verify_of_a"), ("ecdsa_sign_one_key", "ecdsa_verify_of_b"), ("schnorr_sign", "schnorr_verify")):
            fns[name]()
            torch.cuda.synchronize()
            assert bool(flag.all().item()), name + " refused a row"
            fns[key]()
            torch.cuda.synchronize()
            assert bool(verdict.all().item()), name + ": a signature does not verify"
        assert torch.equal(sig_a[0], sig_b[0]), "per-row and one-key forms differ on the shared key"
        fns["public_key"]()
        fns["mul_base_plus_encode"]()
        torch.cuda.synchronize()
        assert torch.equal(pub, pub_idx), "the two routes to a public key differ"

        t = timed(fns)
        med = {k: statistics.median(v) for k, v in t.items()}
        ratios = {
            "ecdsa_sign_to_verify": round(med["ecdsa_sign"] / med["ecdsa_verify_of_a"], 3),
            "ecdsa_sign_one_key_to_verify": round(med["ecdsa_sign_one_key"] / med["ecdsa_verify_of_b"], 3),
            "schnorr_sign_to_verify": round(med["schnorr_sign"] / med["schnorr_verify"], 3),
            "public_key_to_indexed_route": round(med["public_key"] / med["mul_base_plus_encode"], 3),
        }
        res["2^%d" % bits] = {
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
            "ms_reps": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "ns_per_item": {k: round(v * 1e6 / n, 2) for k, v in med.items()},
            "per_second": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            "ratios": ratios,
        }
        for k in t:
            print("2^%-3d %-24s median %9.4f ms  [%9.4f, %9.4f]  %8.2f ns/item" % (bits, k, med[k], min(t[k]), max(t[k]), med[k] * 1e6 / n), flush=True)
        print("2^%-3d ratios %s expected %s" % (bits, ratios, EXPECTED), flush=True)
        del sk, aux, msgs, off, pub, xonly, pub_idx, pts, sig_a, sig_b, sig_c, rec, flag, verdict, scalars, pub_one
    print(json.dumps({k: v["ratios"] for k, v in res.items() if isinstance(v, dict) and "ratios" in v}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
