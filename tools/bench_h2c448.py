#!/usr/bin/env python3
"""RFC 9380 for edwards448 and decaf448 (ncg_xof_shake256 / ncg_ed448_h2c_* / ncg_decaf448_hash_to_*_dev) at 2^16 and 2^18 rows of
32-byte messages, each path beside its yardstick at the same n: device-resident inputs, HIP-event timing on one explicit stream, the
compared paths timed alternating over the same buffers in this process (--reps repetitions of --steps calls each, the MEDIAN of the
repetitions reported, all of them kept).
    xof_shake256 (112 and 168 bytes)   against ncg_shake256_batch_dev of the very bytes the xof absorbs, assembled per row
    ed448 hash_batch, count 2           against ncg_decaf448_from_uniform_batch_dev (three power chains per row each)
    decaf448 hash_to_group              against ncg_shake256_batch_dev(112) followed by ncg_decaf448_from_uniform_batch_dev
The halves (hash_to_field, map_batch count 2 and 1, the two hash_to_scalar) are timed too.  Python decaf448.hashToCurve_batch is timed
at --py-log2n rows with device_hash=False (hashlib on the host, one message at a time) and device_hash=True, wall clock, alternating.
Every path is checked once before it is timed: hash_batch equals hash_to_field followed by map_batch, hash_to_group equals
xof(112) followed by from_uniform, and the first rows equal hashlib's."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from noble_curves_amd import decaf448, get_engine  # noqa: E402

RO = b"edwards448_XOF:SHAKE256_ELL2_RO_"
DECAF = b"decaf448_XOF:SHAKE256_D448MAP_RO_"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", default="16,18")
    ap.add_argument("--py-log2n", type=int, default=16)
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
    gen.manual_seed(9380448)
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
    for bits in [int(b) for b in args.log2n.split(",")]:
        n = 1 << bits
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        off = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * 32).to(dev)
        m, o = msgs.data_ptr(), off.data_ptr()
        pts, pts2, u, out56, out56b, uni, uni168 = u8(n, 112), u8(n, 112), u8(n, 112), u8(n, 56), u8(n, 56), u8(n, 112), u8(n, 168)
        # the yardsticks' plain SHAKE256 inputs, the very bytes the xof absorbs: msg || I2OSP(len, 2) || DST || I2OSP(len(DST), 1), 68 bytes
        # under the decaf448 DST at 112 bytes of output and 67 under the edwards448 DST at 168
        def assembled(dst, out_len):
            tail = out_len.to_bytes(2, "big") + dst + bytes([len(dst)])
            buf = torch.zeros((n, 32 + len(tail)), dtype=torch.uint8, device=dev)
            buf[:, :32] = msgs
            buf[:, 32:] = torch.from_numpy(np.frombuffer(tail, np.uint8).copy()).to(dev)
            return buf, torch.from_numpy(np.arange(n + 1, dtype=np.int64) * buf.shape[1]).to(dev)
        plain, poff = assembled(DECAF, 112)
        plain168, poff168 = assembled(RO, 168)
        pm, po, pm168, po168 = plain.data_ptr(), poff.data_ptr(), plain168.data_ptr(), poff168.data_ptr()
        # checks before timing
        ok(L.ncg_ed448_h2c_hash_batch_dev(h, n, 2, m, o, RO, len(RO), pts.data_ptr(), s))
        ok(L.ncg_ed448_h2c_hash_to_field_batch_dev(h, n, 2, m, o, RO, len(RO), u.data_ptr(), s))
        ok(L.ncg_ed448_h2c_map_batch_dev(h, n, 2, u.data_ptr(), pts2.data_ptr(), s))
        ok(L.ncg_decaf448_hash_to_group_batch_dev(h, n, m, o, DECAF, len(DECAF), out56.data_ptr(), s))
        ok(L.ncg_xof_shake256_batch_dev(h, n, m, o, DECAF, len(DECAF), 112, uni.data_ptr(), s))
        ok(L.ncg_decaf448_from_uniform_batch_dev(h, n, uni.data_ptr(), out56b.data_ptr(), s))
        ok(L.ncg_shake256_batch_dev(h, n, pm, po, 112, uni168.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(pts, pts2), "hash_batch differs from hash_to_field + map_batch"
        assert torch.equal(out56, out56b), "hash_to_group differs from xof(112) + from_uniform"
        assert torch.equal(uni.view(-1), uni168.view(-1)[:n * 112]), "xof differs from SHAKE256 of the assembled input"
        x168 = u8(n, 168)
        ok(L.ncg_xof_shake256_batch_dev(h, n, m, o, RO, len(RO), 168, x168.data_ptr(), s))
        ok(L.ncg_shake256_batch_dev(h, n, pm168, po168, 168, uni168.data_ptr(), s))
        torch.cuda.synchronize()
        assert torch.equal(x168, uni168), "xof(168) differs from SHAKE256 of the assembled input"
        m0 = bytes(msgs[0].cpu().numpy())
        assert bytes(uni[0].cpu().numpy()) == hashlib.shake_256(m0 + (112).to_bytes(2, "big") + DECAF + bytes([len(DECAF)])).digest(112)
        fns = {
            "xof_shake256_112": lambda: ok(L.ncg_xof_shake256_batch_dev(h, n, m, o, DECAF, len(DECAF), 112, uni.data_ptr(), s)),
            "shake256_112": lambda: ok(L.ncg_shake256_batch_dev(h, n, pm, po, 112, uni.data_ptr(), s)),
            "xof_shake256_168": lambda: ok(L.ncg_xof_shake256_batch_dev(h, n, m, o, RO, len(RO), 168, uni168.data_ptr(), s)),
            "shake256_168": lambda: ok(L.ncg_shake256_batch_dev(h, n, pm168, po168, 168, uni168.data_ptr(), s)),
            "ed448_hash_batch_ro": lambda: ok(L.ncg_ed448_h2c_hash_batch_dev(h, n, 2, m, o, RO, len(RO), pts.data_ptr(), s)),
            "ed448_hash_batch_nu": lambda: ok(L.ncg_ed448_h2c_hash_batch_dev(h, n, 1, m, o, RO, len(RO), pts.data_ptr(), s)),
            "decaf448_from_uniform": lambda: ok(L.ncg_decaf448_from_uniform_batch_dev(h, n, uni.data_ptr(), out56b.data_ptr(), s)),
            "ed448_hash_to_field_2": lambda: ok(L.ncg_ed448_h2c_hash_to_field_batch_dev(h, n, 2, m, o, RO, len(RO), u.data_ptr(), s)),
            "ed448_map_batch_2": lambda: ok(L.ncg_ed448_h2c_map_batch_dev(h, n, 2, u.data_ptr(), pts2.data_ptr(), s)),
            "ed448_map_batch_1": lambda: ok(L.ncg_ed448_h2c_map_batch_dev(h, n, 1, u.data_ptr(), pts2.data_ptr(), s)),
            "ed448_hash_to_scalar": lambda: ok(L.ncg_ed448_h2c_hash_to_scalar_batch_dev(h, n, m, o, b"HashToScalar-", 13, out56.data_ptr(), s)),
            "decaf448_hash_to_scalar": lambda: ok(L.ncg_decaf448_hash_to_scalar_batch_dev(h, n, m, o, b"HashToScalar-", 13, out56.data_ptr(), s)),
            "decaf448_hash_to_group": lambda: ok(L.ncg_decaf448_hash_to_group_batch_dev(h, n, m, o, DECAF, len(DECAF), out56.data_ptr(), s)),
        }

        def two_calls():
            ok(L.ncg_shake256_batch_dev(h, n, pm, po, 112, uni.data_ptr(), s))
            ok(L.ncg_decaf448_from_uniform_batch_dev(h, n, uni.data_ptr(), out56b.data_ptr(), s))
        fns["shake256_112_then_from_uniform"] = two_calls
        t = timed(fns)
        med = {k: statistics.median(v) for k, v in t.items()}
        ratios = {
            "xof_112_to_shake256_112": med["xof_shake256_112"] / med["shake256_112"],
            "xof_168_to_shake256_168": med["xof_shake256_168"] / med["shake256_168"],
            "ed448_hash_ro_to_decaf448_from_uniform": med["ed448_hash_batch_ro"] / med["decaf448_from_uniform"],
            "ed448_map_2_to_decaf448_from_uniform": med["ed448_map_batch_2"] / med["decaf448_from_uniform"],
            "decaf448_hash_to_group_to_shake256_then_from_uniform": med["decaf448_hash_to_group"] / med["shake256_112_then_from_uniform"],
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
    # the Python layer: wall clock of one call, the two paths alternating
    n = 1 << args.py_log2n
    rng = np.random.default_rng(448)
    pymsgs = [rng.bytes(32) for _ in range(n)]
    a = decaf448.hashToCurve_batch(pymsgs[:64], device_hash=False)
    assert a == decaf448.hashToCurve_batch(pymsgs[:64], device_hash=True)
    py = {"host_hash": [], "device_hash": []}
    for _ in range(3):
        for key, flag in (("host_hash", False), ("device_hash", True)):
            t0 = time.perf_counter()
            decaf448.hashToCurve_batch(pymsgs, device_hash=flag)
            py[key].append((time.perf_counter() - t0) * 1e3)
    pmed = {k: statistics.median(v) for k, v in py.items()}
    res["python_decaf448_hashToCurve_batch_2^%d" % args.py_log2n] = {
        "ms": {k: round(v, 2) for k, v in pmed.items()}, "ms_reps": {k: [round(x, 2) for x in v] for k, v in py.items()},
        "host_to_device_hash": round(pmed["host_hash"] / pmed["device_hash"], 3)}
    print("python decaf448.hashToCurve_batch 2^%d: %s" % (args.py_log2n, res["python_decaf448_hashToCurve_batch_2^%d" % args.py_log2n]), flush=True)
    print(json.dumps({k: v.get("ratios", v.get("host_to_device_hash")) for k, v in res.items() if isinstance(v, dict)}))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in res.items()) + "\n}\n")   # one size per line


if __name__ == "__main__":
    main()
