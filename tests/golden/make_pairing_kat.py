#!/usr/bin/env python3
"""Writes tests/golden/bls12_381_pairing_kat.json once (python tests/golden/make_pairing_kat.py [reference checkout]).

  "vectors"  the first 32 rows of the reference's test/vectors/bls12-381/go_pairing_vectors/pairing.json: row i is
             e([i+1] G1, [i+1] G2), copied in the order of Fp12.toBytes (the file lists the coefficients reversed,
             test/bls12-381.test.ts:1448-1456)
  the rest   answers of the reference's own code (the unpacked oracle/_ref bundle, polyfill.mjs imported first) on the seeded inputs
             of tests/pairing_helpers.py - only the answers are stored, the tests rebuild the inputs:
             "pairing" 32 x pairing([a] G1, [b] G2); "batch" 8 x pairingBatch with 1..5 pairs; "ops" every Fp12 op of
             ncg_fp12_batch on 8 seeded elements (cyclotomic inputs for the cyclotomic square; mul014 as Fp12.mul by the sparse element); "final_exp" 8 x finalExponentiate;
             "verify" verify / verifyBatch booleans of both signature schemes on the rows of bls12_381_sig_vectors.json: valid,
             wrong message, wrong key, swapped signatures, ZERO key / signature encodings and a key outside the subgroup.
Every element is Fp12.toBytes (12 coefficients of 48 bytes big-endian) in base64, which keeps the file below 150 KB."""
import base64
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pairing_helpers as H  # noqa: E402
from oracle import refjs  # noqa: E402

DRIVER = r"""
import './polyfill.mjs';
import { bls12_381 as bls } from './bls12-381.mjs';
import { readFileSync } from 'fs';
const inp = JSON.parse(readFileSync(process.argv[2], 'utf8'));
const { Fp12 } = bls.fields;
const G1 = bls.G1.Point, G2 = bls.G2.Point;
const hex = (u8) => Buffer.from(u8).toString('hex');
const f12 = (h) => Fp12.fromBytes(Uint8Array.from(Buffer.from(h, 'hex')));
const out = {};
out.pairing = inp.pairing.map(([a, b]) => hex(Fp12.toBytes(bls.pairing(G1.BASE.multiply(BigInt(a)), G2.BASE.multiply(BigInt(b))))));
out.batch = inp.batch.map((rows) => hex(Fp12.toBytes(bls.pairingBatch(rows.map(([a, b]) => ({ g1: G1.BASE.multiply(BigInt(a)), g2: G2.BASE.multiply(BigInt(b)) }))))));
out.ops = {
  mul: inp.ops.a.map((h, i) => hex(Fp12.toBytes(Fp12.mul(f12(h), f12(inp.ops.b[i]))))),
  sqr: inp.ops.a.map((h) => hex(Fp12.toBytes(Fp12.sqr(f12(h))))),
  inv: inp.ops.a.map((h) => hex(Fp12.toBytes(Fp12.inv(f12(h))))),
  conjugate: inp.ops.a.map((h) => hex(Fp12.toBytes(Fp12.conjugate(f12(h))))),
  frobenius1: inp.ops.a.map((h) => hex(Fp12.toBytes(Fp12.frobeniusMap(f12(h), 1)))),
  frobenius2: inp.ops.a.map((h) => hex(Fp12.toBytes(Fp12.frobeniusMap(f12(h), 2)))),
  frobenius3: inp.ops.a.map((h) => hex(Fp12.toBytes(Fp12.frobeniusMap(f12(h), 3)))),
  cyclotomic_sqr: inp.ops.cyc.map((h) => hex(Fp12.toBytes(Fp12._cyclotomicSquare(f12(h))))),
  mul014: inp.ops.a.map((h, i) => hex(Fp12.toBytes(Fp12.mul(f12(h), f12(inp.ops.line[i]))))),
  is_one: inp.ops.a.map((h) => Fp12.eql(f12(h), Fp12.ONE)).concat([Fp12.eql(Fp12.ONE, Fp12.ONE)]),
};
out.final_exp = inp.final_exp.map((h) => hex(Fp12.toBytes(Fp12.finalExponentiate(f12(h)))));
const u8 = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const verify = (S, rows) => rows.map(([sig, msg, pk]) => {
  try { return S.verify(u8(sig), S.hash(u8(msg)), u8(pk)); } catch (e) { return false; }
});
out.verify = {};
for (const [name, S] of [['long', bls.longSignatures], ['short', bls.shortSignatures]]) {
  out.verify[name] = verify(S, inp.verify[name]);
  out.verify[name + '_batch'] = inp.verify[name + '_batch'].map(({ sig, items }) => {
    try { return S.verifyBatch(u8(sig), items.map(([msg, pk]) => ({ message: S.hash(u8(msg)), publicKey: u8(pk) }))); } catch (e) { return false; }
  });
}
console.log(JSON.stringify(out));
"""


def verify_rows():
    """the verify inputs of both schemes as (signature, message, public key) hex rows, and verifyBatch cases; rebuilt by the tests through
    pairing_helpers.verify_rows - kept here beside the driver that answers them"""
    return H.verify_rows()


def main():
    # the reference checkout (argument 1; the default is where the build container keeps it)
    ref = os.path.join(sys.argv[1] if len(sys.argv) > 1 else "/root/reference", "test/vectors/bls12-381/go_pairing_vectors/pairing.json")
    rows = json.load(open(ref))[:32]
    kat = {"vectors": ["".join(reversed(re.findall(r"[0-9a-fA-F]{96}", r))).lower() for r in rows]}
    a = [H.seeded_f12("op/a", i) for i in range(8)]
    b = [H.seeded_f12("op/b", i) for i in range(8)]
    inp = {"pairing": [[str(s) for s in H.seeded_pair_scalars(i)] for i in range(32)],
           "batch": [[[str(x), str(y)] for x, y in H.seeded_batch(j)] for j in range(8)],
           "ops": {"a": [H.f12_hex(x) for x in a], "b": [H.f12_hex(x) for x in b],
                   "cyc": [H.f12_hex(H.seeded_cyclotomic("op/cyc", i)) for i in range(8)],
                   # the reference keeps mul014 inside bls.ts: its answer is Fp12.mul by the sparse element o0 + o1 v + o4 v w
                   "line": [H.f12_hex(H.sparse014(*H.seeded_line(i))) for i in range(8)]},
           "final_exp": [H.f12_hex(H.seeded_f12("fe", i)) for i in range(8)],
           "verify": verify_rows()}
    d = refjs.ref_dir()
    drv, fin = os.path.join(d, "pairing_kat.mjs"), os.path.join(d, "pairing_kat_in.json")
    with open(drv, "w") as f:
        f.write(DRIVER)
    with open(fin, "w") as f:
        json.dump(inp, f)
    r = subprocess.run([refjs.node(), drv, fin], capture_output=True, text=True, timeout=1800)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    kat.update(json.loads(r.stdout.strip().splitlines()[-1]))

    def pack(v):
        if isinstance(v, str):
            return base64.b64encode(bytes.fromhex(v)).decode()
        if isinstance(v, list):
            return [pack(x) for x in v]
        if isinstance(v, dict):
            return {k: (x if k.startswith(("long", "short")) else pack(x)) for k, x in v.items()}
        return v
    kat = pack(kat)
    out = os.path.join(HERE, "bls12_381_pairing_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, separators=(",", ":"))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
