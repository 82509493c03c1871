#!/usr/bin/env python3
"""Writes tests/golden/x25519_kat.json: known answers of the reference's x25519 (src/abstract/montgomery.ts, src/ed25519.ts:266-292)
and ed25519.utils.toMontgomery / toMontgomerySecret, data only, as hex strings.  Run by hand where the reference bundle
(oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_x25519_kat.py
The inputs are built here (seeded, plus the edge rows), a small driver of ours runs them through the reference once, and the answers -
or the message of the error the reference throws - come back as JSON."""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import refjs  # noqa: E402

P = 2**255 - 19
D = -121665 * pow(121666, -1, P) % P
LOW = [0, 1, P - 1, 325606250916557431795983626356110631294008115727848805560023387167927233504,
       39382357235489614581723060781553021112529911719440698176882885853963445705823]

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { ed25519, x25519 } from './ed25519.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const run = (f) => { try { return { out: hex(f()), error: null }; } catch (e) { return { out: null, error: e.message }; } };
const mul = job.mul.map((c) => run(() => x25519.scalarMult(bin(c.scalar), bin(c.u))));
const pub = job.pub.map((s) => run(() => x25519.getPublicKey(bin(s))));
const edpk = job.ed_seeds.map((s) => hex(ed25519.getPublicKey(bin(s))));
const xsec = job.ed_seeds.map((s) => hex(ed25519.utils.toMontgomerySecret(bin(s))));
const mont = edpk.concat(job.ed_bad).map((k) => run(() => ed25519.utils.toMontgomery(bin(k))));
const iter = {};
let k = x25519.GuBytes;
for (let i = 1, u = k; i <= 1000; i++) {
  [k, u] = [x25519.scalarMult(k, u), k];
  if (i === 1 || i % 100 === 0) iter[i] = hex(k);
}
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const errors = {
  u_length: msg(() => x25519.scalarMult(new Uint8Array(32), new Uint8Array(31))),
  u_type: msg(() => x25519.scalarMult(new Uint8Array(32), 'x')),
  scalar_length: msg(() => x25519.scalarMult(new Uint8Array(33), x25519.GuBytes)),
  both_bad: msg(() => x25519.scalarMult(new Uint8Array(33), new Uint8Array(31))),
  low_order_before_scalar: msg(() => x25519.scalarMult(new Uint8Array(33), new Uint8Array(32))),
  public_key_length: msg(() => x25519.getPublicKey(new Uint8Array(31))),
};
console.log(JSON.stringify({ mul, pub, edpk, xsec, mont, iter, errors, gu: hex(x25519.GuBytes) }));
"""


def le(v):
    return int(v).to_bytes(32, "little").hex()


def is_square(v):
    return v % P == 0 or pow(v, (P - 1) // 2, P) == 1


def main():
    if not refjs.available():
        sys.exit("make_x25519_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_x25519_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "x25519_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    rng = random.Random("x25519-kat")
    rb = lambda: bytes(rng.randrange(256) for _ in range(32)).hex()  # noqa: E731
    mul = []

    def add(name, scalar, u):
        mul.append({"name": name, "scalar": scalar, "u": u})

    add("rfc7748-1", "a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
        "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
    add("rfc7748-2", "4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
        "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493")
    alice, bob = "77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a", "5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb"
    apub, bpub = "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a", "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"
    add("alice-bob", alice, bpub)
    add("bob-alice", bob, apub)
    # the low-order set in all its encodings: the five values, p and p + 1 (2^255 - 19 + v < 2^255 for v < 19), each with bit 255 too
    for label, v in zip(("0", "1", "p - 1", "order 8 (a)", "order 8 (b)", "p", "p + 1"), LOW + [P, P + 1]):
        for top in (0, 1 << 255):
            add("low-order %s%s" % (label, ", bit 255 set" if top else ""), rb(), le(v | top))
    for s in ("00" * 32, "ff" * 32):
        for v in (2, 9, P - 2, 2**255 - 20, 2**255 - 1, 9 | 1 << 255):
            add("edge scalar %s u %x" % (s[:2], v), s, le(v))
    for v in (2, 9, P - 2, 2**255 - 20, 2**255 - 1, 9 | 1 << 255):
        add("edge u %x" % v, rb(), le(v))
    for i in range(256):
        add("random %d" % i, rb(), rb())
    pub = [alice, bob, "00" * 32, "ff" * 32] + [rb() for _ in range(28)]
    ed_seeds = [alice] + [rb() for _ in range(64)]
    # rejected Ed25519 keys: y >= p (p itself, and 2^255 - 1), a y with no x on the curve, x = 0 with the sign bit, y = 1
    y_off = next(y for y in range(2, 100) if not is_square((y * y - 1) * pow(D * y * y + 1, -1, P)))
    ed_bad = [le(P), le(2**255 - 1), le(y_off), le(y_off | 1 << 255), le((P - 1) | 1 << 255), le(1 | 1 << 255), le(1)]
    ed_bad_names = ["y = p", "y = 2^255 - 1", "y = %d: no x" % y_off, "y = %d: no x, sign bit" % y_off, "y = p - 1 (x = 0), sign bit",
                    "y = 1 (x = 0), sign bit", "y = 1"]
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"mul": mul, "pub": pub, "ed_seeds": ed_seeds, "ed_bad": ed_bad}, f)
        job = f.name
    try:
        res = subprocess.run([refjs.node(), driver, job], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(job)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["gu"] == le(9)
    for c, o in zip(mul, got["mul"]):
        c.update(o)
    assert mul[0]["out"] == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    assert mul[1]["out"] == "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"
    assert mul[2]["out"] == mul[3]["out"] == "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
    assert got["iter"]["1"] == "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
    assert got["iter"]["1000"] == "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"
    assert got["pub"][0]["out"] == apub and got["pub"][1]["out"] == bpub
    assert got["xsec"][0] == "a8cd44eb8e93319c0570bc11005c0e0189d34ff02f6c17773411ad191293c94f"
    assert got["mont"][0]["out"] == "ed7749b4d989f6957f3bfde6c56767e988e21c9f8784d91d610011cd553f9b06"
    keys = got["edpk"] + ed_bad
    names = ["rfc7748 alice as an ed25519 seed"] + ["random %d" % i for i in range(64)] + ed_bad_names
    kat = {
        "errors": got["errors"],
        "scalar_mult": mul,
        "iterated": got["iter"],
        "public_keys": [dict(scalar=s, **o) for s, o in zip(pub, got["pub"])],
        "to_montgomery": [dict(name=n, publicKey=k, **o) for n, k, o in zip(names, keys, got["mont"])],
        "to_montgomery_secret": [{"secretKey": s, "out": x} for s, x in zip(ed_seeds, got["xsec"])],
    }
    out = os.path.join(HERE, "x25519_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, indent=0, separators=(",", ":"))
    print("%d scalarMult rows (%d rejected), %d public keys, %d toMontgomery rows (%d rejected) -> %s (%d bytes)" % (
        len(mul), sum(c["out"] is None for c in mul), len(pub), len(keys), sum(o["out"] is None for o in got["mont"]), out,
        os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))
    print(sorted({c["error"] for c in mul if c["error"]} | {o["error"] for o in got["mont"] if o["error"]}))


main()
