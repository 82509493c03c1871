#!/usr/bin/env python3
"""Writes tests/golden/ed448_kat.json: known answers of the reference's x448, ed448, ed448ph and ed448.Point (src/ed448.ts over
src/abstract/montgomery.ts and src/abstract/edwards.ts), data only, as hex strings.  Run by hand where the reference bundle
(oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_ed448_kat.py
The inputs are built here (seeded, plus the edge rows), a small driver of ours runs them through the reference once, and the answers -
or the message of the error the reference throws - come back as JSON.  The RFC 7748 section 5.2 / 6.2 and RFC 8032 section 7.4
known answers are asserted on the way."""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import refjs  # noqa: E402

P = 2**448 - 2**224 - 1
N = 2**446 - 13818066809895115352007386748515426880336692474882178609894547503885
D = P - 39081

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { ed448, ed448ph, x448, ED448_TORSION_SUBGROUP } from './ed448.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const run = (f) => { try { return { out: hex(f()), error: null }; } catch (e) { return { out: null, error: e.message }; } };
const mul = job.mul.map((c) => run(() => x448.scalarMult(bin(c.scalar), bin(c.u))));
const pub = job.pub.map((s) => run(() => x448.getPublicKey(bin(s))));
const edpk = job.ed_seeds.map((s) => hex(ed448.getPublicKey(bin(s))));
const xsec = job.ed_seeds.map((s) => hex(ed448.utils.toMontgomerySecret(bin(s))));
const mont = edpk.concat(job.points).map((k) => run(() => ed448.utils.toMontgomery(bin(k))));
const points = edpk.concat(job.points).map((k) => {
  try { const p = ed448.Point.fromBytes(bin(k)).toAffine(); return { x: p.x.toString(16), y: p.y.toString(16), error: null }; }
  catch (e) { return { x: null, y: null, error: e.message }; }
});
const sigs = job.sign.map((c) => {
  const lib = c.ph ? ed448ph : ed448;
  const opts = c.context === null ? undefined : { context: bin(c.context) };
  const sig = opts ? lib.sign(bin(c.msg), bin(c.seed), opts) : lib.sign(bin(c.msg), bin(c.seed));
  return { sig: hex(sig), publicKey: hex(lib.getPublicKey(bin(c.seed))) };
});
const verify = job.verify.map((c) => {
  const lib = c.ph ? ed448ph : ed448;
  const base = sigs[c.row];
  const sig = bin(c.sig === null ? base.sig : c.sig), pk = bin(c.publicKey === null ? base.publicKey : c.publicKey);
  const msg = bin(c.msg === null ? job.sign[c.row].msg : c.msg);
  const ctx = c.context === null ? undefined : { context: bin(c.context) };
  try { return { ok: ctx ? lib.verify(sig, msg, pk, ctx) : lib.verify(sig, msg, pk), error: null }; }
  catch (e) { return { ok: null, error: e.message }; }
});
const iter = {};
let k = x448.GuBytes;
for (let i = 1, u = k; i <= 1000; i++) {
  [k, u] = [x448.scalarMult(k, u), k];
  if (i === 1 || i % 100 === 0) iter[i] = hex(k);
}
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const good = sigs[0];
const errors = {
  u_length: msg(() => x448.scalarMult(new Uint8Array(56), new Uint8Array(55))),
  u_type: msg(() => x448.scalarMult(new Uint8Array(56), 'x')),
  scalar_length: msg(() => x448.scalarMult(new Uint8Array(57), x448.GuBytes)),
  both_bad: msg(() => x448.scalarMult(new Uint8Array(57), new Uint8Array(55))),
  low_order_before_scalar: msg(() => x448.scalarMult(new Uint8Array(57), new Uint8Array(56))),
  public_key_length: msg(() => x448.getPublicKey(new Uint8Array(55))),
  signature_length: msg(() => ed448.verify(new Uint8Array(113), new Uint8Array(1), bin(good.publicKey))),
  verify_public_key_length: msg(() => ed448.verify(bin(good.sig), new Uint8Array(1), new Uint8Array(56))),
  message_type: msg(() => ed448.verify(bin(good.sig), 'x', bin(good.publicKey))),
  context_too_long: msg(() => ed448.verify(bin(good.sig), new Uint8Array(1), bin(good.publicKey), { context: new Uint8Array(256) })),
  secret_key_length: msg(() => ed448.getPublicKey(new Uint8Array(56))),
  point_length: msg(() => ed448.Point.fromBytes(new Uint8Array(56))),
  to_montgomery_secret_length: msg(() => ed448.utils.toMontgomerySecret(new Uint8Array(56))),
  multiply_zero: msg(() => ed448.Point.BASE.multiply(0n)),
  multiply_n: msg(() => ed448.Point.BASE.multiply(ed448.Point.Fn.ORDER)),
  multiply_unsafe_n: msg(() => ed448.Point.BASE.multiplyUnsafe(ed448.Point.Fn.ORDER)),
};
console.log(JSON.stringify({ mul, pub, edpk, xsec, mont, points, sigs, verify, iter, errors, gu: hex(x448.GuBytes),
  torsion: ED448_TORSION_SUBGROUP }));
"""


def le(v, n=56):
    return int(v).to_bytes(n, "little").hex()


def random_rows(count=256):
    """the seeded random (scalar, u) rows: the fixture keeps only their answers, tests/ed448_helpers.py rebuilds the inputs"""
    rng = random.Random("ed448-kat-random")
    return [tuple(bytes(rng.randrange(256) for _ in range(56)).hex() for _ in range(2)) for _ in range(count)]


def has_x(y):
    u, v = (y * y - 1) % P, (D * y * y - 1) % P
    x2 = u * pow(v, P - 2, P) % P
    return x2 == 0 or pow(x2, (P - 1) // 2, P) == 1


def main():
    if not refjs.available():
        sys.exit("make_ed448_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_ed448_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "ed448_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    rng = random.Random("ed448-kat")
    rb = lambda n=56: bytes(rng.randrange(256) for _ in range(n)).hex()  # noqa: E731
    mul = []

    def add(name, scalar, u):
        mul.append({"name": name, "scalar": scalar, "u": u})

    add("rfc7748-1", "3d262fddf9ec8e88495266fea19a34d28882acef045104d0d1aae121700a779c984c24f8cdd78fbff44943eba368f54b29259a4f1c600ad3",
        "06fce640fa3487bfda5f6cf2d5263f8aad88334cbd07437f020f08f9814dc031ddbdc38c19c6da2583fa5429db94ada18aa7a7fb4ef8a086")
    add("rfc7748-2", "203d494428b8399352665ddca42f9de8fef600908e0d461cb021f8c538345dd77c3e4806e25f46d3315c44e0a5b4371282dd2c8d5be3095f",
        "0fbcc2f993cd56d3305b0b7d9e55d4c1a8fb5dbb52f8e9a1e9b6201b165d015894e56c4d3570bee52fe205e28a78b91cdfbde71ce8d157db")
    alice = "9a8f4925d1519f5775cf46b04b5800d4ee9ee8bae8bc5565d498c28dd9c9baf574a9419744897391006382a6f127ab1d9ac2d8c0a598726b"
    bob = "1c306a7ac2a0e2e0990b294470cba339e6453772b075811d8fad0d1d6927c120bb5ee8972b0d3e21374c9c921b09d1b0366f10b65173992d"
    apub = "9b08f7cc31b7e3e67d22d5aea121074a273bd2b83de09c63faa73d2c22c5d9bbc836647241d953d40c5b12da88120d53177f80e532c41fa0"
    bpub = "3eb7a829b0cd20f5bcfc0b599b6feccf6da4627107bdb0d4f345b43027d8b972fc3e34fb4232a13ca706dcb57aec3dae07bdc1c67bf33609"
    add("alice-bob", alice, bpub)
    add("bob-alice", bob, apub)
    # the low-order set in every encoding: 0, 1, p - 1, and p, p + 1 (both below 2^448)
    for label, v in zip(("0", "1", "p - 1", "p", "p + 1"), (0, 1, P - 1, P, P + 1)):
        add("low-order %s" % label, rb(), le(v))
    edge_u = (2, 5, P - 2, P + 2, 2**448 - 1)
    for s in ("00" * 56, "ff" * 56):
        for v in edge_u:
            add("edge scalar %s u %x" % (s[:2], v), s, le(v))
    for v in edge_u:
        add("edge u %x" % v, rb(), le(v))
    for i, (sc, u) in enumerate(random_rows()):
        add("random %d" % i, sc, u)
    pub = [alice, bob, "00" * 56, "ff" * 56] + [rb() for _ in range(4)]
    rfc8032_1 = "c4eab05d357007c632f3dbb48489924d552b08fe0c353a0d4a1f00acda2c463afbea67c5e8d2877c5e3bc397a659949ef8021e954e0a12274e"
    ed_seeds = [rfc8032_1] + [rb(57) for _ in range(8)]
    # encodings at the edges of Point.fromBytes: y >= p, other bits of byte 56, x = 0 with the sign bit, a y with no x, torsion
    y_off = next(y for y in range(2, 100) if not has_x(y))
    points = [le(P, 57), le(P + 1, 57), le(2**448 - 1, 57), le(1 << 448, 57), le(5 | 1 << 454, 57), le(1 | 1 << 455, 57),
              le((P - 1) | 1 << 455, 57), le(y_off, 57), le(y_off | 1 << 455, 57), le(1, 57), le(P - 1, 57), le(0, 57), le(1 << 455, 57)]
    point_names = ["y = p", "y = p + 1", "y = 2^448 - 1", "byte 56 = 0x01", "byte 56 = 0x40", "y = 1 (x = 0), sign bit",
                   "y = p - 1 (x = 0), sign bit", "y = %d: no x" % y_off, "y = %d: no x, sign bit" % y_off, "identity", "order 2",
                   "order 4 (x = p - 1)", "order 4 (x = 1)"]
    sign = [{"seed": rfc8032_1, "msg": "03", "context": None, "ph": False}]
    for i in range(24):
        sign.append({"seed": rb(57), "msg": rb(i % 7 * 9), "context": None if i % 3 == 0 else rb(i % 5 * 3), "ph": i % 4 == 3})
    verify = []
    for i, c in enumerate(sign):
        verify.append({"row": i, "ph": c["ph"], "sig": None, "publicKey": None, "msg": None, "context": c["context"], "name": "valid"})
    for i in (0, 1, 2, 3, 7):
        c = sign[i]
        verify.append({"row": i, "ph": c["ph"], "sig": None, "publicKey": None, "msg": c["msg"] + "00", "context": c["context"],
                       "name": "other message"})
        verify.append({"row": i, "ph": c["ph"], "sig": None, "publicKey": None, "msg": None, "context": "01", "name": "other context"})
        verify.append({"row": i, "ph": not c["ph"], "sig": None, "publicKey": None, "msg": None, "context": c["context"],
                       "name": "other prehash flag"})
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"mul": mul, "pub": pub, "ed_seeds": ed_seeds, "points": points, "sign": sign, "verify": verify}, f)
        job = f.name
    try:
        res = subprocess.run([refjs.node(), driver, job], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(job)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["gu"] == le(5)
    for c, o in zip(mul, got["mul"]):
        c.update(o)
    assert mul[0]["out"] == "ce3e4ff95a60dc6697da1db1d85e6afbdf79b50a2412d7546d5f239fe14fbaadeb445fc66a01b0779d98223961111e21766282f73dd96b6f"
    assert mul[1]["out"] == "884a02576239ff7a2f2f63b2db6a9ff37047ac13568e1e30fe63c4a7ad1b3ee3a5700df34321d62077e63633c575c1c954514e99da7c179d"
    assert mul[2]["out"] == mul[3]["out"] == \
        "07fff4181ac6cc95ec1c16a94a0f74d12da232ce40a77552281d282bb60c0b56fd2464c335543936521c24403085d59a449a5037514a879d"
    assert got["iter"]["1"] == "3f482c8a9f19b01e6c46ee9711d9dc14fd4bf67af30765c2ae2b846a4d23a8cd0db897086239492caf350b51f833868b9bc2b3bca9cf4113"
    assert got["iter"]["1000"] == "aa3b4749d55b9daf1e5b00288826c467274ce3ebbdd5c17b975e09d4af6c67cf10d087202db88286e2b79fceea3ec353ef54faa26e219f38"
    assert got["pub"][0]["out"] == apub and got["pub"][1]["out"] == bpub
    # RFC 8032 section 7.4, "1 octet"
    assert got["edpk"][0] == got["sigs"][0]["publicKey"] == \
        "43ba28f430cdff456ae531545f7ecd0ac834a55d9358c0372bfa0c6c6798c0866aea01eb00742802b8438ea4cb82169c235160627b4c3a9480"
    assert got["sigs"][0]["sig"] == ("26b8f91727bd62897af15e41eb43c377efb9c610d48f2335cb0bd0087810f4352541b143c4b981b7e18f62de8ccdf633fc1bf037ab7cd779"
                                     "805e0dbcc0aae1cbcee1afb2e027df36bc04dcecbf154336c19f0af7e0a6472905e799f1953d2a0ff3348ab21aa4adafd1d234441cf807c03a00")
    assert all(v["ok"] is (c["name"] == "valid") for c, v in zip(verify, got["verify"]))
    keys = got["edpk"] + points
    names = ["rfc8032 1 octet"] + ["random %d" % i for i in range(8)] + point_names
    kat = {
        "errors": got["errors"],
        "torsion": got["torsion"],
        "scalar_mult": [c for c in mul if not c["name"].startswith("random")],
        "scalar_mult_random_out": [c["out"] for c in mul if c["name"].startswith("random")],
        "iterated": got["iter"],
        "public_keys": [dict(scalar=s, **o) for s, o in zip(pub, got["pub"])],
        "ed_public_keys": [{"secretKey": s, "out": k} for s, k in zip(ed_seeds, got["edpk"])],
        "points": [dict(name=n, enc=k, **o) for n, k, o in zip(names, keys, got["points"])],
        "to_montgomery": [dict(name=n, publicKey=k, **o) for n, k, o in zip(names, keys, got["mont"])],
        "to_montgomery_secret": [{"secretKey": s, "out": x} for s, x in zip(ed_seeds, got["xsec"])],
        "signatures": [dict(c, **o) for c, o in zip(sign, got["sigs"])],
        "verify": [dict(c, **o) for c, o in zip(verify, got["verify"])],
    }
    out = os.path.join(HERE, "ed448_kat.json")
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in kat.items()) + "\n}\n")
    print("%d scalarMult rows (%d rejected), %d points (%d rejected), %d toMontgomery rows (%d rejected), %d signatures, %d verify rows "
          "-> %s (%d bytes)" % (len(mul), sum(c["out"] is None for c in mul), len(keys), sum(o["error"] is not None for o in got["points"]),
                                len(keys), sum(o["out"] is None for o in got["mont"]), len(sign), len(verify), out, os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))
    print(sorted({c["error"] for c in mul if c["error"]} | {o["error"] for o in got["mont"] + got["points"] if o["error"]}))


main()
