#!/usr/bin/env python3
"""Writes tests/golden/ed448_sign_kat.json: known answers of the reference's ed448 / ed448ph getPublicKey, getExtendedPublicKey and
sign (src/abstract/edwards.ts:866-930, src/ed448.ts:190-246), data only, as hex strings.  Run by hand where the reference bundle
(oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_ed448_sign_kat.py
The inputs are built here (seeded; the message lengths put the TOTAL absorbed length of the nonce hash and of the challenge hash on
every residue 0, 1, 134, 135 mod 136, ed448_sign_helpers.sign_edge_lengths), a small driver of ours runs them through the reference
once, and the answers - or the message of the error the reference throws - come back as JSON."""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import refjs  # noqa: E402
from ed448_sign_helpers import PH_LENGTHS, sign_edge_lengths  # noqa: E402

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { ed448, ed448ph } from './ed448.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const impl = { ed448, ed448ph };
const keys = job.seeds.map((s) => {
  const e = ed448.utils.getExtendedPublicKey(bin(s));
  return { secretKey: s, publicKey: hex(ed448.getPublicKey(bin(s))), head: hex(e.head), prefix: hex(e.prefix), scalar: e.scalar.toString(16),
           pointBytes: hex(e.pointBytes) };
});
const sign = job.sign.map((c) => {
  const o = { context: bin(c.context) };
  const sig = impl[c.variant].sign(bin(c.msg), bin(c.secretKey), o);
  const pk = impl[c.variant].getPublicKey(bin(c.secretKey));
  if (!impl[c.variant].verify(sig, bin(c.msg), pk, o)) throw new Error('the reference does not verify its own signature');
  if (c.context === '' && hex(impl[c.variant].sign(bin(c.msg), bin(c.secretKey))) !== hex(sig)) throw new Error('no context is not the empty context');
  return hex(sig);
});
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const sk = new Uint8Array(57), m = new Uint8Array(3);
const errors = {
  secret_key_length_56: msg(() => ed448.getPublicKey(new Uint8Array(56))),
  secret_key_length_58: msg(() => ed448.sign(m, new Uint8Array(58))),
  secret_key_length_114: msg(() => ed448ph.sign(m, new Uint8Array(114), { context: m })),
  context_256: msg(() => ed448.sign(m, sk, { context: new Uint8Array(256) })),
  context_256_ph: msg(() => ed448ph.sign(m, sk, { context: new Uint8Array(256) })),
  context_255: msg(() => ed448.sign(m, sk, { context: new Uint8Array(255) })),
};
console.log(JSON.stringify({ keys, sign, errors }));
"""


def main():
    if not refjs.available():
        sys.exit("make_ed448_sign_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_ed448_sign_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "ed448_sign_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    rng = random.Random("ed448-sign-kat")
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    # RFC 8032 section 7.4 "1 octet" first, then 00.., ff.., then seeded keys
    rfc = ("c4eab05d357007c632f3dbb48489924d552b08fe0c353a0d4a1f00acda2c463afbea67c5e8d2877c5e3bc397a659949ef8021e954e0a12274e")
    seeds = [rfc, "00" * 57, "ff" * 57] + [rb(57).hex() for _ in range(27)]
    sign = []

    def add(variant, context, length):
        sign.append({"variant": variant, "context": context.hex(), "secretKey": seeds[len(sign) % 8], "msg": rb(length).hex()})

    for clen in (0, 1, 255):
        ctx = rb(clen)
        for n in sorted(set(sign_edge_lengths(clen)) | {0, 1, 1000}):
            add("ed448", ctx, n)
    # ed448ph hashes the message first: both hashes see 64 bytes, the edges that matter are those of SHAKE256(M, 64) itself
    for n in PH_LENGTHS + (1000,):
        add("ed448ph", b"", n)
    for clen in (1, 255):
        add("ed448ph", rb(clen), 33)
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"seeds": seeds, "sign": sign}, f)
        job = f.name
    try:
        res = subprocess.run([refjs.node(), driver, job], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(job)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    for c, sig in zip(sign, got["sign"]):
        c["sig"] = sig
    # RFC 8032 7.4 "1 octet": the public key
    assert got["keys"][0]["publicKey"] == ("43ba28f430cdff456ae531545f7ecd0ac834a55d9358c0372bfa0c6c6798c0866aea01eb00742802b8438ea4cb82169c23"
                                           "5160627b4c3a9480")
    assert all(k["publicKey"] == k["pointBytes"] for k in got["keys"])
    kat = {"errors": got["errors"], "keys": got["keys"], "sign": sign}
    out = os.path.join(HERE, "ed448_sign_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, indent=0, separators=(",", ":"))
    print("%d keys, %d signatures -> %s (%d bytes)" % (len(seeds), len(sign), out, os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))


main()
