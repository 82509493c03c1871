#!/usr/bin/env python3
"""Writes tests/golden/ed25519_sign_kat.json: known answers of the reference's ed25519 / ed25519ctx / ed25519ph getPublicKey,
getExtendedPublicKey and sign (src/abstract/edwards.ts:870-930, src/ed25519.ts:146-223), data only, as hex strings.  Run by hand
where the reference bundle (oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_ed25519_sign_kat.py
The inputs are built here (seeded; the message lengths sit on both sides of every SHA-512 block edge of the nonce hash and of the
challenge hash, ed25519_sign_helpers.edge_lengths), a small driver of ours runs them through the reference once, and the answers -
or the message of the error the reference throws - come back as JSON."""
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
from ed25519_sign_helpers import edge_lengths  # noqa: E402

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { ed25519, ed25519ctx, ed25519ph } from './ed25519.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const impl = { ed25519, ed25519ctx, ed25519ph };
const keys = job.seeds.map((s) => {
  const e = ed25519.utils.getExtendedPublicKey(bin(s));
  return { secretKey: s, publicKey: hex(ed25519.getPublicKey(bin(s))), head: hex(e.head), prefix: hex(e.prefix), scalar: e.scalar.toString(16),
           pointBytes: hex(e.pointBytes) };
});
const sign = job.sign.map((c) => {
  const o = c.context === null ? {} : { context: bin(c.context) };
  const sig = impl[c.variant].sign(bin(c.msg), bin(c.secretKey), o);
  const pk = impl[c.variant].getPublicKey(bin(c.secretKey));
  if (!impl[c.variant].verify(sig, bin(c.msg), pk, o)) throw new Error('the reference does not verify its own signature');
  return hex(sig);
});
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const sk = new Uint8Array(32), m = new Uint8Array(3);
const errors = {
  secret_key_length_31: msg(() => ed25519.getPublicKey(new Uint8Array(31))),
  secret_key_length_33: msg(() => ed25519.sign(m, new Uint8Array(33))),
  secret_key_length_64: msg(() => ed25519ctx.sign(m, new Uint8Array(64), { context: m })),
  context_on_plain: msg(() => ed25519.sign(m, sk, { context: Uint8Array.of(1) })),
  context_on_plain_verify: msg(() => ed25519.verify(new Uint8Array(64), m, sk, { context: Uint8Array.of(1) })),
  context_256: msg(() => ed25519ctx.sign(m, sk, { context: new Uint8Array(256) })),
  context_256_ph: msg(() => ed25519ph.sign(m, sk, { context: new Uint8Array(256) })),
  empty_context_on_plain: msg(() => ed25519.sign(m, sk, { context: new Uint8Array(0) })),
};
console.log(JSON.stringify({ keys, sign, errors }));
"""


def main():
    if not refjs.available():
        sys.exit("make_ed25519_sign_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_ed25519_sign_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "ed25519_sign_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    rng = random.Random("ed25519-sign-kat")
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    # RFC 8032 section 7.1 TEST 1 first, then seeded keys; 00.. and ff.. are as valid as any
    seeds = ["9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60", "00" * 32, "ff" * 32] + [rb(32).hex() for _ in range(29)]
    sign = []

    def add(variant, context, length):
        sign.append({"variant": variant, "context": None if context is None else context.hex(), "secretKey": seeds[len(sign) % 8],
                     "msg": rb(length).hex()})

    for n in sorted(set(edge_lengths(0)) | {0, 1, 1000}):
        add("ed25519", None, n)
    for clen in (0, 1, 255):
        ctx = rb(clen)
        for n in sorted(set(edge_lengths(34 + clen)) | {0, 1000}):
            add("ed25519ctx", ctx, n)
    # ed25519ph hashes the message first: both hashes see 64 bytes, the edges that matter are those of SHA-512(M) itself
    for n in (0, 1, 111, 112, 239, 240, 1000):
        add("ed25519ph", None, n)
    for clen in (1, 255):
        add("ed25519ph", rb(clen), 33)
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
    assert got["keys"][0]["publicKey"] == "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"   # RFC 8032 7.1 TEST 1
    assert all(k["publicKey"] == k["pointBytes"] for k in got["keys"])
    kat = {"errors": got["errors"], "keys": got["keys"], "sign": sign}
    out = os.path.join(HERE, "ed25519_sign_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, indent=0, separators=(",", ":"))
    print("%d keys, %d signatures -> %s (%d bytes)" % (len(seeds), len(sign), out, os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))


main()
