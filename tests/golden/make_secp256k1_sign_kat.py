#!/usr/bin/env python3
"""Writes tests/golden/secp256k1_sign_kat.json: known answers of the reference's secp256k1.getPublicKey / sign (ECDSA with RFC 6979
nonces, src/abstract/weierstrass.ts:1480-1568) and schnorr.getPublicKey / sign (BIP-340, src/secp256k1.ts:147-221), data only, as
hex strings.  Run by hand where the reference bundle (oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_secp256k1_sign_kat.py
The inputs are built here (seeded; the message lengths sit on both sides of the SHA-256 block edges of the prehash and of the
BIP-340 nonce and challenge hashes), a small driver of ours runs them through the reference once, and the answers - or the message
of the error the reference throws - come back as JSON."""
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

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
MSG_LENGTHS = (0, 1, 55, 56, 63, 64, 119, 120, 1000)

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { secp256k1, schnorr } from './secp256k1.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const keys = job.keys.map((s) => ({
  secretKey: s,
  compressed: hex(secp256k1.getPublicKey(bin(s), true)),
  uncompressed: hex(secp256k1.getPublicKey(bin(s), false)),
  xonly: hex(schnorr.getPublicKey(bin(s))),
}));
const ecdsa = job.ecdsa.map((c) => {
  const o = { prehash: c.prehash, lowS: c.lowS };
  if (c.extraEntropy !== null) o.extraEntropy = bin(c.extraEntropy);
  const out = {};
  for (const format of ['compact', 'recovered', 'der']) out[format] = hex(secp256k1.sign(bin(c.msg), bin(c.secretKey), { ...o, format }));
  const pk = secp256k1.getPublicKey(bin(c.secretKey));
  if (!secp256k1.verify(bin(out.compact), bin(c.msg), pk, { prehash: c.prehash, lowS: c.lowS }))
    throw new Error('the reference does not verify its own signature');
  return out;
});
const sch = job.schnorr.map((c) => {
  const sig = schnorr.sign(bin(c.msg), bin(c.secretKey), bin(c.auxRand));
  if (!schnorr.verify(sig, bin(c.msg), schnorr.getPublicKey(bin(c.secretKey)))) throw new Error('the reference does not verify its own signature');
  return hex(sig);
});
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const be = (v) => bin(v.toString(16).padStart(64, '0'));
const n = BigInt('0x' + job.n);
const m = new Uint8Array(32), good = be(BigInt(3));
const errors = {
  ecdsa_secret_key_0: msg(() => secp256k1.sign(m, be(BigInt(0)))),
  ecdsa_secret_key_n: msg(() => secp256k1.sign(m, be(n))),
  ecdsa_secret_key_max: msg(() => secp256k1.sign(m, be((BigInt(1) << BigInt(256)) - BigInt(1)))),
  ecdsa_secret_key_length_31: msg(() => secp256k1.sign(m, new Uint8Array(31))),
  ecdsa_secret_key_length_33: msg(() => secp256k1.sign(m, new Uint8Array(33))),
  ecdsa_message_not_bytes: msg(() => secp256k1.sign('abc', good)),
  public_key_secret_key_0: msg(() => secp256k1.getPublicKey(be(BigInt(0)))),
  public_key_secret_key_n: msg(() => secp256k1.getPublicKey(be(n))),
  public_key_secret_key_max: msg(() => secp256k1.getPublicKey(be((BigInt(1) << BigInt(256)) - BigInt(1)))),
  public_key_secret_key_length_31: msg(() => secp256k1.getPublicKey(new Uint8Array(31))),
  public_key_secret_key_length_33: msg(() => secp256k1.getPublicKey(new Uint8Array(33))),
  schnorr_secret_key_0: msg(() => schnorr.sign(m, be(BigInt(0)), m)),
  schnorr_secret_key_n: msg(() => schnorr.sign(m, be(n), m)),
  schnorr_secret_key_max: msg(() => schnorr.sign(m, be((BigInt(1) << BigInt(256)) - BigInt(1)), m)),
  schnorr_secret_key_length_31: msg(() => schnorr.sign(m, new Uint8Array(31), m)),
  schnorr_secret_key_length_33: msg(() => schnorr.sign(m, new Uint8Array(33), m)),
  schnorr_public_key_secret_key_0: msg(() => schnorr.getPublicKey(be(BigInt(0)))),
  schnorr_public_key_secret_key_length_31: msg(() => schnorr.getPublicKey(new Uint8Array(31))),
  schnorr_aux_rand_length_31: msg(() => schnorr.sign(m, good, new Uint8Array(31))),
  schnorr_message_not_bytes: msg(() => schnorr.sign('abc', good, m)),
};
console.log(JSON.stringify({ keys, ecdsa, schnorr: sch, errors }));
"""


def main():
    if not refjs.available():
        sys.exit("make_secp256k1_sign_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_secp256k1_sign_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "secp256k1_sign_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    rng = random.Random("secp256k1-sign-kat")
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    be = lambda v: v.to_bytes(32, "big").hex()  # noqa: E731
    keys = [be(1), be(N - 1), be(2), be(N - 2), be((N + 1) // 2), be((N - 1) // 2)] + [be(rng.randrange(1, N)) for _ in range(26)]
    ecdsa = []
    for prehash in (True, False):
        for low_s in (True, False):
            for extra in (False, True):
                for length in MSG_LENGTHS:
                    ecdsa.append({"secretKey": keys[len(ecdsa) % len(keys)], "msg": rb(length).hex(), "prehash": prehash, "lowS": low_s,
                                  "extraEntropy": rb(32).hex() if extra else None})
    schnorr = []
    for aux in ("zero", "seeded"):
        for length in MSG_LENGTHS:
            schnorr.append({"secretKey": keys[(3 * len(schnorr) + 1) % len(keys)], "msg": rb(length).hex(),
                            "auxRand": "00" * 32 if aux == "zero" else rb(32).hex()})
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"keys": keys, "ecdsa": ecdsa, "schnorr": schnorr, "n": "%064x" % N}, f)
        job = f.name
    try:
        res = subprocess.run([refjs.node(), driver, job], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(job)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    for c, sigs in zip(ecdsa, got["ecdsa"]):
        c.update(sigs)
    for c, sig in zip(schnorr, got["schnorr"]):
        c["sig"] = sig
    assert got["keys"][0]["compressed"] == "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"   # G
    kat = {"errors": got["errors"], "keys": got["keys"], "ecdsa": ecdsa, "schnorr": schnorr}
    out = os.path.join(HERE, "secp256k1_sign_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, indent=0, separators=(",", ":"))
    print("%d keys, %d ECDSA rows, %d Schnorr rows -> %s (%d bytes)" % (len(keys), len(ecdsa), len(schnorr), out, os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))


main()
