#!/usr/bin/env python3
"""Writes tests/golden/ristretto255_oprf_kat.json: known answers of the reference's ristretto255_oprf (src/ed25519.ts:682, built by
createOPRF of src/abstract/oprf.ts), data only, as hex strings.  Run by hand where the reference bundle (oracle/_ref/refjs.bundle)
and node exist, never by the tests:
    python tests/golden/make_oprf_kat.py
A small driver of ours runs the three modes through the reference with a RECORDED rng (the bytes are in the file, so the blinds and
the proof nonce can be reproduced), and the answers - or the message of the error the reference throws - come back as JSON.  The
inputs of a batch are written as indices into seeded_inputs(); of the seeded hashToScalar and xmd rows only the answers are written,
their inputs being rebuilt by tests/oprf_helpers.py (seeded_*), which this generator imports too.  The anchors of RFC 9497 A.1.1 / A.1.2 (vector 1)
are asserted here before anything is written."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import refjs  # noqa: E402
import oprf_helpers as oh  # noqa: E402  (the seeded inputs: one definition for the generator and the tests)

L = oh.L

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { ristretto255_oprf as O, ristretto255, ristretto255_hasher } from './ed25519.mjs';
import { expand_message_xmd } from './abstract/hash-to-curve.mjs';
import { sha512 } from '../hashes_shim.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
// an rng that replays recorded bytes, 48 at a time
const replay = (h) => { const b = bin(h); let at = 0; return (n) => { const r = b.slice(at, at + n); at += n; if (r.length !== n) throw new Error('rng ran dry'); return r; }; };
const suite = (mode, info) => (mode === 0 ? O.oprf : mode === 1 ? O.voprf : O.poprf(bin(info)));
const out = { name: O.name, modes: [], errors: {} };
for (const m of job.modes) {
  const S = suite(m.mode, m.info);
  const keys = S.deriveKeyPair(bin(job.seed), bin(job.key_info));
  const sk = keys.secretKey, pk = keys.publicKey;
  const res = { mode: m.mode, info: m.info, skS: hex(sk), pkS: hex(pk), batches: [] };
  for (const b of m.batches) {
    const rng = replay(b.rng);
    const inputs = b.inputs.map(bin);
    const blinds = inputs.map((i) => (m.mode === 2 ? S.blind(i, pk, rng) : S.blind(i, rng)));
    const blinded = blinds.map((x) => x.blinded);
    let evaluated, proof = null;
    if (m.mode === 0) evaluated = blinded.map((x) => S.blindEvaluate(sk, x));
    else {
      const r = m.mode === 1 ? S.blindEvaluateBatch(sk, pk, blinded, rng) : S.blindEvaluateBatch(sk, blinded, rng);
      evaluated = r.evaluated; proof = r.proof;
    }
    let output;
    if (m.mode === 0) output = inputs.map((i, j) => S.finalize(i, blinds[j].blind, evaluated[j]));
    else {
      const items = inputs.map((i, j) => ({ input: i, blind: blinds[j].blind, evaluated: evaluated[j], blinded: blinded[j] }));
      output = m.mode === 1 ? S.finalizeBatch(items, pk, proof) : S.finalizeBatch(items, proof, blinds[0].tweakedKey);
    }
    res.batches.push({ idx: b.idx, rng: b.rng, blind: blinds.map((x) => hex(x.blind)), blinded: blinded.map(hex),
      evaluated: evaluated.map(hex), proof: proof && hex(proof), tweakedKey: m.mode === 2 ? hex(blinds[0].tweakedKey) : null,
      output: output.map(hex), evaluate: inputs.map((i) => hex(S.evaluate(sk, i))) });
  }
  out.modes.push(res);
}
out.anchor = job.anchor.map((a) => {
  const S = suite(a.mode, '');
  const rng = replay(a.rng);
  const b = S.blind(bin(a.input), rng);
  const ev = S.blindEvaluate(bin(a.skS), b.blinded);
  return { mode: a.mode, skS: a.skS, input: a.input, rng: a.rng, blind: hex(b.blind), blinded: hex(b.blinded), evaluated: hex(ev),
    output: hex(S.finalize(bin(a.input), b.blind, ev)) };
});
out.anchor_keys = [0, 1, 2].map((mode) => { const k = suite(mode, '').deriveKeyPair(bin(job.rfc_seed), bin(job.rfc_key_info)); return { mode, skS: hex(k.secretKey), pkS: hex(k.publicKey) }; });
out.hash_to_scalar = job.h2s.map((c) => { let n = ristretto255_hasher.hashToScalar(bin(c.msg), { DST: bin(c.dst) }); let s = ''; for (let i = 0; i < 32; i++) { s += (n & 255n).toString(16).padStart(2, '0'); n >>= 8n; } return s; });
out.xmd = job.xmd.map((c) => hex(expand_message_xmd(bin(c.msg), bin(c.dst), c.len, sha512)));
const V = O.voprf, P2 = O.poprf(new Uint8Array(3));
const k1 = V.deriveKeyPair(bin(job.seed), bin(job.key_info));
const good = V.blind(bin('00'), replay(job.modes[0].batches[0].rng));
const zero = new Uint8Array(32), ff = new Uint8Array(64).fill(255), badEnc = new Uint8Array(32).fill(1);
const le = (n) => { const b = new Uint8Array(32); for (let i = 0; i < 32; i++) { b[i] = Number(n & 255n); n >>= 8n; } return b; };
const ev = V.blindEvaluate(k1.secretKey, k1.publicKey, good.blinded, replay(job.modes[0].batches[0].rng));
out.errors = {
  input_long: msg(() => O.oprf.blind(new Uint8Array(65536))),
  seed_length: msg(() => O.oprf.deriveKeyPair(new Uint8Array(31), new Uint8Array(0))),
  blind_zero: msg(() => O.oprf.finalize(bin('00'), zero, good.blinded)),
  blind_order: msg(() => O.oprf.finalize(bin('00'), le(BigInt(job.L)), good.blinded)),
  secret_zero: msg(() => O.oprf.blindEvaluate(zero, good.blinded)),
  bad_encoding: msg(() => O.oprf.blindEvaluate(k1.secretKey, badEnc)),
  identity_blinded: msg(() => O.oprf.blindEvaluate(k1.secretKey, zero)),
  identity_evaluated: msg(() => O.oprf.finalize(bin('00'), good.blind, zero)),
  identity_public_key: msg(() => V.blindEvaluate(k1.secretKey, zero, good.blinded)),
  identity_tweaked_key: msg(() => P2.finalize(bin('00'), good.blind, ev.evaluated, good.blinded, ev.proof, zero)),
  proof_length: msg(() => V.finalize(bin('00'), good.blind, ev.evaluated, good.blinded, k1.publicKey, new Uint8Array(63))),
  proof_ff: msg(() => V.finalize(bin('00'), good.blind, ev.evaluated, good.blinded, k1.publicKey, ff)),
  proof_zero: msg(() => V.finalize(bin('00'), good.blind, ev.evaluated, good.blinded, k1.publicKey, new Uint8Array(64))),
  expected_array: msg(() => V.blindEvaluateBatch(k1.secretKey, k1.publicKey, good.blinded)),
  rng_type: msg(() => O.oprf.blind(bin('00'), 5)),
};
out.error_inputs = { blinded: hex(good.blinded), blind: hex(good.blind), evaluated: hex(ev.evaluated), proof: hex(ev.proof), skS: hex(k1.secretKey), pkS: hex(k1.publicKey) };
console.log(JSON.stringify(out));
"""

# RFC 9497 A.1.1 vector 1: the blind the RFC lists, as 48 rng bytes that mapHashToField brings to it (blind - 1, zero-extended)
RFC_SEED = "a3" * 32
RFC_KEY_INFO = b"test key".hex()
RFC_BLIND = int.from_bytes(bytes.fromhex("64d37aed22a27f5191de1c1d69fadb899d8862b58eb4220029e036ec4c1f6706"), "little")
ANCHOR = {"skS": "5ebcea5ee37023ccb9fc2d2019f9d7737be85591ae8652ffa9ef0f4d37063b0e", "input": "00",
          "blinded": "609a0ae68c15a3cf6903766461307e5c8bb2f95e7e6550e1ffa2dc99e412803c",
          "evaluated": "7ec6578ae5120958eb2db1745758ff379e77cb64fe77b0b2d8cc917ea0869c7e",
          "output": "527759c3d9366f277d8c6020418d96bb393ba2afb20ff90df23fb7708264e2f3ab9135e3bd69955851de4b1f9fe8a0973396719b7912ba9ee8aa7d0b5e24bcf6"}
ANCHOR_VOPRF = {"skS": "e6f73f344b79b379f1a0dd37e07ff62e38d9f71345ce62ae3a9bc60b04ccd909",
                "pkS": "c803e2cc6b05fc15064549b5920659ca4a77b2cca6f04f6b357009335476ad4e"}


def main():
    if not refjs.available():
        sys.exit("make_oprf_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_oprf_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "oprf_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    inputs = [m.hex() for m in oh.seeded_inputs()]
    sizes = (1, 2, 3, 5)

    def batches(tag):
        out, at = [], 0
        for b, n in enumerate(sizes):
            idx = [(at + j) % len(inputs) for j in range(n)]
            at += n
            out.append({"idx": idx, "inputs": [inputs[j] for j in idx], "rng": oh.seeded_bytes("rng-%s" % tag, b, 48 * (n + 1)).hex()})
        # every input once more as single rows, so that each length is seen in each mode
        out += [{"idx": [j], "inputs": [h], "rng": oh.seeded_bytes("rng1-%s" % tag, j, 96).hex()} for j, h in enumerate(inputs)]
        return out

    infos = ["", b"test info".hex(), oh.seeded_bytes("info", 0, 300).hex()]
    modes = [{"mode": 0, "info": "", "batches": batches("m0")}, {"mode": 1, "info": "", "batches": batches("m1")}] + \
            [{"mode": 2, "info": info, "batches": batches("m2-%d" % j)} for j, info in enumerate(infos)]
    job = {"L": str(L), "seed": RFC_SEED, "key_info": RFC_KEY_INFO, "rfc_seed": RFC_SEED, "rfc_key_info": RFC_KEY_INFO, "modes": modes,
           "anchor": [{"mode": 0, "skS": ANCHOR["skS"], "input": "00", "rng": (RFC_BLIND - 1).to_bytes(48, "little").hex()}],
           "h2s": [{"msg": oh.seeded_scalar_msg(i).hex(), "dst": (b"HashToScalar-" + oh.ctx_of(i % 3)).hex()} for i in range(64)],
           "xmd": [dict(zip(("msg", "dst", "len"), (m.hex(), d.hex(), n))) for m, d, n in map(oh.seeded_xmd_row, range(64))]}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(job, f)
        path = f.name
    try:
        res = subprocess.run([refjs.node(), driver, path], capture_output=True, text=True, timeout=1200)
    finally:
        os.unlink(path)
        os.unlink(driver)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-3000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    a = got["anchor"][0]
    for key, want in ANCHOR.items():
        assert a[key] == want, (key, a[key], want)
    assert a["blind"] == oh.le32(RFC_BLIND).hex()
    assert got["anchor_keys"][0]["skS"] == ANCHOR["skS"], got["anchor_keys"]
    assert {k: got["anchor_keys"][1][k] for k in ANCHOR_VOPRF} == ANCHOR_VOPRF, got["anchor_keys"]
    lines = lambda rows, per: ["".join(rows[j:j + per]) for j in range(0, len(rows), per)]  # noqa: E731
    kat = {"name": got["name"], "seed": RFC_SEED, "key_info": RFC_KEY_INFO, "anchor": got["anchor"], "anchor_keys": got["anchor_keys"],
           "errors": got["errors"], "error_inputs": got["error_inputs"], "modes": got["modes"],
           "seeded": {"hash_to_scalar": lines(got["hash_to_scalar"], 8), "xmd": got["xmd"]}}
    out = os.path.join(HERE, "ristretto255_oprf_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, separators=(",", ":"), indent=None)
        f.write("\n")
    print("%d mode blocks, %d batches each -> %s (%d bytes)" % (len(got["modes"]), len(got["modes"][0]["batches"]), out, os.path.getsize(out)))
    print(json.dumps(got["errors"], indent=1))


main()
