#!/usr/bin/env python3
"""Writes tests/golden/ristretto255_kat.json: known answers of the reference's ristretto255 (_RistrettoPoint and ristretto255_hasher,
src/ed25519.ts:443-668), data only, as hex strings and decimal numbers.  Run by hand where the reference bundle
(oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_ristretto_kat.py
The inputs are the vectors of RFC 9496 appendix A as the reference's test lists them, edge rows, and 256 seeded rows per family; a
small driver of ours runs them through the reference once, and the answers - or the message of the error the reference throws -
come back as JSON.  The listed rows are written with their inputs; of the seeded rows only the ANSWERS are written (16 per line),
their inputs being rebuilt from a counter-mode hash by tests/ristretto_helpers.py (seeded_*), which this generator imports too.  The bundle's SHA-512 is Node's own, so hashToCurve is driven directly (default and custom DST); the RFC 9380 test
of the reference has no point vectors for ristretto255, only the empty-DST message, which is recorded under "errors".
The four constants are the decimal literals of src/ed25519.ts:410-424, passed through as data (the bundle does not export them)."""
import json
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import refjs  # noqa: E402
import ristretto_helpers as rh  # noqa: E402  (the seeded inputs: one definition for the generator and the tests)

REFERENCE = os.path.dirname(refjs.build.__defaults__[0])   # where the reference's checkout lies: the bundle was built from it
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { ristretto255, ristretto255_hasher } from './ed25519.mjs';
const RP = ristretto255.Point;
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const le = (n) => { let s = ''; for (let i = 0; i < 32; i++) { s += (n & 255n).toString(16).padStart(2, '0'); n >>= 8n; } return s; };
const run = (f) => { try { return { out: f(), error: null }; } catch (e) { return { out: null, error: e.message }; } };
const decode = job.decode.map((h) => run(() => {
  const p = RP.fromBytes(bin(h));
  const a = p.ep.toAffine();
  return { affine: le(a.x) + le(a.y), bytes: hex(p.toBytes()) };
}));
const small = [];
for (let i = 0, p = RP.ZERO; i < 16; i++, p = p.add(RP.BASE)) small.push(hex(p.toBytes()));
const derive = job.derive.map((h) => hex(ristretto255_hasher.deriveToCurve(bin(h)).toBytes()));
const hash = job.hash.map((c) => hex(ristretto255_hasher.hashToCurve(bin(c.msg), c.dst === null ? undefined : { DST: bin(c.dst) }).toBytes()));
const mul = job.mul.map((c) => run(() => hex(RP.fromBytes(bin(c.enc)).multiply(BigInt(c.k)).toBytes())));
const eq = job.equals.map((c) => RP.fromBytes(bin(c[0])).equals(RP.fromBytes(bin(c[1]))));
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const errors = {
  length: msg(() => RP.fromBytes(new Uint8Array(31))),
  type: msg(() => RP.fromBytes('x')),
  derive_length: msg(() => ristretto255_hasher.deriveToCurve(new Uint8Array(63))),
  empty_dst: msg(() => ristretto255_hasher.hashToCurve(new Uint8Array(1), { DST: '' })),
  multiply_zero: msg(() => RP.BASE.multiply(0n)),
  multiply_order: msg(() => RP.BASE.multiply(BigInt(job.L))),
  hex_odd: msg(() => RP.fromHex('abc')),
};
const wrapper = hex(ristretto255_hasher.hashToCurve(new Uint8Array(10).fill(5), { DST: 'ristretto255_XMD:SHA-512_R255MAP_RO_' }).toBytes());
console.log(JSON.stringify({ decode, small, derive, hash, mul, eq, errors, wrapper, base: hex(RP.BASE.toBytes()), zero: hex(RP.ZERO.toBytes()) }));
"""


def rfc_vectors():
    """the hex strings of test/rfc9496-ristretto-decaf.test.ts (ristretto255 half), read as DATA from the reference's test file"""
    with open(os.path.join(REFERENCE, "test", "rfc9496-ristretto-decaf.test.ts")) as f:
        text = f.read()
    text = text[:text.index("describe('decaf448'")]
    small = re.findall(r"'([0-9a-f]{64})'", text[text.index("encodingsOfSmallMultiples"):text.index("let B =")])
    bad = re.findall(r"'([0-9a-f]{64})'", text[text.index("badEncodings = ["):text.index("for (const badBytes")])
    labels = re.findall(r"^\s+'([^']+)',$", text[text.index("const labels = ["):text.index("const encodedHashToPoints")], flags=re.M)
    label_out = re.findall(r"'([0-9a-f]{64})'", text[text.index("const encodedHashToPoints"):text.index("for (let i = 0; i < labels.length")])
    vec = text[text.index("const VECTORS = ["):text.index("for (const { I, O } of VECTORS)")]
    ins = ["".join(re.findall(r"'([0-9a-f]{64})'", blk)) for blk in re.findall(r"I:(.*?)O:", vec, flags=re.S)]
    outs = [o.replace(" ", "") for o in re.findall(r"O: '([0-9a-f ]+)'", vec)]
    assert len(small) == 16 and len(bad) == 29 and len(labels) == len(label_out) == 7 and len(ins) == len(outs) == 11
    return small, bad, labels, label_out, ins, outs


def constants():
    with open(os.path.join(REFERENCE, "src", "ed25519.ts")) as f:
        text = f.read()
    out = {}
    for name in ("SQRT_AD_MINUS_ONE", "INVSQRT_A_MINUS_D", "ONE_MINUS_D_SQ", "D_MINUS_ONE_SQ"):
        out[name] = re.search(r"const %s = [^']*'(\d+)'" % name, text).group(1)
    return out


def main():
    if not refjs.available():
        sys.exit("make_ristretto_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_ristretto_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "ristretto_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    import hashlib
    small, bad, labels, label_out, ins, outs = rfc_vectors()
    rng = random.Random("ristretto255-kat")
    le = lambda v: v.to_bytes(32, "little").hex()  # noqa: E731
    sqrt_m1 = pow(2, (P - 1) // 4, P)
    i_even = sqrt_m1 if sqrt_m1 % 2 == 0 else P - sqrt_m1
    edges = [le(i_even), le(P - i_even), le(P - 1), le(P), le(P + 1), le(2**255 - 1), le(1 << 255), le(2**256 - 1), le(2)]
    n = rh.SEEDED
    # listed rows (inputs in the file) and seeded rows (inputs rebuilt by tests/ristretto_helpers.py, answers in the file)
    derive_listed = ins + [hashlib.sha512(s.encode()).hexdigest() for s in labels] + ["00" * 64, "00" * 32 + le(P), le(P - 1) + le(2**255 - 1)]
    derive = derive_listed + [rh.seeded_derive_in(i).hex() for i in range(n)]

    def call(job):
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump(job, f)
            path = f.name
        try:
            res = subprocess.run([refjs.node(), driver, path], capture_output=True, text=True, timeout=1200)
        finally:
            os.unlink(path)
        if res.returncode != 0:
            sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
        return json.loads(res.stdout.strip().splitlines()[-1])

    first = call({"decode": [], "derive": derive, "hash": [], "mul": [], "equals": [], "L": str(L)})
    dout = first["derive"][len(derive_listed):]
    valid = dout[:128]
    listed = small + bad + edges
    decode = listed + [rh.seeded_encoding(i, dout).hex() for i in range(n)]
    names = ["small multiple %d" % i for i in range(16)] + ["rfc bad %d" % i for i in range(29)] + ["edge %d" % i for i in range(len(edges))]
    hash_listed = [{"msg": m.hex(), "dst": None} for m in (b"", b"abc", bytes(10 * [5]))] + \
                  [{"msg": b"abc".hex(), "dst": (b"x" * 300).hex()}]                                 # an oversize DST is hashed first
    hash_rows = hash_listed + [{"msg": rh.seeded_msg(i).hex(), "dst": None} for i in range(n)] + \
        [{"msg": rh.seeded_msg(i).hex(), "dst": rh.seeded_dst(i).hex()} for i in range(n)]
    base = small[1]
    mul = []
    for enc in [base, small[5]] + valid[:6]:
        for k in (1, 2, L - 1, rng.randrange(1, L)):
            mul.append({"enc": enc, "k": str(k)})
    mul += [{"enc": base, "k": "0"}, {"enc": base, "k": str(L)}, {"enc": bad[0], "k": "5"}, {"enc": bad[12], "k": "5"}]
    equals = [[base, base], [base, small[2]], [small[0], small[0]], [valid[0], valid[0]], [valid[0], valid[1]]]
    got = call({"decode": decode, "derive": derive, "hash": hash_rows, "mul": mul, "equals": equals, "L": str(L)})
    assert got["small"] == small and got["base"] == small[1] and got["zero"] == small[0]
    assert got["derive"][:11] == outs and got["derive"][11:18] == label_out and got["derive"][len(derive_listed):] == dout
    assert all(o["error"] for o in got["decode"][16:16 + 29]) and all(o["out"] and o["out"]["bytes"] == h for o, h in zip(got["decode"][:16], small))
    assert got["wrapper"] == "be2194e53cc014665821003f8ecf49e99b7cd16f5326e53f234ecd21c448ee6c" == got["hash"][2]
    seeded_dec = got["decode"][len(listed):]
    assert all(o["out"]["bytes"] == e for o, e in zip(seeded_dec, decode[len(listed):]) if o["out"])
    code = {None: "0", rh.ENC1: "1", rh.ENC2: "2"}
    lines = lambda rows, per: ["".join(rows[j:j + per]) for j in range(0, len(rows), per)]  # noqa: E731
    nl, hl = len(derive_listed), len(hash_listed)
    kat = {
        "constants": constants(),
        "errors": got["errors"],
        "base": got["base"],
        "small_multiples": small,
        "decode": [{"name": nm, "enc": h, "affine": o["out"] and o["out"]["affine"], "bytes": o["out"] and o["out"]["bytes"], "error": o["error"]}
                   for nm, h, o in zip(names, listed, got["decode"])],
        "derive": [{"in": i, "out": o} for i, o in zip(derive_listed, got["derive"])],
        "labels": [{"label": s, "out": o} for s, o in zip(labels, label_out)],
        "hash": [dict(c, out=o) for c, o in zip(hash_listed[:3] + hash_listed[3:], got["hash"][:3] + got["hash"][3:4])],
        "multiply": [dict(c, **o) for c, o in zip(mul, got["mul"])],
        "equals": [{"a": a, "b": b, "out": o} for (a, b), o in zip(equals, got["eq"])],
        "seeded": {
            "decode_verdict": "".join(code[o["error"]] for o in seeded_dec),
            "decode_affine": lines([o["out"]["affine"] for o in seeded_dec if o["out"]][:rh.SEEDED_AFFINE], 8),
            "derive_out": lines(dout, 16),
            "hash_default_out": lines(got["hash"][hl:hl + n], 16),
            "hash_custom_out": lines(got["hash"][hl + n:], 16),
        },
    }
    assert len(got["hash"]) == hl + 2 * n and len(got["derive"]) == nl + n
    out = os.path.join(HERE, "ristretto255_kat.json")
    with open(out, "w") as f:          # one row per line for the listed families, 16 answers per line for the seeded ones
        f.write("{\n" + ",\n".join(
            json.dumps(key) + ":" + (json.dumps(v, separators=(",", ":")) if not isinstance(v, list) or key == "small_multiples" else
                                     "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in v) + "\n]")
            for key, v in kat.items() if key != "seeded") + ",\n\"seeded\":{\n" + ",\n".join(
            json.dumps(key) + ":" + (json.dumps(v) if isinstance(v, str) else "[\n" + ",\n".join(json.dumps(r) for r in v) + "\n]")
            for key, v in kat["seeded"].items()) + "\n}\n}\n")
    kat = rh.kat()
    dec = kat["decode"]
    print("%d decode rows (%d rejected: %s), %d derive, %d hash, %d multiply rows -> %s (%d bytes)" % (
        len(dec), sum(c["error"] is not None for c in dec), sorted({c["error"] for c in dec if c["error"]}), len(kat["derive"]), len(kat["hash"]),
        len(mul), out, os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))
    print(json.dumps(kat["multiply"][-4:], indent=1))


main()
