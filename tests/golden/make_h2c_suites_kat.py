#!/usr/bin/env python3
"""Writes tests/golden/h2c_suites_kat.json: known answers of the reference's secp256k1_hasher (src/secp256k1.ts:330-428) and
ed25519_hasher (src/ed25519.ts:294-405), data only, as hex strings.  Run by hand where the reference bundle
(oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_h2c_suites_kat.py
The RFC 9380 vector files of the reference are not part of the bundle; the reference's own code pins the answers, and the two `abc`
rows of RFC 9380 J.8.1 and J.5.1 are asserted below.  The inputs - the listed rows by name, the exceptional u found with big
integers, 128 seeded rows per suite - come from tests/h2c_suites_helpers.py, which the tests import too, so the file stores
answers only: per listed row the u values of hash_to_field and the point, per map row the point, per seeded row x || y || flag."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import refjs  # noqa: E402
import h2c_suites_helpers as hh  # noqa: E402  (the inputs: one definition for the generator and the tests)

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { secp256k1_hasher } from './secp256k1.mjs';
import { ed25519_hasher } from './ed25519.mjs';
import { hash_to_field } from './abstract/hash-to-curve.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const h64 = (n) => n.toString(16).padStart(64, '0');
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const out = {};
for (const [name, hasher] of [['secp256k1', secp256k1_hasher], ['ed25519', ed25519_hasher]]) {
  const P = hasher.Point;
  const pt = (p) => { const a = p.toAffine(); return { x: h64(a.x), y: h64(a.y), inf: p.equals(P.ZERO) ? 1 : 0 }; };
  const j = job[name];
  const t0 = Date.now();
  const hash = j.hash.map((c) => {
    const o = { DST: bin(c.dst) };
    const u = hash_to_field(bin(c.msg), c.count, Object.assign({}, hasher.defaults, o)).map((e) => h64(e[0]));
    return Object.assign({ u }, pt(c.count === 2 ? hasher.hashToCurve(bin(c.msg), o) : hasher.encodeToCurve(bin(c.msg), o)));
  });
  const ms = (Date.now() - t0) / Math.max(1, j.hash.length);
  const scalar = j.scalar.map((c) => h64(hasher.hashToScalar(bin(c.msg), c.dst === null ? undefined : { DST: bin(c.dst) })));
  const map = j.map.map((u) => pt(hasher.mapToCurve(BigInt(u))));
  const pair = j.pair.map((c) => pt(hasher.mapToCurve(BigInt(c[0])).add(hasher.mapToCurve(BigInt(c[1])))));
  const d = hasher.defaults;
  const errors = {
    empty_dst: msg(() => hasher.hashToCurve(new Uint8Array(1), { DST: '' })),
    empty_dst_bytes: msg(() => hasher.encodeToCurve(new Uint8Array(1), { DST: new Uint8Array(0) })),
    map_number: msg(() => hasher.mapToCurve(5)),
    map_array: msg(() => hasher.mapToCurve([5n])),
    msg_string: msg(() => hasher.hashToCurve('abc')),
    scalar_empty_dst: msg(() => hasher.hashToScalar(new Uint8Array(1), { DST: '' })),
  };
  out[name] = { hash, scalar, map, pair, errors, ms_per_hash: ms,
                defaults: { DST: d.DST, encodeDST: d.encodeDST, p: d.p.toString(), m: d.m, k: d.k, expand: d.expand },
                defaults_is_copy: hasher.defaults !== hasher.defaults };
}
console.log(JSON.stringify(out));
"""

PINS = {
    "secp256k1": ("3377e01eab42db296b512293120c6cee72b6ecf9f9205760bd9ff11fb3cb2c4b", "7f95890f33efebd1044d382a01b1bee0900fb6116f94688d487c6c7b9c8371f6"),
    "ed25519": ("608040b42285cc0d72cbb3985c6b04c935370c7361f4b7fbdb1ae7f8c1a8ecad", "1a8395b88338f22e435bbd301183e7f20a5f9de643f11882fb237f88268a5531"),
}


def main():
    if not refjs.available():
        sys.exit("make_h2c_suites_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_h2c_suites_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "h2c_suites_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    job, layout = {}, {}
    for suite in hh.SUITES:
        listed = hh.listed_rows(suite)
        seeded = [hh.seeded_row(suite, i) for i in range(hh.SEEDED)]
        hash_rows = [{"msg": m.hex(), "dst": d.hex(), "count": c} for _, m, d, c in listed]
        hash_rows += [{"msg": r[1].hex(), "dst": r[2].hex(), "count": r[3]} for r in seeded if r[0] == "hash"]
        exc = hh.exception_us(suite)
        maps = hh.edge_us(suite) + list(exc.values())
        pairs = hh.pair_rows(suite) + [(r[1], r[2]) for r in seeded if r[0] == "map"]
        job[suite] = {"hash": hash_rows, "scalar": [{"msg": m.hex(), "dst": None if d is None else d.hex()} for _, m, d in hh.scalar_rows(suite)],
                      "map": [str(u) for u in maps], "pair": [[str(a), str(b)] for a, b in pairs]}
        layout[suite] = (listed, seeded, exc)
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(job, f)
        path = f.name
    try:
        res = subprocess.run([refjs.node(), driver, path], capture_output=True, text=True, timeout=3000)
    finally:
        os.unlink(path)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    kat = {}
    for suite, (listed, seeded, exc) in layout.items():
        g = got[suite]
        nl, ne, npair = len(listed), len(hh.edge_us(suite)), len(hh.pair_rows(suite))
        by_name = {name: o for (name, _, _, _), o in zip(listed, g["hash"])}
        assert (by_name["abc/rfc/ro"]["x"], by_name["abc/rfc/ro"]["y"]) == PINS[suite], "RFC 9380 abc vector"
        # the u values agree with hashlib's expand_message_xmd (the bundle's hashes are node's own)
        for (name, m, d, c), o in zip(listed, g["hash"]):
            assert [int(u, 16) for u in o["u"]] == hh.hash_to_field(suite, m, d, c), name
        seeded_hash, seeded_pair = iter(g["hash"][nl:]), iter(g["pair"][npair:])
        answers = [next(seeded_hash) if r[0] == "hash" else next(seeded_pair) for r in seeded]
        flat = ["%s%s%02x" % (o["x"], o["y"], o["inf"]) for o in answers]
        kat[suite] = {
            "defaults": g["defaults"], "defaults_is_copy": g["defaults_is_copy"], "errors": g["errors"],
            "hash": [dict(name=name, **o) for (name, _, _, _), o in zip(listed, g["hash"])],
            "scalar": [{"name": name, "out": o} for (name, _, _), o in zip(hh.scalar_rows(suite), g["scalar"])],
            "map": [dict(u=str(u), **o) for u, o in zip(hh.edge_us(suite), g["map"])],
            "exceptions": [dict(name=name, u=str(u), **o) for (name, u), o in zip(exc.items(), g["map"][ne:])],
            "pairs": [dict(u0=str(a), u1=str(b), **o) for (a, b), o in zip(hh.pair_rows(suite), g["pair"])],
            "seeded": ["".join(flat[j:j + 4]) for j in range(0, len(flat), 4)],
        }
        print("%s: %d listed, %d exceptions %s, %.2f ms per hash under the bundle" % (suite, nl, len(exc), sorted(exc), g["ms_per_hash"]))
    s, e = kat["secp256k1"], kat["ed25519"]
    assert s["map"][0]["x"] == "bf6ce2abc92f03c7abfb18752134acc036b8e8ef46a7ed2634a86727c12d6ac1", "secp256k1 mapToCurve(0)"
    assert e["map"][0]["inf"] == 1 and (int(e["map"][0]["x"], 16), int(e["map"][0]["y"], 16)) == (0, 1), "ed25519 mapToCurve(0) is ZERO"
    assert s["scalar"][1]["out"] == "0afe998ff82d0b7ca5673a6c8dcaf2a0cd1361d1d1b2a4e4f57f4dc9a0305788", "secp256k1 hashToScalar(abc)"
    out = os.path.join(HERE, "h2c_suites_kat.json")
    with open(out, "w") as f:          # one row per line
        f.write("{\n" + ",\n".join(
            json.dumps(suite) + ":{\n" + ",\n".join(
                json.dumps(key) + ":" + ("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in v) + "\n]" if isinstance(v, list)
                                         else json.dumps(v, separators=(",", ":")))
                for key, v in rows.items()) + "\n}" for suite, rows in kat.items()) + "\n}\n")
    print("->", out, os.path.getsize(out), "bytes")
    print(json.dumps(s["errors"], indent=1))


main()
