#!/usr/bin/env python3
"""Writes tests/golden/h2c448_kat.json: known answers of the reference's ed448_hasher (src/ed448.ts:313-417), decaf448_hasher
(:662-701), hash_to_field and expand_message_xof (src/abstract/hash-to-curve.ts), data only, as hex strings.  Run by hand where the
reference bundle (oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_h2c448_kat.py
The inputs - the listed rows by name, the exceptional u found with big integers, 128 seeded rows per suite - come from
tests/h2c448_helpers.py, which the tests import too, so the file stores answers only: per listed row the u values of hash_to_field
and the point, per map row the point, per seeded row x || y or the decaf448 encoding.  The `pins` are inline vectors of the
reference's test/rfc9496-ristretto-decaf.test.ts copied as data and asserted below."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import refjs  # noqa: E402
import h2c448_helpers as hh  # noqa: E402  (the inputs: one definition for the generator and the tests)

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { ed448_hasher, decaf448_hasher } from './ed448.mjs';
import { hash_to_field, expand_message_xof } from './abstract/hash-to-curve.mjs';
import { shake256 } from '../hashes_shim.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const hex = (b) => Buffer.from(b).toString('hex');
const h112 = (n) => n.toString(16).padStart(112, '0');
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const P = ed448_hasher.Point;
const pt = (p) => { const a = p.toAffine(); return { x: h112(a.x), y: h112(a.y), zero: p.equals(P.ZERO) ? 1 : 0 }; };
const opt = (d) => (d === null ? undefined : { DST: bin(d) });
const out = {};
out.hash = job.hash.map((c) => {
  const o = { DST: bin(c.dst) };
  const u = hash_to_field(bin(c.msg), c.count, Object.assign({}, ed448_hasher.defaults, o)).map((e) => h112(e[0]));
  return Object.assign({ u }, pt(c.count === 2 ? ed448_hasher.hashToCurve(bin(c.msg), o) : ed448_hasher.encodeToCurve(bin(c.msg), o)));
});
out.scalar = job.scalar.map((c) => h112(ed448_hasher.hashToScalar(bin(c.msg), opt(c.dst))));
out.decaf_scalar = job.scalar.map((c) => h112(decaf448_hasher.hashToScalar(bin(c.msg), opt(c.dst))));
out.decaf = job.decaf.map((c) => hex(decaf448_hasher.hashToCurve(bin(c.msg), { DST: bin(c.dst) }).toBytes()));
out.xof = job.xof.map((c) => hex(expand_message_xof(bin(c.msg), bin(c.dst), c.len, 224, shake256)));
out.map = job.map.map((u) => pt(ed448_hasher.mapToCurve(BigInt(u))));
out.pair = job.pair.map((c) => pt(ed448_hasher.mapToCurve(BigInt(c[0])).add(ed448_hasher.mapToCurve(BigInt(c[1])))));
const d = ed448_hasher.defaults;
out.errors = {
  empty_dst: msg(() => ed448_hasher.hashToCurve(new Uint8Array(1), { DST: '' })),
  empty_dst_bytes: msg(() => ed448_hasher.encodeToCurve(new Uint8Array(1), { DST: new Uint8Array(0) })),
  map_number: msg(() => ed448_hasher.mapToCurve(5)),
  map_array: msg(() => ed448_hasher.mapToCurve([5n])),
  msg_string: msg(() => ed448_hasher.hashToCurve('abc')),
  scalar_empty_dst: msg(() => ed448_hasher.hashToScalar(new Uint8Array(1), { DST: '' })),
  decaf_empty_dst: msg(() => decaf448_hasher.hashToCurve(new Uint8Array(1), { DST: '' })),
  decaf_scalar_empty_dst: msg(() => decaf448_hasher.hashToScalar(new Uint8Array(1), { DST: '' })),
};
out.defaults = { DST: d.DST, encodeDST: d.encodeDST, p: d.p.toString(), m: d.m, k: d.k, expand: d.expand };
out.defaults_is_copy = ed448_hasher.defaults !== ed448_hasher.defaults;
console.log(JSON.stringify(out));
"""

# decaf448_hasher.hashToCurve(new Uint8Array(10).fill(5), { DST: 'decaf448_XOF:SHAKE256_D448MAP_RO_' }).toBytes() as the reference's
# test/rfc9496-ristretto-decaf.test.ts ('decaf448_hasher and wrapper helpers') states it: the row "fill5" of decaf_rows
PINS = {"fill5": "1287dea7519af966cf537a58f614e8b39b93a7c0b989bcdb4f94af8f2573ab59589accb0d2a2097b5f30c1d721619470f21e78613bbfc4b6"}


def main():
    if not refjs.available():
        sys.exit("make_h2c448_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_h2c448_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "h2c448_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    listed, exc = hh.listed_rows(), hh.exception_us()
    seeded = {suite: [hh.seeded_row(suite, i) for i in range(hh.SEEDED)] for suite in hh.SEEDED_SUITES}
    hash_rows = [{"msg": m.hex(), "dst": d.hex(), "count": c} for _, m, d, c in listed]
    hash_rows += [{"msg": m.hex(), "dst": d.hex(), "count": c} for suite, c in (("ro", 2), ("nu", 1)) for m, d in seeded[suite]]
    decaf_rows = [{"msg": m.hex(), "dst": d.hex()} for _, m, d in hh.decaf_rows()]
    decaf_rows += [{"msg": m.hex(), "dst": d.hex()} for m, d in seeded["decaf"]]
    maps = hh.edge_us() + list(exc.values()) + hh.seeded_us()
    pairs = hh.pair_rows() + hh.seeded_pairs()
    job = {"hash": hash_rows, "decaf": decaf_rows,
           "scalar": [{"msg": m.hex(), "dst": None if d is None else d.hex()} for _, m, d in hh.scalar_rows()],
           "xof": [{"msg": m.hex(), "dst": d.hex(), "len": n} for _, m, d, n in hh.xof_rows()],
           "map": [str(u) for u in maps], "pair": [[str(a), str(b)] for a, b in pairs]}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(job, f)
        path = f.name
    try:
        res = subprocess.run([refjs.node(), driver, path], capture_output=True, text=True, timeout=3000)
    finally:
        os.unlink(path)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    g = json.loads(res.stdout.strip().splitlines()[-1])
    nl, ne, nx, npair, nd = len(listed), len(hh.edge_us()), len(exc), len(hh.pair_rows()), len(hh.decaf_rows())
    by_name = {name: o for (name, _, _), o in zip(hh.decaf_rows(), g["decaf"])}
    for name, enc in PINS.items():
        assert by_name[name] == enc, "the reference's inline vector " + name
    for o in g["map"][ne:ne + nx]:
        assert o["zero"] == 1, "an exceptional u maps to ZERO"
    xy = lambda o: o["x"] + o["y"]  # noqa: E731
    S = hh.SEEDED
    kat = {
        "defaults": g["defaults"], "defaults_is_copy": g["defaults_is_copy"], "errors": g["errors"],
        "pins": [{"name": name, "out": enc} for name, enc in PINS.items()],
        "hash": [dict(name=name, **o) for (name, _, _, _), o in zip(listed, g["hash"])],
        "scalar": [{"name": name, "out": o} for (name, _, _), o in zip(hh.scalar_rows(), g["scalar"])],
        "decaf_scalar": [{"name": name, "out": o} for (name, _, _), o in zip(hh.scalar_rows(), g["decaf_scalar"])],
        "decaf": [{"name": name, "out": o} for (name, _, _), o in zip(hh.decaf_rows(), g["decaf"])],
        "xof": [{"name": name, "out": o} for (name, _, _, _), o in zip(hh.xof_rows(), g["xof"])],
        "map": [dict(u=str(u), **o) for u, o in zip(hh.edge_us(), g["map"])],
        "exceptions": [dict(name=name, u=str(u), **o) for (name, u), o in zip(exc.items(), g["map"][ne:])],
        "seeded_map": [o["x"] + o["y"] for o in g["map"][ne + nx:]],
        "pairs": [dict(u0=str(a), u1=str(b), **o) for (a, b), o in zip(hh.pair_rows(), g["pair"])],
        "seeded_pairs": [xy(o) for o in g["pair"][npair:]],
        "seeded_ro": [xy(o) for o in g["hash"][nl:nl + S]],
        "seeded_nu": [xy(o) for o in g["hash"][nl + S:nl + 2 * S]],
        "seeded_decaf": g["decaf"][nd:],
    }
    out = os.path.join(HERE, "h2c448_kat.json")
    with open(out, "w") as f:          # one row per line
        f.write("{\n" + ",\n".join(
            json.dumps(key) + ":" + ("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in v) + "\n]" if isinstance(v, list)
                                     else json.dumps(v, separators=(",", ":")))
            for key, v in kat.items()) + "\n}\n")
    print("%d listed, %d exceptions %s ->" % (nl, nx, sorted(exc)), out, os.path.getsize(out), "bytes")
    print(json.dumps(kat["errors"], indent=1))


main()
