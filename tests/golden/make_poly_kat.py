#!/usr/bin/env python3
"""Writes tests/golden/poly_kat.json: known answers of the reference's poly() (src/abstract/fft.ts:583-926) over
bls12_381.fields.Fr and bn254.fields.Fr with generator 7n, data only, as decimal strings.  Run by hand where the reference bundle
(oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_poly_kat.py
The inputs are built here (seeded), a small driver of ours runs them through the reference's poly / FFT / rootsOfUnity once with and
once without the `fft` argument, and the answers come back as JSON."""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import refjs  # noqa: E402

ORDERS = {
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    "bn254": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
}
LENGTHS = (1, 2, 3, 4, 8, 16)

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { FFT, poly, rootsOfUnity } from './abstract/fft.mjs';
import { bls12_381 } from './bls12-381.mjs';
import { bn254 } from './bn254.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const Fr = job.field === 'bn254' ? bn254.fields.Fr : bls12_381.fields.Fr;
const roots = rootsOfUnity(Fr, 7n);
const fft = FFT(roots, Fr);
const P0 = poly(Fr, roots), P1 = poly(Fr, roots, undefined, fft);
const big = (v) => (Array.isArray(v) ? v.map(BigInt) : BigInt(v));
const str = (v) => (Array.isArray(v) ? v.map((x) => x.toString()) : typeof v === 'bigint' ? v.toString() : v);
const run = (P, c) => {
  switch (c.op) {
    case 'add': return P.add(big(c.a), big(c.b));
    case 'sub': return P.sub(big(c.a), big(c.b));
    case 'dot': return P.dot(big(c.a), big(c.b));
    case 'mul': return P.mul(big(c.a), big(c.b));
    case 'scale': return P.mul(big(c.a), big(c.x));
    case 'convolve': return P.convolve(big(c.a), big(c.b));
    case 'shift': return P.shift(big(c.a), big(c.x));
    case 'eval': return P.eval(big(c.a), big(c.b));
    case 'monomial_basis': return P.monomial.basis(big(c.x), c.n);
    case 'monomial_eval': return P.monomial.eval(big(c.a), big(c.x));
    case 'lagrange_basis': return P.lagrange.basis(big(c.x), c.n, c.brp);
    case 'lagrange_eval': return P.lagrange.eval(big(c.a), big(c.x), c.brp);
    case 'vanishing': return P.vanishing(big(c.a));
    case 'degree': return P.degree(big(c.a));
    case 'extend': return P.extend(big(c.a), c.n);
    case 'roots': return c.brp ? roots.brp(c.n) : roots.roots(c.n);
    case 'omega': return roots.omega(c.n);
  }
  throw new Error('unknown op ' + c.op);
};
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const out = job.cases.map((c) => {
  const r = { plain: str(run(P0, c)) };
  if (c.fft) r.fft = str(run(P1, c));
  return r;
});
const Pfix = poly(Fr, roots, undefined, undefined, 4);
const errors = {
  mismatched: msg(() => P0.add([1n, 2n], [1n])),
  fixed_length: msg(() => Pfix.add([1n], [1n])),
  fixed_length_shift: msg(() => Pfix.shift([1n, 2n], 3n)),
  lagrange_basis_length: msg(() => P0.lagrange.basis(2n, 3)),
  lagrange_eval_length: msg(() => P0.lagrange.eval([1n, 2n, 3n], 2n)),
  not_poly_bigint: msg(() => P0.add(5n, [1n])),
  not_poly_string: msg(() => P0.add('x', [1n])),
  not_poly_b: msg(() => P0.add([1n], 5n)),
  not_poly_shift: msg(() => P0.shift(7n, 3n)),
  fft_length: msg(() => P1.mul([1n, 2n, 3n], [1n, 2n, 3n])),
  out_of_range: msg(() => bn254.fields.Fr.fromBytes(new Uint8Array(32).fill(255))),
};
console.log(JSON.stringify({ out, errors }));
"""


def inputs(rng, r, n):
    """n values that include 0, 1, r - 1, r - 2 (as far as n allows) and seeded uniform ones"""
    special = [r - 1, 0, 1, r - 2]
    v = [rng.randrange(r) for _ in range(n)]
    for i, s in enumerate(special[:n]):
        v[(i * 5 + 1) % n if n > 4 else i] = s
    return v


def cases_for(name, r):
    rng = random.Random("poly-kat-" + name)
    omega = {}
    odd, p2 = r - 1, 0
    while odd % 2 == 0:
        odd //= 2
        p2 += 1
    w = pow(7, odd, r)
    for bits in range(p2, -1, -1):
        omega[bits] = w
        w = w * w % r
    cs = []

    def add(op, fft=False, **kw):
        c = {"op": op, "fft": fft}
        for k, v in kw.items():
            c[k] = [str(x) for x in v] if isinstance(v, list) else (str(v) if k in ("x",) else v)
        cs.append(c)

    for bits in range(5):
        add("omega", n=bits)
        add("roots", n=bits, brp=False)
        add("roots", n=bits, brp=True)
    for n in LENGTHS:
        a, b = inputs(rng, r, n), inputs(rng, r, n)[::-1]
        pow2 = n & (n - 1) == 0
        for op in ("add", "sub", "dot", "eval"):
            add(op, a=a, b=b)
        add("add", a=[r - 1] * n, b=[r - 1] * n)
        add("dot", a=[r - 1] * n, b=[r - 1] * n)
        add("mul", fft=pow2, a=a, b=b)
        add("convolve", fft=True, a=a, b=b)
        add("convolve", fft=True, a=a, b=b[:max(1, n // 2)])
        for x in (0, 1, r - 1, rng.randrange(r)):
            add("scale", a=a, x=x)
            add("shift", a=a, x=x)
            add("monomial_eval", a=a, x=x)
            add("monomial_basis", x=x, n=n)
        add("vanishing", a=a)
        add("degree", a=a)
        add("degree", a=a[:-1] + [0])
        add("extend", a=a, n=n + 3)
        add("extend", a=a, n=max(0, n - 1))
        if pow2:
            bits = n.bit_length() - 1
            xs = [rng.randrange(r), 0] + sorted({pow(omega[bits], k, r) for k in (0, n // 2, n - 1)})
            for x in xs:
                for brp in (False, True):
                    add("lagrange_basis", x=x, n=n, brp=brp)
                    add("lagrange_eval", a=a, x=x, brp=brp)
    for n in (3, 5):   # the quadratic product of a length that is no power of two, on a second pair
        add("mul", a=inputs(rng, r, n), b=inputs(rng, r, n))
    add("mul", a=[1, 2, 3, r - 1], b=[5, 0, r - 2, 7], fft=True)
    add("convolve", a=[1, 2, 3], b=[4, 5], fft=True)
    add("vanishing", a=[1, 2, 3])
    return cs


def main():
    if not refjs.available():
        sys.exit("make_poly_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()     # the copy laid out like the reference's repository: it has bn254 beside bls12-381
    if not hooked:
        sys.exit("make_poly_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "poly_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    kat = {"generator": "7", "vectors": [], "fields": {}}
    index = {}

    def vec(v):
        """vectors are stored once: a case names its a, b and list-valued out by their index in "vectors" (out as {"v": index})"""
        key = tuple(v)
        if key not in index:
            index[key] = len(kat["vectors"])
            kat["vectors"].append(list(v))
        return index[key]

    for name, r in ORDERS.items():
        cs = cases_for(name, r)
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump({"field": name, "cases": cs}, f)
            job = f.name
        try:
            res = subprocess.run([refjs.node(), driver, job], capture_output=True, text=True, timeout=600)
        finally:
            os.unlink(job)
        if res.returncode != 0:
            sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
        got = json.loads(res.stdout.strip().splitlines()[-1])
        for c, o in zip(cs, got["out"]):
            if c["fft"]:
                assert o["fft"] == o["plain"], ("the reference's FFT and quadratic forms disagree", c)
            c["out"] = {"v": vec(o["plain"])} if isinstance(o["plain"], list) else o["plain"]
        for c in cs:
            for k in ("a", "b"):
                if k in c:
                    c[k] = vec(c[k])
        kat["fields"][name] = {"order": str(r), "cases": cs}
        if "errors" in kat:
            assert kat["errors"] == got["errors"], (kat["errors"], got["errors"])
        kat["errors"] = got["errors"]
    out = os.path.join(HERE, "poly_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, separators=(",", ":"))
    print("%d + %d cases -> %s (%d bytes)" % (len(kat["fields"]["bls12_381"]["cases"]), len(kat["fields"]["bn254"]["cases"]), out,
                                              os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))


main()
