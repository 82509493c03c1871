#!/usr/bin/env python3
"""Writes tests/golden/bn254_g1_eip196.json: the bn254 G1 ECADD / ECMUL known answers of the reference's vectors
(test/vectors/bn254/eth-dump.js NOBLE_DUMP_EC_ADD / NOBLE_DUMP_EC_MUL, and the add / mul cases of seda.js), data only.
EIP-196 pads short inputs with zeros and fails on points off the curve; only inputs on the curve or (0, 0) with a
result are kept (off-curve inputs are outside the engine's contract).  Coordinates and scalars as hex strings.
    python tests/golden/make_bn254_golden.py <reference test/vectors/bn254 directory>"""
import json
import os
import re
import sys

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def ok(x, y):
    return (x, y) == (0, 0) or (x < P and y < P and (y * y - x ** 3 - 3) % P == 0)


def words(hexstr, n):
    h = hexstr.ljust(64 * n, "0")[:64 * n]
    return [int(h[64 * i:64 * i + 64], 16) for i in range(n)]


def main(vdir):
    add, mul = [], []
    with open(os.path.join(vdir, "eth-dump.js")) as f:
        for line in f:
            m = re.match(r"NOBLE_DUMP_EC_(ADD|MUL) *([0-9a-f]*) 0x([0-9a-f]*)", line.strip())
            if not m or not m.group(3):
                continue
            kind, inp, out = m.groups()
            o = words(out, 2)
            if kind == "ADD":
                x1, y1, x2, y2 = words(inp, 4)
                if ok(x1, y1) and ok(x2, y2):
                    add.append({"a": [hex(x1), hex(y1)], "b": [hex(x2), hex(y2)], "out": [hex(o[0]), hex(o[1])], "src": "eth-dump"})
            else:
                x, y, k = words(inp, 3)
                if ok(x, y):
                    mul.append({"p": [hex(x), hex(y)], "k": hex(k), "out": [hex(o[0]), hex(o[1])], "src": "eth-dump"})
    with open(os.path.join(vdir, "seda.js")) as f:
        src = f.read()
    for kind in ("add", "mul"):
        body = src[src.index("%s: [" % kind):]
        body = body[:body.index("],")]
        for obj in re.findall(r"\{(.*?)\}", body, re.S):
            kv = dict(re.findall(r"(\w+):\s*'([0-9a-f]*)'", obj))
            o = words(kv["result"], 2)
            if kind == "add":
                a = [int(kv["x1"], 16), int(kv["y1"], 16)]
                b = [int(kv["x2"], 16), int(kv["y2"], 16)]
                if ok(*a) and ok(*b):
                    add.append({"a": [hex(v) for v in a], "b": [hex(v) for v in b], "out": [hex(o[0]), hex(o[1])], "src": "seda"})
            else:
                pt = [int(kv["x"], 16), int(kv["y"], 16)]
                if ok(*pt):
                    mul.append({"p": [hex(v) for v in pt], "k": hex(int(kv["scalar"], 16)), "out": [hex(o[0]), hex(o[1])], "src": "seda"})
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bn254_g1_eip196.json")
    with open(out, "w") as f:
        json.dump({"add": add, "mul": mul}, f, indent=0)
    print("add %d mul %d -> %s" % (len(add), len(mul), out))


main(sys.argv[1])
