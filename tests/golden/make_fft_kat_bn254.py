#!/usr/bin/env python3
"""Writes tests/golden/fft_kat_bn254.json: the `bn254 roots` and `bn254 brp` known answers of the reference's
test/fft.test.ts ('cache and fixed vectors': rootsOfUnity(bn254.fields.Fr, 7n).roots(3) / .brp(3)), data only, as decimal
strings in the manner of fft_kat.json.
    python tests/golden/make_fft_kat_bn254.py <reference test/fft.test.ts>"""
import json
import os
import re
import sys


def array_before(src, label):
    """the bigint literals of the array that the assertion labelled `label` compares against"""
    end = src.index("'%s'" % label)
    start = src.rindex("[", 0, end)
    return re.findall(r"(\d+)n", src[start:end])


def main(path):
    with open(path) as f:
        src = f.read()
    roots, brp = array_before(src, "bn254 roots"), array_before(src, "bn254 brp")
    assert len(roots) == 8 and len(brp) == 8 and roots[0] == "1" and sorted(roots) == sorted(brp)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fft_kat_bn254.json")
    with open(out, "w") as f:
        json.dump({"generator": "7", "roots3": roots, "brp3": brp}, f, indent=0)
    print("roots3 %d brp3 %d -> %s" % (len(roots), len(brp), out))


main(sys.argv[1])
