#!/usr/bin/env python3
"""Writes tests/golden/decaf448_kat.json: known answers of the reference's decaf448.Point and decaf448_hasher (src/ed448.ts), data
only, as hex strings.  Run by hand where the reference bundle (oracle/_ref/refjs.bundle) and node exist, never by the tests:
    python tests/golden/make_decaf448_kat.py
The inputs are built here (seeded, plus the edge rows), a small driver of ours runs them through the reference once, and the answers -
or the message of the error the reference throws - come back as JSON.  The published vectors are asserted on the way and recorded:
RFC 9496 appendix A.2 (the multiples 0..15 of the generator, the invalid encodings, the hash-to-group vectors) and the RFC 9380
hash_to_decaf448 known answer."""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import refjs  # noqa: E402

P = 2**448 - 2**224 - 1
N = 2**446 - 13818066809895115352007386748515426880336692474882178609894547503885
D = P - 39081
# src/ed448.ts:451-457 (module-local there, so recorded here and checked against d below)
SQRT_MINUS_D = 98944233647732219769177004876929019128417576295529901074099889598043702116001257856802131563896515373927712232092845883226922417596214
RANGE = "invalid field element: outside of range 0..ORDER"      # Fp448.fromBytes (src/abstract/modular.ts) for s >= p
INVSQRT_MINUS_D = 315019913931389607337177038330951043522456072897266928557328499619017160722351061360252776265186336876723201881398623946864393857820716

DRIVER = r"""
import '../polyfill.mjs';
import fs from 'fs';
import { decaf448, decaf448_hasher, ed448 } from './ed448.mjs';
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const DP = decaf448.Point, EP = ed448.Point;
const hex = (b) => Buffer.from(b).toString('hex');
const bin = (h) => Uint8Array.from(Buffer.from(h, 'hex'));
const big = (h) => BigInt('0x' + h);
const msg = (f) => { try { f(); } catch (e) { return e.message; } return null; };
const run = (f) => { try { return { out: f(), error: null }; } catch (e) { return { out: null, error: e.message }; } };
const aff = (p) => { const a = p.toAffine(); return { x: a.x.toString(16), y: a.y.toString(16) }; };
const multiples = job.multiples.map((k) => { const p = DP.BASE.multiplyUnsafe(big(k)); return Object.assign({ enc: hex(p.toBytes()) }, aff(p)); });
const walk = [];
for (let i = 0, p = DP.ZERO; i < 16; i++, p = p.add(DP.BASE)) walk.push(hex(p.toBytes()));
const decode = job.decode.map((e) => {
  try { const p = DP.fromBytes(bin(e)); if (hex(p.toBytes()) !== e) throw new Error('decode then encode differs'); return Object.assign({ error: null }, aff(p)); }
  catch (err) { return { x: null, y: null, error: err.message }; }
});
const mul = job.mul.map((c) => ({
  multiply: run(() => hex(DP.fromBytes(bin(c.enc)).multiply(big(c.k)).toBytes())),
  multiplyUnsafe: run(() => hex(DP.fromBytes(bin(c.enc)).multiplyUnsafe(big(c.k)).toBytes())),
}));
const add = job.add.map((c) => {
  const a = DP.fromBytes(bin(c.a)), b = DP.fromBytes(bin(c.b));
  return { add: hex(a.add(b).toBytes()), subtract: hex(a.subtract(b).toBytes()), negate: hex(a.negate().toBytes()), double: hex(a.double().toBytes()) };
});
const equals = job.equals.map((c) => DP.fromAffine({ x: big(c.x1), y: big(c.y1) }).equals(DP.fromAffine({ x: big(c.x2), y: big(c.y2) })));
const encode_affine = job.encode_affine.map((c) => hex(DP.fromAffine({ x: big(c.x), y: big(c.y) }).toBytes()));
const encode_ext = job.encode_ext.map((c) => hex(new DP(new EP(big(c.X), big(c.Y), big(c.Z), big(c.T))).toBytes()));
const derive = job.derive.map((h) => hex(decaf448_hasher.deriveToCurve(bin(h)).toBytes()));
const opts = (c) => (c.dst === null ? undefined : { DST: c.dst_is_text ? Buffer.from(c.dst, 'hex').toString('latin1') : bin(c.dst) });
const hash = job.hash.map((c) => ({
  curve: hex(decaf448_hasher.hashToCurve(bin(c.msg), opts(c)).toBytes()),
  scalar: decaf448_hasher.hashToScalar(bin(c.msg), opts(c)).toString(16),
}));
const errors = {
  length: msg(() => DP.fromBytes(new Uint8Array(55))),
  length_57: msg(() => DP.fromBytes(new Uint8Array(57))),
  type: msg(() => DP.fromBytes('00')),
  derive_length: msg(() => decaf448_hasher.deriveToCurve(new Uint8Array(111))),
  equals_other: msg(() => DP.BASE.equals(EP.BASE)),
  add_other: msg(() => DP.BASE.add(EP.BASE)),
  multiply_zero: msg(() => DP.BASE.multiply(0n)),
  multiply_n: msg(() => DP.BASE.multiply(DP.Fn.ORDER)),
  multiply_unsafe_n: msg(() => DP.BASE.multiplyUnsafe(DP.Fn.ORDER)),
  multiply_unsafe_negative: msg(() => DP.BASE.multiplyUnsafe(-1n)),
  empty_dst: msg(() => decaf448_hasher.hashToCurve(new Uint8Array(1), { DST: '' })),
  empty_dst_scalar: msg(() => decaf448_hasher.hashToScalar(new Uint8Array(1), { DST: new Uint8Array(0) })),
  from_hex_odd: msg(() => DP.fromHex('0')),
};
console.log(JSON.stringify({ multiples, walk, decode, mul, add, equals, encode_affine, encode_ext, derive, hash, errors,
  base: aff(DP.BASE), zero: aff(DP.ZERO), ed_base: aff(EP.BASE), order: DP.Fn.ORDER.toString(16) }));
"""

# RFC 9496 appendix A.2, as the reference's test data quotes it
RFC_MULTIPLES = [
    "00" * 56,
    "6666666666666666666666666666666666666666666666666666666633333333333333333333333333333333333333333333333333333333",
    "c898eb4f87f97c564c6fd61fc7e49689314a1f818ec85eeb3bd5514ac816d38778f69ef347a89fca817e66defdedce178c7cc709b2116e75",
    "a0c09bf2ba7208fda0f4bfe3d0f5b29a543012306d43831b5adc6fe7f8596fa308763db15468323b11cf6e4aeb8c18fe44678f44545a69bc",
    "b46f1836aa287c0a5a5653f0ec5ef9e903f436e21c1570c29ad9e5f596da97eeaf17150ae30bcb3174d04bc2d712c8c7789d7cb4fda138f4",
    "1c5bbecf4741dfaae79db72dface00eaaac502c2060934b6eaaeca6a20bd3da9e0be8777f7d02033d1b15884232281a41fc7f80eed04af5e",
    "86ff0182d40f7f9edb7862515821bd67bfd6165a3c44de95d7df79b8779ccf6460e3c68b70c16aaa280f2d7b3f22d745b97a89906cfc476c",
    "502bcb6842eb06f0e49032bae87c554c031d6d4d2d7694efbf9c468d48220c50f8ca28843364d70cee92d6fe246e61448f9db9808b3b2408",
    "0c9810f1e2ebd389caa789374d78007974ef4d17227316f40e578b336827da3f6b482a4794eb6a3975b971b5e1388f52e91ea2f1bcb0f912",
    "20d41d85a18d5657a29640321563bbd04c2ffbd0a37a7ba43a4f7d263ce26faf4e1f74f9f4b590c69229ae571fe37fa639b5b8eb48bd9a55",
    "e6b4b8f408c7010d0601e7eda0c309a1a42720d6d06b5759fdc4e1efe22d076d6c44d42f508d67be462914d28b8edce32e7094305164af17",
    "be88bbb86c59c13d8e9d09ab98105f69c2d1dd134dbcd3b0863658f53159db64c0e139d180f3c89b8296d0ae324419c06fa87fc7daaf34c1",
    "a456f9369769e8f08902124a0314c7a06537a06e32411f4f93415950a17badfa7442b6217434a3a05ef45be5f10bd7b2ef8ea00c431edec5",
    "186e452c4466aa4383b4c00210d52e7922dbf9771e8b47e229a9b7b73c8d10fd7ef0b6e41530f91f24a3ed9ab71fa38b98b2fe4746d51d68",
    "4ae7fdcae9453f195a8ead5cbe1a7b9699673b52c40ab27927464887be53237f7f3a21b938d40d0ec9e15b1d5130b13ffed81373a53e2b43",
    "841981c3bfeec3f60cfeca75d9d8dc17f46cf0106f2422b59aec580a58f342272e3a5e575a055ddb051390c54c24c6ecb1e0aceb075f6056",
]
RFC_INVALID = [
    # non-canonical field encodings
    "8e24f838059ee9fef1e209126defe53dcd74ef9b6304601c6966099effffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "86fcc7212bd4a0b980928666dc28c444a605ef38e09fb569e28d4443ffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "866d54bd4c4ff41a55d4eefdbeca73cbd653c7bd3135b383708ec0bdffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "4a380ccdab9c86364a89e77a464d64f9157538cfdfa686adc0d5ece4ffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "f22d9d4c945dd44d11e0b1d3d3d358d959b4844d83b08c44e659d79fffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "8cdffc681aa99e9c818c8ef4c3808b58e86acdef1ab68c8477af185bffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "0e1c12ac7b5920effbd044e897c57634e2d05b5c27f8fa3df8a086a1ffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    # negative field elements
    "15141bd2121837ef71a0016bd11be757507221c26542244f23806f3fd3496b7d4c36826276f3bf5deea2c60c4fa4cec69946876da497e795",
    "455d380238434ab740a56267f4f46b7d2eb2dd8ee905e51d7b0ae8a6cb2bae501e67df34ab21fa45946068c9f233939b1d9521a998b7cb93",
    "810b1d8e8bf3a9c023294bbfd3d905a97531709bdc0f42390feedd7010f77e98686d400c9c86ed250ceecd9de0a18888ffecda0f4ea1c60d",
    "d3af9cc41be0e5de83c0c6273bedcb9351970110044a9a41c7b9b2267cdb9d7bf4dc9c2fdb8bed32878184604f1d9944305a8df4274ce301",
    "9312bcab09009e4330ff89c4bc1e9e000d863efc3c863d3b6c507a40fd2cdefde1bf0892b4b5ed9780b91ed1398fb4a7344c605aa5efda74",
    "53d11bce9e62a29d63ed82ae93761bdd76e38c21e2822d6ebee5eb1c5b8a03eaf9df749e2490eda9d8ac27d1f71150de93668074d18d1c3a",
    "697c1aed3cd8858515d4be8ac158b229fe184d79cb2b06e49210a6f3a7cd537bcd9bd390d96c4ab6a4406da5d93640726285370cfa95df80",
    # a non-square ratio
    "58ad48715c9a102569b68b88362a4b0645781f5a19eb7e59c6a4686fd0f0750ff42e3d7af1ab38c29d69b670f31258919c9fdbf6093d06c0",
    "8ca37ee2b15693f06e910cf43c4e32f1d5551dda8b1e48cb6ddd55e440dbc7b296b601919a4e4069f59239ca247ff693f7daa42f086122b1",
    "982c0ec7f43d9f97c0a74b36db0abd9ca6bfb98123a90782787242c8a523cdc76df14a910d54471127e7662a1059201f902940cd39d57af5",
    "baa9ab82d07ca282b968a911a6c3728d74bf2fe258901925787f03ee4be7e3cb6684fd1bcfe5071a9a974ad249a4aaa8ca81264216c68574",
    "2ed9ffe2ded67a372b181ac524996402c42970629db03f5e8636cbaf6074b523d154a7a8c4472c4c353ab88cd6fec7da7780834cc5bd5242",
    "f063769e4241e76d815800e4933a3a144327a30ec40758ad3723a788388399f7b3f5d45b6351eb8eddefda7d5bff4ee920d338a8b89d8b63",
    "5a0104f1f55d152ceb68bc138182499891d90ee8f09b40038ccc1e07cb621fd462f781d045732a4f0bda73f0b2acf94355424ff0388d4b9c",
]
RFC_HASH_IN = [
    "cbb8c991fd2f0b7e1913462d6463e4fd2ce4ccdd28274dc2ca1f4165d5ee6cdccea57be3416e166fd06718a31af45a2f8e987e301be59ae6673e963001dbbda80df47014a21a26d6c7eb4ebe0312aa6fffb8d1b26bc62ca40ed51f8057a635a02c2b8c83f48fa6a2d70f58a1185902c0",
    "b6d8da654b13c3101d6634a231569e6b85961c3f4b460a08ac4a5857069576b64428676584baa45b97701be6d0b0ba18ac28d443403b45699ea0fbd1164f5893d39ad8f29e48e399aec5902508ea95e33bc1e9e4620489d684eb5c26bc1ad1e09aba61fabc2cdfee0b6b6862ffc8e55a",
    "36a69976c3e5d74e4904776993cbac27d10f25f5626dd45c51d15dcf7b3e6a5446a6649ec912a56895d6baa9dc395ce9e34b868d9fb2c1fc72eb6495702ea4f446c9b7a188a4e0826b1506b0747a6709f37988ff1aeb5e3788d5076ccbb01a4bc6623c92ff147a1e21b29cc3fdd0e0f4",
    "d5938acbba432ecd5617c555a6a777734494f176259bff9dab844c81aadcf8f7abd1a9001d89c7008c1957272c1786a4293bb0ee7cb37cf3988e2513b14e1b75249a5343643d3c5e5545a0c1a2a4d3c685927c38bc5e5879d68745464e2589e000b31301f1dfb7471a4f1300d6fd0f99",
    "4dec58199a35f531a5f0a9f71a53376d7b4bdd6bbd2904234a8ea65bbacbce2a542291378157a8f4be7b6a092672a34d85e473b26ccfbd4cdc6739783dc3f4f6ee3537b7aed81df898c7ea0ae89a15b5559596c2a5eeacf8b2b362f3db2940e3798b63203cae77c4683ebaed71533e51",
    "df2aa1536abb4acab26efa538ce07fd7bca921b13e17bc5ebcba7d1b6b733deda1d04c220f6b5ab35c61b6bcb15808251cab909a01465b8ae3fc770850c66246d5a9eae9e2877e0826e2b8dc1bc08009590bc6778a84e919fbd28e02a0f9c49b48dc689eb5d5d922dc01469968ee81b5",
    "e9fb440282e07145f1f7f5ecf3c273212cd3d26b836b41b02f108431488e5e84bd15f2418b3d92a3380dd66a374645c2a995976a015632d36a6c2189f202fc766e1c82f50ad9189be190a1f0e8f9b9e69c9c18cc98fdd885608f68bf0fdedd7b894081a63f70016a8abf04953affbefa",
]
RFC_HASH_OUT = [
    "0c709c9607dbb01c94513358745b7c23953d03b33e39c7234e268d1d6e24f34014ccbc2216b965dd231d5327e591dc3c0e8844ccfd568848",
    "76ab794e28ff1224c727fa1016bf7f1d329260b7218a39aea2fdb17d8bd9119017b093d641cedf74328c327184dc6f2a64bd90eddccfcdab",
    "c8d7ac384143500e50890a1c25d643343accce584caf2544f9249b2bf4a6921082be0e7f3669bb5ec24535e6c45621e1f6dec676edd8b664",
    "62beffc6b8ee11ccd79dbaac8f0252c750eb052b192f41eeecb12f2979713b563caf7d22588eca5e80995241ef963e7ad7cb7962f343a973",
    "f4ccb31d263731ab88bed634304956d2603174c66da38742053fa37dd902346c3862155d68db63be87439e3d68758ad7268e239d39c4fd3b",
    "7e79b00e8e0a76a67c0040f62713b8b8c6d6f05e9c6d02592e8a22ea896f5deacc7c7df5ed42beae6fedb9000285b482aa504e279fd49c32",
    "20b171cb16be977f15e013b9752cf86c54c631c4fc8cbf7c03c4d3ac9b8e8640e7b0e9300b987fe0ab5044669314f6ed1650ae037db853f1",
]
# RFC 9380 hash_to_decaf448 (appendix B.2's construction) of ten bytes 0x05 under the default DST, as the reference's tests quote it
RFC9380_MSG = "05" * 10
RFC9380_OUT = "1287dea7519af966cf537a58f614e8b39b93a7c0b989bcdb4f94af8f2573ab59589accb0d2a2097b5f30c1d721619470f21e78613bbfc4b6"


def le(v, n=56):
    return int(v).to_bytes(n, "little").hex()


def hx(v):
    return "%x" % v


def ed_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + t, P - 2, P) % P, (y1 * y2 - x1 * x2) * pow(1 - t, P - 2, P) % P)


def is_square(v):
    v %= P
    return v == 0 or pow(v, (P - 1) // 2, P) == 1


def decodes(s):
    """whether an even canonical s is an encoding: u2 u1^2 a square"""
    u1 = (1 + s * s) % P
    return is_square((u1 * u1 - 4 * D * s * s) * u1 * u1)


def main():
    if not refjs.available():
        sys.exit("make_decaf448_kat: the reference bundle or node is missing")
    refjs.ref_dir()
    hooked = refjs.hooked_dir()
    if not hooked:
        sys.exit("make_decaf448_kat: the bundle has no js_hooked/ copy")
    driver = os.path.join(hooked, "src", "decaf448_kat_driver.mjs")
    with open(driver, "w") as f:
        f.write(DRIVER)
    assert SQRT_MINUS_D ** 2 % P == 39081 and SQRT_MINUS_D % 2 == 0 and SQRT_MINUS_D * INVSQRT_MINUS_D % P == 1
    rng = random.Random("decaf448-kat")
    rb = lambda n=56: bytes(rng.randrange(256) for _ in range(n)).hex()  # noqa: E731
    ks = list(range(16)) + [N - 1, N - 2, 2**445] + [rng.randrange(N) for _ in range(8)]
    multiples = [hx(k) for k in ks]
    # encodings to refuse: s = p, p + 1, 2^448 - 1 (not canonical), odd s, even canonical s with a non-square ratio; and to accept
    bad_even = [s for s in range(2, 400, 2) if not decodes(s)][:4]
    good_even = [s for s in range(2, 400, 2) if decodes(s)][:4]
    edge_decode = [le(P), le(P + 1), le(2**448 - 1), le(1), le(P - 2), le(3)] + [le(s) for s in bad_even] + [le(P - 1)] + [le(s) for s in good_even]
    decode = RFC_MULTIPLES + RFC_INVALID + edge_decode
    derive = list(RFC_HASH_IN)
    halves = (0, 1, P - 1, P, P + 1, 2**448 - 1)
    for a in halves:
        derive.append(le(a) + rb())
        derive.append(rb() + le(a))
        derive.append(le(a) + le(a))                       # equal halves: the doubling through the complete addition
    derive.append(le(0) + le(1))
    derive.append(le(P) + le(0))
    eq_half = rb()
    derive.append(eq_half + eq_half)
    derive += [rb(112) for _ in range(8)]
    hash_rows = [{"msg": RFC9380_MSG, "dst": None, "dst_is_text": False}]
    for i, m in enumerate(("", "00", rb(7), rb(200))):
        hash_rows.append({"msg": m, "dst": None, "dst_is_text": False})
        hash_rows.append({"msg": m, "dst": b"QUUX-V01-CS02-with-decaf448".hex(), "dst_is_text": i % 2 == 0})
        hash_rows.append({"msg": m, "dst": (b"oversize-%d-" % i + b"x" * (250 + i * 3)).hex(), "dst_is_text": i % 2 == 1})
    hash_rows.append({"msg": rb(5), "dst": (b"d" * 255).hex(), "dst_is_text": True})     # the longest DST taken as it is
    hash_rows.append({"msg": rb(5), "dst": (b"d" * 256).hex(), "dst_is_text": True})     # the shortest oversize one
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"multiples": multiples, "decode": decode, "mul": [], "add": [], "equals": [], "encode_affine": [], "encode_ext": [],
                   "derive": [], "hash": []}, f)
        job1 = f.name
    # first pass: the multiples, whose encodings and affine representatives the other rows are built from
    try:
        res = subprocess.run([refjs.node(), driver, job1], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(job1)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    first = json.loads(res.stdout.strip().splitlines()[-1])
    pts = [(int(m["x"], 16), int(m["y"], 16)) for m in first["multiples"]]
    encs = [m["enc"] for m in first["multiples"]]
    mul = []
    for i, k in enumerate((0, 1, 2, N - 1, N, 2**445) + tuple(rng.randrange(N) for _ in range(10))):
        mul.append({"enc": encs[1 + (5 * i) % (len(encs) - 1)], "k": hx(k)})
    mul.append({"enc": encs[0], "k": hx(7)})                                             # the identity
    mul.append({"enc": RFC_INVALID[0], "k": hx(7)})                                      # refused before the scalar is looked at
    add = [{"a": encs[i], "b": encs[j]} for i, j in ((1, 2), (2, 1), (5, 5), (0, 3), (3, 0), (16, 1), (20, 25), (7, 16 + 3))]
    torsion = [(0, 1), (0, P - 1), (1, 0), (P - 1, 0)]
    equals = []
    for i in (1, 17):
        for t in torsion:
            q = ed_add(pts[i], t)
            equals.append({"x1": hx(pts[i][0]), "y1": hx(pts[i][1]), "x2": hx(q[0]), "y2": hx(q[1])})
        equals.append({"x1": hx(pts[i][0]), "y1": hx(pts[i][1]), "x2": hx(pts[i + 1][0]), "y2": hx(pts[i + 1][1])})
    equals.append({"x1": hx(0), "y1": hx(1), "x2": hx(0), "y2": hx(P - 1)})
    equals.append({"x1": hx(0), "y1": hx(1), "x2": hx(1), "y2": hx(0)})
    ed_base = (int(first["ed_base"]["x"], 16), int(first["ed_base"]["y"], 16))
    encode_affine = [{"x": hx(x), "y": hx(y)} for x, y in torsion]                       # the four small-order Ed448 points
    encode_affine.append({"x": hx(ed_base[0]), "y": hx(ed_base[1])})                     # a point outside 2 E
    for i in (2, 18):
        for t in torsion:                                                                # the coset: (0, -1) keeps the bytes
            q = ed_add(pts[i], t)
            encode_affine.append({"x": hx(q[0]), "y": hx(q[1])})
    encode_ext = []
    for i in (3, 19, 0):
        x, y = pts[i]
        for z in (1, 2, P - 1, rng.randrange(1, P)):
            encode_ext.append({"X": hx(x * z % P), "Y": hx(y * z % P), "Z": hx(z), "T": hx(x * y * z % P)})
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"multiples": multiples, "decode": decode, "mul": mul, "add": add, "equals": equals, "encode_affine": encode_affine,
                   "encode_ext": encode_ext, "derive": derive, "hash": hash_rows}, f)
        job = f.name
    try:
        res = subprocess.run([refjs.node(), driver, job], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(job)
    if res.returncode != 0:
        sys.exit("reference run failed: " + (res.stderr or res.stdout)[-2000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    # ---- the published vectors
    assert got["walk"] == RFC_MULTIPLES and encs[:16] == RFC_MULTIPLES
    nd = len(RFC_MULTIPLES)
    assert all(o["error"] is None for o in got["decode"][:nd])        # and the driver checked decode -> encode
    inv = got["decode"][nd:nd + len(RFC_INVALID)]
    # a non-canonical s never reaches 'encoding 1': Fp.fromBytes refuses it first, with its own message
    assert [o["error"] for o in inv] == [RANGE] * 7 + ["invalid decaf448 encoding 1"] * 7 + ["invalid decaf448 encoding 2"] * 7
    assert got["derive"][:len(RFC_HASH_IN)] == RFC_HASH_OUT
    assert got["hash"][0]["curve"] == RFC9380_OUT
    assert int(got["order"], 16) == N
    ed2 = ed_add(ed_base, ed_base)
    assert (int(got["base"]["x"], 16), int(got["base"]["y"], 16)) == ed2 == pts[1]      # BASE is twice the Ed448 base
    edge = got["decode"][nd + len(RFC_INVALID):]
    assert [o["error"] for o in edge[:6]] == [RANGE] * 3 + ["invalid decaf448 encoding 1"] * 3
    assert [o["error"] for o in edge[6:10]] == ["invalid decaf448 encoding 2"] * 4 and all(o["error"] is None for o in edge[11:])
    names = (["rfc9496 multiple %d" % i for i in range(16)] + ["rfc9496 invalid %d" % i for i in range(len(RFC_INVALID))]
             + ["s = p", "s = p + 1", "s = 2^448 - 1", "s = 1", "s = p - 2", "s = 3"] + ["s = %d: non-square" % s for s in bad_even]
             + ["s = p - 1"] + ["s = %d" % s for s in good_even])
    kat = {
        "consts": {"sqrt_minus_d": str(SQRT_MINUS_D), "invsqrt_minus_d": str(INVSQRT_MINUS_D), "one_minus_d": "39082",
                   "one_minus_two_d": "78163"},
        "base": got["base"], "zero": got["zero"], "ed_base": got["ed_base"],
        "errors": got["errors"],
        "multiples": [dict(k=k, **o) for k, o in zip(multiples, got["multiples"])],
        "decode": [dict(name=n, enc=e, **o) for n, e, o in zip(names, decode, got["decode"])],
        "mul": [dict(c, **o) for c, o in zip(mul, got["mul"])],
        "add": [dict(c, **o) for c, o in zip(add, got["add"])],
        "equals": [dict(c, equal=o) for c, o in zip(equals, got["equals"])],
        "encode_affine": [dict(c, enc=o) for c, o in zip(encode_affine, got["encode_affine"])],
        "encode_ext": [dict(c, enc=o) for c, o in zip(encode_ext, got["encode_ext"])],
        "derive": [{"uniform": u, "enc": o} for u, o in zip(derive, got["derive"])],
        "hash": [dict(c, **o) for c, o in zip(hash_rows, got["hash"])],
    }
    out = os.path.join(HERE, "decaf448_kat.json")
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in kat.items()) + "\n}\n")
    print("%d multiples, %d decode rows (%d rejected), %d mul, %d add, %d equals, %d + %d encode, %d derive, %d hash rows -> %s (%d bytes)"
          % (len(multiples), len(decode), sum(o["error"] is not None for o in got["decode"]), len(mul), len(add), len(equals),
             len(encode_affine), len(encode_ext), len(derive), len(hash_rows), out, os.path.getsize(out)))
    print(json.dumps(kat["errors"], indent=1))
    print([o for o in got["equals"]])


main()
