"""Shared by the bls12-381 pairing tests: a plain-integer restatement of the reference's Fp2 / Fp6 / Fp12 tower
(src/abstract/tower.ts:393-1092), Miller loop (src/abstract/bls.ts:476-666) and final exponentiation
(src/bls12-381.ts:160-276) - checked bit for bit against the fixture tests/golden/bls12_381_pairing_kat.json and then the
oracle for random batches - the wire codecs of include/ncg.h (GT = 12 coefficients of 48 LE bytes in tower order), the
seeded inputs of the fixture and the ctypes side of the ht_fp12_op / ht_pairing host twins (csrc/hosttest.hip).
Fp2 = (c0, c1), Fp6 = (c0, c1, c2) of Fp2, Fp12 = (c0, c1) of Fp6."""
import base64
import ctypes
import hashlib
import json
import os

import numpy as np

import hosttest

HERE = os.path.dirname(os.path.abspath(__file__))
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BLS_X = 0xD201000000010000
G1 = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
      0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
G2 = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
       0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
      (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
       0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))
ZERO_MSG = "pairing is not available for ZERO point"
# ncg_fp12_batch ops
OP_MUL, OP_SQR, OP_INV, OP_CONJ, OP_FROB1, OP_FROB2, OP_FROB3, OP_CYC_SQR, OP_MUL014, OP_FINAL_EXP, OP_IS_ONE = range(11)
BAD_ZERO, BAD_G1, BAD_G1_SUBGROUP, BAD_G2, BAD_G2_SUBGROUP = 1, 2, 3, 4, 5
CHECK_SUBGROUP = 1                  # NCG_PAIRING_CHECK_SUBGROUP

# ---------------------------------------------------------------- Fp2 (tower.ts:393-561)
F2_ZERO, F2_ONE = (0, 0), (1, 0)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    if isinstance(b, int):
        return (a[0] * b % P, a[1] * b % P)
    t0, t1 = a[0] * b[0] % P, a[1] * b[1] % P
    return ((t0 - t1) % P, ((a[0] + a[1]) * (b[0] + b[1]) - (t0 + t1)) % P)


def f2_sqr(a):
    return ((a[0] + a[1]) * (a[0] - a[1]) % P, 2 * a[0] * a[1] % P)


def f2_inv(a):
    """tower.ts:458-475; the inverse of 0 is 0 here as on the device (a^(p-2)), where the reference throws"""
    f = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (f * a[0] % P, f * -a[1] % P)


def f2_mul_nr(a):                                            # (u + 1) a
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_frob(a, power):
    return f2_conj(a) if power % 2 else a


def f2_pow(a, e):
    r = F2_ONE
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_sqr(a)
        e >>= 1
    return r


def f2_mul_by_b(a):                                          # bls12-381.ts:252-257
    t0, t1 = a[0] * 4 % P, a[1] * 4 % P
    return ((t0 - t1) % P, (t0 + t1) % P)


def f2_fp4_square(a, b):                                     # tower.ts:533-541
    a2, b2 = f2_sqr(a), f2_sqr(b)
    return f2_add(f2_mul_nr(b2), a2), f2_sub(f2_sub(f2_sqr(f2_add(a, b)), a2), b2)


# ---------------------------------------------------------------- Fp6 (tower.ts:563-816)
F6_ZERO, F6_ONE = (F2_ZERO, F2_ZERO, F2_ZERO), (F2_ONE, F2_ZERO, F2_ZERO)


def frobenius_coefficients(mul, div, rows=12):
    """calcFrobeniusCoefficients (tower.ts:136-179): (u + 1)^((mul p^k - mul) / div) for k = 0 .. rows - 1"""
    return [f2_pow((1, 1), (mul * P ** k - mul) // div) for k in range(rows)]


FROB6_C1 = frobenius_coefficients(1, 3, 6)
FROB6_C2 = frobenius_coefficients(2, 3, 6)
FROB12 = frobenius_coefficients(1, 6, 12)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul(a, b):
    c0, c1, c2 = a
    r0, r1, r2 = b
    t0, t1, t2 = f2_mul(c0, r0), f2_mul(c1, r1), f2_mul(c2, r2)
    return (f2_add(t0, f2_mul_nr(f2_sub(f2_mul(f2_add(c1, c2), f2_add(r1, r2)), f2_add(t1, t2)))),
            f2_add(f2_sub(f2_mul(f2_add(c0, c1), f2_add(r0, r1)), f2_add(t0, t1)), f2_mul_nr(t2)),
            f2_sub(f2_add(t1, f2_mul(f2_add(c0, c2), f2_add(r0, r2))), f2_add(t0, t2)))


def f6_sqr(a):
    c0, c1, c2 = a
    t0, t1, t3, t4 = f2_sqr(c0), f2_mul(f2_mul(c0, c1), 2), f2_mul(f2_mul(c1, c2), 2), f2_sqr(c2)
    return (f2_add(f2_mul_nr(t3), t0), f2_add(f2_mul_nr(t4), t1),
            f2_sub(f2_sub(f2_add(f2_add(t1, f2_sqr(f2_add(f2_sub(c0, c1), c2))), t3), t0), t4))


def f6_mul_nr(a):
    return (f2_mul_nr(a[2]), a[0], a[1])


def f6_inv(a):
    c0, c1, c2 = a
    t0 = f2_sub(f2_sqr(c0), f2_mul_nr(f2_mul(c2, c1)))
    t1 = f2_sub(f2_mul_nr(f2_sqr(c2)), f2_mul(c0, c1))
    t2 = f2_sub(f2_sqr(c1), f2_mul(c0, c2))
    t4 = f2_inv(f2_add(f2_mul_nr(f2_add(f2_mul(c2, t1), f2_mul(c1, t2))), f2_mul(c0, t0)))
    return (f2_mul(t4, t0), f2_mul(t4, t1), f2_mul(t4, t2))


def f6_frob(a, power):
    if power % 6 == 0:
        return a
    return (f2_frob(a[0], power), f2_mul(f2_frob(a[1], power), FROB6_C1[power % 6]),
            f2_mul(f2_frob(a[2], power), FROB6_C2[power % 6]))


# ---------------------------------------------------------------- Fp12 (tower.ts:822-1092)
F12_ONE = (F6_ONE, F6_ZERO)


def f12_mul(a, b):
    t1, t2 = f6_mul(a[0], b[0]), f6_mul(a[1], b[1])
    return (f6_add(t1, f6_mul_nr(t2)), f6_sub(f6_mul(f6_add(a[0], a[1]), f6_add(b[0], b[1])), f6_add(t1, t2)))


def f12_sqr(a):
    ab = f6_mul(a[0], a[1])
    return (f6_sub(f6_sub(f6_mul(f6_add(f6_mul_nr(a[1]), a[0]), f6_add(a[0], a[1])), ab), f6_mul_nr(ab)), f6_add(ab, ab))


def f12_conj(a):
    return (a[0], f6_neg(a[1]))


def f12_inv(a):
    t = f6_inv(f6_sub(f6_sqr(a[0]), f6_mul_nr(f6_sqr(a[1]))))
    return (f6_mul(a[0], t), f6_neg(f6_mul(a[1], t)))


def f12_frob(a, power):
    p = power % 12
    if p == 0:
        return a
    if p == 6:
        return f12_conj(a)
    c = f6_frob(a[1], power)
    k = FROB12[p]
    return (f6_frob(a[0], power), tuple(f2_mul(x, k) for x in c))


def f12_cyclotomic_sqr(a):                                   # tower.ts:1058-1079
    (c0c0, c0c1, c0c2), (c1c0, c1c1, c1c2) = a
    t3, t4 = f2_fp4_square(c0c0, c1c1)
    t5, t6 = f2_fp4_square(c1c0, c0c2)
    t7, t8 = f2_fp4_square(c0c1, c1c2)
    t9 = f2_mul_nr(t8)
    k = lambda t, c, op: f2_add(f2_mul(op(t, c), 2), t)      # noqa: E731
    return ((k(t3, c0c0, f2_sub), k(t5, c0c1, f2_sub), k(t7, c0c2, f2_sub)),
            (k(t9, c1c0, f2_add), k(t4, c1c1, f2_add), k(t6, c1c2, f2_add)))


def f12_pow(a, e):
    r = F12_ONE
    while e:
        if e & 1:
            r = f12_mul(r, a)
        a = f12_sqr(a)
        e >>= 1
    return r


def f12_mul014(f, o0, o1, o4):                               # bls.ts:476-519 with o1, o4 already scaled
    (a0, a1, a2), (b0, b1, b2) = f
    t0_0, t0_1 = f2_mul(a0, o0), f2_mul(a1, o1)
    t0 = (f2_add(f2_mul_nr(f2_sub(f2_mul(f2_add(a1, a2), o1), t0_1)), t0_0),
          f2_sub(f2_sub(f2_mul(f2_add(o0, o1), f2_add(a0, a1)), t0_0), t0_1),
          f2_add(f2_sub(f2_mul(f2_add(a0, a2), o0), t0_0), t0_1))
    t1 = (f2_mul_nr(f2_mul(b2, o4)), f2_mul(b0, o4), f2_mul(b1, o4))
    s0, s1, s2, o14 = f2_add(a0, b0), f2_add(a1, b1), f2_add(a2, b2), f2_add(o1, o4)
    t2_0, t2_1 = f2_mul(s0, o0), f2_mul(s1, o14)
    t2 = (f2_add(f2_mul_nr(f2_sub(f2_mul(f2_add(s1, s2), o14), t2_1)), t2_0),
          f2_sub(f2_sub(f2_mul(f2_add(o0, o14), f2_add(s0, s1)), t2_0), t2_1),
          f2_add(f2_sub(f2_mul(f2_add(s0, s2), o0), t2_0), t2_1))
    return ((f2_add(f2_mul_nr(t1[2]), t0[0]), f2_add(t1[0], t0[1]), f2_add(t1[1], t0[2])),
            tuple(f2_sub(f2_sub(t2[i], t0[i]), t1[i]) for i in range(3)))


def cyclotomic_exp_x(a):
    """bls12CyclotomicExpX (bls12-381.ts:231-242): a^|x|.  The reference squares in compressed form; the element is the same."""
    z = a
    for bit in range(BLS_X.bit_length() - 2, -1, -1):
        z = f12_cyclotomic_sqr(z)
        if (BLS_X >> bit) & 1:
            z = f12_mul(z, a)
    return z


def final_exponentiate(num):                                 # bls12-381.ts:258-276
    pmx = lambda v: f12_conj(cyclotomic_exp_x(v))             # noqa: E731
    t0 = f12_mul(f12_frob(num, 6), f12_inv(num))
    t1 = f12_mul(f12_frob(t0, 2), t0)
    t2 = pmx(t1)
    t3 = f12_mul(f12_conj(f12_cyclotomic_sqr(t1)), t2)
    t4 = pmx(t3)
    t5 = pmx(t4)
    t6 = f12_mul(pmx(t5), f12_cyclotomic_sqr(t2))
    t7 = pmx(t6)
    a = f12_frob(f12_mul(t2, t5), 2)
    b = f12_frob(f12_mul(t4, t1), 3)
    c = f12_frob(f12_mul(t6, f12_conj(t1)), 1)
    d = f12_mul(f12_mul(t7, f12_conj(t3)), t1)
    return f12_mul(f12_mul(f12_mul(a, b), c), d)


# ---------------------------------------------------------------- Miller loop (bls.ts:414-425, 575-666)
def naf(a):
    res = []
    while a > 1:
        if a & 1 == 0:
            res.insert(0, 0)
        elif a & 3 == 3:
            res.insert(0, -1)
            a += 1
        else:
            res.insert(0, 1)
        a >>= 1
    return res


ATE_NAF = naf(BLS_X)
F2_DIV2 = f2_inv((2, 0))


def _point_double(R):
    Rx, Ry, Rz = R
    t0, t1 = f2_sqr(Ry), f2_sqr(Rz)
    t2 = f2_mul_by_b(f2_mul(t1, 3))
    t3 = f2_mul(t2, 3)
    t4 = f2_sub(f2_sub(f2_sqr(f2_add(Ry, Rz)), t1), t0)
    line = (f2_sub(t2, t0), f2_mul(f2_sqr(Rx), 3), f2_neg(t4))
    nx = f2_mul(f2_mul(f2_mul(f2_sub(t0, t3), Rx), Ry), F2_DIV2)
    ny = f2_sub(f2_sqr(f2_mul(f2_add(t0, t3), F2_DIV2)), f2_mul(f2_sqr(t2), 3))
    return line, (nx, ny, f2_mul(t0, t4))


def _point_add(R, Qx, Qy):
    Rx, Ry, Rz = R
    t0 = f2_sub(Ry, f2_mul(Qy, Rz))
    t1 = f2_sub(Rx, f2_mul(Qx, Rz))
    line = (f2_sub(f2_mul(t0, Qx), f2_mul(t1, Qy)), f2_neg(t0), t1)
    t2 = f2_sqr(t1)
    t3, t4 = f2_mul(t2, t1), f2_mul(t2, Rx)
    t5 = f2_add(f2_sub(t3, f2_mul(t4, 2)), f2_mul(f2_sqr(t0), Rz))
    return line, (f2_mul(t1, t5), f2_sub(f2_mul(f2_sub(t4, t5), t0), f2_mul(t3, Ry)), f2_mul(Rz, t3))


def miller_loop(pairs):
    """millerLoopBatch over [(g1 affine, g2 affine)] with the squaring shared, conjugated (x is negative); not exponentiated"""
    f = F12_ONE
    Rs = [(Q[0], Q[1], F2_ONE) for _, Q in pairs]
    for i, bit in enumerate(ATE_NAF):
        if i:
            f = f12_sqr(f)
        for j, ((Px, Py), (Qx, Qy)) in enumerate(pairs):
            lines = []
            ln, Rs[j] = _point_double(Rs[j])
            lines.append(ln)
            if bit:
                ln, Rs[j] = _point_add(Rs[j], Qx, f2_neg(Qy) if bit == -1 else Qy)
                lines.append(ln)
            for c0, c1, c2 in lines:
                f = f12_mul014(f, c0, f2_mul(c1, Px), f2_mul(c2, Py))
    return f12_conj(f)


def on_curve_g1(pt):
    return (pt[1] * pt[1] - pt[0] ** 3 - 4) % P == 0


def on_curve_g2(pt):
    return f2_sub(f2_sqr(pt[1]), f2_add(f2_mul(f2_sqr(pt[0]), pt[0]), (4, 4))) == F2_ZERO


def pairing_batch(pairs):
    """bls.pairingBatch (bls.ts:670-693) on affine points; ZERO is (0, 0)"""
    for g1, g2 in pairs:
        if g1 == (0, 0) or g2 == (F2_ZERO, F2_ZERO):
            raise ValueError(ZERO_MSG)
        if not on_curve_g1(g1) or not on_curve_g2(g2):
            raise ValueError("bad point: equation left != right")
    return final_exponentiate(miller_loop(pairs))


def pairing(g1, g2):
    return pairing_batch([(g1, g2)])


# ---------------------------------------------------------------- group arithmetic on affine points, for building inputs
class _Curve:
    def __init__(self, add, sub, mul, sqr, inv, zero):
        self.fadd, self.fsub, self.fmul, self.fsqr, self.finv, self.zero = add, sub, mul, sqr, inv, zero

    def add(self, a, b):
        if a is None:
            return b
        if b is None:
            return a
        if a[0] == b[0]:
            if self.fadd(a[1], b[1]) == self.zero:
                return None
            lam = self.fmul(self.fmul(self.fsqr(a[0]), 3), self.finv(self.fmul(a[1], 2)))
        else:
            lam = self.fmul(self.fsub(b[1], a[1]), self.finv(self.fsub(b[0], a[0])))
        x = self.fsub(self.fsub(self.fsqr(lam), a[0]), b[0])
        return (x, self.fsub(self.fmul(lam, self.fsub(a[0], x)), a[1]))

    def mul(self, a, k):
        r = None
        while k:
            if k & 1:
                r = self.add(r, a)
            a = self.add(a, a)
            k >>= 1
        return r


C1 = _Curve(lambda a, b: (a + b) % P, lambda a, b: (a - b) % P, lambda a, b: a * b % P, lambda a: a * a % P,
            lambda a: pow(a, -1, P), 0)
C2 = _Curve(f2_add, f2_sub, f2_mul, f2_sqr, f2_inv, F2_ZERO)


def g1_mul(k):
    return C1.mul(G1, k % R)


def g2_mul(k):
    return C2.mul(G2, k % R)


# ---------------------------------------------------------------- wire format
def fp_bytes(v):
    return int(v).to_bytes(48, "little")


def g1_wire(pt):
    return fp_bytes(pt[0]) + fp_bytes(pt[1])


def g2_wire(pt):
    return b"".join(fp_bytes(c) for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]))


def f2_wire(a):
    return fp_bytes(a[0]) + fp_bytes(a[1])


def f12_coeffs(a):
    return [c for six in a for two in six for c in two]


def f12_wire(a):
    return b"".join(fp_bytes(c) for c in f12_coeffs(a))


def f12_from_coeffs(c):
    c = [int(v) for v in c]
    two = [(c[2 * i], c[2 * i + 1]) for i in range(6)]
    return (tuple(two[:3]), tuple(two[3:]))


def f12_from_wire(b):
    b = bytes(b)
    assert len(b) == 576
    return f12_from_coeffs([int.from_bytes(b[48 * i:48 * i + 48], "little") for i in range(12)])


def f12_hex(a):
    """Fp12.toBytes of the reference as hex: the same order, each coefficient 48 bytes big-endian"""
    return "".join("%096x" % c for c in f12_coeffs(a))


def f12_from_hex(h):
    return f12_from_coeffs([int(h[96 * i:96 * i + 96], 16) for i in range(12)])


def f12_from_b64(s):
    """an element of the fixture: Fp12.toBytes in base64"""
    return f12_from_hex(base64.b64decode(s).hex())


# ---------------------------------------------------------------- seeded inputs (the fixture stores only the answers)
def seeded_int(tag, i, mod):
    out = b"".join(hashlib.sha512(b"bls12-381-pairing-kat/%s/%d/%d" % (tag.encode(), i, c)).digest() for c in range(2))
    return int.from_bytes(out, "little") % mod


def seeded_f12(tag, i):
    return f12_from_coeffs([seeded_int("%s/%d" % (tag, k), i, P) for k in range(12)])


def seeded_cyclotomic(tag, i):
    """an element of the cyclotomic subgroup: the easy part of the final exponentiation of a seeded element"""
    a = seeded_f12(tag, i)
    t0 = f12_mul(f12_conj(a), f12_inv(a))
    return f12_mul(f12_frob(t0, 2), t0)


def seeded_f2(tag, i):
    return (seeded_int(tag + "/0", i, P), seeded_int(tag + "/1", i, P))


def seeded_pair_scalars(i):
    return seeded_int("pair/a", i, R - 1) + 1, seeded_int("pair/b", i, R - 1) + 1


def sparse014(o0, o1, o4):
    """the Fp12 element o0 + o1 v + o4 v w that mul014 multiplies by"""
    return ((o0, o1, F2_ZERO), (F2_ZERO, o4, F2_ZERO))


def seeded_line(i):
    return tuple(seeded_f2("op/line/%d" % k, i) for k in range(3))


def torsion_points():
    """points ON the curves and OUTSIDE the prime-order subgroups (tests/smallorder.py): order 3 in E(Fp), order 13 in E'(Fp2)"""
    import smallorder
    return smallorder.g1_order3_points()[0].toAffine(), smallorder.point_of_order("g2", 13).toAffine()


BATCH_SIZES = [1, 2, 3, 4, 5, 1, 3, 5]            # the 8 pairingBatch products of the fixture


def seeded_batch(j):
    return [(seeded_int("batch/a/%d" % j, t, R - 1) + 1, seeded_int("batch/b/%d" % j, t, R - 1) + 1) for t in range(BATCH_SIZES[j])]


_kat = None


def kat():
    global _kat
    if _kat is None:
        with open(os.path.join(HERE, "golden", "bls12_381_pairing_kat.json")) as f:
            _kat = json.load(f)
    return _kat


# ---------------------------------------------------------------- host twins
_bound = False


def _lib():
    global _bound
    L = hosttest.lib()
    if not _bound:
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        L.ht_fp12_op.argtypes = [i32, vp, vp, vp, i32, i32]
        L.ht_pairing.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp]
        L.ht_pairing.restype = ctypes.c_longlong
        L.ht_tower_consts.argtypes = [vp]
        _bound = True
    return L


def _buf(b):
    return np.frombuffer(bytearray(b) if len(b) else bytearray(16), dtype=np.uint8).copy()


def ht_fp12_op(op, a_rows, b_rows=None, raw=False):
    """rows of wire bytes in (raw: 672 bytes of stored limbs per row of a), Fp12 tuples out (OP_IS_ONE: booleans)"""
    n = len(a_rows)
    a = _buf(b"".join(a_rows))
    b = _buf(b"".join(b_rows) if b_rows else b"")
    out = np.zeros(n * 576 + 16, dtype=np.uint8)
    assert _lib().ht_fp12_op(op, a.ctypes.data, b.ctypes.data, out.ctypes.data, n, 1 if raw else 0) == 0
    if op == OP_IS_ONE:
        return [bool(v) for v in out[:n]]
    return [f12_from_wire(out[576 * i:576 * i + 576].tobytes()) for i in range(n)]


def ht_pairing(pairs, offsets, flags=0):
    """(GT per group, is_one per group), or (index, code) of the first refused pair"""
    n, ng = len(pairs), len(offsets) - 1
    g1 = _buf(b"".join(g1_wire(p) for p, _ in pairs))
    g2 = _buf(b"".join(g2_wire(q) for _, q in pairs))
    off = np.asarray(offsets, dtype=np.uint32)
    gt = np.zeros(ng * 576 + 16, dtype=np.uint8)
    one = np.zeros(ng + 16, dtype=np.uint8)
    code = np.zeros(1, dtype=np.uint32)
    bad = _lib().ht_pairing(g1.ctypes.data, g2.ctypes.data, n, off.ctypes.data, ng, flags, gt.ctypes.data, one.ctypes.data, code.ctypes.data)
    if bad >= 0:
        return int(bad), int(code[0])
    return [f12_from_wire(gt[576 * i:576 * i + 576].tobytes()) for i in range(ng)], [bool(v) for v in one[:ng]]


def ht_tower_consts():
    out = np.zeros(3 * 4 * 2 * 12, dtype=np.uint32)
    _lib().ht_tower_consts(out.ctypes.data)
    w = [int.from_bytes(out[12 * i:12 * i + 12].tobytes(), "little") for i in range(24)]
    return [[(w[(t * 4 + k) * 2], w[(t * 4 + k) * 2 + 1]) for k in range(4)] for t in range(3)]


# limbs of the storage form (fe29.hpp): 14 limbs of 29 bits, Montgomery R = 2^406
R29 = 1 << 406


def stored_limbs(value):
    """a raw integer below 256 p -> the 14 stored words"""
    assert 0 <= value < 256 * P
    return b"".join(((value >> (29 * i)) & ((1 << 29) - 1) if i < 13 else value >> (29 * 13)).to_bytes(4, "little") for i in range(14))


def stored_to_int(value):
    """the field element a raw stored integer stands for"""
    return value * pow(R29, -1, P) % P


# ---------------------------------------------------------------- verify rows of the fixture (both signature schemes)
VERIFY_VALID = 6                     # rows of tests/golden/bls12_381_sig_vectors.json used per scheme


def verify_rows():
    """{"long": [(sig, msg, pk) hex], "short": [...], "long_batch": [{"sig", "items": [(msg, pk)]}], "short_batch": [...]}: the
    first VERIFY_VALID signature vectors of each scheme as they are, then the same rows with the wrong message, the wrong key, swapped
    signatures, the ZERO encoding as key / as signature, and a key outside the prime-order subgroup (tests/smallorder.py); the
    verifyBatch cases aggregate the first three signatures - once with their messages, once with one message changed."""
    import smallorder
    from oracle.curves import BlsG1, BlsG2
    from oracle.weierstrass import (bls_g1_decode_compressed, bls_g1_encode_compressed, bls_g2_decode_compressed,
                                    bls_g2_encode_compressed)
    with open(os.path.join(HERE, "golden", "bls12_381_sig_vectors.json")) as f:
        vec = json.load(f)
    out = {}
    for name, key, Pub, pub_enc, Sig, sig_enc, sig_dec, torsion in (
            ("long", "g2", BlsG1, bls_g1_encode_compressed, BlsG2, bls_g2_encode_compressed, bls_g2_decode_compressed,
             smallorder.g1_order3_points()[0]),
            ("short", "g1", BlsG2, bls_g2_encode_compressed, BlsG1, bls_g1_encode_compressed, bls_g1_decode_compressed,
             smallorder.point_of_order("g2", 13))):
        rows = []
        for v in vec[key][:VERIFY_VALID]:
            pk = pub_enc(Pub.BASE.multiplyUnsafe(int(v["priv"], 16) % R)).hex()      # Fn.fromBytes reduces (bls12-381.ts:156)
            rows.append((v["sig"], v["msg"], pk))
        zero_pk, zero_sig = "c0" + "00" * (len(rows[0][2]) // 2 - 1), "c0" + "00" * (len(rows[0][0]) // 2 - 1)
        bad = [(rows[0][0], rows[1][1] + "00", rows[0][2]), (rows[0][0], rows[0][1], rows[1][2]), (rows[3][0], rows[2][1], rows[2][2]),
               (rows[0][0], rows[0][1], zero_pk), (zero_sig, rows[0][1], rows[0][2]), (rows[0][0], rows[0][1], pub_enc(torsion).hex())]
        mixed = []
        for i in range(VERIFY_VALID):                # valid and invalid interleaved
            mixed += [rows[i], bad[i]]
        out[name] = [list(r) for r in mixed]
        agg = Sig.ZERO
        for r in rows[:3]:
            agg = agg.add(sig_dec(Sig, bytes.fromhex(r[0])))
        agg = sig_enc(agg).hex()
        items = [[r[1], r[2]] for r in rows[:3]]
        out[name + "_batch"] = [{"sig": agg, "items": items}, {"sig": agg, "items": [[items[0][0] + "ff", items[0][1]]] + items[1:]},
                                {"sig": rows[0][0], "items": items[:1]}]
    return out
