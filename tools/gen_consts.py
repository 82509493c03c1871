#!/usr/bin/env python3
"""Generates noble-curves_amd/csrc/consts_gen.hpp: Montgomery constants (32-bit limbs,
little-endian) for the three base fields and the curve constants of the hot path.
Values restate reference src/secp256k1.ts:48-64, src/ed25519.ts:49-65,102-104,
src/bls12-381.ts:134-158,321-345.  Run: python tools/gen_consts.py
"""
import os

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "noble-curves_amd", "csrc", "consts_gen.hpp")


def limbs(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def arr(name, x, n):
    return "  static constexpr uint32_t %s[%d] = {%s};\n" % (
        name, n, ", ".join("0x%08xu" % l for l in limbs(x, n)))


def field(name, p, n, extra=None, fold=None):
    """fold = (c_lo, c_hi, final_subs): plain residues, 2^256 folded as c (special-form prime);
    otherwise Montgomery constants with R = 2^(32 n)."""
    R = 1 if fold else 1 << (32 * n)
    inv = (-pow(p, -1, 1 << 32)) % (1 << 32)
    s = "struct %s {\n  static constexpr int N = %d;\n" % (name, n)
    s += arr("P", p, n)
    s += "  static constexpr uint32_t INV = 0x%08xu;  // -p^-1 mod 2^32\n" % inv
    s += arr("R1", R % p, n)        # Montgomery form of 1
    s += arr("R2", R * R % p, n)    # to-Montgomery multiplier
    s += "  static constexpr bool TOP_SPARE = %s;  // top bit of p clear: CIOS carries never overflow\n" % (
        "true" if p < (1 << (32 * n - 1)) else "false")
    if fold:
        s += "  static constexpr bool FOLD = true;   // plain residues; R1 = R2 = 1\n"
        s += "  static constexpr uint32_t FOLD_LO = 0x%08xu;\n  static constexpr uint32_t FOLD_HI = %du;\n" % (fold[0], fold[1])
        s += "  static constexpr int FINAL_SUBS = %d;\n" % fold[2]
    else:
        s += "  static constexpr bool FOLD = false;  // Montgomery form\n"
    for k, v in (extra or {}).items():
        s += arr(k, v * R % p, n)   # constants stored in Montgomery form
    s += "};\n\n"
    return s


def limbs29(x, n):
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(n)]


def arr29(name, x, n):
    return "  static constexpr uint32_t %s[%d] = {%s};\n" % (
        name, n, ", ".join("0x%08xu" % l for l in limbs29(x, n)))


def field29(name, p, n, extra=None):
    """Montgomery constants for radix 2^29 with n limbs (R = 2^(29 n))."""
    R = 1 << (29 * n)
    inv = (-pow(p, -1, 1 << 29)) % (1 << 29)
    s = "struct %s {\n  static constexpr int N = %d;\n  static constexpr int BITS = 29;\n" % (name, n)
    s += arr29("P", p, n)
    s += "  static constexpr uint32_t INV = 0x%08xu;  // -p^-1 mod 2^29\n" % inv
    s += arr29("R1", R % p, n)
    s += arr29("R2", R * R % p, n)
    # 2^k * p for k = 0..12 (subtraction offsets), normalised limbs
    s += "  static constexpr uint32_t PMUL[13][%d] = {\n" % n
    for k in range(13):
        s += "    {%s},\n" % ", ".join("0x%08xu" % l for l in limbs29(p << k, n))
    s += "  };\n"
    for k, v in (extra or {}).items():
        s += arr29(k, v * R % p, n)
    if n % 2 == 0:  # host-side twin in radix 2^58 (same R): limbs pair up
        inv58 = (-pow(p, -1, 1 << 58)) % (1 << 58)
        s += "  static constexpr uint64_t P58[%d] = {%s};\n" % (
            n // 2, ", ".join("0x%016xull" % ((p >> (58 * i)) & ((1 << 58) - 1)) for i in range(n // 2)))
        s += "  static constexpr uint64_t INV58 = 0x%016xull;  // -p^-1 mod 2^58\n" % inv58
    s += "};\n\n"
    return s


def field9(name, p, extra=None):
    """Constants of the carry-free radix-2^29 form of a 256-bit special prime (fe9.hpp): 9 limbs, plain
    residues, 2^261 folded as C = C0 + C1*2^29; BIAS[K] = a multiple of p whose limbs are all >= K*U
    (U = 2^29 + 2^19, the limb unit of the bound types) for subtraction without borrows."""
    M = (1 << 29) - 1
    U = (1 << 29) + (1 << 19)
    C = (1 << 261) % p
    c0, c1 = C & M, C >> 29
    assert c0 < (1 << 15) and c1 < (1 << 10)
    s = "struct %s {\n" % name
    s += arr29("P", p, 9)
    s += "  static constexpr uint32_t C0 = %du, C1 = %du;  // 2^261 mod p = C0 + C1 * 2^29\n" % (c0, c1)
    s += "  static constexpr uint32_t PINV = 0x%08xu;  // p^-1 mod 2^29\n" % pow(p, -1, 1 << 29)
    s += "  static constexpr int JMAX = %d;  // a value with limbs < B*U is below JMAX*B*p\n" % (
        (U * sum(1 << (29 * i) for i in range(9)) + p - 1) // p)
    # the division-step inversion (fe9_inv.hpp): p in balanced signed limbs of 30 bits (all but three are zero for a
    # prime 2^k - c with a small c) and p^-1 mod 2^30
    p30, cy = [], 0
    for i in range(9):
        l = ((p >> (30 * i)) & ((1 << 30) - 1)) + cy
        cy = 1 if (l >= (1 << 29) and i < 8) else 0
        p30.append(l - (cy << 30))
    assert sum(l << (30 * i) for i, l in enumerate(p30)) == p and all(abs(l) < (1 << 17) for l in p30)
    s += "  static constexpr int32_t P30[9] = {%s};  // p in signed limbs of 30 bits\n" % ", ".join("%d" % l for l in p30)
    s += "  static constexpr uint32_t PINV30 = 0x%08xu;  // p^-1 mod 2^30\n" % pow(p, -1, 1 << 30)
    s += "  static constexpr uint32_t BIAS[8][9] = {\n"
    for k in range(8):
        base = sum((k * U) << (29 * i) for i in range(9))
        t = (-base) % p
        lim = [k * U + ((t >> (29 * i)) & M) for i in range(9)]
        assert sum(l << (29 * i) for i, l in enumerate(lim)) % p == 0 and all(k * U <= l < (k + 1) * U for l in lim)
        s += "    {%s},\n" % ", ".join("0x%08xu" % l for l in lim)
    s += "  };\n"
    for k, v in (extra or {}).items():
        s += arr29(k, v % p, 9)
    s += "};\n\n"
    return s


def main():
    kp = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F
    kn = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
    beta = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
    ep = (1 << 255) - 19
    ed = 0x52036CEE2B6FFE738CC740797779E89800700A4D4141D8AB75EB4DCA135978A3
    sqrtm1 = 19681161376707505956807079304988542015446066515923890162744021073123829784752
    bp = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    out = "// GENERATED by tools/gen_consts.py - do not edit.\n#pragma once\n#include <stdint.h>\nnamespace ncg {\n\n"
    out += field("ParamsSecpP", kp, 8, {"BETA": beta, "B3": 21}, fold=(977, 1, 1))
    out += field("ParamsEdP", ep, 8, {"D": ed, "D2": 2 * ed % ep, "SQRT_M1": sqrtm1}, fold=(38, 0, 2))
    out += field("ParamsBlsP", bp, 12, {})
    out += field9("Fe9SecpPR", kp, {"BETA": beta})
    # ristretto255 (src/ed25519.ts:410-424), from d and sqrt(-1) with a = -1.  p = 5 (mod 8): a square root of a residue v is
    # v^((p+3)/8), times sqrt(-1) when that squares to -v.  a d - 1 and a - d are the same number, -1 - d: the reference's
    # sqrt(a d - 1) is its ODD root and 1 / sqrt(a - d) the inverse of its EVEN root (RFC 9496 section 4.1 lists the same values;
    # the test of the fixture compares them with the decimals of src/ed25519.ts).
    def ed_sqrt_even(v):
        v %= ep
        x = pow(v, (ep + 3) // 8, ep)
        if x * x % ep != v:
            x = x * sqrtm1 % ep
        assert x * x % ep == v, "not a square"
        return x if x % 2 == 0 else ep - x
    assert sqrtm1 * sqrtm1 % ep == ep - 1
    sqrt_ad_minus_one = ep - ed_sqrt_even(-ed - 1)
    invsqrt_a_minus_d = pow(ed_sqrt_even(-1 - ed), -1, ep)
    assert sqrt_ad_minus_one ** 2 % ep == (-ed - 1) % ep and invsqrt_a_minus_d ** 2 * (-1 - ed) % ep == 1
    rist = {"SQRT_AD_MINUS_ONE": sqrt_ad_minus_one, "INVSQRT_A_MINUS_D": invsqrt_a_minus_d,
            "ONE_MINUS_D_SQ": (1 - ed * ed) % ep, "D_MINUS_ONE_SQ": (ed - 1) ** 2 % ep}
    out += field9("Fe9EdPR", ep, {"D": ed, "D2": 2 * ed % ep, "SQRT_M1": sqrtm1, **rist})
    g1_beta = 0x5F19672FDF76CE51BA69C6076A0F77EADDB3A93BE6F89688DE17D813620A00022E01FFFFFFFEFFFE
    # G2 psi endomorphism coefficients (src/abstract/tower.ts:240-241 with base 1/(u+1),
    # src/bls12-381.ts:283): PSI_X = base^((p-1)/3), PSI_Y = base^((p-1)/2) in Fp2 = Fp[u]/(u^2+1)
    def f2mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % bp, (a[0] * b[1] + a[1] * b[0]) % bp)

    def f2pow(a, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = f2mul(r, a)
            a = f2mul(a, a)
            e >>= 1
        return r
    ninv = pow(2, -1, bp)
    base = (ninv, (-ninv) % bp)                      # 1/(1+u) = (1-u)/2
    assert f2mul(base, (1, 1)) == (1, 0)
    psi_x = f2pow(base, (bp - 1) // 3)
    psi_y = f2pow(base, (bp - 1) // 2)
    out += field29("ParamsBls29", bp, 14, {"FOUR": 4, "G1_BETA": g1_beta, "HALF": ninv,
                                           "PSI_X_C0": psi_x[0], "PSI_X_C1": psi_x[1],
                                           "PSI_Y_C0": psi_y[0], "PSI_Y_C1": psi_y[1]})
    # hash-to-curve constants (RFC 9380 8.8, E.2, E.3; src/bls12-381.ts:668-851) in radix-2^29
    # Montgomery form, read from tools/h2c_constants.json (numbers extracted from the reference)
    import json
    hk = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "h2c_constants.json")))
    R29 = 1 << (29 * 14)

    def m29(v):
        return "{%s}" % ", ".join("0x%08xu" % l for l in limbs29(int(v) % bp * R29 % bp, 14))
    out += "struct BlsH2c {\n"
    for k in ("xnum", "xden", "ynum", "yden"):
        rows = hk["G1"][k]
        out += "  static constexpr int ISO1_%s_N = %d;\n" % (k.upper(), len(rows))
        out += "  static constexpr uint32_t ISO1_%s[%d][14] = {\n%s\n  };\n" % (
            k.upper(), len(rows), ",\n".join("    " + m29(v) for v in rows))
    for k in ("xnum", "xden", "ynum", "yden"):
        rows = hk["G2"][k]
        out += "  static constexpr int ISO2_%s_N = %d;\n" % (k.upper(), len(rows))
        out += "  static constexpr uint32_t ISO2_%s[%d][2][14] = {\n%s\n  };\n" % (
            k.upper(), len(rows), ",\n".join("    {%s, %s}" % (m29(a), m29(b)) for a, b in rows))
    z1 = int(hk["G1"]["Z"])
    c2 = pow((-z1) % bp, (bp + 1) // 4, bp)             # sqrt(-Z), sqrt_ratio_3mod4 constant c2
    assert c2 * c2 % bp == (-z1) % bp
    for name, v in (("SWU1_A", hk["G1"]["A"]), ("SWU1_B", hk["G1"]["B"]), ("SWU1_Z", z1), ("SWU1_C2", c2)):
        out += "  static constexpr uint32_t %s[14] = %s;\n" % (name, m29(v))
    for name, v in (("SWU2_A", hk["G2"]["A"]), ("SWU2_B", hk["G2"]["B"]), ("SWU2_Z", hk["G2"]["Z"])):
        out += "  static constexpr uint32_t %s[2][14] = {%s, %s};\n" % (name, m29(v[0]), m29(v[1]))
    # K = sqrt(-norm(Z)) for the G2 SWU constant Z = -(2 + u): norm(Z) = 5 is a non-residue (Z is a non-square
    # of Fp2) and so is -1, hence -5 is a residue.  Used to turn sqrt(-norm(w)) into sqrt(norm(Z w)).
    z2 = [int(v) % bp for v in hk["G2"]["Z"]]
    nz = (z2[0] * z2[0] + z2[1] * z2[1]) % bp
    kk = pow((-nz) % bp, (bp + 1) // 4, bp)
    assert kk * kk % bp == (-nz) % bp
    out += "  static constexpr uint32_t SWU2_K[14] = %s;  // sqrt(-norm(SWU2_Z)) in Fp\n" % m29(kk)
    psi2_x = f2pow(base, (bp * bp - 1) // 3)            # src/abstract/tower.ts:249
    assert psi2_x[1] == 0 and f2pow(base, (bp * bp - 1) // 2) == (bp - 1, 0)
    out += "  static constexpr uint32_t PSI2_X[14] = %s;  // in Fp\n" % m29(psi2_x[0])
    out += "};\n\n"
    # Frobenius coefficients of the Fp6 / Fp12 tower over v^3 = u + 1, w^2 = v (src/abstract/tower.ts:136-179
    # calcFrobeniusCoefficients, used at :587-602 and :865-875): rows k = 0..3 of
    #   FROB6_C1[k] = (u+1)^((p^k - 1)/3), FROB6_C2[k] = (u+1)^((2 p^k - 2)/3), FROB12[k] = (u+1)^((p^k - 1)/6)
    out += "// Frobenius coefficients of Fp6 / Fp12 (powers 0..3), radix-2^29 Montgomery form, [k][c0 | c1][limb]\nstruct BlsTower {\n"
    for name, mul, div in (("FROB6_C1", 1, 3), ("FROB6_C2", 2, 3), ("FROB12", 1, 6)):
        rows = []
        for k in range(4):
            num = mul * bp ** k - mul
            assert num % div == 0
            rows.append(f2pow((1, 1), num // div))
        out += "  static constexpr uint32_t %s[4][2][14] = {\n%s\n  };\n" % (
            name, ",\n".join("    {%s, %s}" % (m29(a), m29(b)) for a, b in rows))
    out += "};\n\n"
    out += "// exponents / thresholds for bls12-381 Fp square roots and the compressed-point sort bit\nstruct BlsFpConsts {\n"
    out += arr("SQRT_EXP", (bp + 1) // 4, 12)          # p = 3 mod 4: sqrt(a) = a^((p+1)/4)
    out += arr("SQRT_EXP_M1", (bp - 3) // 4, 12)       # a^((p-3)/4): sqrt candidate and its inverse at once
    out += arr("HALF_P", (bp - 1) // 2, 12)            # y > (p-1)/2  <=>  sort bit
    out += arr("P32", bp, 12)
    out += "};\n\n"
    # GLV constants (libsecp256k1-style 384-bit reciprocals of the reference's basis,
    # src/secp256k1.ts:58-64): g1 = round(2^384*b2/n), g2 = round(2^384*(-b1)/n)
    a1 = 0x3086D221A7D46BCDE86C90E49284EB15
    mb1 = 0xE4437ED6010E88286F547FA90ABFE4C3
    a2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
    b2 = a1
    g1 = ((b2 << 384) + kn // 2) // kn
    g2 = ((mb1 << 384) + kn // 2) // kn
    out += "struct SecpGlv {\n"
    out += arr("G1", g1, 8) + arr("G2", g2, 8)
    out += arr("A1", a1, 5) + arr("MB1", mb1, 5) + arr("A2", a2, 5) + arr("B2", b2, 5)
    out += arr("N", kn, 8)
    out += "};\n\n"
    bls_r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    ed_l = 0x1000000000000000000000000000000014DEF9DEA2F79CD65812631A5CF5D3ED
    # bls12-381 scalar field Fr as a Montgomery field for the NTT (src/bls12-381.ts bls12_381_Fr;
    # src/abstract/fft.ts).  INV2 = 1/2 for the 1/N scale of the inverse transform.
    out += field("ParamsBlsR", bls_r, 8, {"INV2": (bls_r + 1) // 2})
    # Fr in radix 2^29 for the NTT butterflies (fr29.hpp): R = 2^261, r = 1 (mod 2^29) so -r^-1 = -1 and
    # the Montgomery quotient digit is the negated low limb; C255 = 2^255 - r folds the bits at and above
    # 2^255; BIAS = 3 r with limbs 0..7 in [2^29, 2^30) for the subtraction a + BIAS - t; K261 = 2^261 mod r
    # (plain 8 x 32-bit integer) moves the twiddle table from R = 2^256 to R = 2^261.
    assert bls_r % (1 << 29) == 1
    m29 = (1 << 29) - 1
    low = sum(1 << (29 * i + 29) for i in range(8))
    rest = 3 * bls_r - low
    assert rest > 0
    bias = [((rest >> (29 * i)) & m29) + (1 << 29) for i in range(8)] + [rest >> 232]
    assert sum(b << (29 * i) for i, b in enumerate(bias)) == 3 * bls_r
    out += "struct Fr29PR {\n"
    out += arr29("P", bls_r, 9) + arr29("C255", (1 << 255) - bls_r, 9)
    out += "  static constexpr uint32_t BIAS[9] = {%s};  // 3 r\n" % ", ".join("0x%08xu" % b for b in bias)
    out += arr("K261", (1 << 261) % bls_r, 8)
    out += arr29("ONE", (1 << 261) % bls_r, 9)
    out += "};\n\n"
    out += "// group orders (Fn.ORDER of the reference's curves), 8 LE limbs\nstruct Orders {\n"
    out += arr("SECP_N", kn, 8) + arr("ED_L", ed_l, 8) + arr("BLS_R", bls_r, 8)
    out += "};\n\n"
    # generators in wire format (x || y, LE 32-bit limbs; Fp2 = c0, c1)
    kgx = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
    kgy = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
    g1x = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
    g1y = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
    g2 = [0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
          0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E,
          0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
          0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE]
    def wire(vals, n):
        w = []
        for v in vals:
            w += limbs(v, n)
        return ", ".join("0x%08xu" % l for l in w)
    out += "// generators (Point.BASE) in the wire format of include/ncg.h\nstruct BasePoints {\n"
    out += "  static constexpr uint32_t SECP[16] = {%s};\n" % wire([kgx, kgy], 8)
    out += "  static constexpr uint32_t G1[24] = {%s};\n" % wire([g1x, g1y], 12)
    out += "  static constexpr uint32_t G2[48] = {%s};\n" % wire(g2, 12)
    out += "};\n\n"
    # bn254 scalar field Fr for the NTT (src/bn254.ts bn254_Fr; src/abstract/fft.ts): the 8 x 32-bit Montgomery field of the
    # table builder, and the radix-2^29 form of the butterflies (fr29.hpp, Fr29Bn).  r = 2^28 + 1 (mod 2^29), so
    # -r^-1 = 2^28 - 1 (mod 2^29): the Montgomery quotient digit of a column t is ((t & 1) << 28) - t, and q r[0] is a real
    # term of every column.  C254 = 2^254 - r folds the bits at and above 2^254 (r has 254 bits); BIAS = 3 r with limbs 0..7
    # in [2^29, 2^30); K261 and ONE as for bls12-381.
    bn_r = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
    assert bn_r.bit_length() == 254 and (bn_r - 1) % (1 << 28) == 0 and (bn_r - 1) % (1 << 29) != 0   # 2-adicity 28
    assert bn_r % (1 << 29) == (1 << 28) + 1 and (-pow(bn_r, -1, 1 << 29)) % (1 << 29) == (1 << 28) - 1
    for t in (0, 1, 2, 3, m29, m29 - 1, 0x12345678 & m29):                     # the quotient digit cancels the low limb
        q = (((t & 1) << 28) - t) % (1 << 29)
        assert (t + q * (bn_r & m29)) % (1 << 29) == 0
    assert pow(5, (bn_r - 1) // 2, bn_r) == bn_r - 1 and pow(7, (bn_r - 1) // 2, bn_r) == bn_r - 1      # non-residues
    assert all(pow(g, (bn_r - 1) // 2, bn_r) == 1 for g in (2, 3, 4))           # findGenerator stops at 5
    # columns of fr29_mont: 9 products of a limb below 6 * 2^29 (limb 8: 2^32) with an exact limb, 9 of q with a limb of r
    assert (8 * 6 + 8) * (1 << 58) + sum(limbs29(bn_r, 9)) * (1 << 29) + (1 << 36) < (1 << 64)
    # a pass: values below 2^256 in, + 3 r per stage, 10 stages; two folds at 2^254 come below 2^256, three below 2 r
    c254 = (1 << 254) - bn_r
    top = (1 << 256) + 30 * bn_r
    assert top < (1 << 259)
    f1 = (1 << 254) + (top >> 254) * c254
    f2 = (1 << 254) + (f1 >> 254) * c254
    f3 = (1 << 254) + (f2 >> 254) * c254
    assert f2 < (1 << 256) and f2 >= 2 * bn_r and f3 < 2 * bn_r
    assert top * bn_r // (1 << 261) + bn_r < 5 * bn_r // 4                     # a product stays below 1.25 r
    rest = 3 * bn_r - low
    assert rest > 0
    bias = [((rest >> (29 * i)) & m29) + (1 << 29) for i in range(8)] + [rest >> 232]
    assert sum(b << (29 * i) for i, b in enumerate(bias)) == 3 * bn_r
    assert all((1 << 29) <= b < (1 << 30) for b in bias[:8]) and bias[8] > (5 * bn_r // 4) >> 232
    out += field("ParamsBn254R", bn_r, 8, {"INV2": (bn_r + 1) // 2})
    out += "struct Fr29Bn254R {\n"
    out += arr29("P", bn_r, 9) + arr29("C254", c254, 9)
    out += "  static constexpr uint32_t BIAS[9] = {%s};  // 3 r\n" % ", ".join("0x%08xu" % b for b in bias)
    out += arr("K261", (1 << 261) % bn_r, 8)
    out += arr29("ONE", (1 << 261) % bn_r, 9)
    out += "};\n\n"
    # decaf448 (src/ed448.ts:446-457, 515-520; RFC 9496 section 5.1) in the radix-2^28 form of fe448.hpp: 16 limbs, plain residues.
    # p = 3 (mod 4): the square root of a residue v is v^((p + 1) / 4).  -d = 39081; the reference's sqrt(-d) is the EVEN root and
    # 1 / sqrt(-d) its inverse (the host test compares both with the decimals of src/ed448.ts).  The base
    # point is twice the Ed448 base (Gx, Gy), computed here by the affine doubling for a = 1.
    gp = (1 << 448) - (1 << 224) - 1
    gd = gp - 39081
    root = pow(39081, (gp + 1) // 4, gp)
    assert root * root % gp == 39081
    sqrt_minus_d = root if root % 2 == 0 else gp - root
    invsqrt_minus_d = pow(sqrt_minus_d, -1, gp)
    assert invsqrt_minus_d ** 2 * 39081 % gp == 1
    ggx = 0x4f1970c66bed0ded221d15a622bf36da9e146570470f1767ea6de324a3d3a46412ae1af72ab66511433b80e18b00938e2626a82bc70cc05e
    ggy = 0x693f46716eb6bc248876203756c9c7624bea73736ca3984087789c1e05a0c2d73ad3ff1ce67c39c4fdbd132c4ed7c8ad9808795bf230fa14
    assert (ggx * ggx + ggy * ggy - 1 - gd * ggx * ggx * ggy * ggy) % gp == 0
    gt = gd * ggx * ggx * ggy * ggy % gp
    dbx = 2 * ggx * ggy * pow(1 + gt, -1, gp) % gp
    dby = (ggy * ggy - ggx * ggx) * pow(1 - gt, -1, gp) % gp
    assert (dbx * dbx + dby * dby - 1 - gd * dbx * dbx * dby * dby) % gp == 0

    def arr28(name, x):
        return "  static constexpr uint32_t %s[16] = {%s};\n" % (
            name, ", ".join("0x%08xu" % ((x >> (28 * i)) & ((1 << 28) - 1)) for i in range(16)))
    out += "// decaf448 over GF(2^448 - 2^224 - 1): 16 limbs in radix 2^28 (fe448.hpp)\nstruct Decaf448Consts {\n"
    out += arr28("ONE_MINUS_D", (1 - gd) % gp) + arr28("ONE_MINUS_TWO_D", (1 - 2 * gd) % gp)
    out += arr28("SQRT_MINUS_D", sqrt_minus_d) + arr28("INVSQRT_MINUS_D", invsqrt_minus_d)
    out += arr28("BASE_X", dbx) + arr28("BASE_Y", dby)
    out += "};\n\n"
    # RFC 9380 suites for secp256k1 and edwards25519 (h2c_suites.hpp), plain residues in the radix-2^29 form of fe9.hpp.
    # secp256k1 (RFC 9380 section 8.7, appendix E.1; src/secp256k1.ts:345-401): E' : y^2 = x^3 + A' x + B', Z = -11 and the 3-isogeny
    # E' -> E, coefficients in ascending degree.  C2 = sqrt(-Z) of sqrt_ratio_3mod4 (either root: SWU fixes the sign of y afterwards).
    swu_a = 0x3f8731abdd661adca08a5558f0f5d272e953d363cb6f0e5d405447c01a444533
    swu_b, swu_z = 1771, kp - 11
    iso = {
        "XNUM": [0x8e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38daaaaa8c7,
                 0x7d3d4c80bc321d5b9f315cea7fd44c5d595d2fc0bf63b92dfff1044f17c6581,
                 0x534c328d23f234e6e2a413deca25caece4506144037c40314ecbd0b53d9dd262,
                 0x8e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38daaaaa88c],
        "XDEN": [0xd35771193d94918a9ca34ccbb7b640dd86cd409542f8487d9fe6b745781eb49b,
                 0xedadc6f64383dc1df7c4b2d51b54225406d36b641f5e41bbc52a56612a8c6d14, 1],
        "YNUM": [0x4bda12f684bda12f684bda12f684bda12f684bda12f684bda12f684b8e38e23c,
                 0xc75e0c32d5cb7c0fa9d0a54b12a0a6d5647ab046d686da6fdffc90fc201d71a3,
                 0x29a6194691f91a73715209ef6512e576722830a201be2018a765e85a9ecee931,
                 0x2f684bda12f684bda12f684bda12f684bda12f684bda12f684bda12f38e38d84],
        "YDEN": [0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffff93b,
                 0x7a06534bb8bdb49fd5e9e6632722c2989467c1bfc8e8d978dfb425d2685c2573,
                 0x6484aa716545ca2cf3a70c3fa8fe337e0a3d21162f0d6299a7bf8192bfd2a76f, 1],
    }
    assert kp % 4 == 3 and pow(swu_z, (kp - 1) // 2, kp) == kp - 1                     # Z is a non-square
    swu_c2 = pow(11, (kp + 1) // 4, kp)
    assert swu_c2 * swu_c2 % kp == 11
    # the isogeny carries E' to y^2 = x^3 + 7: checked on the image of one point of E'
    xe = 1
    while pow((xe ** 3 + swu_a * xe + swu_b) % kp, (kp - 1) // 2, kp) != 1:
        xe += 1
    ye = pow((xe ** 3 + swu_a * xe + swu_b) % kp, (kp + 1) // 4, kp)
    ev = {k: sum(c * pow(xe, i, kp) for i, c in enumerate(v)) % kp for k, v in iso.items()}
    xi, yi = ev["XNUM"] * pow(ev["XDEN"], -1, kp) % kp, ye * ev["YNUM"] * pow(ev["YDEN"], -1, kp) % kp
    assert (yi * yi - xi ** 3 - 7) % kp == 0
    out += "// RFC 9380 suite secp256k1_XMD:SHA-256_SSWU_RO_ (h2c_suites.hpp): 9 limbs in radix 2^29, plain residues\nstruct SecpH2c {\n"
    for k, rows in iso.items():
        out += "  static constexpr int ISO_%s_N = %d;\n" % (k, len(rows))
        out += "  static constexpr uint32_t ISO_%s[%d][9] = {\n%s\n  };\n" % (
            k, len(rows), ",\n".join("    {%s}" % ", ".join("0x%08xu" % l for l in limbs29(v % kp, 9)) for v in rows))
    out += arr29("SWU_A", swu_a, 9) + arr29("SWU_B", swu_b, 9) + arr29("SWU_Z", swu_z, 9) + arr29("SWU_C2", swu_c2, 9)
    out += "};\n\n"
    # edwards25519 (RFC 9380 appendix G.2.1, G.2.2; src/ed25519.ts:294-379): J = 486662, c2 = 2^((p + 3) / 8), c3 = sqrt(-1) (the
    # field's SQRT_M1: either root, the sign of y is fixed afterwards) and the EVEN root c1 of -(J + 2) of the map to Edwards form
    ell2_c2 = pow(2, (ep + 3) // 8, ep)
    ell2_c1_edwards = ed_sqrt_even(-486664)
    assert ell2_c1_edwards % 2 == 0 and ell2_c1_edwards ** 2 % ep == (-486664) % ep
    out += "// RFC 9380 suite edwards25519_XMD:SHA-512_ELL2_RO_ (h2c_suites.hpp): 9 limbs in radix 2^29, plain residues\nstruct EdH2c {\n"
    out += arr29("ELL2_J", 486662, 9) + arr29("ELL2_C2", ell2_c2, 9) + arr29("ELL2_C1_EDWARDS", ell2_c1_edwards, 9)
    out += "};\n\n"
    out += "}  // namespace ncg\n"
    with open(OUT, "w") as f:
        f.write(out)
    print("wrote", os.path.normpath(OUT))


if __name__ == "__main__":
    main()
