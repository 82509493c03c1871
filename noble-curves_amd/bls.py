"""Host mirror of the reference's bls12-381 pairing interface (`bls12_381.pairing`, `.pairingBatch`, `.fields.Fp12`,
`.longSignatures` / `.shortSignatures` verification - src/abstract/bls.ts:646-698, :795-873, src/abstract/tower.ts:822-1092):
argument checks and messages here, every field operation in `libncg.so` (`ncg_pairing_batch`, `ncg_fp12_batch`, the
decoders, the hash-to-curve maps and the MSM).  An Fp12 element is the nested tuple of the reference's object:
((c0, c1, c2), (c0, c1, c2)) of Fp2 = (c0, c1) integers.  Signing and key generation are not offered: the engine works on
public data.
"""
import numpy as np

from . import _native
from . import curve as _curve
from . import h2c as _h2c
from ._native import get_engine

G1Point, G2Point = _curve.bls12_381_G1_Point, _curve.bls12_381_G2_Point
_P = G1Point.Fp.ORDER
ZERO_MSG = "pairing is not available for ZERO point"


# ---------------------------------------------------------------- Fp12 <-> wire
def _f12_coeffs(a):
    try:
        (a0, a1, a2), (b0, b1, b2) = a
        cs = [int(c) for two in (a0, a1, a2, b0, b1, b2) for c in (two[0], two[1])]
    except (TypeError, ValueError, IndexError):
        raise TypeError("invalid field element: expected Fp12")
    if len(cs) != 12 or any(not 0 <= c < _P for c in cs):
        raise ValueError("invalid field element: expected Fp12 with coefficients in [0, p)")
    return cs


def _f12_wire(a):
    return b"".join(c.to_bytes(48, "little") for c in _f12_coeffs(a))


def _f12_from_wire(row):
    row = bytes(row)
    c = [int.from_bytes(row[48 * i:48 * i + 48], "little") for i in range(12)]
    two = [(c[2 * i], c[2 * i + 1]) for i in range(6)]
    return (tuple(two[:3]), tuple(two[3:]))


def _f2_wire(a):
    c0, c1 = int(a[0]), int(a[1])
    if not (0 <= c0 < _P and 0 <= c1 < _P):
        raise ValueError("invalid field element: expected Fp2 with coefficients in [0, p)")
    return c0.to_bytes(48, "little") + c1.to_bytes(48, "little")


class _Fp12:
    """bls12_381.fields.Fp12 (tower.ts:822-1092): single elements and `*Batch` forms, one launch each"""
    BYTES = 576
    ZERO = (((0, 0),) * 3, ((0, 0),) * 3)
    ONE = (((1, 0), (0, 0), (0, 0)), ((0, 0),) * 3)

    def _run(self, op, xs, bs=None, engine=None):
        xs = list(xs)
        if not xs:
            return []
        a = np.frombuffer(b"".join(_f12_wire(x) for x in xs), dtype=np.uint8)
        b = None
        if op == _native.FP12_MUL:
            b = np.frombuffer(b"".join(_f12_wire(y) for y in bs), dtype=np.uint8)
        elif op == _native.FP12_MUL014:
            b = np.frombuffer(b"".join(_f2_wire(o) for row in bs for o in row), dtype=np.uint8)
        out = (engine or get_engine()).fp12_batch(op, a, b)
        if op == _native.FP12_IS_ONE:
            return [bool(v) for v in out]
        return [_f12_from_wire(out[i]) for i in range(len(xs))]

    def mulBatch(self, xs, ys, engine=None):
        xs, ys = list(xs), list(ys)
        if len(xs) != len(ys):
            raise ValueError("arrays of operands must have equal length")
        return self._run(_native.FP12_MUL, xs, ys, engine)

    def sqrBatch(self, xs, engine=None):
        return self._run(_native.FP12_SQR, xs, engine=engine)

    def invBatch(self, xs, engine=None):
        return self._run(_native.FP12_INV, xs, engine=engine)

    def conjugateBatch(self, xs, engine=None):
        return self._run(_native.FP12_CONJUGATE, xs, engine=engine)

    def frobeniusMapBatch(self, xs, power, engine=None):
        power %= 12
        if power == 0:
            return list(xs)
        if power == 6:                                        # tower.ts:1028
            return self.conjugateBatch(xs, engine)
        if power not in (1, 2, 3):
            raise ValueError("noble-gpu: Fp12.frobeniusMap: powers 0, 1, 2, 3 and 6 only")
        return self._run(_native.FP12_FROBENIUS1 + power - 1, xs, engine=engine)

    def cyclotomicSquareBatch(self, xs, engine=None):
        return self._run(_native.FP12_CYCLOTOMIC_SQR, xs, engine=engine)

    def mul014Batch(self, xs, lines, engine=None):
        """x * (o0 + o1 v + o4 v w) per row; lines: [(o0, o1, o4)] of Fp2"""
        xs, lines = list(xs), [tuple(r) for r in lines]
        if len(xs) != len(lines) or any(len(r) != 3 for r in lines):
            raise ValueError("arrays of operands must have equal length")
        return self._run(_native.FP12_MUL014, xs, lines, engine)

    def finalExponentiateBatch(self, xs, engine=None):
        return self._run(_native.FP12_FINAL_EXP, xs, engine=engine)

    def isOneBatch(self, xs, engine=None):
        return self._run(_native.FP12_IS_ONE, xs, engine=engine)

    def mul(self, a, b):
        return self.mulBatch([a], [b])[0]

    def sqr(self, a):
        return self.sqrBatch([a])[0]

    def inv(self, a):
        return self.invBatch([a])[0]

    def div(self, a, b):
        return self.mul(a, self.inv(b))

    def conjugate(self, a):
        return self.conjugateBatch([a])[0]

    def frobeniusMap(self, a, power):
        return self.frobeniusMapBatch([a], power)[0]

    def _cyclotomicSquare(self, a):
        return self.cyclotomicSquareBatch([a])[0]

    def finalExponentiate(self, a):
        return self.finalExponentiateBatch([a])[0]

    def eql(self, a, b):
        return _f12_coeffs(a) == _f12_coeffs(b)

    def toBytes(self, a):
        """tower.ts:995-998: the 12 coefficients in tower order, 48 bytes big-endian each"""
        return b"".join(c.to_bytes(48, "big") for c in _f12_coeffs(a))

    def fromBytes(self, b):
        b = bytes(b)
        if len(b) != self.BYTES:
            raise ValueError("fromBytes invalid length=%d" % len(b))
        c = [int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(12)]
        if any(v >= _P for v in c):
            raise ValueError("invalid field element: out of range")
        two = [(c[2 * i], c[2 * i + 1]) for i in range(6)]
        return (tuple(two[:3]), tuple(two[3:]))


Fp12 = _Fp12()


# ---------------------------------------------------------------- pairings
def _check_pairs(pairs):
    if not isinstance(pairs, (list, tuple)):
        raise TypeError('"pairs" expected Array')
    out = []
    for i, pair in enumerate(pairs):
        if isinstance(pair, dict):
            if "g1" not in pair or "g2" not in pair:
                raise TypeError('"pairs[%d]" expected object with g1 and g2' % i)
            g1, g2 = pair["g1"], pair["g2"]
        else:
            g1, g2 = pair
        if not isinstance(g1, G1Point):
            raise TypeError('"pairs[%d].g1" expected G1 point, got type=%s' % (i, type(g1).__name__))
        if not isinstance(g2, G2Point):
            raise TypeError('"pairs[%d].g2" expected G2 point, got type=%s' % (i, type(g2).__name__))
        if g1.is0() or g2.is0():                              # bls.ts:685
            raise ValueError(ZERO_MSG)
        out.append((g1, g2))
    return out


def _on_curve_g1(pt):
    return (pt.y * pt.y - pt.x * pt.x * pt.x - 4) % _P == 0


def _on_curve_g2(pt):
    (x0, x1), (y0, y1) = pt.x, pt.y
    s0, s1 = x0 * x0 - x1 * x1, 2 * x0 * x1                  # x^2, then x^3 + 4 (1 + u)
    return ((y0 * y0 - y1 * y1) - (s0 * x0 - s1 * x1) - 4) % _P == 0 and (2 * y0 * y1 - (s0 * x1 + s1 * x0) - 4) % _P == 0


def _run_pairing(pairs, offsets, engine, check_subgroup=True):
    eng = engine or get_engine()
    if check_subgroup and pairs:                              # assertValidity (bls.ts:687-688) in the reference's order: the curve
        for g1, g2 in pairs:                                  # equation first (weierstrass.ts:748-766; the device checks it again), then
            if not (_on_curve_g1(g1) and _on_curve_g2(g2)):   # the torsion test, a batch multiply
                raise ValueError("bad point: equation left != right")
        for c, pts in ((G1Point, [p for p, _ in pairs]), (G2Point, [q for _, q in pairs])):
            if not all(_curve.isTorsionFreeBatch(c, pts, eng)):
                raise ValueError("bad point: not in prime-order subgroup")
    g1 = np.frombuffer(b"".join(p._wire() for p, _ in pairs), dtype=np.uint8)
    g2 = np.frombuffer(b"".join(q._wire() for _, q in pairs), dtype=np.uint8)
    try:
        gt, one = eng.pairing_batch(g1, g2, offsets)
    except _native.NativeError as e:
        if getattr(e, "bad_index", -1) >= 0:                  # the reference's own text, without the engine's prefix and position
            for ref in (ZERO_MSG, "bad point: equation left != right", "bad point: not in prime-order subgroup"):
                if ref in str(e):
                    raise ValueError(ref)
        raise
    return [_f12_from_wire(gt[i]) for i in range(len(offsets) - 1)], [bool(v) for v in one]


def pairingBatch(pairs, groups=None, engine=None):
    """bls.pairingBatch(pairs) (bls.ts:670-693): finalExponentiate of the product of the Miller values.  pairs: [(g1, g2)] or
    [{"g1": .., "g2": ..}].  groups: a list of group sizes summing to len(pairs) - then the list of the groups' products,
    one launch for all of them (an empty group gives Fp12.ONE)."""
    pairs = _check_pairs(pairs)
    if groups is None:
        if not pairs:
            return Fp12.ONE                                   # millerLoopBatch of no pairs (bls.ts:652-653)
        return _run_pairing(pairs, [0, len(pairs)], engine)[0][0]
    sizes = [int(s) for s in groups]
    if any(s < 0 for s in sizes) or sum(sizes) != len(pairs):
        raise ValueError("group sizes must be non-negative and sum to the number of pairs")
    if not sizes:
        return []
    return _run_pairing(pairs, np.concatenate([[0], np.cumsum(sizes)]), engine)[0]


def pairing(g1, g2, engine=None):
    """bls.pairing(Q, P) (bls.ts:695-699)"""
    if not isinstance(g1, G1Point):
        raise TypeError('"Q" expected G1 point, got type=%s' % type(g1).__name__)
    if not isinstance(g2, G2Point):
        raise TypeError('"P" expected G2 point, got type=%s' % type(g2).__name__)
    return pairingBatch([(g1, g2)], engine=engine)


def pairingRows(pairs, engine=None):
    """[pairing(g1, g2) for g1, g2 in pairs] in one launch"""
    return pairingBatch(pairs, [1] * len(pairs), engine)


# ---------------------------------------------------------------- signatures (verification side)
def _a_non_empty(arr):
    if not isinstance(arr, (list, tuple)) or len(arr) == 0:
        raise ValueError("expected non-empty array")


class _Signatures:
    """bls.longSignatures (keys in G1, signatures in G2) / bls.shortSignatures (the other way round), bls.ts:700-900: the
    verifying half.  Keys and signatures are points or their compressed encodings, messages are points of the signature
    group (`hash`)."""

    def __init__(self, short):
        self.short = short
        self.PubPoint, self.SigPoint = (G2Point, G1Point) if short else (G1Point, G2Point)
        self.hasher = _h2c.bls12_381_G1_hasher if short else _h2c.bls12_381_G2_hasher

    def hash(self, message, DST=None):
        """hashToCurve with the suite's default DST (bls.ts:720-728)"""
        return self.hasher.hashToCurve(message, {"DST": DST} if DST is not None else None)

    def hashBatch(self, messages, DST=None):
        return self.hasher.hashToCurveBatch(list(messages), {"DST": DST} if DST is not None else None)

    def verifyMessagesBatch(self, items, DST=None, engine=None):
        """[verify(signature, hash(message), publicKey)] for rows of BYTES (signature, message, publicKey) in ONE native call
        (ncg_bls_verify_batch): decoding with the subgroup tests, the map to the curve, the pairings and the comparison with ONE run
        on the device; only hash_to_field (SHA-256) runs here.  False where the reference returns false or its fromBytes throws."""
        rows = [tuple(bytes.fromhex(v) if isinstance(v, str) else bytes(v) for v in it) for it in items]
        if not rows:
            return []
        pw, sw = (96, 48) if self.short else (48, 96)
        verdict, good = [False] * len(rows), [i for i, r in enumerate(rows) if len(r[0]) == sw and len(r[2]) == pw]
        if not good:
            return verdict
        o = self.hasher._opts({"DST": DST} if DST is not None else None)
        u = b"".join(int(c).to_bytes(48, "little") for i in good for e in _h2c.hash_to_field(rows[i][1], 2, o) for c in e)
        ok = (engine or get_engine()).bls_verify_batch(1 if self.short else 0, np.frombuffer(b"".join(rows[i][2] for i in good), dtype=np.uint8),
                                                        np.frombuffer(b"".join(rows[i][0] for i in good), dtype=np.uint8),
                                                        np.frombuffer(u, dtype=np.uint8))
        for k, i in enumerate(good):
            verdict[i] = bool(ok[k])
        return verdict

    def _norm(self, cls, items, what, engine):
        """points as they are, encodings through the batch decoder (with its subgroup test); None where fromBytes throws"""
        out, enc, at = list(items), [], []
        for i, v in enumerate(out):
            if isinstance(v, cls):
                continue
            if isinstance(v, str):
                v = bytes.fromhex(v)
            if not isinstance(v, (bytes, bytearray, memoryview)):
                raise TypeError('"%s" expected point or Uint8Array, got type=%s' % (what, type(v).__name__))
            if len(bytes(v)) != (96 if cls is G2Point else 48):
                out[i] = None
                continue
            enc.append(bytes(v))
            at.append(i)
        for i, p in zip(at, _curve.fromBytesBatch(cls, enc, engine=engine) if enc else []):
            out[i] = p
        return out

    def _amsg(self, m):
        if not isinstance(m, self.SigPoint):
            raise ValueError("expected valid message hashed to %s curve" % ("G1" if self.short else "G2"))
        return m

    def _pair(self, pub, sig):
        return (sig, pub) if self.short else (pub, sig)

    def verifyRows(self, items, engine=None):
        """[verify(signature, message, publicKey) for each (signature, message, publicKey)] with one decode per group, one pairing
        launch of groups of two: e(-pk, H(m)) e(G, sig) = 1 (bls.ts:795-818).  False wherever the reference returns false or its
        fromBytes throws: undecodable, ZERO or out-of-subgroup key or signature."""
        items = [tuple(it) for it in items]
        if not items:
            return []
        msgs = [self._amsg(it[1]) for it in items]
        sigs = self._norm(self.SigPoint, [it[0] for it in items], "signature", engine)
        pubs = self._norm(self.PubPoint, [it[2] for it in items], "publicKey", engine)
        eng = engine or get_engine()
        live = [i for i in range(len(items)) if sigs[i] is not None and pubs[i] is not None
                and not (sigs[i].is0() or pubs[i].is0() or msgs[i].is0())]
        # assertValidity of pairingBatch: only points handed in as OBJECTS are not known to lie in the subgroups (what the decoder
        # returned is); messages are objects always
        for cls, col, given in ((self.SigPoint, sigs, [it[0] for it in items]), (self.SigPoint, msgs, msgs),
                                (self.PubPoint, pubs, [it[2] for it in items])):
            idx = [i for i in live if isinstance(given[i], cls)]
            tf = _curve.isTorsionFreeBatch(cls, [col[i] for i in idx], eng) if idx else []
            bad = {i for i, ok in zip(idx, tf) if not ok}
            live = [i for i in live if i not in bad]
        verdict = [False] * len(items)
        if not live:
            return verdict
        pairs = []
        for i in live:
            pairs.append(self._pair(pubs[i].negate(), msgs[i]))
            pairs.append(self._pair(self.PubPoint.BASE, sigs[i]))
        try:
            _, one = _run_pairing(pairs, np.arange(0, 2 * len(live) + 1, 2), eng, check_subgroup=False)
        except ValueError:                                    # a point off its curve: the reference's verify catches and says false
            return [self.verifyRows([items[i]], eng)[0] if len(items) > 1 else False for i in range(len(items))]
        for k, i in enumerate(live):
            verdict[i] = one[k]
        return verdict

    def verify(self, signature, message, publicKey, engine=None):
        return self.verifyRows([(signature, message, publicKey)], engine)[0]

    def verifyBatch(self, signature, items, engine=None):
        """bls.ts:822-854: keys grouped by message (the same object, as in the reference), one product of pairings"""
        _a_non_empty(items)
        rows = [(it["message"], it["publicKey"]) if isinstance(it, dict) else tuple(it) for it in items]
        msgs = [self._amsg(m) for m, _ in rows]
        sig = self._norm(self.SigPoint, [signature], "signature", engine)[0]
        pubs = self._norm(self.PubPoint, [k for _, k in rows], "publicKey", engine)
        if sig is None or any(p is None for p in pubs):
            return False
        groups = {}
        for m, p in zip(msgs, pubs):
            groups.setdefault(id(m), (m, []))[1].append(p)
        try:
            pairs = []
            for m, keys in groups.values():
                pairs.append(self._pair(keys[0] if len(keys) == 1 else _curve.sumPoints(self.PubPoint, keys, engine), m))
            pairs.append(self._pair(self.PubPoint.BASE.negate(), sig))
            return Fp12.eql(pairingBatch(pairs, engine=engine), Fp12.ONE)
        except ValueError:
            return False

    def aggregatePublicKeys(self, publicKeys, engine=None):
        return self._aggregate(self.PubPoint, publicKeys, engine)

    def aggregateSignatures(self, signatures, engine=None):
        return self._aggregate(self.SigPoint, signatures, engine)

    def _aggregate(self, cls, items, engine):
        _a_non_empty(items)
        if all(isinstance(v, (bytes, bytearray, memoryview)) for v in items):
            return _curve.aggregateFromBytes(cls, items, engine=engine)
        pts = self._norm(cls, items, "point", engine)
        if any(p is None for p in pts):
            raise ValueError("invalid point encoding")
        return _curve.sumPoints(cls, pts, engine)


longSignatures = _Signatures(short=False)
shortSignatures = _Signatures(short=True)
