"""Host mirror of the reference's FFT and poly interfaces for the bls12-381 and bn254 scalar fields
(src/abstract/fft.ts): `rootsOfUnity(Fr, 7)` / `FFT(roots, Fr).direct|inverse(values, brpInput,
brpOutput)` with the same names, argument meaning and error messages; the transform itself runs in
`libncg.so` (`ncg_ntt`, field NCG_FIELD_BLS12_381_FR or NCG_FIELD_BN254_FR by the ORDER of the field).  The host side only does what the reference does once per field: the
2-adic chain of primitive roots (:238-241) - a handful of modular exponentiations.
`poly(Fr, roots, create, fft, length)` (:583-926) keeps the reference's names and messages too; its vector work runs in
`ncg_poly_*`, only create / degree / extend / clone / vanishing stay on the host.
"""
import numpy as np

from . import _native
from ._native import get_engine

BLS12_381_FR_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


BN254_FR_ORDER = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


class _Fr:
    """The slice of IField (src/abstract/modular.ts:429-607) the FFT front end touches."""
    BYTES = 32
    ONE = 1
    ZERO = 0

    def __init__(self, order):
        self.ORDER = order
        self.BITS = order.bit_length()

    def pow(self, a, e):
        return pow(a, e, self.ORDER)


bls12_381_Fr = _Fr(BLS12_381_FR_ORDER)
bn254_Fr = _Fr(BN254_FR_ORDER)
# ORDER -> field id of ncg_ntt (include/ncg.h)
_DEVICE_FIELDS = {BLS12_381_FR_ORDER: _native.FIELD_BLS12_381_FR, BN254_FR_ORDER: _native.FIELD_BN254_FR}


def isPowerOfTwo(x):                       # fft.ts:56-59
    return isinstance(x, int) and x > 0 and (x & (x - 1)) == 0


def nextPowerOfTwo(n):                     # fft.ts:72-76
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def log2(n):                               # fft.ts:116-119
    return n.bit_length() - 1


def reverseBits(n, bits):                  # fft.ts:93-99
    r = 0
    for _ in range(bits):
        r = (r << 1) | (n & 1)
        n >>= 1
    return r


def bitReversalPermutation(values):        # fft.ts:136-171 (copying form)
    n = len(values)
    if n < 2 or not isPowerOfTwo(n):
        raise ValueError("n must be a power of 2 and greater than 1. Got " + str(n))
    bits = log2(n)
    return [values[reverseBits(i, bits)] for i in range(n)]


class RootsOfUnity:
    """fft.ts:230-312 for a field whose ORDER matches a device field (bls12-381 Fr, bn254 Fr)."""

    def __init__(self, field, generator=None):
        if getattr(field, "ORDER", None) not in _DEVICE_FIELDS:
            raise ValueError("noble-gpu: the device NTT is built for the bls12-381 and bn254 scalar fields only")
        if generator is not None and (not isinstance(generator, int) or isinstance(generator, bool)):
            raise TypeError('"generator" expected bigint, got type=' + type(generator).__name__)
        odd, p2 = field.ORDER - 1, 0
        while odd & 1 == 0:
            odd >>= 1
            p2 += 1
        if generator is None:              # findGenerator :175-180
            generator = 2
            while pow(generator, field.ORDER >> 1, field.ORDER) == 1:
                generator += 1
        self.field = field
        self.info = {"G": generator, "oddFactor": odd, "powerOfTwo": p2}
        self._omegas = [0] * (p2 + 1)
        self._omegas[p2] = pow(generator, odd, field.ORDER)
        for i in range(p2, 0, -1):
            self._omegas[i - 1] = self._omegas[i] * self._omegas[i] % field.ORDER
        self._cache = {}

    def _check(self, bits):
        if not isinstance(bits, int) or isinstance(bits, bool) or bits < 0:
            raise ValueError("wrong u32 integer: bits")
        if bits > 31 or bits > self.info["powerOfTwo"]:
            raise ValueError("rootsOfUnity: wrong bits %d powerOfTwo=%d" % (bits, self.info["powerOfTwo"]))
        return bits

    def omega(self, bits):
        return self._omegas[self._check(bits)]

    def roots(self, bits):
        """Natural-order table; served by the device as the forward transform of the delta at 1."""
        self._check(bits)
        if bits not in self._cache:
            n = 1 << bits
            delta = [0] * n
            if n > 1:
                delta[1] = 1
                self._cache[bits] = FFT(self, self.field).direct(delta)
            else:
                self._cache[bits] = [1]
        return self._cache[bits]

    def brp(self, bits):
        r = self.roots(bits)
        return bitReversalPermutation(r) if bits else list(r)

    def inverse(self, bits):               # fft.ts:296-304
        r = self.roots(bits)
        return [r[0]] + r[1:][::-1]

    def clear(self):
        self._cache = {}


def rootsOfUnity(field, generator=None):
    return RootsOfUnity(field, generator)


class FFT:
    """fft.ts:518-577.  `values`: list of ints in [0, r) (or a uint8 array [N, 32], little-endian
    canonical residues, returned in kind)."""

    def __init__(self, roots, opts=None, engine=None):
        if not isinstance(roots, RootsOfUnity):
            raise TypeError("noble-gpu: FFT expects the RootsOfUnity returned by rootsOfUnity()")
        self.roots = roots
        self._engine = engine

    def _run(self, values, inverse, brpInput, brpOutput):
        raw = isinstance(values, np.ndarray)
        N = values.shape[0] if raw else len(values)
        if not isPowerOfTwo(N):
            raise ValueError("FFT: Polynomial size should be power of two")
        bits = log2(N)
        order = self.roots.field.ORDER
        if raw:
            data = np.ascontiguousarray(values, dtype=np.uint8).reshape(N, 32)
        else:
            for v in values:
                if not isinstance(v, int) or isinstance(v, bool) or not (0 <= v < order):
                    raise ValueError("invalid field element: outside of range 0..ORDER")
            data = _native.ints_to_le(values, 32)
        eng = self._engine or get_engine()
        out = eng.ntt(bits, data, self.roots.omega(bits), inverse=inverse, brp_input=brpInput, brp_output=brpOutput,
                      field=_DEVICE_FIELDS[order])
        return out if raw else _native.le_to_ints(out, 32)

    def direct(self, values, brpInput=False, brpOutput=False):
        return self._run(values, False, bool(brpInput), bool(brpOutput))

    def inverse(self, values, brpInput=False, brpOutput=False):
        return self._run(values, True, bool(brpInput), bool(brpOutput))


# ---------------------------------------------------------------- poly (fft.ts:583-926)
def _js_typeof(v):
    """the word the reference's messages print for a value of this kind (`typeof`)"""
    if v is None:
        return "undefined"
    if isinstance(v, bool):
        return "boolean"
    if isinstance(v, int):
        return "bigint"
    if isinstance(v, float):
        return "number"
    if isinstance(v, str):
        return "string"
    if callable(v):
        return "function"
    return "object"


class _PolyGroup:
    """a namespace of functions (`monomial`, `lagrange`)"""

    def __init__(self, **fns):
        self.__dict__.update(fns)


class Poly:
    """fft.ts:710-926 for the two device fields.  Polynomials are lists of ints in [0, r) or uint8 arrays [N, 32] (little-endian
    canonical residues), returned in kind; with a `create` of the caller's, list results are copied into create(len)."""

    def __init__(self, field, roots, create=None, fft=None, length=None, engine=None):
        if getattr(field, "ORDER", None) not in _DEVICE_FIELDS:
            raise ValueError("noble-gpu: the device poly is built for the bls12-381 and bn254 scalar fields only")
        if not isinstance(roots, RootsOfUnity):
            raise TypeError("noble-gpu: poly expects the RootsOfUnity returned by rootsOfUnity()")
        self.field = field
        self.roots = roots
        self._own_create = create
        self.create = create or (lambda n, elm=None: [field.ZERO if elm is None else elm] * n)
        self.fft = fft
        self.length = length
        self._engine = engine
        self._fid = _DEVICE_FIELDS[field.ORDER]
        self.monomial = _PolyGroup(basis=self._monomial_basis, eval=self._monomial_eval)
        self.lagrange = _PolyGroup(basis=self._lagrange_basis, eval=self._lagrange_eval)

    # ---- argument handling: the reference's checks and messages, raised before the engine is touched
    @staticmethod
    def _is_poly(x):
        return isinstance(x, (list, tuple)) or (isinstance(x, np.ndarray) and x.ndim >= 1)

    def _check_poly(self, title, value):
        if not self._is_poly(value):
            raise TypeError('"%s" expected polynomial, got type=%s' % (title, _js_typeof(value)))

    @staticmethod
    def _len(p):
        return p.shape[0] if isinstance(p, np.ndarray) else len(p)

    def _check_fixed(self, L):
        if self.length is not None and L != self.length:
            raise ValueError("poly: expected fixed length %d, got %d" % (self.length, L))

    def _check_length(self, a, b=None):
        self._check_poly("a", a)
        L = self._len(a)
        if b is not None:
            self._check_poly("b", b)
            if self._len(b) != L:
                raise ValueError("poly: mismatched lengths %d vs %d" % (L, self._len(b)))
        self._check_fixed(L)
        return L

    def _elem(self, v):
        if not isinstance(v, int) or isinstance(v, bool) or not (0 <= v < self.field.ORDER):
            raise ValueError("invalid field element: outside of range 0..ORDER")
        return v

    def _wire(self, p):
        if isinstance(p, np.ndarray):
            return np.ascontiguousarray(p, dtype=np.uint8).reshape(-1, 32)
        return _native.ints_to_le([self._elem(v) for v in p], 32)

    def _ints(self, p):
        return _native.le_to_ints(p, 32) if isinstance(p, np.ndarray) else list(p)

    def _back(self, data, like):
        if isinstance(like, np.ndarray):
            return data
        vals = _native.le_to_ints(data, 32)
        if self._own_create is None:
            return vals
        out = self._own_create(len(vals))
        for i, v in enumerate(vals):
            out[i] = v
        return out

    def _eng(self):
        return self._engine or get_engine()

    @staticmethod
    def _pow2(n, what="poly.lagrange"):
        if not isPowerOfTwo(n):
            raise ValueError("%s: expected power of two length, got %s" % (what, n))
        return log2(n)

    # ---- host side
    def extend(self, a, n):                                   # :776-783
        self._check_length(a)
        out = self.create(n, self.field.ZERO)
        vals = self._ints(a)
        for i in range(min(len(vals), n)):
            out[i] = vals[i]
        return out

    def degree(self, a):                                      # :784-788
        self._check_length(a)
        vals = self._ints(a)
        for i in range(len(vals) - 1, -1, -1):
            if vals[i] != 0:
                return i
        return -1

    def clone(self, a):                                       # :851-856
        self._check_length(a)
        if isinstance(a, np.ndarray):
            return a.copy()
        out = self.create(len(a))
        for i, v in enumerate(a):
            out[i] = v
        return out

    def vanishing(self, roots):                               # :912-924
        self._check_poly("roots", roots)
        rs = self._ints(roots)
        self._check_fixed(len(rs))
        r = self.field.ORDER
        out = self.create(len(rs) + 1, self.field.ZERO)
        out[0] = self.field.ONE
        for root in rs:
            neg = (r - self._elem(root)) % r
            for j in range(len(rs), 0, -1):
                out[j] = (out[j] * neg + out[j - 1]) % r
            out[0] = out[0] * neg % r
        return out

    # ---- device side
    def _pointwise(self, op, a, b):
        L = self._check_length(a, b)
        A, B = self._wire(a), self._wire(b)
        if L == 0:
            return self._back(A, a)
        return self._back(self._eng().poly_pointwise(op, A, B, field=self._fid), a)

    def add(self, a, b):                                      # :789-794
        return self._pointwise(_native.POLY_ADD, a, b)

    def sub(self, a, b):                                      # :795-800
        return self._pointwise(_native.POLY_SUB, a, b)

    def dot(self, a, b):                                      # :801-806
        return self._pointwise(_native.POLY_DOT, a, b)

    def _cyclic(self, bits, A, B):
        return self._eng().poly_mul(bits, self.roots.omega(bits), A, B, field=self._fid)

    def mul(self, a, b):                                      # :807-831
        if not self._is_poly(b):
            L = self._check_length(a)
            A = self._wire(a)
            s = self._elem(b)
            return self._back(self._eng().poly_scale(A, s, field=self._fid) if L else A, a)
        L = self._check_length(a, b)
        if L and not isPowerOfTwo(L) and self.fft is not None:
            return self.fft.inverse(self.fft.direct(a, False, True), True, False)   # raises the FFT's power-of-two error
        A, B = self._wire(a), self._wire(b)
        if L == 0:
            return self._back(A, a)
        if isPowerOfTwo(L):
            return self._back(self._cyclic(log2(L), A, B), a)
        # the quadratic product mod x^L - 1 (:816-824): the linear product, folded once
        full = self._cyclic(log2(nextPowerOfTwo(2 * L - 1)), A, B)
        return self._back(self._eng().poly_pointwise(_native.POLY_ADD, full[:L], full[L:2 * L], field=self._fid), a)

    def convolve(self, a, b):                                 # :832-837
        self._check_poly("a", a)
        self._check_poly("b", b)
        n = nextPowerOfTwo(self._len(a) + self._len(b) - 1)
        self._check_fixed(self._len(a))
        self._check_fixed(self._len(b))
        self._check_fixed(n)
        A, B = self._wire(a), self._wire(b)
        return self._back(self._cyclic(log2(n), A, B), a)

    def shift(self, p, factor):                               # :838-850
        self._check_poly("p", p)
        self._check_fixed(self._len(p))
        P = self._wire(p)
        f = self._elem(factor)
        return self._back(self._eng().poly_scale(P, f, powers=True, field=self._fid) if self._len(p) else P, p)

    def eval(self, a, basis):                                 # :857-862
        self._check_length(a, basis)
        A, B = self._wire(a), self._wire(basis)
        return self._eng().poly_eval(A, B, field=self._fid)

    def _monomial_basis(self, x, n):                          # :864-872
        ones = _native.ints_to_le([self.field.ONE] * n, 32)
        x = self._elem(x)
        return self._back(self._eng().poly_scale(ones, x, powers=True, field=self._fid) if n else ones, None)

    def _monomial_eval(self, a, x):                           # :873-879
        self._check_length(a)
        A, x = self._wire(a), self._elem(x)
        return self._eng().poly_eval_monomial(A, [x], field=self._fid)[0]

    def _find_omega_index(self, x, n, brp=False):             # :764-770
        bits = self._pow2(n)
        if pow(x, n, self.field.ORDER) != 1:
            return -1
        table = self.roots.brp(bits) if brp else self.roots.roots(bits)
        return table.index(x)

    def _lagrange_basis(self, x, n, brp=False):               # :882-901
        bits = self._pow2(n)
        x = self._elem(x)
        out = self._eng().poly_lagrange_basis(bits, self.roots.omega(bits), x, brp=bool(brp), field=self._fid)
        return self._back(out, None)

    def _lagrange_eval(self, a, x, brp=False):                # :902-910
        L = self._check_length(a)
        self._pow2(L)
        A = self._wire(a)
        idx = self._find_omega_index(self._elem(x), L, bool(brp))
        if idx != -1:
            return _native.le_to_ints(A[idx:idx + 1], 32)[0]
        bits = log2(L)
        basis = self._eng().poly_lagrange_basis(bits, self.roots.omega(bits), x, brp=bool(brp), field=self._fid)
        return self._eng().poly_eval(A, basis, field=self._fid)


def poly(field, roots, create=None, fft=None, length=None, engine=None):
    return Poly(field, roots, create, fft, length, engine)
