"""The argument checks of every buffer-taking entry point of the C ABI, host and _dev forms, as one table; and every
staged host-pointer wrapper against its _dev form, bit for bit.

The table is safe to run on a shared GPU whatever the library under test does: every non-NULL pointer of a _dev row is a
zeroed 4 KB device buffer (host rows: a 4 KB host buffer) and n = 1, so a check that went missing runs on valid memory and
fails the test instead of faulting; the message buffer of a _dev form is never NULL while an offset is non-zero."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from helpers import load_golden
from noble_curves_amd import get_engine
from noble_curves_amd._native import BLS12_381_G1, BLS12_381_G2, BN254_G1, ED25519, POINT_BYTES, SECP256K1

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -4
S, G1, G2, BN = SECP256K1, BLS12_381_G1, BLS12_381_G2, BN254_G1
ENC = {SECP256K1: 33, ED25519: 32, BLS12_381_G1: 48, BLS12_381_G2: 96}
BLS_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

# Argument templates: C curve, F field, N batch size, P resident set; B a buffer the form requires (a host buffer in host
# forms, a device buffer in _dev forms), h a host pointer the form requires, b / o an optional host or (b in _dev forms)
# device output, M / m the message buffer of a _dev / host form (never set to NULL by the table), S the stream, digits
# literal ints.  Each entry: function, template, curve or field of the valid rows, refused curves or fields besides the
# unassigned ones, substring of that refusal.
UNSUP = "unsupported curve %d"
SPECS = [
    ("ncg_mul_var_batch", "C N B B B b", S, [], UNSUP),
    ("ncg_mul_var_batch_dev", "C N B B B B S", S, [], UNSUP),
    ("ncg_add_pairs_batch", "C N B B 0 B b", S, [], UNSUP),
    ("ncg_add_pairs_batch_dev", "C N B B 0 B B S", S, [], UNSUP),
    ("ncg_mul_base_batch", "C N B B b", S, [BN], UNSUP),
    ("ncg_mul_base_batch_dev", "C N B B B S", S, [BN], UNSUP),
    ("ncg_msm", "C N B B B o", S, [], UNSUP),
    ("ncg_msm_dev", "C N B B h o S", S, [], UNSUP),
    ("ncg_normalize_batch", "C N B B b", S, [], UNSUP),
    ("ncg_normalize_batch_dev", "C N B B B S", S, [], UNSUP),
    ("ncg_decode_points_batch", "C N B 0 B B b", S, [BN], UNSUP),
    ("ncg_decode_points_batch_dev", "C N B 0 B B B S", S, [BN], UNSUP),
    ("ncg_encode_points_batch", "C N B B B", S, [BN], UNSUP),
    ("ncg_encode_points_batch_dev", "C N B B B S", S, [BN], UNSUP),
    ("ncg_map_to_curve_batch", "C N 1 B B b", G1, [S, BN], UNSUP),
    ("ncg_map_to_curve_batch_dev", "C N 1 B B B S", G1, [S, BN], UNSUP),
    ("ncg_aggregate_encoded", "C N B 0 B o o", G1, [BN], UNSUP),
    ("ncg_ecdsa_verify_batch", "C N B B B 0 B", S, [G1, BN], "secp256k1 only"),
    ("ncg_ecdsa_verify_batch_dev", "C N B B B 0 B S", S, [G1, BN], "secp256k1 only"),
    ("ncg_ecdsa_recover_batch", "C N B B B B", S, [G1, BN], "secp256k1 only"),
    ("ncg_ecdsa_recover_batch_dev", "C N B B B B S", S, [G1, BN], "secp256k1 only"),
    ("ncg_ecdsa_verify_batch_msgs", "C N B m B B 0 B", S, [G1, BN], "secp256k1 only"),
    ("ncg_ecdsa_verify_batch_msgs_dev", "C N B M B B 0 B S", S, [G1, BN], "secp256k1 only"),
    ("ncg_ed25519_verify_batch", "N B B B 1 B", None, [], None),
    ("ncg_ed25519_verify_batch_dev", "N B B B 1 B S", None, [], None),
    ("ncg_ed25519_challenge_batch_dev", "N B B M B B S", None, [], None),
    ("ncg_ed25519_verify_batch_msgs", "N B B m B 1 B", None, [], None),
    ("ncg_ed25519_verify_batch_msgs_dev", "N B B M B 1 B S", None, [], None),
    ("ncg_schnorr_verify_batch", "N B B B B", None, [], None),
    ("ncg_schnorr_verify_batch_dev", "N B B B B S", None, [], None),
    ("ncg_schnorr_verify_batch_msgs", "N B m B B B", None, [], None),
    ("ncg_schnorr_verify_batch_msgs_dev", "N B M B B B S", None, [], None),
    ("ncg_ntt", "F 3 N h B B 0", 0, [1, 2], "unsupported field %d"),
    ("ncg_ntt_dev", "F 3 N h B B 0 S", 0, [1, 2], "unsupported field %d"),
    ("ncg_field_check", "F 0 0 N B B B", 0, [-1, 15], "unknown field %d"),
    ("ncg_msm_resident", "P B B o", None, [], None),
    ("ncg_msm_resident_dev", "P B h o S", None, [], None),
    ("ncg_mul_var_batch_resident", "P B B b", None, [], None),
    ("ncg_mul_var_batch_resident_dev", "P B B B S", None, [], None),
]
MSM_FAMILY = ("ncg_msm", "ncg_msm_dev", "ncg_aggregate_encoded", "ncg_msm_resident", "ncg_msm_resident_dev")
# the host forms that used to stage a whole batch before the _dev form refused its size
STAGING_HOST_FORMS = ("ncg_mul_var_batch", "ncg_add_pairs_batch", "ncg_mul_base_batch", "ncg_normalize_batch",
                      "ncg_decode_points_batch", "ncg_encode_points_batch", "ncg_map_to_curve_batch", "ncg_ed25519_verify_batch")


def _err(L, h):
    return (L.ncg_last_error(h) or b"").decode()


def _args(tmpl, dev, H, D, sel=None, over=None):
    """The argument list of a template: every slot real unless `over` names it (index -> value)."""
    over = over or {}
    out = []
    for i, t in enumerate(tmpl.split()):
        if i in over:
            out.append(over[i])
        elif t in "CF":
            out.append(sel)
        elif t == "N":
            out.append(1)
        elif t in "BM":
            out.append(D if dev else H)
        elif t == "b":
            out.append(D if dev else H)
        elif t == "o":   # (typed: some prototypes declare it uint8_t*)
            out.append(ctypes.cast(ctypes.c_void_p(H), ctypes.POINTER(ctypes.c_uint8)) if H else None)
        elif t in "hm":
            out.append(H)
        elif t == "S":
            out.append(None)
        elif t == "P":
            out.append(sel)
        else:
            out.append(int(t))
    return out


def _rows(L, h, H, D, handles):
    """(label, call, expected status, expected message substring or None)"""
    rows = []
    for fn, tmpl, sel, refused, refusal in SPECS:
        f = getattr(L, fn)
        dev = fn.endswith("_dev")
        toks = tmpl.split()
        resident = "P" in toks
        if resident:
            sel = handles["one"]

        def row(label, status, sub, ctx=h, over=None):
            a = _args(tmpl, dev, H, D, sel, over)
            rows.append(("%s %s" % (fn, label), lambda f=f, a=a, ctx=ctx: f(ctx, *a), status, sub))

        row("NULL ctx", INVALID, None, ctx=None)
        if "C" in toks or "F" in toks:
            k = toks.index("C" if "C" in toks else "F")
            for bad in ([4, 9] if "C" in toks else []) + refused:
                row("refuses %d" % bad, UNSUPPORTED, refusal % bad if "%d" in refusal else refusal, over={k: bad})
        if "N" in toks:
            nulls = {i: None for i, t in enumerate(toks) if t in "BbhomM"}
            empty = (INVALID, "NULL output") if fn in MSM_FAMILY else (OK, None)
            row("n = 0, every buffer NULL", *empty, over={toks.index("N"): 0, **nulls})
        if resident:
            nulls = {i: None for i, t in enumerate(toks) if t in "Bbho"}
            empty = (INVALID, "NULL output") if fn in MSM_FAMILY else (OK, None)
            row("empty set, every buffer NULL", *empty, over={0: handles["empty"], **nulls})
            row("NULL handle", INVALID, "handle does not belong to this context", over={0: None})
            row("foreign handle", INVALID, "handle does not belong to this context", over={0: handles["foreign"]})
        for i, t in enumerate(toks):
            if t == "B":   # (ncg_field_check has always said "bad arguments" for every argument fault)
                row("arg %d NULL" % i, INVALID, "field_check" if fn == "ncg_field_check" else "NULL buffer", over={i: None})
            elif t == "h":
                row("arg %d NULL" % i, INVALID, "NULL", over={i: None})
    # the operations' own rules
    for fn in ("ncg_map_to_curve_batch", "ncg_map_to_curve_batch_dev"):
        dev = fn.endswith("_dev")
        for count in (0, 3):
            a = [G1, 1, count] + ([D, D, D, None] if dev else [H, H, H])
            rows.append(("%s count %d" % (fn, count), lambda f=getattr(L, fn), a=a: f(h, *a), INVALID, "count must be 1 or 2"))
    for fn in ("ncg_ntt", "ncg_ntt_dev"):
        dev = fn.endswith("_dev")
        tail = [H, D, D, 0, None] if dev else [H, H, H, 0]
        for log2n in (-1, 29):
            rows.append(("%s log2n %d" % (fn, log2n), lambda f=getattr(L, fn), a=[0, log2n, 1] + tail: f(h, *a), INVALID, "out of range"))
        # (batch 65536 is refused before any buffer is looked at: all NULL here)
        a = [0, 3, 65536, None, None, None, 0] + ([None] if dev else [])
        rows.append(("%s batch 65536" % fn, lambda f=getattr(L, fn), a=a: f(h, *a), INVALID, "too large"))
    rows.append(("ncg_field_check n 2^24 + 1", lambda: L.ncg_field_check(h, 0, 0, 0, (1 << 24) + 1, None, None, None), INVALID, None))
    bad_off = np.array([5, 3], dtype=np.uint64)
    gap_off = np.array([0, 4], dtype=np.uint64)
    hp = lambda x: x.ctypes.data
    for label, call in (
            ("ncg_ed25519_verify_batch_msgs", lambda o, m: L.ncg_ed25519_verify_batch_msgs(h, 1, H, H, m, hp(o), 1, H)),
            ("ncg_ecdsa_verify_batch_msgs", lambda o, m: L.ncg_ecdsa_verify_batch_msgs(h, S, 1, H, m, hp(o), H, 0, H)),
            ("ncg_schnorr_verify_batch_msgs", lambda o, m: L.ncg_schnorr_verify_batch_msgs(h, 1, H, m, hp(o), H, H))):
        rows.append((label + " decreasing offsets", lambda c=call: c(bad_off, H), INVALID, "offsets must not decrease"))
        rows.append((label + " NULL messages", lambda c=call: c(gap_off, None), INVALID, "NULL message buffer"))
    # the challenge hash takes no message buffer when every message is empty (offsets: zeroed device memory)
    rows.append(("ncg_ed25519_challenge_batch_dev NULL messages, empty messages",
                 lambda: L.ncg_ed25519_challenge_batch_dev(h, 1, D, D, None, D, D, None), OK, None))
    # the resident-set constructors
    out = ctypes.c_void_p()
    bad = ctypes.c_int64()
    rows += [
        ("ncg_points_upload NULL ctx", lambda: L.ncg_points_upload(None, S, 1, H, ctypes.byref(out)), INVALID, None),
        ("ncg_points_upload refuses 4", lambda: L.ncg_points_upload(h, 4, 1, H, ctypes.byref(out)), UNSUPPORTED, "unsupported curve 4"),
        ("ncg_points_upload NULL points", lambda: L.ncg_points_upload(h, S, 1, None, ctypes.byref(out)), INVALID, "NULL buffer"),
        ("ncg_points_from_encoded NULL ctx", lambda: L.ncg_points_from_encoded(None, S, 1, H, 0, ctypes.byref(out), ctypes.byref(bad)),
         INVALID, None),
        ("ncg_points_from_encoded refuses bn254", lambda: L.ncg_points_from_encoded(h, BN, 1, H, 0, ctypes.byref(out), ctypes.byref(bad)),
         UNSUPPORTED, "unsupported curve 5"),
        ("ncg_points_from_encoded NULL encodings", lambda: L.ncg_points_from_encoded(h, S, 1, None, 0, ctypes.byref(out), ctypes.byref(bad)),
         INVALID, "NULL buffer"),
        ("ncg_points_from_encoded NULL out", lambda: L.ncg_points_from_encoded(h, S, 1, H, 0, None, ctypes.byref(bad)), INVALID, None),
    ]
    return rows


def test_argument_checks_of_every_entry_point():
    eng = get_engine()
    L, h = eng.lib, eng.h
    hbuf = np.zeros(4096, dtype=np.uint8)
    dbuf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    H, D = hbuf.ctypes.data, dbuf.data_ptr()
    one, empty = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.ncg_points_upload(h, S, 1, H, ctypes.byref(one)) == OK
    assert L.ncg_points_upload(h, S, 0, None, ctypes.byref(empty)) == OK
    other = ctypes.c_void_p()
    assert L.ncg_init(0, ctypes.byref(other)) == OK
    foreign = ctypes.c_void_p()
    assert L.ncg_points_upload(other, S, 1, H, ctypes.byref(foreign)) == OK
    handles = {"one": one, "empty": empty, "foreign": foreign}
    try:
        failures = []
        rows = _rows(L, h, H, D, handles)
        for label, call, status, sub in rows:
            hbuf[:] = 0                   # (a call that succeeds writes its outputs there; offsets and inputs must read 0)
            dbuf.zero_()
            torch.cuda.synchronize()
            rc = call()
            msg = _err(L, h)
            assert L.ncg_sync(h) == OK
            if rc != status or (sub is not None and sub not in msg):
                failures.append("%s: got %d %r, want %d %r" % (label, rc, msg, status, sub))
        assert not failures, "\n".join(failures)
        assert len(rows) > 150
        assert L.ncg_sync(h) == OK
        # the table wrote nothing outside its buffers' first bytes, and the context still works
        k = np.zeros((1, 32), dtype=np.uint8)
        k[0, 0] = 1
        o, f = eng.mul_base_batch(SECP256K1, k)
        assert int.from_bytes(o[0, :32].tobytes(), "little") == 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
        assert not f[0]
    finally:
        L.ncg_points_free(foreign)
        L.ncg_destroy(other)
        L.ncg_points_free(one)
        L.ncg_points_free(empty)


def test_host_forms_reject_oversized_batches_before_staging():
    """n = 2^31 with every buffer NULL: refused for its size, before any buffer is looked at or staged."""
    eng = get_engine()
    L, h = eng.lib, eng.h
    for fn, tmpl, sel, _, _ in SPECS:
        if fn not in STAGING_HOST_FORMS:
            continue
        toks = tmpl.split()
        nulls = {i: None for i, t in enumerate(toks) if t in "Bbhom"}
        a = _args(tmpl, False, None, None, sel, {toks.index("N"): 1 << 31, **nulls})
        assert getattr(L, fn)(h, *a) == INVALID, fn
        assert "too large" in _err(L, h), (fn, _err(L, h))


# ---- host form == _dev form ------------------------------------------------------------------------------------------

def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _odd(a):
    """the same bytes at an odd host address"""
    raw = np.empty(a.nbytes + 1, np.uint8)
    raw[1:] = _bytes(a)
    return raw[1:]


def _dev(a):
    return torch.from_numpy(_bytes(a).copy()).to("cuda")


class _Run:
    def __init__(self, eng, seed):
        self.eng, self.L, self.h = eng, eng.lib, eng.h
        self.rng = np.random.default_rng(seed)

    def check(self, host_fn, dev_fn, ins, out_bytes, drop=()):
        """host_fn(*host inputs, *host outputs) and dev_fn(*device inputs, *device outputs) on the same bytes; every output
        the host form got (those in `drop` are NULL there) equals the _dev form's.  The first input sits at an odd address."""
        L, h = self.L, self.h
        hin = [_odd(ins[0])] + [_bytes(x) for x in ins[1:]]
        hout = [np.full(b, 0xA5, np.uint8) for b in out_bytes]
        din = [_dev(x) for x in ins]
        dout = [torch.full((b,), 0xA5, dtype=torch.uint8, device="cuda") for b in out_bytes]
        torch.cuda.synchronize()
        rc = host_fn(*[x.ctypes.data for x in hin], *[None if i in drop else o.ctypes.data for i, o in enumerate(hout)])
        assert rc == OK, _err(L, h)
        rc = dev_fn(*[t.data_ptr() for t in din], *[t.data_ptr() for t in dout])
        assert rc == OK, _err(L, h)
        assert L.ncg_sync(h) == OK
        for i, o in enumerate(hout):
            if i not in drop:
                assert o.tobytes() == dout[i].cpu().numpy().tobytes(), "output %d differs" % i
        return hout

    def scalars(self, n):
        k = self.rng.integers(0, 256, (n, 32), dtype=np.uint8)
        k[:, 31] &= 0x0F
        k[::7] = 0                       # infinity
        return k

    def points(self, curve, n, garbage=True):
        o, f = self.eng.mul_base_batch(curve, self.scalars(n))
        o = o.copy()
        if garbage:
            o[5::13] = self.rng.integers(0, 256, o[5::13].shape, dtype=np.uint8)   # off the curve
        return o

    def field(self, n, fb, top):
        x = self.rng.integers(0, 256, (n, fb), dtype=np.uint8)
        x[:, fb - 1] %= top
        return x


def _sizes(row_bytes):
    """a small n that is not a multiple of 256, and one whose largest host buffer reaches 1 MB (PinSet pins it)"""
    return (299, ((1 << 20) + row_bytes - 1) // row_bytes + 3)


def _case_add_pairs(r, L, h):
    for curve, sub in ((S, 0), (G2, 1)):
        pb = POINT_BYTES[curve]
        for n in _sizes(pb):
            a, b = r.points(curve, n), r.points(curve, n)
            b[::5] = a[::5]                                           # doublings
            drop = (1,) if n < 1000 else ()
            r.check(lambda a_, b_, o, f: L.ncg_add_pairs_batch(h, curve, n, a_, b_, sub, o, f),
                    lambda a_, b_, o, f: L.ncg_add_pairs_batch_dev(h, curve, n, a_, b_, sub, o, f, None), [a, b], [n * pb, n], drop)


def _case_mul_base(r, L, h):
    for curve in (S, G1):
        pb = POINT_BYTES[curve]
        for n in _sizes(pb):
            k = r.scalars(n)
            k[3::11] = 0xFF                                           # not below the order
            r.check(lambda k_, o, f: L.ncg_mul_base_batch(h, curve, n, k_, o, f),
                    lambda k_, o, f: L.ncg_mul_base_batch_dev(h, curve, n, k_, o, f, None), [k], [n * pb, n], (1,) if n < 1000 else ())


def _case_normalize(r, L, h):
    for curve in (S, G1):
        pb = POINT_BYTES[curve]
        fb = pb // 2
        for n in _sizes(pb * 3 // 2):
            p = r.points(curve, n)
            z = np.zeros((n, fb), np.uint8)
            z[:, :8] = r.rng.integers(0, 256, (n, 8), dtype=np.uint8)
            z[::9] = 0                                                # infinity
            proj = np.concatenate([p, z], axis=1)
            r.check(lambda i, o, f: L.ncg_normalize_batch(h, curve, n, i, o, f),
                    lambda i, o, f: L.ncg_normalize_batch_dev(h, curve, n, i, o, f, None), [proj], [n * pb, n], (1,) if n < 1000 else ())


def _encode(r, L, h, curve, pts, valid_only=False):
    """compressed encodings; valid_only: rows without one (the secp256k1 identity) repeat a row that has one"""
    n = pts.shape[0]
    enc = np.zeros((n, ENC[curve]), np.uint8)
    ok = np.zeros(n, np.uint8)
    assert L.ncg_encode_points_batch(h, curve, n, pts.ctypes.data, enc.ctypes.data, ok.ctypes.data) == OK
    if valid_only:
        enc[ok == 0] = enc[np.argmax(ok)]
    return enc


def _case_decode_encode(r, L, h):
    for curve in (S, G1):
        pb, eb = POINT_BYTES[curve], ENC[curve]
        for n in _sizes(pb):
            enc = _encode(r, L, h, curve, r.points(curve, n, garbage=False))
            enc[4::17] = r.rng.integers(0, 256, enc[4::17].shape, dtype=np.uint8)   # rejected encodings
            r.check(lambda e, o, ok, f: L.ncg_decode_points_batch(h, curve, n, e, 0, o, ok, f),
                    lambda e, o, ok, f: L.ncg_decode_points_batch_dev(h, curve, n, e, 0, o, ok, f, None), [enc], [n * pb, n, n],
                    (2,) if n < 1000 else ())
    for curve in (S, G2):
        pb, eb = POINT_BYTES[curve], ENC[curve]
        for n in _sizes(pb):
            pts = r.points(curve, n)
            r.check(lambda p, o, ok: L.ncg_encode_points_batch(h, curve, n, p, o, ok),
                    lambda p, o, ok: L.ncg_encode_points_batch_dev(h, curve, n, p, o, ok, None), [pts], [n * eb, n])


def _case_map_to_curve(r, L, h):
    for curve, count in ((G1, 1), (G2, 2)):
        pb = POINT_BYTES[curve]
        comps = count * (pb // 2) // 48
        for n in _sizes(pb):
            u = np.concatenate([r.field(n, 48, 0x1A) for _ in range(comps)], axis=1)
            r.check(lambda u_, o, f: L.ncg_map_to_curve_batch(h, curve, n, count, u_, o, f),
                    lambda u_, o, f: L.ncg_map_to_curve_batch_dev(h, curve, n, count, u_, o, f, None), [u], [n * pb, n],
                    (1,) if n < 1000 else ())


def _case_ntt(r, L, h):
    for log2n, batch, flags in ((5, 3, 0), (15, 1, 1)):
        omega = pow(7, (BLS_R - 1) >> log2n, BLS_R)
        om = np.frombuffer(omega.to_bytes(32, "little"), np.uint8).copy()
        m = batch << log2n
        data = r.field(m, 32, 0x70)
        r.check(lambda i, o: L.ncg_ntt(h, 0, log2n, batch, om.ctypes.data, i, o, flags),
                lambda i, o: L.ncg_ntt_dev(h, 0, log2n, batch, om.ctypes.data, i, o, flags, None), [data], [m * 32])


def _blob(r, msgs):
    """messages back to back behind 5 bytes that are no message, and their absolute offsets"""
    blob = np.frombuffer(b"\x11" * 5 + b"".join(msgs), np.uint8).copy()
    off = (5 + np.cumsum([0] + [len(m) for m in msgs])).astype(np.uint64)
    return blob, off


def _case_ed25519(r, L, h):
    rows = load_golden("ed25519_vectors.json")[:64]
    for n in _sizes(64):
        idx = np.arange(n) % len(rows)
        sig = np.stack([np.frombuffer(bytes.fromhex(rows[i]["sig"]), np.uint8) for i in idx])
        pk = np.stack([np.frombuffer(bytes.fromhex(rows[i]["pk"]), np.uint8) for i in idx])
        msgs = [bytes.fromhex(rows[i]["msg"]) for i in idx]
        sig[3::10, 40] ^= 1                                           # rejected rows
        blob, off = _blob(r, msgs)
        r.check(lambda s, p, m, o_, ok: L.ncg_ed25519_verify_batch_msgs(h, n, s, p, m, o_, 1, ok),
                lambda s, p, m, o_, ok: L.ncg_ed25519_verify_batch_msgs_dev(h, n, s, p, m, o_, 1, ok, None), [sig, pk, blob, off], [n])
        # the challenge scalars of the same rows, then the k-taking verify
        ks = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        d = [_dev(x) for x in (sig, pk, blob, off)]
        assert L.ncg_ed25519_challenge_batch_dev(h, n, *[t.data_ptr() for t in d], ks.data_ptr(), None) == OK
        assert L.ncg_sync(h) == OK
        k = ks.cpu().numpy().reshape(n, 32)
        got = r.check(lambda s, p, k_, ok: L.ncg_ed25519_verify_batch(h, n, s, p, k_, 1, ok),
                      lambda s, p, k_, ok: L.ncg_ed25519_verify_batch_dev(h, n, s, p, k_, 1, ok, None), [sig, pk, k], [n])
        assert got[0].any() and not got[0].all()


def _signed_secp(r, count):
    """(sig64, msg, hash32, pub33) rows signed with low S (test_gpu_ecdsa.sign_batch)"""
    from oracle.curves import SECP256K1_N as N, makeRng
    from test_gpu_ecdsa import keys_for, sign_batch
    rng = makeRng(0xAB1)
    ds = [rng.rndBelow(N - 1) + 1 for _ in range(count)]
    msgs = [b"row %d" % i * (i % 5) for i in range(count)]
    hs = [hashlib.sha256(m).digest() for m in msgs]
    sigs = sign_batch(ds, [int.from_bytes(x, "big") for x in hs], rng)
    return sigs, msgs, hs, keys_for(ds)


def _case_ecdsa(r, L, h):
    sigs, msgs, hs, pubs = _signed_secp(r, 40)
    for n in _sizes(65):
        idx = np.arange(n) % len(sigs)
        sig = np.stack([np.frombuffer(sigs[i], np.uint8) for i in idx])
        hsh = np.stack([np.frombuffer(hs[i], np.uint8) for i in idx])
        pub = np.stack([np.frombuffer(pubs[i], np.uint8) for i in idx])
        sig[3::10, 50] ^= 1
        pub[6::15] = 0                                                # invalid keys
        got = r.check(lambda s, x, p, ok: L.ncg_ecdsa_verify_batch(h, S, n, s, x, p, 1, ok),
                      lambda s, x, p, ok: L.ncg_ecdsa_verify_batch_dev(h, S, n, s, x, p, 1, ok, None), [sig, hsh, pub], [n])
        assert got[0].any() and not got[0].all()
        blob, off = _blob(r, [msgs[i] for i in idx])
        r.check(lambda s, m, o_, p, ok: L.ncg_ecdsa_verify_batch_msgs(h, S, n, s, m, o_, p, 1, ok),
                lambda s, m, o_, p, ok: L.ncg_ecdsa_verify_batch_msgs_dev(h, S, n, s, m, o_, p, 1, ok, None), [sig, blob, off, pub], [n])
        rec = np.concatenate([sig, (idx % 2).astype(np.uint8)[:, None]], axis=1)
        r.check(lambda s, x, o, ok: L.ncg_ecdsa_recover_batch(h, S, n, s, x, o, ok),
                lambda s, x, o, ok: L.ncg_ecdsa_recover_batch_dev(h, S, n, s, x, o, ok, None), [rec, hsh], [n * 64, n])


def _case_schnorr(r, L, h):
    rows = load_golden("secp256k1_schnorr.json")
    for n in _sizes(64):
        idx = np.arange(n) % len(rows)
        sig = np.stack([np.frombuffer(bytes.fromhex(rows[i]["sig"]), np.uint8) for i in idx])
        pk = np.stack([np.frombuffer(bytes.fromhex(rows[i]["pub"]), np.uint8) for i in idx])
        blob, off = _blob(r, [bytes.fromhex(rows[i]["msg"]) for i in idx])
        got = r.check(lambda s, m, o_, p, ok: L.ncg_schnorr_verify_batch_msgs(h, n, s, m, o_, p, ok),
                      lambda s, m, o_, p, ok: L.ncg_schnorr_verify_batch_msgs_dev(h, n, s, m, o_, p, ok, None), [sig, blob, off, pk], [n])
        assert got[0].any() and not got[0].all()
        e = r.rng.integers(0, 256, (n, 32), dtype=np.uint8)
        r.check(lambda s, e_, p, ok: L.ncg_schnorr_verify_batch(h, n, s, e_, p, ok),
                lambda s, e_, p, ok: L.ncg_schnorr_verify_batch_dev(h, n, s, e_, p, ok, None), [sig, e, pk], [n])


def _case_resident(r, L, h):
    for curve in (S, G1):
        pb = POINT_BYTES[curve]
        for n in _sizes(pb):
            if curve == G1:   # decoded bls12-381 sets are subgroup-checked: the endomorphism paths
                enc = _odd(_encode(r, L, h, curve, r.points(curve, n, garbage=False)))
                hp, bad = ctypes.c_void_p(), ctypes.c_int64()
                assert L.ncg_points_from_encoded(h, curve, n, enc.ctypes.data, 0, ctypes.byref(hp), ctypes.byref(bad)) == OK
                assert bad.value == -1
            else:   # (on the curve: an MSM adds in no fixed order, which only a group law makes irrelevant)
                pts = r.points(curve, n, garbage=False)
                hp = ctypes.c_void_p()
                assert L.ncg_points_upload(h, curve, n, pts.ctypes.data, ctypes.byref(hp)) == OK
            try:
                k = r.scalars(n)
                r.check(lambda k_, o, f: L.ncg_mul_var_batch_resident(h, hp, k_, o, f),
                        lambda k_, o, f: L.ncg_mul_var_batch_resident_dev(h, hp, k_, o, f, None), [k], [n * pb, n],
                        (1,) if n < 1000 else ())
                # the MSM's result comes back to host memory in both forms
                hk, dk = _odd(k), _dev(k)
                outs = []
                for fn, kp in ((L.ncg_msm_resident, hk.ctypes.data), (L.ncg_msm_resident_dev, dk.data_ptr())):
                    o = np.full(pb, 0xA5, np.uint8)
                    f = ctypes.c_uint8(7)
                    args = (h, hp, kp, o.ctypes.data, ctypes.byref(f)) + ((None,) if fn is L.ncg_msm_resident_dev else ())
                    assert fn(*args) == OK, _err(L, h)
                    outs.append((o.tobytes(), f.value))
                assert outs[0] == outs[1]
            finally:
                L.ncg_points_free(hp)


def _case_from_encoded(r, L, h):
    """ncg_points_from_encoded and ncg_aggregate_encoded against decode / MSM _dev forms"""
    hip = ctypes.CDLL("libamdhip64.so")
    for curve in (S, G1):
        pb, eb = POINT_BYTES[curve], ENC[curve]
        for n in _sizes(eb):
            enc = _encode(r, L, h, curve, r.points(curve, n, garbage=False), valid_only=True)
            d_pts = torch.zeros(n * pb, dtype=torch.uint8, device="cuda")
            d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
            d_inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
            d_enc = _dev(enc)
            assert L.ncg_decode_points_batch_dev(h, curve, n, d_enc.data_ptr(), 0, d_pts.data_ptr(), d_ok.data_ptr(), d_inf.data_ptr(), None) == OK
            assert L.ncg_sync(h) == OK
            assert d_ok.cpu().numpy().all()
            hp, bad = ctypes.c_void_p(), ctypes.c_int64(7)
            enc_odd = _odd(enc)
            assert L.ncg_points_from_encoded(h, curve, n, enc_odd.ctypes.data, 0, ctypes.byref(hp), ctypes.byref(bad)) == OK
            try:
                got = np.zeros(n * pb, np.uint8)
                assert hip.hipMemcpy(ctypes.c_void_p(got.ctypes.data), ctypes.c_void_p(L.ncg_points_dev(hp)), ctypes.c_size_t(n * pb), 2) == 0
                assert got.tobytes() == d_pts.cpu().numpy().tobytes()
            finally:
                L.ncg_points_free(hp)
            # the sum of the decoded points: aggregate_encoded against msm_dev on unit scalars
            ones = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
            ones[:, 0] = 1
            torch.cuda.synchronize()
            want, wf = np.zeros(pb, np.uint8), ctypes.c_uint8(7)
            assert L.ncg_msm_dev(h, curve, n, d_pts.data_ptr(), ones.data_ptr(), want.ctypes.data, ctypes.byref(wf), None) == OK
            got, gf = np.full(pb, 0xA5, np.uint8), ctypes.c_uint8(7)
            drop = n < 1000
            assert L.ncg_aggregate_encoded(h, curve, n, enc_odd.ctypes.data, 0, got.ctypes.data, None if drop else ctypes.byref(gf),
                                           ctypes.byref(bad)) == OK
            assert got.tobytes() == want.tobytes() and bad.value == -1 and (drop or gf.value == wf.value)
            # a rejected encoding: the same index from the host forms as from the decoder's verdicts
            enc[n // 3] = 0xFF
            hp = ctypes.c_void_p()
            assert L.ncg_points_from_encoded(h, curve, n, enc.ctypes.data, 0, ctypes.byref(hp), ctypes.byref(bad)) == INVALID
            assert bad.value == n // 3 and not hp.value
            assert L.ncg_aggregate_encoded(h, curve, n, enc.ctypes.data, 0, got.ctypes.data, None, ctypes.byref(bad)) == INVALID
            assert bad.value == n // 3


def _case_field_check(r, L, h):
    """no _dev form: the small batch must be the prefix of the large one, its input at an odd address"""
    for field in (0, 8):
        small, big = _sizes(9 * 4)
        a = r.rng.integers(0, 1 << 28, (big, 9), dtype=np.uint32)
        b = r.rng.integers(0, 1 << 28, (big, 9), dtype=np.uint32)
        wo = 8 if field == 0 else 9
        outs = []
        for n, ap in ((big, a), (small, _odd(a[:small]))):
            o = np.full((n, wo), 0xA5A5A5A5, np.uint32)
            assert L.ncg_field_check(h, field, 0, 0, n, ap.ctypes.data, b.ctypes.data, o.ctypes.data) == OK, _err(L, h)
            outs.append(o)
        assert outs[1].tobytes() == outs[0][:small].tobytes()


CASES = {name[len("_case_"):]: fn for name, fn in list(globals().items()) if name.startswith("_case_")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_form_equals_dev_form(case):
    eng = get_engine()
    CASES[case](_Run(eng, 0x5EED + len(case)), eng.lib, eng.h)
