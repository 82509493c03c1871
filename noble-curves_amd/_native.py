"""ctypes binding of libncg.so (include/ncg.h) plus wire-format marshalling helpers.

The library is built in-tree by `__graft_entry__.build()` (or `make -C noble-curves_amd/csrc`).
It is loaded lazily and LOUDLY: a missing library or a missing GPU raises NativeError - no
silent fallback exists.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

SECP256K1, ED25519, BLS12_381_G1, BLS12_381_G2, BN254_G1 = 0, 1, 2, 3, 5
POINT_BYTES = {SECP256K1: 64, ED25519: 64, BLS12_381_G1: 96, BLS12_381_G2: 192, BN254_G1: 64}
FIELD_BYTES = {SECP256K1: 32, ED25519: 32, BLS12_381_G1: 48, BLS12_381_G2: 48, BN254_G1: 32}
FIELD_BLS12_381_FR = 0
H2C_SECP256K1, H2C_EDWARDS25519 = 0, 1       # suites of ncg_h2c_*: secp256k1_XMD:SHA-256_SSWU, edwards25519_XMD:SHA-512_ELL2
FIELD_BN254_FR = 5
POLY_ADD, POLY_SUB, POLY_DOT = 0, 1, 2
POLY_MAX_POINTS = 8
X25519_ONE_SCALAR = 1   # ncg_x25519_batch flag: one secret for every row
ED25519_SIGN_EXPANDED, ED25519_SIGN_ONE_KEY, ED25519_SIGN_PREHASH = 1, 2, 4   # ncg_ed25519_sign_batch flags
ED25519_DOM_MAX = 289
ECDSA_LOW_S, SECP_SIGN_ONE_KEY = 1, 4   # ncg_ecdsa_sign_batch / ncg_schnorr_sign_batch flags
SECP_PK_COMPRESSED, SECP_PK_UNCOMPRESSED, SECP_PK_XONLY = 0, 1, 2   # ncg_secp256k1_public_key_batch flags
SECP_PK_BYTES = {SECP_PK_COMPRESSED: 33, SECP_PK_UNCOMPRESSED: 65, SECP_PK_XONLY: 32}
# ncg_secp256k1_sign_check: {op: words per row of (a, b, out)}, the table of include/ncg.h (csrc/secp256k1_sign.hpp)
SECP_SIGN_CHECK_WORDS = {0: (24, 1, 8), 1: (8, 1, 16), 2: (32, 1, 18), 3: (24, 1, 8), 4: (24, 1, 18)}
RISTRETTO_ONE_SCALAR = 1   # ncg_ristretto_mul_batch flag: one scalar for every row
OPRF_RISTRETTO255_SHA512 = 0            # ncg_oprf_* suite
OPRF_ONE_SCALAR, OPRF_INVERT = 1, 2     # ncg_oprf_mul_batch / ncg_oprf_evaluate_batch flags
# ncg_fp12_batch ops (enum ncg_fp12_op); a GT element is GT_BYTES on the wire
(FP12_MUL, FP12_SQR, FP12_INV, FP12_CONJUGATE, FP12_FROBENIUS1, FP12_FROBENIUS2, FP12_FROBENIUS3, FP12_CYCLOTOMIC_SQR, FP12_MUL014,
 FP12_FINAL_EXP, FP12_IS_ONE) = range(11)
GT_BYTES = 576
PAIRING_CHECK_SUBGROUP = 1   # ncg_pairing_batch flag: the reference's isTorsionFree on every operand
BLS_LONG_SIGNATURES, BLS_SHORT_SIGNATURES = 0, 1   # ncg_bls_verify_batch schemes
# ncg_field_check: {field: words per row of (a, b, out)}, the table of csrc/selfcheck.hpp (15 is unassigned)
FIELD_CHECK_WORDS = {
    0: (9, 9, 8), 1: (9, 9, 8), 2: (12, 12, 12), 3: (28, 28, 12), 4: (56, 56, 24), 5: (18, 18, 9), 6: (18, 18, 9), 7: (27, 18, 27),
    8: (9, 9, 9), 9: (9, 9, 9), 10: (36, 36, 36), 11: (36, 36, 36), 12: (56, 56, 56), 13: (112, 112, 112), 14: (36, 36, 36),
    16: (36, 9, 36), 17: (36, 9, 36)}
X448_ONE_SCALAR = 1     # ncg_x448_batch flag: one secret for every row
ED448_ONE_SCALAR = 1    # ncg_ed448_mul_batch flag: one scalar for every row
ED448_SIGN_EXPANDED, ED448_SIGN_ONE_KEY, ED448_PREHASH = 1, 2, 4   # ncg_ed448_sign_batch flags (PREHASH: challenge and verify_msgs too)
ED448_DOM_MAX, ED448_KEY_BYTES = 265, 172
# ncg_ed448_sign_check: op -> words per row of a, b, out
ED448_SIGN_CHECK_WORDS = {0: (50, 0, 50), 1: (29, 0, 14), 2: (28, 14, 14), 3: (43, 30, 30)}
# ncg_fe448_check: {op: words per row of (a, b, out)}, the table of include/ncg.h (csrc/ed448.hpp)
FE448_CHECK_WORDS = {0: (16, 16, 16), 1: (16, 0, 16), 2: (16, 16, 48), 3: (16, 16, 16), 4: (16, 0, 14), 5: (14, 0, 16), 6: (16, 0, 16),
                     7: (16, 0, 16), 8: (64, 16, 64), 9: (48, 48, 48), 10: (48, 0, 48)}
DECAF448_ONE_SCALAR = 1  # ncg_decaf448_mul_batch flag: one scalar for every row
# ncg_decaf448_check: {op: words per row of (a, b, out)}, the table of include/ncg.h (csrc/decaf448.hpp)
DECAF448_CHECK_WORDS = {0: (16, 16, 17), 1: (64, 0, 14), 2: (16, 0, 64)}
ENCODED_BYTES = {SECP256K1: 33, ED25519: 32, BLS12_381_G1: 48, BLS12_381_G2: 96}   # compressed toBytes


class NativeError(RuntimeError):
    pass


def lib_path():
    """In-tree library; NCG_LIB overrides it (A/B runs of alternative builds)."""
    return os.environ.get("NCG_LIB") or os.path.join(_HERE, "libncg.so")


_lib = None
_lib_lock = threading.Lock()


def load_library():
    """dlopen libncg.so and declare prototypes; raises NativeError if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise NativeError(
                "noble-gpu: %s is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % path)
        try:
            lib = ctypes.CDLL(path)
        except OSError as e:  # pragma: no cover
            raise NativeError("noble-gpu: cannot load %s: %s" % (path, e))
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.ncg_init.argtypes = [i32, ctypes.POINTER(vp)]
        lib.ncg_init.restype = i32
        lib.ncg_destroy.argtypes = [vp]
        lib.ncg_destroy.restype = None
        lib.ncg_last_error.argtypes = [vp]
        lib.ncg_last_error.restype = ctypes.c_char_p
        lib.ncg_sync.argtypes = [vp]
        lib.ncg_sync.restype = i32
        lib.ncg_version.argtypes = []
        lib.ncg_version.restype = ctypes.c_char_p
        lib.ncg_point_bytes.argtypes = [i32]
        lib.ncg_point_bytes.restype = i32
        lib.ncg_field_bytes.argtypes = [i32]
        lib.ncg_field_bytes.restype = i32
        lib.ncg_mul_var_batch.argtypes = [vp, i32, sz, vp, vp, vp, vp]
        lib.ncg_mul_var_batch.restype = i32
        lib.ncg_mul_var_batch_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
        lib.ncg_mul_var_batch_dev.restype = i32
        lib.ncg_ubench.argtypes = [vp, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_float)]
        lib.ncg_ubench.restype = i32
        for name, args in _OPTIONAL_PROTOS.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.argtypes = args
                fn.restype = i32
        lib.ncg_points_free.argtypes = [vp]
        lib.ncg_points_free.restype = None
        lib.ncg_points_count.argtypes = [vp]
        lib.ncg_points_count.restype = sz
        lib.ncg_points_dev.argtypes = [vp]
        lib.ncg_points_dev.restype = vp
        lib.ncg_multi_destroy.argtypes = [vp]
        lib.ncg_multi_destroy.restype = None
        lib.ncg_multi_ctx.argtypes = [vp, i32]
        lib.ncg_multi_ctx.restype = vp
        lib.ncg_multi_last_error.argtypes = [vp]
        lib.ncg_multi_last_error.restype = ctypes.c_char_p
        _lib = lib
        return lib


_vp, _sz, _i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
_OPTIONAL_PROTOS = {
    "ncg_decode_points_batch": [_vp, _i32, _sz, _vp, _i32, _vp, _vp, _vp],
    "ncg_decode_points_batch_dev": [_vp, _i32, _sz, _vp, _i32, _vp, _vp, _vp, _vp],
    "ncg_add_pairs_batch": [_vp, _i32, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_add_pairs_batch_dev": [_vp, _i32, _sz, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_aggregate_encoded": [_vp, _i32, _sz, _vp, _i32, _vp, _vp, _vp],
    "ncg_encode_points_batch": [_vp, _i32, _sz, _vp, _vp, _vp],
    "ncg_encode_points_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_map_to_curve_batch": [_vp, _i32, _sz, _i32, _vp, _vp, _vp],
    "ncg_map_to_curve_batch_dev": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, _vp],
    "ncg_ntt": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _i32],
    "ncg_ntt_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _i32, _vp],
    "ncg_poly_pointwise": [_vp, _i32, _i32, _sz, _vp, _vp, _vp],
    "ncg_poly_pointwise_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_poly_scale": [_vp, _i32, _sz, _vp, _vp, _i32, _vp],
    "ncg_poly_scale_dev": [_vp, _i32, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_poly_eval": [_vp, _i32, _sz, _vp, _vp, _vp],
    "ncg_poly_eval_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_poly_eval_monomial": [_vp, _i32, _sz, _vp, _i32, _vp, _vp],
    "ncg_poly_eval_monomial_dev": [_vp, _i32, _sz, _vp, _i32, _vp, _vp, _vp],
    "ncg_poly_lagrange_basis": [_vp, _i32, _i32, _vp, _vp, _i32, _vp],
    "ncg_poly_lagrange_basis_dev": [_vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "ncg_poly_mul": [_vp, _i32, _i32, _vp, _sz, _vp, _sz, _vp, _vp],
    "ncg_poly_mul_dev": [_vp, _i32, _i32, _vp, _sz, _vp, _sz, _vp, _vp, _vp],
    "ncg_normalize_batch": [_vp, _i32, _sz, _vp, _vp, _vp],
    "ncg_normalize_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_msm": [_vp, _i32, _sz, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8)],
    "ncg_msm_dev": [_vp, _i32, _sz, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8), _vp],
    "ncg_mul_base_batch": [_vp, _i32, _sz, _vp, _vp, _vp],
    "ncg_mul_base_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed25519_verify_batch": [_vp, _sz, _vp, _vp, _vp, _i32, _vp],
    "ncg_ed25519_verify_batch_dev": [_vp, _sz, _vp, _vp, _vp, _i32, _vp, _vp],
    "ncg_ed25519_verify_batch_msgs": [_vp, _sz, _vp, _vp, _vp, _vp, _i32, _vp],
    "ncg_ed25519_verify_batch_msgs_dev": [_vp, _sz, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "ncg_ed25519_challenge_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_ed25519_public_key_batch": [_vp, _sz, _vp, _vp],
    "ncg_ed25519_public_key_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed25519_expand_key_batch": [_vp, _sz, _vp, _vp],
    "ncg_ed25519_expand_key_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed25519_sign_batch": [_vp, _sz, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed25519_sign_batch_dev": [_vp, _sz, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_x25519_batch": [_vp, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_x25519_batch_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_x25519_base_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_x25519_base_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed25519_to_montgomery_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed25519_to_montgomery_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_x448_batch": [_vp, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_x448_batch_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_x448_base_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_x448_base_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed448_decode_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed448_decode_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed448_encode_batch": [_vp, _sz, _vp, _vp],
    "ncg_ed448_encode_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed448_add_pairs_batch": [_vp, _sz, _vp, _vp, _i32, _vp],
    "ncg_ed448_add_pairs_batch_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_ed448_mul_batch": [_vp, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_ed448_mul_batch_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_ed448_mul_base_batch": [_vp, _sz, _vp, _vp],
    "ncg_ed448_mul_base_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed448_to_montgomery_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed448_to_montgomery_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed448_verify_batch": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed448_verify_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_fe448_check": [_vp, _i32, _i32, _sz, _vp, _vp, _vp],
    "ncg_shake256_batch": [_vp, _sz, _vp, _vp, _sz, _vp],
    "ncg_shake256_batch_dev": [_vp, _sz, _vp, _vp, _sz, _vp, _vp],
    "ncg_ed448_challenge_batch_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed448_verify_batch_msgs": [_vp, _sz, _vp, _vp, _i32, _vp, _sz, _vp, _vp, _vp],
    "ncg_ed448_verify_batch_msgs_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed448_public_key_batch": [_vp, _sz, _vp, _vp],
    "ncg_ed448_public_key_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed448_expand_key_batch": [_vp, _sz, _vp, _vp],
    "ncg_ed448_expand_key_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ed448_sign_batch": [_vp, _sz, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ed448_sign_batch_dev": [_vp, _sz, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_ed448_sign_check": [_vp, _i32, _i32, _sz, _vp, _vp, _vp],
    "ncg_decaf448_decode_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_decaf448_decode_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_decaf448_encode_batch": [_vp, _sz, _vp, _vp],
    "ncg_decaf448_encode_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_decaf448_equals_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_decaf448_equals_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_decaf448_from_uniform_batch": [_vp, _sz, _vp, _vp],
    "ncg_decaf448_from_uniform_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_decaf448_mul_batch": [_vp, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_decaf448_mul_batch_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_decaf448_mul_base_batch": [_vp, _sz, _vp, _vp],
    "ncg_decaf448_mul_base_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_decaf448_check": [_vp, _i32, _i32, _sz, _vp, _vp, _vp],
    "ncg_ristretto_decode_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ristretto_decode_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ristretto_encode_batch": [_vp, _sz, _vp, _vp],
    "ncg_ristretto_encode_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ristretto_equals_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ristretto_equals_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ristretto_from_uniform_batch": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ristretto_from_uniform_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ristretto_mul_batch": [_vp, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_ristretto_mul_batch_dev": [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_ristretto_mul_base_batch": [_vp, _sz, _vp, _vp],
    "ncg_ristretto_mul_base_batch_dev": [_vp, _sz, _vp, _vp, _vp],
    "ncg_ristretto_msm": [_vp, _sz, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int64)],
    "ncg_ristretto_msm_dev": [_vp, _sz, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int64), _vp],
    "ncg_xmd_sha512_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp],
    "ncg_xmd_sha512_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp],
    "ncg_ristretto_hash_to_group_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_ristretto_hash_to_group_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp],
    "ncg_ristretto_hash_to_scalar_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _vp],
    "ncg_ristretto_hash_to_scalar_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_oprf_blind_batch": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_blind_batch_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_mul_batch": [_vp, _i32, _sz, _vp, _vp, _i32, _vp, _vp],
    "ncg_oprf_mul_batch_dev": [_vp, _i32, _sz, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_oprf_finalize_batch": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_oprf_finalize_batch_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_evaluate_batch": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _sz, _vp, _i32, _vp, _vp],
    "ncg_oprf_evaluate_batch_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _sz, _vp, _i32, _vp, _vp, _vp],
    "ncg_oprf_composite_scalars_batch": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_composite_scalars_batch_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_generate_proof": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_generate_proof_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_verify_proof": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_verify_proof_dev": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_oprf_check": [_vp, _i32, _i32, _sz, _vp, _vp, _vp],
    "ncg_h2c_hash_batch": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_h2c_hash_batch_dev": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, _sz, _vp, _vp, _vp],
    "ncg_h2c_map_batch": [_vp, _i32, _sz, _i32, _vp, _vp, _vp],
    "ncg_h2c_map_batch_dev": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, _vp],
    "ncg_h2c_hash_to_scalar_batch": [_vp, _i32, _sz, _vp, _vp, _vp, _sz, _vp],
    "ncg_h2c_hash_to_scalar_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_h2c_hash_to_field_batch": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, _sz, _vp],
    "ncg_h2c_hash_to_field_batch_dev": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_xmd_sha256_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp],
    "ncg_xmd_sha256_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp],
    "ncg_h2c_check": [_vp, _i32, _sz, _vp, _vp],
    "ncg_xof_shake256_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp],
    "ncg_xof_shake256_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp],
    "ncg_ed448_h2c_hash_batch": [_vp, _sz, _i32, _vp, _vp, _vp, _sz, _vp],
    "ncg_ed448_h2c_hash_batch_dev": [_vp, _sz, _i32, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_ed448_h2c_map_batch": [_vp, _sz, _i32, _vp, _vp],
    "ncg_ed448_h2c_map_batch_dev": [_vp, _sz, _i32, _vp, _vp, _vp],
    "ncg_ed448_h2c_hash_to_field_batch": [_vp, _sz, _i32, _vp, _vp, _vp, _sz, _vp],
    "ncg_ed448_h2c_hash_to_field_batch_dev": [_vp, _sz, _i32, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_ed448_h2c_hash_to_scalar_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _vp],
    "ncg_ed448_h2c_hash_to_scalar_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_decaf448_hash_to_group_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _vp],
    "ncg_decaf448_hash_to_group_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_decaf448_hash_to_scalar_batch": [_vp, _sz, _vp, _vp, _vp, _sz, _vp],
    "ncg_decaf448_hash_to_scalar_batch_dev": [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp],
    "ncg_h2c448_check": [_vp, _i32, _sz, _vp, _vp],
    "ncg_pairing_batch": [_vp, _sz, _vp, _vp, _sz, _vp, _i32, _vp, _vp, ctypes.POINTER(ctypes.c_int64)],
    "ncg_pairing_batch_dev": [_vp, _sz, _vp, _vp, _sz, _vp, _i32, _vp, _vp, ctypes.POINTER(ctypes.c_int64), _vp],
    "ncg_bls_verify_batch": [_vp, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_bls_verify_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_fp12_batch": [_vp, _i32, _sz, _vp, _vp, _vp],
    "ncg_fp12_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_points_upload": [_vp, _i32, _sz, _vp, ctypes.POINTER(_vp)],
    "ncg_points_from_encoded": [_vp, _i32, _sz, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_int64)],
    "ncg_points_curve": [_vp],
    "ncg_msm_resident": [_vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8)],
    "ncg_msm_resident_dev": [_vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8), _vp],
    "ncg_ecdsa_verify_batch": [_vp, _i32, _sz, _vp, _vp, _vp, _i32, _vp],
    "ncg_ecdsa_recover_batch": [_vp, _i32, _sz, _vp, _vp, _vp, _vp],
    "ncg_ecdsa_recover_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_schnorr_verify_batch": [_vp, _sz, _vp, _vp, _vp, _vp],
    "ncg_ecdsa_verify_batch_msgs": [_vp, _i32, _sz, _vp, _vp, _vp, _vp, _i32, _vp],
    "ncg_ecdsa_verify_batch_msgs_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "ncg_schnorr_verify_batch_msgs": [_vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_schnorr_verify_batch_msgs_dev": [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_schnorr_verify_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "ncg_ecdsa_verify_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _i32, _vp, _vp],
    "ncg_secp256k1_public_key_batch": [_vp, _sz, _vp, _i32, _vp, _vp],
    "ncg_secp256k1_public_key_batch_dev": [_vp, _sz, _vp, _i32, _vp, _vp, _vp],
    "ncg_ecdsa_sign_batch": [_vp, _i32, _sz, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_ecdsa_sign_batch_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    "ncg_ecdsa_sign_batch_msgs": [_vp, _i32, _sz, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_ecdsa_sign_batch_msgs_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    "ncg_schnorr_sign_batch": [_vp, _sz, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "ncg_schnorr_sign_batch_dev": [_vp, _sz, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "ncg_secp256k1_sign_check": [_vp, _i32, _i32, _sz, _vp, _vp, _vp],
    "ncg_points_verify_subgroup": [_vp, _vp, ctypes.POINTER(ctypes.c_int64)],
    "ncg_points_in_subgroup": [_vp],
    "ncg_points_precompute": [_vp, _vp],
    "ncg_points_precomputed": [_vp],
    "ncg_mul_var_batch_resident": [_vp, _vp, _vp, _vp, _vp],
    "ncg_mul_var_batch_resident_dev": [_vp, _vp, _vp, _vp, _vp, _vp],
    "ncg_field_check": [_vp, _i32, _i32, _i32, _sz, _vp, _vp, _vp],
    "ncg_comm_unique_id": [_vp],
    "ncg_comm_init": [_vp, _i32, _i32, _vp],
    "ncg_comm_destroy": [_vp],
    "ncg_comm_size": [_vp],
    "ncg_comm_rank": [_vp],
    "ncg_comm_count": [_vp, _vp, _vp],
    "ncg_msm_sharded_dev": [_vp, _i32, _sz, _sz, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8), _vp],
    "ncg_msm_split_dev": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8), _vp],
    "ncg_msm_shard_local_dev": [_vp, _i32, _sz, _sz, _vp, _vp, _vp, _vp],
    "ncg_msm_shard_combine": [_vp, _i32, _sz, _i32, _vp, _vp, ctypes.POINTER(ctypes.c_uint8), _vp],
    "ncg_msm_sharded_windows_dev": [_vp, _i32, _sz, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8), _vp],
    "ncg_msm_shard_windows_local_dev": [_vp, _i32, _sz, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "ncg_msm_split_windows_dev": [_vp, _i32, _sz, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8), _vp],
    "ncg_msm_async_submit": [_vp, _i32, _i32, _sz, _vp, _vp, _vp, _i32, _vp],
    "ncg_msm_async_collect": [_vp, _i32, _vp, ctypes.POINTER(ctypes.c_uint8)],
    "ncg_msm_async_collect_slot": [_vp, _i32, _vp],
    "ncg_msm_set_tuning": [_vp, _i32, _i32],
    "ncg_msm_last_plan": [_vp, ctypes.POINTER(ctypes.c_int)],
    "ncg_multi_init": [ctypes.POINTER(_i32), _i32, ctypes.POINTER(_vp)],
    "ncg_multi_devices": [_vp],
    "ncg_msm_multi": [_vp, _i32, _sz, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint8)],
}
COMM_ID_BYTES = 128


# ---------------------------------------------------------------- wire helpers (numpy, no torch)
def ints_to_le(values, nbytes):
    """list of non-negative ints -> uint8 array [len, nbytes], little-endian."""
    out = np.empty((len(values), nbytes), dtype=np.uint8)
    for i, v in enumerate(values):
        out[i] = np.frombuffer(int(v).to_bytes(nbytes, "little"), dtype=np.uint8)
    return out


def le_to_ints(arr, nbytes):
    """uint8 array [..., nbytes] -> list of ints."""
    flat = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1, nbytes)
    return [int.from_bytes(row.tobytes(), "little") for row in flat]


class Engine:
    """One native context (one GPU).  Methods take/return numpy uint8 arrays in wire format,
    or raw device pointers for the *_dev variants (torch tensors: pass .data_ptr())."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.device = device
        h = ctypes.c_void_p()
        rc = self.lib.ncg_init(device, ctypes.byref(h))
        if rc != 0:
            raise NativeError((self.lib.ncg_last_error(None) or b"").decode() or "noble-gpu: ncg_init failed (%d)" % rc)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ncg_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = (self.lib.ncg_last_error(self.h) or b"").decode()
            raise NativeError(msg or "noble-gpu: native call failed (%d)" % rc)

    def version(self):
        return self.lib.ncg_version().decode()

    def sync(self):
        self._check(self.lib.ncg_sync(self.h))

    # ---- batch variable-base multiply -------------------------------------------------------
    def mul_var_batch(self, curve, points, scalars, out=None, inf=None):
        """points: uint8 [n, POINT_BYTES]; scalars: uint8 [n, 32] -> (out [n, PB], is_inf [n]).  `out` / `inf`: result arrays the
        caller keeps (and may pin once with host_register) - a fresh 64 MB array per call costs first-touch page faults and a page
        lock before the first result byte lands (2^20 secp256k1 pairs: 43-52 ms per call against 10 with kept, pinned arrays)."""
        pb = POINT_BYTES[curve]
        points = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, pb)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = points.shape[0]
        if scalars.shape[0] != n:
            raise ValueError("arrays of points and scalars must have equal length")
        if out is None:
            out = np.empty((n, pb), dtype=np.uint8)
        elif out.dtype != np.uint8 or out.shape != (n, pb) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous uint8 array of shape (n, point bytes)")
        if inf is None:
            inf = np.empty((n,), dtype=np.uint8)
        elif inf.dtype != np.uint8 or inf.shape != (n,) or not inf.flags["C_CONTIGUOUS"]:
            raise ValueError("inf must be a C-contiguous uint8 array of shape (n,)")
        if n:
            self._check(self.lib.ncg_mul_var_batch(self.h, curve, n, points.ctypes.data, scalars.ctypes.data,
                                                   out.ctypes.data, inf.ctypes.data))
        return out, inf

    def decode_points_batch(self, curve, encoded, zip215=False):
        """encoded uint8 [n, 33|32|48|96] -> (affine [n, PB], ok [n] bool, is_inf [n] bool)."""
        enc_bytes = ENCODED_BYTES[curve]
        pb = POINT_BYTES[curve]
        enc = np.ascontiguousarray(encoded, dtype=np.uint8).reshape(-1, enc_bytes)
        n = enc.shape[0]
        out = np.zeros((n, pb), dtype=np.uint8)
        ok = np.zeros((n,), dtype=np.uint8)
        inf = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_decode_points_batch(self.h, curve, n, enc.ctypes.data, 1 if zip215 else 0,
                                                         out.ctypes.data, ok.ctypes.data, inf.ctypes.data))
        return out, ok.astype(bool), inf.astype(bool)

    def add_pairs_batch(self, curve, a, b, subtract=False):
        """a, b uint8 [n, PB] affine wire points -> (a[i] + b[i] (or a[i] - b[i]) [n, PB], is_inf [n])."""
        pb = POINT_BYTES[curve]
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, pb)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, pb)
        if a.shape != b.shape:
            raise ValueError("noble-gpu: add_pairs_batch: operand arrays differ in length")
        out = np.empty_like(a)
        inf = np.empty((a.shape[0],), dtype=np.uint8)
        if a.shape[0]:
            self._check(self.lib.ncg_add_pairs_batch(self.h, curve, a.shape[0], a.ctypes.data, b.ctypes.data,
                                                     1 if subtract else 0, out.ctypes.data, inf.ctypes.data))
        return out, inf

    def aggregate_encoded(self, curve, encoded, zip215=False):
        """encoded uint8 [n, ENCODED_BYTES] -> (affine [PB], is_inf, bad_index): sum of the decoded points;
        bad_index >= 0 (and no result) when an entry does not decode."""
        enc = np.ascontiguousarray(encoded, dtype=np.uint8).reshape(-1, ENCODED_BYTES[curve])
        out = np.zeros((POINT_BYTES[curve],), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        bad = ctypes.c_int64(-1)
        rc = self.lib.ncg_aggregate_encoded(self.h, curve, enc.shape[0], enc.ctypes.data, 1 if zip215 else 0,
                                            out.ctypes.data, ctypes.byref(inf), ctypes.byref(bad))
        if rc and bad.value >= 0:
            return None, False, int(bad.value)
        self._check(rc)
        return out, bool(inf.value), -1

    def encode_points_batch(self, curve, affine):
        """affine uint8 [n, PB] -> (encoded [n, 33|32|48|96], ok [n] bool): compressed Point.toBytes."""
        pb = POINT_BYTES[curve]
        aff = np.ascontiguousarray(affine, dtype=np.uint8).reshape(-1, pb)
        n = aff.shape[0]
        out = np.zeros((n, ENCODED_BYTES[curve]), dtype=np.uint8)
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_encode_points_batch(self.h, curve, n, aff.ctypes.data, out.ctypes.data,
                                                         ok.ctypes.data))
        return out, ok.astype(bool)

    def normalize_batch(self, curve, proj):
        """proj uint8 [n, 3*FIELD_BYTES*(2 for Fp2)] (X || Y || Z) -> (affine [n, PB], is_inf [n])."""
        pb = POINT_BYTES[curve]
        proj = np.ascontiguousarray(proj, dtype=np.uint8).reshape(-1, pb // 2 * 3)
        n = proj.shape[0]
        out = np.empty((n, pb), dtype=np.uint8)
        inf = np.empty((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_normalize_batch(self.h, curve, n, proj.ctypes.data, out.ctypes.data,
                                                     inf.ctypes.data))
        return out, inf

    def mul_base_batch(self, curve, scalars):
        """scalars uint8 [n, 32] -> (out [n, PB], is_inf [n]) with out[i] = scalars[i] * BASE."""
        pb = POINT_BYTES[curve]
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = scalars.shape[0]
        out = np.empty((n, pb), dtype=np.uint8)
        inf = np.empty((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_mul_base_batch(self.h, curve, n, scalars.ctypes.data, out.ctypes.data,
                                                    inf.ctypes.data))
        return out, inf

    def mul_base_batch_dev(self, curve, n, d_scalars, d_out, d_inf, stream=None):
        self._check(self.lib.ncg_mul_base_batch_dev(self.h, curve, n, d_scalars, d_out, d_inf, stream))

    def mul_var_batch_dev(self, curve, n, d_points, d_scalars, d_out, d_inf, stream=None):
        self._check(self.lib.ncg_mul_var_batch_dev(self.h, curve, n, d_points, d_scalars, d_out, d_inf, stream))

    # ---- pinned host buffers ---------------------------------------------------------------------
    def host_register(self, arr):
        """Pin a long-lived numpy array once (ncg_host_register): host-pointer calls on it then run at PCIe speed."""
        fn = self.lib.ncg_host_register
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int
        if fn(arr.ctypes.data, arr.nbytes) != 0:
            raise NativeError((self.lib.ncg_last_error(None) or b"").decode() or "noble-gpu: host_register failed")

    def host_unregister(self, arr):
        fn = self.lib.ncg_host_unregister
        fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
        fn(arr.ctypes.data)

    # ---- multi-scalar multiplication -----------------------------------------------------------
    def msm(self, curve, points, scalars):
        """sum_i scalars[i]*points[i]; returns (affine wire bytes [PB], is_inf bool)."""
        pb = POINT_BYTES[curve]
        points = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, pb)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = points.shape[0]
        if scalars.shape[0] != n:
            raise ValueError("arrays of points and scalars must have equal length")
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm(self.h, curve, n, points.ctypes.data if n else None,
                                     scalars.ctypes.data if n else None, out.ctypes.data, ctypes.byref(inf)))
        return out, bool(inf.value)

    def msm_dev(self, curve, n, d_points, d_scalars, stream=None):
        """device-resident inputs (raw pointers); result comes back to the host."""
        pb = POINT_BYTES[curve]
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm_dev(self.h, curve, n, d_points, d_scalars, out.ctypes.data, ctypes.byref(inf),
                                         stream))
        return out, bool(inf.value)

    # ---- resident point sets (include/ncg.h "resident point sets") -------------------------------
    def upload_points(self, curve, points):
        """points uint8 [n, PB] -> ResidentPoints (device-resident until .free() / garbage collection)."""
        pb = POINT_BYTES[curve]
        points = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, pb)
        h = ctypes.c_void_p()
        self._check(self.lib.ncg_points_upload(self.h, curve, points.shape[0], points.ctypes.data if points.size else None,
                                               ctypes.byref(h)))
        return ResidentPoints(self, h, curve)

    def upload_encoded(self, curve, encoded, zip215=False):
        """encoded uint8 [n, ENCODED_BYTES] -> (ResidentPoints | None, bad_index): decoded and validated on the device."""
        enc = np.ascontiguousarray(encoded, dtype=np.uint8).reshape(-1, ENCODED_BYTES[curve])
        h = ctypes.c_void_p()
        bad = ctypes.c_int64(-1)
        rc = self.lib.ncg_points_from_encoded(self.h, curve, enc.shape[0], enc.ctypes.data if enc.size else None,
                                              1 if zip215 else 0, ctypes.byref(h), ctypes.byref(bad))
        if rc and bad.value >= 0:
            return None, int(bad.value)
        self._check(rc)
        return ResidentPoints(self, h, curve), -1

    # ---- multi-GPU MSM, one process per GPU (include/ncg.h "multi-GPU MSM" (1)) ------------------
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL unique id (rank 0 creates it and ships it to the other ranks)."""
        lib = load_library()
        buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
        rc = lib.ncg_comm_unique_id(buf)
        if rc != 0:
            raise NativeError((lib.ncg_last_error(None) or b"").decode() or "noble-gpu: ncg_comm_unique_id failed")
        return bytes(buf)

    def comm_init(self, nranks, rank, unique_id):
        """Collective: joins this context to the communicator named by `unique_id`."""
        uid = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self.lib.ncg_comm_init(self.h, nranks, rank, uid))
        self._has_comm = True

    def comm_size(self):
        return self.lib.ncg_comm_size(self.h)

    def comm_count(self):
        """(ranks, my rank) as the RCCL communicator itself reports them (ncclCommCount / ncclCommUserRank); (0, -1) without one."""
        n, me = ctypes.c_int(0), ctypes.c_int(-1)
        self._check(self.lib.ncg_comm_count(self.h, ctypes.byref(n), ctypes.byref(me)))
        return int(n.value), int(me.value)

    def has_comm(self):
        """True between comm_init and comm_destroy (comm_size() reads 1 both without a communicator and with one of a single rank)."""
        return bool(getattr(self, "_has_comm", False))

    def comm_destroy(self):
        self._has_comm = False
        self._check(self.lib.ncg_comm_destroy(self.h))

    def msm_sharded_dev(self, curve, n_local, d_points, d_scalars, stream=None, n_max=0):
        """Collective MSM over the union of all ranks' device-resident shards (RCCL all-gather of the
        grouped window sums + on-device add); every rank gets (affine wire bytes [PB], is_inf)."""
        pb = POINT_BYTES[curve]
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm_sharded_dev(self.h, curve, n_local, n_max, d_points, d_scalars, out.ctypes.data,
                                                 ctypes.byref(inf), stream))
        return out, bool(inf.value)

    def msm_plan_info(self, curve, n):
        """{c, nwin, nb, ngroups} of the window plan for an n-point MSM (ncg_msm_plan_info)."""
        out = (ctypes.c_int * 4)()
        fn = self.lib.ncg_msm_plan_info
        fn.argtypes, fn.restype = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)], ctypes.c_int
        if fn(curve, n, out) != 0:
            raise NativeError("noble-gpu: msm_plan_info: bad arguments")
        return {"c": out[0], "nwin": out[1], "nb": out[2], "ngroups": out[3]}

    def msm_shard_slot_bytes(self, curve):
        fn = self.lib.ncg_msm_shard_slot_bytes
        fn.argtypes, fn.restype = [ctypes.c_int], ctypes.c_size_t
        return int(fn(curve))

    def msm_shard_local_dev(self, curve, n_local, d_points, d_scalars, stream=None, n_max=0):
        """This rank's part of a sharded MSM with a host-staged exchange: per-shard phase on the device, the slot
        (window-plan header + grouped window sums, fixed size per curve) comes back as a uint8 array."""
        slot = np.zeros((self.msm_shard_slot_bytes(curve),), dtype=np.uint8)
        self._check(self.lib.ncg_msm_shard_local_dev(self.h, curve, n_local, n_max, d_points, d_scalars, slot.ctypes.data, stream))
        return slot

    def msm_shard_combine(self, curve, n_max, slots, stream=None):
        """slots: uint8 [nparts, slot_bytes] in rank order -> (affine wire bytes [PB], is_inf): upload, header check,
        adding kernel, finish - what ncg_msm_sharded_dev runs after its all-gather."""
        slots = np.ascontiguousarray(slots, dtype=np.uint8)
        pb = POINT_BYTES[curve]
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm_shard_combine(self.h, curve, n_max, int(slots.shape[0]), slots.ctypes.data, out.ctypes.data,
                                                   ctypes.byref(inf), stream))
        return out, bool(inf.value)

    def msm_split_dev(self, curve, n, parts, d_points, d_scalars, stream=None):
        """The sharded pipeline on this one GPU: `parts` slices, per-shard phase each, multi-GPU combine
        kernel, finish (ncg_msm_split_dev)."""
        pb = POINT_BYTES[curve]
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm_split_dev(self.h, curve, n, parts, d_points, d_scalars, out.ctypes.data,
                                               ctypes.byref(inf), stream))
        return out, bool(inf.value)

    # ---- window-sharded MSM (include/ncg.h "WINDOW-sharded mode"): every rank holds all points and scalars ----
    @staticmethod
    def _res_handle(resident):
        return resident.h if resident is not None else None

    def msm_sharded_windows_dev(self, curve, n, d_points, d_scalars, stream=None, resident=None):
        """Collective: rank r runs its range of the windows of ONE n-point MSM; the slots are concatenated (precomputed
        sets: added).  `resident`: a ResidentPoints of this engine instead of d_points."""
        pb = POINT_BYTES[resident.curve if resident is not None else curve]
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm_sharded_windows_dev(self.h, curve, n, d_points, self._res_handle(resident), d_scalars,
                                                         out.ctypes.data, ctypes.byref(inf), stream))
        return out, bool(inf.value)

    def msm_shard_windows_local_dev(self, curve, n, part, nparts, d_points, d_scalars, stream=None, resident=None):
        """Part `part` of `nparts` of a window-sharded MSM with a host-staged exchange: the slot as a uint8 array."""
        c = resident.curve if resident is not None else curve
        slot = np.zeros((self.msm_shard_slot_bytes(c),), dtype=np.uint8)
        self._check(self.lib.ncg_msm_shard_windows_local_dev(self.h, curve, n, part, nparts, d_points, self._res_handle(resident),
                                                             d_scalars, slot.ctypes.data, stream))
        return slot

    def msm_split_windows_dev(self, curve, n, parts, d_points, d_scalars, stream=None, resident=None):
        """The window-sharded pipeline on this one GPU: the parts in turn, then the concatenation / finish."""
        pb = POINT_BYTES[resident.curve if resident is not None else curve]
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm_split_windows_dev(self.h, curve, n, parts, d_points, self._res_handle(resident), d_scalars,
                                                       out.ctypes.data, ctypes.byref(inf), stream))
        return out, bool(inf.value)

    # ---- several MSMs in flight (include/ncg.h "Several MSMs in flight") --------------------------------------
    ASYNC_WINDOWS = 1

    def msm_async_lanes(self):
        fn = self.lib.ncg_msm_async_lanes
        fn.argtypes, fn.restype = [], ctypes.c_int
        return int(fn())

    def msm_async_submit(self, lane, curve, n, d_points, d_scalars, stream=None, resident=None, flags=0):
        self._check(self.lib.ncg_msm_async_submit(self.h, lane, curve, n, d_points, self._res_handle(resident), d_scalars, flags, stream))

    def msm_async_collect(self, lane, curve):
        pb = POINT_BYTES[curve]
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self._check(self.lib.ncg_msm_async_collect(self.h, lane, out.ctypes.data, ctypes.byref(inf)))
        return out, bool(inf.value)

    @staticmethod
    def async_part(part, nparts):
        """flags for msm_async_submit: ONE part of a window-sharded MSM (NCG_MSM_ASYNC_PART)."""
        return 2 | (part << 8) | (nparts << 20)

    def msm_async_collect_slot(self, lane, curve):
        slot = np.zeros((self.msm_shard_slot_bytes(curve),), dtype=np.uint8)
        self._check(self.lib.ncg_msm_async_collect_slot(self.h, lane, slot.ctypes.data))
        return slot

    def msm_set_tuning(self, seg=0, run_serial=-1):
        """Diagnostics: entries per accumulate lane / serial pieces per cut bucket (0 / -1 = defaults)."""
        self._check(self.lib.ncg_msm_set_tuning(self.h, seg, run_serial))

    def msm_last_plan(self):
        out = (ctypes.c_int * 8)()
        self._check(self.lib.ncg_msm_last_plan(self.h, out))
        keys = ("c", "nwin", "nb", "w0", "nwin_total", "seg", "run_serial", "long_runs")
        return dict(zip(keys, [int(v) for v in out]))

    # ---- ed25519 batch verify --------------------------------------------------------------------
    def ed25519_verify_batch(self, sigs, pks, ks, zip215=True):
        """sigs uint8 [n,64], pks [n,32], ks [n,32] (challenge scalars, LE) -> bool array [n]."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        pks = np.ascontiguousarray(pks, dtype=np.uint8).reshape(-1, 32)
        ks = np.ascontiguousarray(ks, dtype=np.uint8).reshape(-1, 32)
        n = sigs.shape[0]
        if pks.shape[0] != n or ks.shape[0] != n:
            raise ValueError("arrays of signatures, public keys and challenges must have equal length")
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed25519_verify_batch(self.h, n, sigs.ctypes.data, pks.ctypes.data,
                                                          ks.ctypes.data, 1 if zip215 else 0, ok.ctypes.data))
        return ok.astype(bool)

    # ---- Ed25519 signing: seeds uint8 [n, 32], expanded key rows [n, 96] (scalar || prefix || A), signatures [n, 64] ----------
    def ed25519_public_key_batch(self, seeds):
        """eddsa.getPublicKey per row"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((seeds.shape[0], 32), dtype=np.uint8)
        if seeds.shape[0]:
            self._check(self.lib.ncg_ed25519_public_key_batch(self.h, seeds.shape[0], seeds.ctypes.data, out.ctypes.data))
        return out

    def ed25519_expand_key_batch(self, seeds):
        """getExtendedPublicKey per row, as the 96-byte rows that ed25519_sign_batch takes with expanded=True"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((seeds.shape[0], 96), dtype=np.uint8)
        if seeds.shape[0]:
            self._check(self.lib.ncg_ed25519_expand_key_batch(self.h, seeds.shape[0], seeds.ctypes.data, out.ctypes.data))
        return out

    def ed25519_sign_batch(self, keys, msgs_blob, msg_off, dom=b"", expanded=False, one_key=False, prehash=False):
        """keys: seeds [n, 32] or expanded rows [n, 96] (ONE row with one_key); msgs_blob / msg_off as for
        ed25519_verify_batch_msgs; dom: the domain prefix of ed25519ctx / ed25519ph -> (signatures uint8 [n, 64], ok bool [n])."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 96 if expanded else 32)
        blob = np.ascontiguousarray(msgs_blob, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(msg_off, dtype=np.uint64).reshape(-1)
        n = off.shape[0] - 1
        if n < 0 or keys.shape[0] != (1 if one_key else n):
            raise ValueError("arrays of keys and message offsets must have matching lengths")
        dom = bytes(dom)
        flags = (ED25519_SIGN_EXPANDED if expanded else 0) | (ED25519_SIGN_ONE_KEY if one_key else 0) | (ED25519_SIGN_PREHASH if prehash else 0)
        sig, ok = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed25519_sign_batch(self.h, n, keys.ctypes.data, flags, dom if dom else None, len(dom),
                                                        blob.ctypes.data if blob.size else None, off.ctypes.data, sig.ctypes.data,
                                                        ok.ctypes.data))
        return sig, ok.astype(bool)

    # ---- X25519 / toMontgomery: rows of 32 bytes -> (out uint8 [n, 32], ok bool [n]); a refused row is zero ----------------
    def x25519_batch(self, scalars, us, one_scalar=False):
        """x25519.scalarMult per row: scalars uint8 [n, 32] raw (clamped by the library), or ONE row with one_scalar; us [n, 32]."""
        us = np.ascontiguousarray(us, dtype=np.uint8).reshape(-1, 32)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = us.shape[0]
        if scalars.shape[0] != (1 if one_scalar else n):
            raise ValueError("arrays of scalars and u coordinates must have equal length")
        out, ok = np.zeros((n, 32), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_x25519_batch(self.h, n, scalars.ctypes.data, us.ctypes.data, X25519_ONE_SCALAR if one_scalar else 0,
                                                  out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def x25519_base_batch(self, scalars):
        """x25519.getPublicKey per row"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = scalars.shape[0]
        out, ok = np.zeros((n, 32), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_x25519_base_batch(self.h, n, scalars.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ed25519_to_montgomery_batch(self, pks):
        """ed25519.utils.toMontgomery per row"""
        pks = np.ascontiguousarray(pks, dtype=np.uint8).reshape(-1, 32)
        n = pks.shape[0]
        out, ok = np.zeros((n, 32), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed25519_to_montgomery_batch(self.h, n, pks.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    # ---- X448 / Ed448: field elements and scalars uint8 [n, 56], encodings [n, 57], signatures [n, 114], affine points [n, 112];
    # a refused row is zero with ok False -------------------------------------------------------------------------------------
    def _rows(self, a, width):
        return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, width)

    def x448_batch(self, scalars, us, one_scalar=False):
        """x448.scalarMult per row: scalars [n, 56] raw (clamped by the library), or ONE row with one_scalar; us [n, 56]."""
        us, scalars = self._rows(us, 56), self._rows(scalars, 56)
        n = us.shape[0]
        if scalars.shape[0] != (1 if one_scalar else n):
            raise ValueError("arrays of scalars and u coordinates must have equal length")
        out, ok = np.zeros((n, 56), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_x448_batch(self.h, n, scalars.ctypes.data, us.ctypes.data, X448_ONE_SCALAR if one_scalar else 0,
                                                out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def x448_base_batch(self, scalars):
        """x448.getPublicKey per row"""
        scalars = self._rows(scalars, 56)
        n = scalars.shape[0]
        out, ok = np.zeros((n, 56), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_x448_base_batch(self.h, n, scalars.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ed448_decode_batch(self, enc):
        """ed448 Point.fromBytes (strict) per row -> (x || y [n, 112], ok bool [n])"""
        enc = self._rows(enc, 57)
        n = enc.shape[0]
        out, ok = np.zeros((n, 112), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_decode_batch(self.h, n, enc.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ed448_encode_batch(self, affine):
        """Point.toBytes of affine points [n, 112] -> [n, 57]"""
        affine = self._rows(affine, 112)
        n = affine.shape[0]
        out = np.zeros((n, 57), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_encode_batch(self.h, n, affine.ctypes.data, out.ctypes.data))
        return out

    def ed448_add_pairs_batch(self, a, b, subtract=False):
        """Point.add / Point.subtract of affine points [n, 112] -> [n, 112]"""
        a, b = self._rows(a, 112), self._rows(b, 112)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("arrays of points must have equal length")
        out = np.zeros((n, 112), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_add_pairs_batch(self.h, n, a.ctypes.data, b.ctypes.data, 1 if subtract else 0, out.ctypes.data))
        return out

    def ed448_mul_batch(self, enc, ks, one_scalar=False):
        """fromBytes(enc).multiplyUnsafe(k).toBytes() per row: enc [n, 57], ks [n, 56] (or ONE row) -> ([n, 57], ok bool [n])"""
        enc, ks = self._rows(enc, 57), self._rows(ks, 56)
        n = enc.shape[0]
        if ks.shape[0] != (1 if one_scalar else n):
            raise ValueError("arrays of points and scalars must have equal length")
        out, ok = np.zeros((n, 57), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_mul_batch(self.h, n, enc.ctypes.data, ks.ctypes.data, ED448_ONE_SCALAR if one_scalar else 0,
                                                     out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ed448_mul_base_batch(self, ks):
        """BASE.multiplyUnsafe(k).toBytes() per row: ks [n, 56] -> [n, 57]"""
        ks = self._rows(ks, 56)
        n = ks.shape[0]
        out = np.zeros((n, 57), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_mul_base_batch(self.h, n, ks.ctypes.data, out.ctypes.data))
        return out

    def ed448_to_montgomery_batch(self, pks):
        """ed448.utils.toMontgomery per row: [n, 57] -> ([n, 56], ok bool [n])"""
        pks = self._rows(pks, 57)
        n = pks.shape[0]
        out, ok = np.zeros((n, 56), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_to_montgomery_batch(self.h, n, pks.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ed448_verify_batch(self, sigs, pks, ks):
        """ed448 verify (strict, cofactored) with the challenges given: sigs [n, 114], pks [n, 57], ks [n, 56] -> bool [n]"""
        sigs, pks, ks = self._rows(sigs, 114), self._rows(pks, 57), self._rows(ks, 56)
        n = sigs.shape[0]
        if pks.shape[0] != n or ks.shape[0] != n:
            raise ValueError("arrays of signatures, public keys and challenges must have equal length")
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_verify_batch(self.h, n, sigs.ctypes.data, pks.ctypes.data, ks.ctypes.data, ok.ctypes.data))
        return ok.astype(bool)

    def fe448_check(self, op, variant, a_words, b_words):
        """The lane code of GF(2^448 - 2^224 - 1), X448 and Ed448 on raw uint32 rows (ncg_fe448_check; FE448_CHECK_WORDS has the
        widths): a [n, wa], b [n, wb] (any array where wb = 0) -> [n, wo]; an unknown op gives [n, 16] zeros."""
        wa, wb, wo = FE448_CHECK_WORDS.get(op, (0, 0, 16))
        a = np.ascontiguousarray(a_words, dtype=np.uint32)
        b = np.ascontiguousarray(b_words, dtype=np.uint32)
        n = a.shape[0]
        if (wa and a.shape[1] != wa) or (wb and (b.shape[0] != n or b.shape[1] != wb)):
            raise ValueError("fe448_check: op %d takes rows of %d and %d words" % (op, wa, wb))
        out = np.zeros((n, wo), dtype=np.uint32)
        if n:
            self._check(self.lib.ncg_fe448_check(self.h, op, variant, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    # ---- SHAKE256, Ed448 signing and verification from messages: seeds [n, 57], expanded key rows [n, 172] (scalar || prefix || A ||
    # 2 zero bytes), signatures [n, 114]; dom is the whole domain prefix "SigEd448" || phflag || len(ctx) || ctx ------------------
    @staticmethod
    def _blob_off(msgs_blob, msg_off):
        blob = np.ascontiguousarray(msgs_blob, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(msg_off, dtype=np.uint64).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError("message offsets: n + 1 values are needed")
        return blob, off, off.shape[0] - 1

    def shake256_batch(self, msgs_blob, msg_off, out_len):
        """SHAKE256(message i, out_len) per row -> uint8 [n, out_len]"""
        blob, off, n = self._blob_off(msgs_blob, msg_off)
        out = np.zeros((n, out_len), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_shake256_batch(self.h, n, blob.ctypes.data if blob.size else None, off.ctypes.data, out_len,
                                                    out.ctypes.data))
        return out

    def shake256_batch_dev(self, n, d_msgs, d_off, out_len, d_out, stream=None):
        self._check(self.lib.ncg_shake256_batch_dev(self.h, n, d_msgs, d_off, out_len, d_out, stream))

    def ed448_challenge_batch_dev(self, n, d_sigs, d_pks, dom, d_msgs, d_off, d_ks, prehash=False, stream=None):
        dom = bytes(dom)
        self._check(self.lib.ncg_ed448_challenge_batch_dev(self.h, n, d_sigs, d_pks, ED448_PREHASH if prehash else 0, dom if dom else None,
                                                           len(dom), d_msgs, d_off, d_ks, stream))

    def ed448_verify_batch_msgs(self, sigs, pks, msgs_blob, msg_off, dom, prehash=False):
        """ed448 verify (strict, cofactored) from the messages: the challenge hash runs on the device -> bool [n]"""
        sigs, pks = self._rows(sigs, 114), self._rows(pks, 57)
        blob, off, n = self._blob_off(msgs_blob, msg_off)
        if sigs.shape[0] != n or pks.shape[0] != n:
            raise ValueError("arrays of signatures, public keys and message offsets must have matching lengths")
        dom = bytes(dom)
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_verify_batch_msgs(self.h, n, sigs.ctypes.data, pks.ctypes.data, ED448_PREHASH if prehash else 0,
                                                             dom if dom else None, len(dom), blob.ctypes.data if blob.size else None,
                                                             off.ctypes.data, ok.ctypes.data))
        return ok.astype(bool)

    def ed448_verify_batch_msgs_dev(self, n, d_sigs, d_pks, dom, d_msgs, d_off, d_ok, prehash=False, stream=None):
        dom = bytes(dom)
        self._check(self.lib.ncg_ed448_verify_batch_msgs_dev(self.h, n, d_sigs, d_pks, ED448_PREHASH if prehash else 0, dom if dom else None,
                                                             len(dom), d_msgs, d_off, d_ok, stream))

    def ed448_public_key_batch(self, seeds):
        """eddsa.getPublicKey per row: [n, 57] -> [n, 57]"""
        seeds = self._rows(seeds, 57)
        out = np.zeros((seeds.shape[0], 57), dtype=np.uint8)
        if seeds.shape[0]:
            self._check(self.lib.ncg_ed448_public_key_batch(self.h, seeds.shape[0], seeds.ctypes.data, out.ctypes.data))
        return out

    def ed448_public_key_batch_dev(self, n, d_seeds, d_out, stream=None):
        self._check(self.lib.ncg_ed448_public_key_batch_dev(self.h, n, d_seeds, d_out, stream))

    def ed448_expand_key_batch(self, seeds):
        """getExtendedPublicKey per row, as the 172-byte rows that ed448_sign_batch takes with expanded=True"""
        seeds = self._rows(seeds, 57)
        out = np.zeros((seeds.shape[0], ED448_KEY_BYTES), dtype=np.uint8)
        if seeds.shape[0]:
            self._check(self.lib.ncg_ed448_expand_key_batch(self.h, seeds.shape[0], seeds.ctypes.data, out.ctypes.data))
        return out

    def ed448_expand_key_batch_dev(self, n, d_seeds, d_out, stream=None):
        self._check(self.lib.ncg_ed448_expand_key_batch_dev(self.h, n, d_seeds, d_out, stream))

    def ed448_sign_batch(self, keys, msgs_blob, msg_off, dom, expanded=False, one_key=False, prehash=False):
        """keys: seeds [n, 57] or expanded rows [n, 172] (ONE row with one_key); msgs_blob / msg_off as for ed448_verify_batch_msgs
        -> (signatures uint8 [n, 114], ok bool [n])."""
        keys = self._rows(keys, ED448_KEY_BYTES if expanded else 57)
        blob, off, n = self._blob_off(msgs_blob, msg_off)
        if keys.shape[0] != (1 if one_key else n):
            raise ValueError("arrays of keys and message offsets must have matching lengths")
        dom = bytes(dom)
        flags = (ED448_SIGN_EXPANDED if expanded else 0) | (ED448_SIGN_ONE_KEY if one_key else 0) | (ED448_PREHASH if prehash else 0)
        sig, ok = np.zeros((n, 114), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_sign_batch(self.h, n, keys.ctypes.data, flags, dom if dom else None, len(dom),
                                                      blob.ctypes.data if blob.size else None, off.ctypes.data, sig.ctypes.data,
                                                      ok.ctypes.data))
        return sig, ok.astype(bool)

    def ed448_sign_batch_dev(self, n, d_keys, dom, d_msgs, d_off, d_sigs, d_ok, flags=0, stream=None):
        dom = bytes(dom)
        self._check(self.lib.ncg_ed448_sign_batch_dev(self.h, n, d_keys, flags, dom if dom else None, len(dom), d_msgs, d_off, d_sigs, d_ok,
                                                      stream))

    def ed448_sign_check(self, op, a_words, b_words):
        """The lane code of Keccak-f[1600], the reduction mod the Ed448 group order and signing with a given nonce on raw uint32 rows
        (ncg_ed448_sign_check; ED448_SIGN_CHECK_WORDS has the widths): a [n, wa], b [n, wb] (any array where wb = 0) -> [n, wo];
        an unknown op gives [n, 16] zeros."""
        wa, wb, wo = ED448_SIGN_CHECK_WORDS.get(op, (0, 0, 16))
        a = np.ascontiguousarray(a_words, dtype=np.uint32)
        b = np.ascontiguousarray(b_words, dtype=np.uint32)
        n = a.shape[0]
        if (wa and a.shape[1] != wa) or (wb and (b.shape[0] != n or b.shape[1] != wb)):
            raise ValueError("ed448_sign_check: op %d takes rows of %d and %d words" % (op, wa, wb))
        out = np.zeros((n, wo), dtype=np.uint32)
        if n:
            self._check(self.lib.ncg_ed448_sign_check(self.h, op, 0, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    # ---- decaf448: encodings and scalars uint8 [n, 56], Edwards representatives (Ed448 affine points) and uniform bytes [n, 112] ----
    def decaf448_decode_batch(self, enc):
        """DecafPoint.fromBytes per row -> (representatives x || y [n, 112], ok bool [n]); a refused row is zero"""
        enc = self._rows(enc, 56)
        n = enc.shape[0]
        out, ok = np.zeros((n, 112), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_decaf448_decode_batch(self.h, n, enc.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def decaf448_encode_batch(self, affine):
        """DecafPoint.toBytes of any points of the curve [n, 112] -> [n, 56]"""
        affine = self._rows(affine, 112)
        n = affine.shape[0]
        out = np.zeros((n, 56), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_decaf448_encode_batch(self.h, n, affine.ctypes.data, out.ctypes.data))
        return out

    def decaf448_equals_batch(self, a, b):
        """DecafPoint.equals per row of representatives [n, 112] -> bool [n]"""
        a, b = self._rows(a, 112), self._rows(b, 112)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("arrays of points must have equal length")
        out = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_decaf448_equals_batch(self.h, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out.astype(bool)

    def decaf448_from_uniform_batch(self, bytes112):
        """decaf448_hasher.deriveToCurve(row).toBytes() per row of 112 uniform bytes -> [n, 56]"""
        b = self._rows(bytes112, 112)
        n = b.shape[0]
        out = np.zeros((n, 56), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_decaf448_from_uniform_batch(self.h, n, b.ctypes.data, out.ctypes.data))
        return out

    def decaf448_mul_batch(self, enc, ks, one_scalar=False):
        """fromBytes(enc).multiplyUnsafe(k).toBytes() per row: enc [n, 56], ks [n, 56] (or ONE row) -> ([n, 56], ok bool [n])"""
        enc, ks = self._rows(enc, 56), self._rows(ks, 56)
        n = enc.shape[0]
        if ks.shape[0] != (1 if one_scalar else n):
            raise ValueError("arrays of points and scalars must have equal length")
        out, ok = np.zeros((n, 56), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_decaf448_mul_batch(self.h, n, enc.ctypes.data, ks.ctypes.data, DECAF448_ONE_SCALAR if one_scalar else 0,
                                                        out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def decaf448_mul_base_batch(self, ks):
        """DecafPoint.BASE.multiplyUnsafe(k).toBytes() per row: ks [n, 56] -> [n, 56]"""
        ks = self._rows(ks, 56)
        n = ks.shape[0]
        out = np.zeros((n, 56), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_decaf448_mul_base_batch(self.h, n, ks.ctypes.data, out.ctypes.data))
        return out

    def decaf448_check(self, op, a_words, b_words):
        """The lane code of decaf448 on raw uint32 rows (ncg_decaf448_check; DECAF448_CHECK_WORDS has the widths): a [n, wa],
        b [n, wb] (any array where wb = 0) -> [n, wo]; an unknown op gives [n, 16] zeros."""
        wa, wb, wo = DECAF448_CHECK_WORDS.get(op, (0, 0, 16))
        a = np.ascontiguousarray(a_words, dtype=np.uint32)
        b = np.ascontiguousarray(b_words, dtype=np.uint32)
        n = a.shape[0]
        if (wa and a.shape[1] != wa) or (wb and (b.shape[0] != n or b.shape[1] != wb)):
            raise ValueError("decaf448_check: op %d takes rows of %d and %d words" % (op, wa, wb))
        out = np.zeros((n, wo), dtype=np.uint32)
        if n:
            self._check(self.lib.ncg_decaf448_check(self.h, op, 0, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    # ---- ristretto255: encodings and scalars uint8 [n, 32], Edwards representatives (ed25519 wire points) [n, 64] ------------
    def ristretto_decode_batch(self, enc):
        """RistrettoPoint.fromBytes per row -> (representatives [n, 64], ok bool [n]); a rejected row is zero"""
        enc = np.ascontiguousarray(enc, dtype=np.uint8).reshape(-1, 32)
        n = enc.shape[0]
        out, ok = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ristretto_decode_batch(self.h, n, enc.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ristretto_encode_batch(self, pts):
        """toBytes of every wire point -> [n, 32]"""
        pts = np.ascontiguousarray(pts, dtype=np.uint8).reshape(-1, 64)
        out = np.zeros((pts.shape[0], 32), dtype=np.uint8)
        if pts.shape[0]:
            self._check(self.lib.ncg_ristretto_encode_batch(self.h, pts.shape[0], pts.ctypes.data, out.ctypes.data))
        return out

    def ristretto_equals_batch(self, a, b):
        """a[i].equals(b[i]) on wire points -> bool [n]"""
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 64)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, 64)
        if a.shape != b.shape:
            raise ValueError("arrays of points must have equal length")
        out = np.zeros((a.shape[0],), dtype=np.uint8)
        if a.shape[0]:
            self._check(self.lib.ncg_ristretto_equals_batch(self.h, a.shape[0], a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out.astype(bool)

    def ristretto_from_uniform_batch(self, bytes64, want_affine=False):
        """deriveToCurve(bytes64[i]).toBytes() -> (encodings [n, 32], representatives [n, 64] or None)"""
        b = np.ascontiguousarray(bytes64, dtype=np.uint8).reshape(-1, 64)
        n = b.shape[0]
        out = np.zeros((n, 32), dtype=np.uint8)
        aff = np.zeros((n, 64), dtype=np.uint8) if want_affine else None
        if n:
            self._check(self.lib.ncg_ristretto_from_uniform_batch(self.h, n, b.ctypes.data, out.ctypes.data,
                                                                  aff.ctypes.data if want_affine else None))
        return out, aff

    def ristretto_mul_batch(self, enc, scalars, one_scalar=False):
        """fromBytes(enc[i]).multiply(k[i]).toBytes() -> (out [n, 32], ok bool [n]); scalars [n, 32], or ONE row with one_scalar"""
        enc = np.ascontiguousarray(enc, dtype=np.uint8).reshape(-1, 32)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = enc.shape[0]
        if scalars.shape[0] != (1 if one_scalar else n):
            raise ValueError("arrays of points and scalars must have equal length")
        out, ok = np.zeros((n, 32), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ristretto_mul_batch(self.h, n, enc.ctypes.data, scalars.ctypes.data,
                                                         RISTRETTO_ONE_SCALAR if one_scalar else 0, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ristretto_mul_base_batch(self, scalars):
        """BASE.multiply(k[i]).toBytes() -> [n, 32]"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((scalars.shape[0], 32), dtype=np.uint8)
        if scalars.shape[0]:
            self._check(self.lib.ncg_ristretto_mul_base_batch(self.h, scalars.shape[0], scalars.ctypes.data, out.ctypes.data))
        return out

    def ristretto_msm(self, enc, scalars):
        """toBytes(sum k[i] fromBytes(enc[i])) -> uint8 [32]; NativeError naming the index of an encoding that does not decode
        (its position is also the `bad_index` attribute of the error)"""
        enc = np.ascontiguousarray(enc, dtype=np.uint8).reshape(-1, 32)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = enc.shape[0]
        if scalars.shape[0] != n:
            raise ValueError("arrays of points and scalars must have equal length")
        out, bad = np.zeros((32,), dtype=np.uint8), ctypes.c_int64(-1)
        rc = self.lib.ncg_ristretto_msm(self.h, n, enc.ctypes.data if n else None, scalars.ctypes.data if n else None, out.ctypes.data,
                                        ctypes.byref(bad))
        if rc:
            err = NativeError((self.lib.ncg_last_error(self.h) or b"").decode() or "noble-gpu: native call failed (%d)" % rc)
            err.bad_index = int(bad.value)
            raise err
        return out

    # ---- OPRF over ristretto255 (RFC 9497): elements and scalars uint8 [n, 32], outputs [n, 64], messages a blob with offsets; status
    # uint8 [n]: 0 ok, 1 undecodable, 2 identity, 3 scalar zero or not below L -----------------------------------------------------
    @staticmethod
    def _blob(msgs):
        off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        if len(msgs):
            off[1:] = np.cumsum([len(m) for m in msgs])
        return np.frombuffer(b"".join(bytes(m) for m in msgs), dtype=np.uint8), off

    def xmd_sha512_batch(self, msgs, dst, out_len):
        """expand_message_xmd over SHA-512 of every message -> uint8 [n, out_len]"""
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out = np.zeros((n, out_len), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_xmd_sha512_batch(self.h, n, blob.ctypes.data if blob.size else None, off.ctypes.data, dst, len(dst),
                                                      out_len, out.ctypes.data))
        return out

    def ristretto_hash_to_group_batch(self, msgs, dst, want_affine=False):
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out, aff = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ristretto_hash_to_group_batch(self.h, n, blob.ctypes.data if blob.size else None, off.ctypes.data, dst,
                                                                   len(dst), out.ctypes.data, aff.ctypes.data if want_affine else None))
        return out, aff

    def ristretto_hash_to_scalar_batch(self, msgs, dst):
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out = np.zeros((n, 32), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ristretto_hash_to_scalar_batch(self.h, n, blob.ctypes.data if blob.size else None, off.ctypes.data, dst,
                                                                    len(dst), out.ctypes.data))
        return out

    def oprf_blind_batch(self, mode, inputs, blinds, suite=0):
        blob, off = self._blob(inputs)
        blinds = np.ascontiguousarray(blinds, dtype=np.uint8).reshape(-1, 32)
        n = len(inputs)
        if blinds.shape[0] != n:
            raise ValueError("arrays of inputs and blinds must have equal length")
        out, st = np.zeros((n, 32), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_oprf_blind_batch(self.h, suite, mode, n, blob.ctypes.data if blob.size else None, off.ctypes.data,
                                                      blinds.ctypes.data, out.ctypes.data, st.ctypes.data))
        return out, st

    def oprf_mul_batch(self, elements, scalars, one_scalar=False, invert=False, suite=0):
        elements = np.ascontiguousarray(elements, dtype=np.uint8).reshape(-1, 32)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = elements.shape[0]
        if scalars.shape[0] != (1 if one_scalar else n):
            raise ValueError("arrays of elements and scalars must have equal length")
        out, st = np.zeros((n, 32), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_oprf_mul_batch(self.h, suite, n, elements.ctypes.data, scalars.ctypes.data,
                                                    (OPRF_ONE_SCALAR if one_scalar else 0) | (OPRF_INVERT if invert else 0), out.ctypes.data,
                                                    st.ctypes.data))
        return out, st

    def oprf_finalize_batch(self, mode, inputs, blinds, evaluated, info=None, suite=0):
        blob, off = self._blob(inputs)
        blinds = np.ascontiguousarray(blinds, dtype=np.uint8).reshape(-1, 32)
        evaluated = np.ascontiguousarray(evaluated, dtype=np.uint8).reshape(-1, 32)
        n = len(inputs)
        if blinds.shape[0] != n or evaluated.shape[0] != n:
            raise ValueError("arrays of inputs, blinds and elements must have equal length")
        info = None if info is None else bytes(info)
        out, st = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_oprf_finalize_batch(self.h, suite, mode, n, blob.ctypes.data if blob.size else None, off.ctypes.data,
                                                         info if info else None, len(info or b""), blinds.ctypes.data, evaluated.ctypes.data,
                                                         out.ctypes.data, st.ctypes.data))
        return out, st

    def oprf_evaluate_batch(self, mode, inputs, scalar, invert=False, info=None, suite=0):
        """the one scalar against every input"""
        blob, off = self._blob(inputs)
        scalar = np.ascontiguousarray(scalar, dtype=np.uint8).reshape(1, 32)
        info = None if info is None else bytes(info)
        n = len(inputs)
        out, st = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_oprf_evaluate_batch(self.h, suite, mode, n, blob.ctypes.data if blob.size else None, off.ctypes.data,
                                                         info if info else None, len(info or b""), scalar.ctypes.data,
                                                         OPRF_ONE_SCALAR | (OPRF_INVERT if invert else 0), out.ctypes.data, st.ctypes.data))
        return out, st

    def oprf_composite_scalars_batch(self, mode, B, C, D, suite=0):
        C = np.ascontiguousarray(C, dtype=np.uint8).reshape(-1, 32)
        D = np.ascontiguousarray(D, dtype=np.uint8).reshape(-1, 32)
        n = C.shape[0]
        if D.shape[0] != n:
            raise ValueError("arrays of elements must have equal length")
        out, st = np.zeros((n, 32), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_oprf_composite_scalars_batch(self.h, suite, mode, n, bytes(B), C.ctypes.data, D.ctypes.data, out.ctypes.data,
                                                                  st.ctypes.data))
        return out, st

    def oprf_generate_proof(self, mode, k32, B, C, D, r32, suite=0):
        C = np.ascontiguousarray(C, dtype=np.uint8).reshape(-1, 32)
        D = np.ascontiguousarray(D, dtype=np.uint8).reshape(-1, 32)
        if D.shape[0] != C.shape[0] or not C.shape[0]:
            raise ValueError("arrays of elements must have equal, non-zero length")
        out = np.zeros((64,), dtype=np.uint8)
        self._check(self.lib.ncg_oprf_generate_proof(self.h, suite, mode, C.shape[0], bytes(k32), bytes(B), C.ctypes.data, D.ctypes.data,
                                                     bytes(r32), out.ctypes.data))
        return out.tobytes()

    def oprf_verify_proof(self, mode, B, C, D, proof64, suite=0):
        C = np.ascontiguousarray(C, dtype=np.uint8).reshape(-1, 32)
        D = np.ascontiguousarray(D, dtype=np.uint8).reshape(-1, 32)
        if D.shape[0] != C.shape[0] or not C.shape[0]:
            raise ValueError("arrays of elements must have equal, non-zero length")
        ok = np.zeros((1,), dtype=np.uint8)
        self._check(self.lib.ncg_oprf_verify_proof(self.h, suite, mode, C.shape[0], bytes(B), C.ctypes.data, D.ctypes.data, bytes(proof64),
                                                   ok.ctypes.data))
        return bool(ok[0])

    def oprf_check(self, op, variant, a, b):
        """the lane code of csrc/oprf.hpp on raw rows (include/ncg.h has the table): a uint8 [n, 4 wa], b [n, 32] -> out [n, 4 wo]"""
        wa, wo = (16 if op == 2 else 8), (16 if op == 3 else 8)
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 4 * wa)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((a.shape[0], 4 * wo), dtype=np.uint8)
        if a.shape[0]:
            self._check(self.lib.ncg_oprf_check(self.h, op, variant, a.shape[0], a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    # ---- bls12-381 pairings: G1 / G2 affine wire points [n, 96] / [n, 192], GT elements uint8 [n, 576] ---------------------
    def _pairing_error(self, rc, bad):
        err = NativeError((self.lib.ncg_last_error(self.h) or b"").decode() or "noble-gpu: native call failed (%d)" % rc)
        err.bad_index = int(bad.value)
        return err

    def pairing_batch(self, g1, g2, group_offsets, want_gt=True, flags=0):
        """pairingBatch of every group -> (GT [n_groups, 576] or None, is_one bool [n_groups]); group_offsets: n_groups + 1
        ascending pair offsets.  NativeError with the attribute bad_index for a ZERO or invalid operand."""
        g1 = np.ascontiguousarray(g1, dtype=np.uint8).reshape(-1, 96)
        g2 = np.ascontiguousarray(g2, dtype=np.uint8).reshape(-1, 192)
        off = np.ascontiguousarray(group_offsets, dtype=np.uint32).reshape(-1)
        n, ng = g1.shape[0], off.shape[0] - 1
        if g2.shape[0] != n:
            raise ValueError("arrays of G1 and G2 points must have equal length")
        if ng < 0:
            raise ValueError("group offsets must hold at least one entry")
        gt = np.zeros((ng, 576), dtype=np.uint8) if want_gt else None
        one, bad = np.zeros((ng,), dtype=np.uint8), ctypes.c_int64(-1)
        rc = self.lib.ncg_pairing_batch(self.h, n, g1.ctypes.data if n else None, g2.ctypes.data if n else None, ng, off.ctypes.data, flags,
                                        gt.ctypes.data if want_gt and ng else None, one.ctypes.data if ng else None, ctypes.byref(bad))
        if rc:
            raise self._pairing_error(rc, bad)
        return gt, one.astype(bool)

    def pairing_batch_dev(self, n_pairs, g1_ptr, g2_ptr, group_offsets, out_gt_ptr, out_is_one_ptr, stream=None, flags=0):
        """device-resident variant; group_offsets stays a host array.  Returns after the result is complete."""
        off = np.ascontiguousarray(group_offsets, dtype=np.uint32).reshape(-1)
        bad = ctypes.c_int64(-1)
        rc = self.lib.ncg_pairing_batch_dev(self.h, n_pairs, g1_ptr, g2_ptr, off.shape[0] - 1, off.ctypes.data, flags, out_gt_ptr, out_is_one_ptr,
                                            ctypes.byref(bad), stream)
        if rc:
            raise self._pairing_error(rc, bad)

    def bls_verify_batch(self, scheme, pk_enc, sig_enc, u):
        """verify per row from bytes: scheme 0 pk [n, 48] / sig [n, 96] / u [n, 192], scheme 1 pk [n, 96] / sig [n, 48] / u [n, 96]
        (u = hash_to_field of the message, count 2) -> bool [n]"""
        if scheme not in (BLS_LONG_SIGNATURES, BLS_SHORT_SIGNATURES):    # the library's own refusal and message
            self._check(self.lib.ncg_bls_verify_batch(self.h, scheme, 1, None, None, None, None))
        pw, sw, uw = (48, 96, 192) if scheme == 0 else (96, 48, 96)
        pk = np.ascontiguousarray(pk_enc, dtype=np.uint8).reshape(-1, pw)
        sig = np.ascontiguousarray(sig_enc, dtype=np.uint8).reshape(-1, sw)
        u = np.ascontiguousarray(u, dtype=np.uint8).reshape(-1, uw)
        n = pk.shape[0]
        if sig.shape[0] != n or u.shape[0] != n:
            raise ValueError("arrays of keys, signatures and messages must have equal length")
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_bls_verify_batch(self.h, scheme, n, pk.ctypes.data, sig.ctypes.data, u.ctypes.data, ok.ctypes.data))
        return ok.astype(bool)

    def bls_verify_batch_dev(self, scheme, n, pk_ptr, sig_ptr, u_ptr, out_ok_ptr, stream=None):
        self._check(self.lib.ncg_bls_verify_batch_dev(self.h, scheme, n, pk_ptr, sig_ptr, u_ptr, out_ok_ptr, stream))

    def fp12_batch(self, op, a, b=None):
        """bls12_381.fields.Fp12 per row: out[i] = op(a[i], b[i]) -> [n, 576], or bool [n] for FP12_IS_ONE"""
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 576)
        n = a.shape[0]
        bw = 576 if op == FP12_MUL else 288 if op == FP12_MUL014 else 0
        if bw:
            b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, bw)
            if b.shape[0] != n:
                raise ValueError("arrays of operands must have equal length")
        out = np.zeros((n,), dtype=np.uint8) if op == FP12_IS_ONE else np.zeros((n, 576), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_fp12_batch(self.h, op, n, a.ctypes.data, b.ctypes.data if bw else None, out.ctypes.data))
        return out.astype(bool) if op == FP12_IS_ONE else out

    def fp12_batch_dev(self, op, n, a_ptr, b_ptr, out_ptr, stream=None):
        self._check(self.lib.ncg_fp12_batch_dev(self.h, op, n, a_ptr, b_ptr, out_ptr, stream))

    def ed25519_verify_batch_msgs(self, sigs, pks, msgs_blob, msg_off, zip215=True):
        """sigs uint8 [n,64], pks [n,32], msgs_blob uint8 [total], msg_off uint64 [n+1] -> bool array [n];
        the challenge hash SHA-512(R || A || M) mod L runs on the device."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        pks = np.ascontiguousarray(pks, dtype=np.uint8).reshape(-1, 32)
        blob = np.ascontiguousarray(msgs_blob, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(msg_off, dtype=np.uint64).reshape(-1)
        n = sigs.shape[0]
        if pks.shape[0] != n or off.shape[0] != n + 1:
            raise ValueError("arrays of signatures, public keys and message offsets must have matching lengths")
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed25519_verify_batch_msgs(self.h, n, sigs.ctypes.data, pks.ctypes.data,
                                                               blob.ctypes.data if blob.size else None, off.ctypes.data,
                                                               1 if zip215 else 0, ok.ctypes.data))
        return ok.astype(bool)

    def ed25519_verify_batch_msgs_dev(self, n, d_sigs, d_pks, d_msgs, d_off, zip215, d_ok, stream=None):
        self._check(self.lib.ncg_ed25519_verify_batch_msgs_dev(self.h, n, d_sigs, d_pks, d_msgs, d_off,
                                                               1 if zip215 else 0, d_ok, stream))

    def ed25519_challenge_batch_dev(self, n, d_sigs, d_pks, d_msgs, d_off, d_ks, stream=None):
        self._check(self.lib.ncg_ed25519_challenge_batch_dev(self.h, n, d_sigs, d_pks, d_msgs, d_off, d_ks, stream))

    def ed25519_verify_batch_dev(self, n, d_sigs, d_pks, d_ks, zip215, d_ok, stream=None):
        self._check(self.lib.ncg_ed25519_verify_batch_dev(self.h, n, d_sigs, d_pks, d_ks, 1 if zip215 else 0,
                                                          d_ok, stream))

    def ecdsa_verify_batch(self, sigs, hashes, pubs, low_s=True):
        """secp256k1: sigs uint8 [n,64] (r || s big-endian), hashes [n,32], pubs [n,33] SEC1 compressed or [n,65]
        uncompressed -> bool [n] (ecdsa.verify with prehash: false, format 'compact'; weierstrass.ts:1571-1620)."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        hashes = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
        pubs = np.ascontiguousarray(pubs, dtype=np.uint8)
        n = sigs.shape[0]
        kb = 65 if (pubs.ndim == 2 and pubs.shape[1] == 65) else 33
        pubs = pubs.reshape(-1, kb)
        if hashes.shape[0] != n or pubs.shape[0] != n:
            raise ValueError("arrays of signatures, message hashes and public keys must have equal length")
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            flags = (1 if low_s else 0) | (2 if kb == 65 else 0)
            self._check(self.lib.ncg_ecdsa_verify_batch(self.h, SECP256K1, n, sigs.ctypes.data, hashes.ctypes.data,
                                                        pubs.ctypes.data, flags, ok.ctypes.data))
        return ok.astype(bool)

    def ecdsa_recover_batch(self, sigs65, hashes):
        """secp256k1: sigs65 uint8 [n,65] (recid || r || s), hashes [n,32] -> (affine points [n,64], ok [n] bool):
        Signature.recoverPublicKey (weierstrass.ts:1391-1407)."""
        sigs = np.ascontiguousarray(sigs65, dtype=np.uint8).reshape(-1, 65)
        hashes = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
        n = sigs.shape[0]
        if hashes.shape[0] != n:
            raise ValueError("arrays of signatures and message hashes must have equal length")
        out = np.zeros((n, 64), dtype=np.uint8)
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ecdsa_recover_batch(self.h, SECP256K1, n, sigs.ctypes.data, hashes.ctypes.data,
                                                         out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    @staticmethod
    def _msg_blob(msgs):
        off = np.zeros((len(msgs) + 1,), np.uint64)
        if len(msgs):
            off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        blob = np.frombuffer(b"".join(bytes(m) for m in msgs), np.uint8) if len(msgs) and off[-1] else np.zeros((0,), np.uint8)
        return blob, off

    def ecdsa_verify_batch_msgs(self, sigs, msgs, pubs, low_s=True):
        """The same as ecdsa_verify_batch from the messages themselves: SHA-256 (the reference's prehash) on the device."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        pubs = np.ascontiguousarray(pubs, dtype=np.uint8)
        n = sigs.shape[0]
        kb = 65 if (pubs.ndim == 2 and pubs.shape[1] == 65) else 33
        pubs = pubs.reshape(-1, kb)
        if len(msgs) != n or pubs.shape[0] != n:
            raise ValueError("arrays of signatures, messages and public keys must have equal length")
        blob, off = self._msg_blob(msgs)
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            flags = (1 if low_s else 0) | (2 if kb == 65 else 0)
            self._check(self.lib.ncg_ecdsa_verify_batch_msgs(self.h, SECP256K1, n, sigs.ctypes.data, blob.ctypes.data if blob.size else None,
                                                             off.ctypes.data, pubs.ctypes.data, flags, ok.ctypes.data))
        return ok.astype(bool)

    def schnorr_verify_batch_msgs(self, sigs, msgs, pubs):
        """BIP-340 verification from the messages: the tagged challenge hash runs on the device too."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        pubs = np.ascontiguousarray(pubs, dtype=np.uint8).reshape(-1, 32)
        n = sigs.shape[0]
        if len(msgs) != n or pubs.shape[0] != n:
            raise ValueError("arrays of signatures, messages and public keys must have equal length")
        blob, off = self._msg_blob(msgs)
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_schnorr_verify_batch_msgs(self.h, n, sigs.ctypes.data, blob.ctypes.data if blob.size else None,
                                                               off.ctypes.data, pubs.ctypes.data, ok.ctypes.data))
        return ok.astype(bool)

    def schnorr_verify_batch(self, sigs, challenges, pubs):
        """BIP-340: sigs uint8 [n,64], challenges [n,32] (e mod n, big-endian), pubs [n,32] x-only -> bool [n]
        (src/secp256k1.ts:228-258 after the host-side tagged hash)."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        es = np.ascontiguousarray(challenges, dtype=np.uint8).reshape(-1, 32)
        pubs = np.ascontiguousarray(pubs, dtype=np.uint8).reshape(-1, 32)
        n = sigs.shape[0]
        if es.shape[0] != n or pubs.shape[0] != n:
            raise ValueError("arrays of signatures, challenges and public keys must have equal length")
        ok = np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_schnorr_verify_batch(self.h, n, sigs.ctypes.data, es.ctypes.data, pubs.ctypes.data,
                                                          ok.ctypes.data))
        return ok.astype(bool)

    def schnorr_verify_batch_dev(self, n, d_sigs, d_es, d_pubs, d_ok, stream=None):
        self._check(self.lib.ncg_schnorr_verify_batch_dev(self.h, n, d_sigs, d_es, d_pubs, d_ok, stream))

    def ecdsa_verify_batch_dev(self, n, d_sigs, d_hashes, d_pubs, low_s, d_ok, stream=None, uncompressed=False):
        self._check(self.lib.ncg_ecdsa_verify_batch_dev(self.h, SECP256K1, n, d_sigs, d_hashes, d_pubs,
                                                        (1 if low_s else 0) | (2 if uncompressed else 0), d_ok, stream))

    # ---- secp256k1 signing: keys, hashes, extra entropy and aux rows uint8 [n, 32] big-endian, signatures [n, 64] ----------------
    def secp256k1_public_key_batch(self, secret_keys, mode=SECP_PK_COMPRESSED):
        """secp256k1.getPublicKey (33 or 65 bytes) / schnorr.getPublicKey (x-only, 32 bytes) per row -> (keys uint8 [n, w], ok bool [n]);
        a key outside [1, n) gives a zero row and ok False"""
        sk = np.ascontiguousarray(secret_keys, dtype=np.uint8).reshape(-1, 32)
        n = sk.shape[0]
        out, ok = np.zeros((n, SECP_PK_BYTES[mode]), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_secp256k1_public_key_batch(self.h, n, sk.ctypes.data, mode, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def ecdsa_sign_batch(self, secret_keys, hashes=None, msgs=None, extra=None, low_s=True, one_key=False):
        """ECDSA with RFC 6979 nonces over 32-byte hashes (prehash: false) or, with msgs, over SHA-256 of each message computed on the
        device (prehash: true).  secret_keys [n, 32], or ONE row with one_key; extra: None or [n, 32] extra entropy
        -> (signatures uint8 [n, 64] r || s, recovery ids uint8 [n], ok bool [n]); a refused row is zero."""
        sk = np.ascontiguousarray(secret_keys, dtype=np.uint8).reshape(-1, 32)
        if (hashes is None) == (msgs is None):
            raise ValueError("ecdsa_sign_batch takes hashes or messages")
        if msgs is None:
            hashes = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
            n = hashes.shape[0]
        else:
            n = len(msgs)
            blob, off = self._msg_blob(msgs)
        if sk.shape[0] != (1 if one_key else n):
            raise ValueError("arrays of secret keys and messages must have matching lengths")
        if extra is not None:
            extra = np.ascontiguousarray(extra, dtype=np.uint8).reshape(-1, 32)
            if extra.shape[0] != n:
                raise ValueError("one row of extra entropy per message")
        flags = (ECDSA_LOW_S if low_s else 0) | (SECP_SIGN_ONE_KEY if one_key else 0)
        sig, rec, ok = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            xp = None if extra is None else extra.ctypes.data
            if msgs is None:
                self._check(self.lib.ncg_ecdsa_sign_batch(self.h, SECP256K1, n, sk.ctypes.data, hashes.ctypes.data, xp, flags, sig.ctypes.data,
                                                          rec.ctypes.data, ok.ctypes.data))
            else:
                self._check(self.lib.ncg_ecdsa_sign_batch_msgs(self.h, SECP256K1, n, sk.ctypes.data, blob.ctypes.data if blob.size else None,
                                                               off.ctypes.data, xp, flags, sig.ctypes.data, rec.ctypes.data, ok.ctypes.data))
        return sig, rec, ok.astype(bool)

    def schnorr_sign_batch(self, secret_keys, aux, msgs, one_key=False):
        """BIP-340 signatures without the reference's self-verification: secret_keys [n, 32] (ONE row with one_key), aux [n, 32]
        -> (signatures uint8 [n, 64], ok bool [n]); a refused row is zero."""
        sk = np.ascontiguousarray(secret_keys, dtype=np.uint8).reshape(-1, 32)
        aux = np.ascontiguousarray(aux, dtype=np.uint8).reshape(-1, 32)
        n = len(msgs)
        if sk.shape[0] != (1 if one_key else n) or aux.shape[0] != n:
            raise ValueError("arrays of secret keys, aux rows and messages must have matching lengths")
        blob, off = self._msg_blob(msgs)
        sig, ok = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_schnorr_sign_batch(self.h, n, sk.ctypes.data, aux.ctypes.data, blob.ctypes.data if blob.size else None,
                                                        off.ctypes.data, SECP_SIGN_ONE_KEY if one_key else 0, sig.ctypes.data, ok.ctypes.data))
        return sig, ok.astype(bool)

    def secp256k1_sign_check(self, op, a_words, b_words, variant=0):
        """The lane code of secp256k1 signing on raw uint32 rows (ncg_secp256k1_sign_check; SECP_SIGN_CHECK_WORDS has the widths):
        a [n, wa], b [n, wb] -> out [n, wo]; an op nobody defines gives rows of 16 zero words."""
        wa, wb, wo = SECP_SIGN_CHECK_WORDS.get(op, (1, 1, 0))
        a = np.ascontiguousarray(a_words, dtype=np.uint32).reshape(-1, wa) if op in SECP_SIGN_CHECK_WORDS else np.ascontiguousarray(a_words, dtype=np.uint32)
        b = np.ascontiguousarray(b_words, dtype=np.uint32).reshape(-1, wb) if op in SECP_SIGN_CHECK_WORDS else np.ascontiguousarray(b_words, dtype=np.uint32)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("secp256k1_sign_check: op %d takes rows of %d and %d words" % (op, wa, wb))
        out = np.zeros((n, wo if wo else 16), dtype=np.uint32)
        if n:
            self._check(self.lib.ncg_secp256k1_sign_check(self.h, op, variant, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def map_to_curve_batch(self, curve, u, count):
        """u uint8 [n, count * FIELD_BYTES * (2 for G2)] -> (affine [n, PB], is_inf [n]):
        clearCofactor(sum of the `count` mapped points) per row (bls12-381 G1 / G2)."""
        pb = POINT_BYTES[curve]
        u = np.ascontiguousarray(u, dtype=np.uint8).reshape(-1, count * pb // 2)
        n = u.shape[0]
        out = np.empty((n, pb), dtype=np.uint8)
        inf = np.empty((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_map_to_curve_batch(self.h, curve, n, count, u.ctypes.data, out.ctypes.data,
                                                        inf.ctypes.data))
        return out, inf

    def map_to_curve_batch_dev(self, curve, n, count, d_u, d_out, d_inf, stream):
        self._check(self.lib.ncg_map_to_curve_batch_dev(self.h, curve, n, count, d_u, d_out, d_inf, stream))

    # ---- RFC 9380 for secp256k1 and edwards25519 (suite H2C_SECP256K1 / H2C_EDWARDS25519): messages a list of byte strings, points
    # affine wire rows uint8 [n, 64] of the suite's curve with is_inf uint8 [n], count 2 (hashToCurve) or 1 (encodeToCurve) ----------
    def h2c_hash_batch(self, suite, msgs, dst, count):
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out, inf = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_h2c_hash_batch(self.h, suite, n, count, blob.ctypes.data if blob.size else None, off.ctypes.data, dst,
                                                    len(dst), out.ctypes.data, inf.ctypes.data))
        return out, inf

    def h2c_map_batch(self, suite, u48, count):
        """u48 uint8 [n, count * 48]: count values per row, 48 bytes little-endian each, any value below 2^384"""
        u48 = np.ascontiguousarray(u48, dtype=np.uint8).reshape(-1, count * 48)
        n = u48.shape[0]
        out, inf = np.zeros((n, 64), dtype=np.uint8), np.zeros((n,), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_h2c_map_batch(self.h, suite, n, count, u48.ctypes.data, out.ctypes.data, inf.ctypes.data))
        return out, inf

    def h2c_hash_to_scalar_batch(self, suite, msgs, dst):
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out = np.zeros((n, 32), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_h2c_hash_to_scalar_batch(self.h, suite, n, blob.ctypes.data if blob.size else None, off.ctypes.data, dst,
                                                              len(dst), out.ctypes.data))
        return out

    def h2c_hash_to_field_batch(self, suite, msgs, dst, count):
        """-> uint8 [n, count * 32]: the reduced elements, little-endian"""
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out = np.zeros((n, count * 32), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_h2c_hash_to_field_batch(self.h, suite, n, count, blob.ctypes.data if blob.size else None, off.ctypes.data,
                                                             dst, len(dst), out.ctypes.data))
        return out

    def xmd_sha256_batch(self, msgs, dst, out_len):
        """expand_message_xmd over SHA-256 of every message -> uint8 [n, out_len]"""
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out = np.zeros((n, out_len), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_xmd_sha256_batch(self.h, n, blob.ctypes.data if blob.size else None, off.ctypes.data, dst, len(dst),
                                                      out_len, out.ctypes.data))
        return out

    def h2c_check(self, op, a):
        """the lane code of csrc/h2c_suites.hpp on raw words: a uint32 [n, 24] -> uint32 [n, 24] (ncg_h2c_check)"""
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 24)
        out = np.zeros_like(a)
        if a.shape[0]:
            self._check(self.lib.ncg_h2c_check(self.h, op, a.shape[0], a.ctypes.data, out.ctypes.data))
        return out

    # ---- RFC 9380 for edwards448 (edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_) and the hash side of decaf448: messages a list of byte
    # strings, elements / scalars / encodings uint8 [n, 56] little-endian, points x || y uint8 [n, 112] with the identity as (0, 1) ----
    def _h2c448_rows(self, fn, msgs, dst, width, *lead):
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out = np.zeros((n, width), dtype=np.uint8)
        if n:
            self._check(fn(self.h, n, *lead, blob.ctypes.data if blob.size else None, off.ctypes.data, dst, len(dst), out.ctypes.data))
        return out

    def xof_shake256_batch(self, msgs, dst, out_len):
        """expand_message_xof over SHAKE256 of every message -> uint8 [n, out_len]"""
        blob, off = self._blob(msgs)
        dst, n = bytes(dst), len(msgs)
        out = np.zeros((n, out_len), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_xof_shake256_batch(self.h, n, blob.ctypes.data if blob.size else None, off.ctypes.data, dst, len(dst),
                                                        out_len, out.ctypes.data))
        return out

    def ed448_h2c_hash_batch(self, msgs, dst, count):
        """hashToCurve (count 2) / encodeToCurve (count 1) -> uint8 [n, 112]"""
        return self._h2c448_rows(self.lib.ncg_ed448_h2c_hash_batch, msgs, dst, 112, count)

    def ed448_h2c_map_batch(self, u56, count):
        """u56 uint8 [n, count * 56]: count values per row, 56 bytes little-endian each, any value below 2^448 -> uint8 [n, 112]"""
        u56 = np.ascontiguousarray(u56, dtype=np.uint8).reshape(-1, count * 56)
        n = u56.shape[0]
        out = np.zeros((n, 112), dtype=np.uint8)
        if n:
            self._check(self.lib.ncg_ed448_h2c_map_batch(self.h, n, count, u56.ctypes.data, out.ctypes.data))
        return out

    def ed448_h2c_hash_to_field_batch(self, msgs, dst, count):
        """-> uint8 [n, count * 56]: the reduced elements, little-endian"""
        return self._h2c448_rows(self.lib.ncg_ed448_h2c_hash_to_field_batch, msgs, dst, count * 56, count)

    def ed448_h2c_hash_to_scalar_batch(self, msgs, dst):
        return self._h2c448_rows(self.lib.ncg_ed448_h2c_hash_to_scalar_batch, msgs, dst, 56)

    def decaf448_hash_to_group_batch(self, msgs, dst):
        """decaf448_hasher.hashToCurve -> the encoded elements uint8 [n, 56]"""
        return self._h2c448_rows(self.lib.ncg_decaf448_hash_to_group_batch, msgs, dst, 56)

    def decaf448_hash_to_scalar_batch(self, msgs, dst):
        return self._h2c448_rows(self.lib.ncg_decaf448_hash_to_scalar_batch, msgs, dst, 56)

    def h2c448_check(self, op, a):
        """the lane code of csrc/h2c448.hpp on raw words: a uint32 [n, 42] -> uint32 [n, 42] (ncg_h2c448_check)"""
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 42)
        out = np.zeros_like(a)
        if a.shape[0]:
            self._check(self.lib.ncg_h2c448_check(self.h, op, a.shape[0], a.ctypes.data, out.ctypes.data))
        return out

    @staticmethod
    def _ntt_flags(inverse, brp_input, brp_output):
        return (1 if inverse else 0) | (2 if brp_input else 0) | (4 if brp_output else 0)

    def ntt(self, log2n, data, omega, inverse=False, brp_input=False, brp_output=False, field=FIELD_BLS12_381_FR):
        """data uint8 [batch * 2^log2n, 32] (canonical LE residues of the scalar field `field`: FIELD_BLS12_381_FR or
        FIELD_BN254_FR) -> transformed copy; omega: int, the primitive 2^log2n-th root of unity (roots.omega(log2n))."""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, 32)
        n = 1 << log2n
        if data.shape[0] % n:
            raise ValueError("noble-gpu: ntt: data is not a whole number of 2^%d-point polynomials" % log2n)
        out = np.empty_like(data)
        om = np.frombuffer(int(omega).to_bytes(32, "little"), dtype=np.uint8).copy()
        if data.shape[0]:
            self._check(self.lib.ncg_ntt(self.h, field, log2n, data.shape[0] // n, om.ctypes.data,
                                         data.ctypes.data, out.ctypes.data,
                                         self._ntt_flags(inverse, brp_input, brp_output)))
        return out

    def ntt_dev(self, log2n, batch, omega, d_in, d_out, stream, inverse=False, brp_input=False, brp_output=False,
                field=FIELD_BLS12_381_FR):
        om = np.frombuffer(int(omega).to_bytes(32, "little"), dtype=np.uint8).copy()
        self._check(self.lib.ncg_ntt_dev(self.h, field, log2n, batch, om.ctypes.data, d_in, d_out,
                                         self._ntt_flags(inverse, brp_input, brp_output), stream))

    # ---- polynomial arithmetic on vectors of scalar-field elements (ncg_poly_*) ------------------
    @staticmethod
    def _fr_vec(data):
        return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, 32)

    @staticmethod
    def _fr_small(values):
        """ints -> the host operand of a poly call: uint8 [len, 32]"""
        return ints_to_le([int(v) for v in values], 32)

    def poly_pointwise(self, op, a, b, field=FIELD_BLS12_381_FR):
        """a, b uint8 [n, 32] -> a[i] + b[i] (POLY_ADD), a[i] - b[i] (POLY_SUB) or a[i] * b[i] (POLY_DOT)"""
        a, b = self._fr_vec(a), self._fr_vec(b)
        if a.shape != b.shape:
            raise ValueError("noble-gpu: poly_pointwise: operand arrays differ in length")
        out = np.empty_like(a)
        self._check(self.lib.ncg_poly_pointwise(self.h, field, op, a.shape[0], a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def poly_pointwise_dev(self, op, n, d_a, d_b, d_out, stream, field=FIELD_BLS12_381_FR):
        self._check(self.lib.ncg_poly_pointwise_dev(self.h, field, op, n, d_a, d_b, d_out, stream))

    def poly_scale(self, a, scalar, powers=False, field=FIELD_BLS12_381_FR):
        """a uint8 [n, 32], scalar int -> a[i] * scalar, or a[i] * scalar^i with powers (the reference's shift)"""
        a = self._fr_vec(a)
        out = np.empty_like(a)
        s = self._fr_small([scalar])
        self._check(self.lib.ncg_poly_scale(self.h, field, a.shape[0], a.ctypes.data, s.ctypes.data, 1 if powers else 0, out.ctypes.data))
        return out

    def poly_scale_dev(self, n, d_a, scalar, powers, d_out, stream, field=FIELD_BLS12_381_FR):
        s = self._fr_small([scalar])
        self._check(self.lib.ncg_poly_scale_dev(self.h, field, n, d_a, s.ctypes.data, 1 if powers else 0, d_out, stream))

    def poly_eval(self, a, basis, field=FIELD_BLS12_381_FR):
        """sum a[i] * basis[i] -> int"""
        a, basis = self._fr_vec(a), self._fr_vec(basis)
        if a.shape != basis.shape:
            raise ValueError("noble-gpu: poly_eval: operand arrays differ in length")
        out = np.empty((1, 32), dtype=np.uint8)
        self._check(self.lib.ncg_poly_eval(self.h, field, a.shape[0], a.ctypes.data, basis.ctypes.data, out.ctypes.data))
        return le_to_ints(out, 32)[0]

    def poly_eval_dev(self, n, d_a, d_basis, d_out32, stream, field=FIELD_BLS12_381_FR):
        self._check(self.lib.ncg_poly_eval_dev(self.h, field, n, d_a, d_basis, d_out32, stream))

    def poly_eval_monomial(self, a, xs, field=FIELD_BLS12_381_FR):
        """[sum a[i] * x^i for x in xs] (1 to POLY_MAX_POINTS points, one pass over a) -> list of ints"""
        a = self._fr_vec(a)
        x = self._fr_small(xs)
        out = np.empty((max(len(xs), 1), 32), dtype=np.uint8)
        self._check(self.lib.ncg_poly_eval_monomial(self.h, field, a.shape[0], a.ctypes.data, len(xs), x.ctypes.data, out.ctypes.data))
        return le_to_ints(out, 32)[:len(xs)]

    def poly_eval_monomial_dev(self, n, d_a, xs, d_out, stream, field=FIELD_BLS12_381_FR):
        x = self._fr_small(xs)
        self._check(self.lib.ncg_poly_eval_monomial_dev(self.h, field, n, d_a, len(xs), x.ctypes.data, d_out, stream))

    def poly_lagrange_basis(self, log2n, omega, x, brp=False, field=FIELD_BLS12_381_FR):
        """L_i(x) over the 2^log2n roots of unity of omega (bit-reversed order with brp) -> uint8 [2^log2n, 32]"""
        om, xx = self._fr_small([omega]), self._fr_small([x])
        out = np.empty((1 << log2n, 32), dtype=np.uint8)
        self._check(self.lib.ncg_poly_lagrange_basis(self.h, field, log2n, om.ctypes.data, xx.ctypes.data, 1 if brp else 0, out.ctypes.data))
        return out

    def poly_lagrange_basis_dev(self, log2n, omega, x, brp, d_out, stream, field=FIELD_BLS12_381_FR):
        om, xx = self._fr_small([omega]), self._fr_small([x])
        self._check(self.lib.ncg_poly_lagrange_basis_dev(self.h, field, log2n, om.ctypes.data, xx.ctypes.data, 1 if brp else 0, d_out, stream))

    def poly_mul(self, log2n, omega, a, b, field=FIELD_BLS12_381_FR):
        """cyclic product of length 2^log2n of a (na <= 2^log2n rows) and b (nb rows), zero-extended on the device"""
        a, b = self._fr_vec(a), self._fr_vec(b)
        om = self._fr_small([omega])
        out = np.empty((1 << log2n, 32), dtype=np.uint8)
        self._check(self.lib.ncg_poly_mul(self.h, field, log2n, om.ctypes.data, a.shape[0], a.ctypes.data, b.shape[0], b.ctypes.data,
                                          out.ctypes.data))
        return out

    def poly_mul_dev(self, log2n, omega, na, d_a, nb, d_b, d_out, stream, field=FIELD_BLS12_381_FR):
        om = self._fr_small([omega])
        self._check(self.lib.ncg_poly_mul_dev(self.h, field, log2n, om.ctypes.data, na, d_a, nb, d_b, d_out, stream))

    def field_check(self, field, op, variant, a_words, b_words):
        """Device field code on raw operands (ncg_field_check): a_words, b_words uint32 [n, 9] (fields 0/1),
        [n, 12] (field 2), [n, 28] (field 3: raw Fe29 limbs [a, c]), [n, 56] (field 4: lane-paired Fp2 raw limbs),
        [n, 18] (fields 5/6: fused Fe9 expressions, raw limbs [a, c] and [b, d]), a [n, 27] and b [n, 18] (field 7:
        secp256k1 ladder pieces) or [n, 9] (field 8: fr29 raw limbs, variant 0 bls12-381 Fr, 1 bn254 Fr; field 9: bn254 Montgomery raw limbs) -> uint32
        [n, 8 | 8 | 12 | 12 | 24 | 9 | 9 | 27 | 9 | 9].  Fields 3 / 4, op 7: out[:, 0] = f_eqz of the element a taken at the value bound
        `variant` (4, 66 or 128: the bounds under the branches of the group law), the rest zero.
        Fields 10-14: the group law of the MSM buckets on STORED accumulators (secp256k1, ed25519, bls12-381 G1, lane-paired G2,
        bn254 G1): a, b and the result [n, 36 | 36 | 56 | 112 | 36] raw words in acc_load's layout (for ops 0 / 1 b starts with a
        stored input point).  ops 0 madd(a, b), 1 madd(a, -b), 2 add, 3 dbl; fields 12 / 13 also the four-lane form: 8 add, 9 / 10
        add with out aliasing a / b, 11 dbl, 12 dbl in place, 13 copy (elsewhere those leave out zero).
        Field 16: the X25519 ladder pieces, a [n, 36], b [n, 9] -> [n, 36] (op 0 one ladder step on raw limbs, 1 decodeU + low-order
        flag, 2 adjustScalarBytes; include/ncg.h).  Field 17: the ristretto255 pieces, the same shapes (op 0 SQRT_RATIO_M1, 1 the
        encoder on X Y Z T, 2 the Elligator map)."""
        a = np.ascontiguousarray(a_words, dtype=np.uint32)
        b = np.ascontiguousarray(b_words, dtype=np.uint32)
        n = a.shape[0]
        if field not in FIELD_CHECK_WORDS:
            raise ValueError("field_check: unknown field %d" % field)
        wa, wb, wo = FIELD_CHECK_WORDS[field]
        if a.shape != (n, wa) or b.shape != (n, wb):   # the library reads n * wa and n * wb words
            raise ValueError("field_check: field %d takes a [n, %d] and b [n, %d]" % (field, wa, wb))
        out = np.zeros((n, wo), dtype=np.uint32)
        if n:
            self._check(self.lib.ncg_field_check(self.h, field, op, variant, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def ubench(self, kind, blocks, threads, iters):
        ms = ctypes.c_float()
        self._check(self.lib.ncg_ubench(self.h, kind, blocks, threads, iters, ctypes.byref(ms)))
        return ms.value


class ResidentPoints:
    """A point set kept in device memory (ncg_points): run MSMs / batch multiplies against it with only
    the scalars crossing."""

    def __init__(self, engine, handle, curve):
        self.engine, self.h, self.curve = engine, handle, curve

    def __len__(self):
        return int(self.engine.lib.ncg_points_count(self.h)) if self.h else 0

    def dev_ptr(self):
        return self.engine.lib.ncg_points_dev(self.h)

    def verify_subgroup(self):
        """bls12-381 G1 / G2: run the reference's subgroup test on every point once (ncg_points_verify_subgroup);
        if all pass, MSMs on this set take the endomorphism path.  Returns -1, or the index of the first point
        outside the prime-order subgroup (the set then keeps the generic path)."""
        bad = ctypes.c_int64(-1)
        self.engine._check(self.engine.lib.ncg_points_verify_subgroup(self.engine.h, self.h, ctypes.byref(bad)))
        return int(bad.value)

    def precompute(self):
        """Build the window-shifted copies of the set once (ncg_points_precompute: the device form of
        interleavedMSMUnsafe's per-point tables, curve.ts:907-959); later MSMs add every window into one bucket
        set.  Returns True if the shared-bucket path is active afterwards (sets of >= 4096 Weierstrass points)."""
        self.engine._check(self.engine.lib.ncg_points_precompute(self.engine.h, self.h))
        return self.precomputed

    @property
    def precomputed(self):
        return bool(self.engine.lib.ncg_points_precomputed(self.h)) if self.h else False

    @property
    def in_subgroup(self):
        """True once the set is known to lie in the prime-order subgroup (decoded, or verified)."""
        return bool(self.engine.lib.ncg_points_in_subgroup(self.h)) if self.h else False

    def free(self):
        if getattr(self, "h", None):
            self.engine.lib.ncg_points_free(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            if getattr(self.engine, "h", None):
                self.free()
        except Exception:
            pass

    def msm(self, scalars):
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        if scalars.shape[0] != len(self):
            raise ValueError("arrays of points and scalars must have equal length")
        out = np.zeros((POINT_BYTES[self.curve],), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self.engine._check(self.engine.lib.ncg_msm_resident(self.engine.h, self.h, scalars.ctypes.data if scalars.size else None,
                                                            out.ctypes.data, ctypes.byref(inf)))
        return out, bool(inf.value)

    def msm_dev(self, d_scalars, stream=None):
        """The same with the scalars already on the device (raw pointer, 32 B LE each, len(self) of them)."""
        out = np.zeros((POINT_BYTES[self.curve],), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        self.engine._check(self.engine.lib.ncg_msm_resident_dev(self.engine.h, self.h, d_scalars, out.ctypes.data,
                                                                ctypes.byref(inf), stream))
        return out, bool(inf.value)

    def mul_var_batch(self, scalars):
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = len(self)
        if scalars.shape[0] != n:
            raise ValueError("arrays of points and scalars must have equal length")
        out = np.empty((n, POINT_BYTES[self.curve]), dtype=np.uint8)
        inf = np.empty((n,), dtype=np.uint8)
        if n:
            self.engine._check(self.engine.lib.ncg_mul_var_batch_resident(self.engine.h, self.h, scalars.ctypes.data,
                                                                          out.ctypes.data, inf.ctypes.data))
        return out, inf

    def mul_var_batch_dev(self, d_scalars, d_out, d_inf, stream=None):
        """The same with scalars, results and infinity flags in device memory (raw pointers)."""
        self.engine._check(self.engine.lib.ncg_mul_var_batch_resident_dev(self.engine.h, self.h, d_scalars, d_out, d_inf, stream))


class MultiEngine:
    """One process driving several GPUs (include/ncg.h "multi-GPU MSM" (2)): a context per device and one
    RCCL communicator over the set; `msm` shards host arrays over the devices."""

    def __init__(self, device_ids):
        self.lib = load_library()
        ids = (ctypes.c_int * len(device_ids))(*device_ids)
        h = ctypes.c_void_p()
        rc = self.lib.ncg_multi_init(ids, len(device_ids), ctypes.byref(h))
        if rc != 0:
            raise NativeError((self.lib.ncg_last_error(None) or b"").decode() or "noble-gpu: ncg_multi_init failed (%d)" % rc)
        self.h = h

    def devices(self):
        return self.lib.ncg_multi_devices(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ncg_multi_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def msm(self, curve, points, scalars):
        pb = POINT_BYTES[curve]
        points = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, pb)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = points.shape[0]
        if scalars.shape[0] != n:
            raise ValueError("arrays of points and scalars must have equal length")
        out = np.zeros((pb,), dtype=np.uint8)
        inf = ctypes.c_uint8(0)
        rc = self.lib.ncg_msm_multi(self.h, curve, n, points.ctypes.data if n else None,
                                    scalars.ctypes.data if n else None, out.ctypes.data, ctypes.byref(inf))
        if rc != 0:
            raise NativeError((self.lib.ncg_multi_last_error(self.h) or b"").decode() or "noble-gpu: msm_multi failed")
        return out, bool(inf.value)


_engines = {}


def get_engine(device=None):
    """Process-wide engine for `device` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    eng = _engines.get(device)
    if eng is None:
        eng = Engine(device)
        _engines[device] = eng
    return eng
