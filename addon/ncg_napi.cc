// N-API addon: the binding a noble-curves maintainer would add to reach libncg.so from the
// reference's TypeScript/JavaScript side.  Synchronous, like every call on
// the reference's path (there is no async anywhere in src/abstract/curve.ts).
//
//   init(deviceId = 0)                               -> undefined (throws Error('noble-gpu: ...'))
//   msm(curveId, points: Uint8Array, scalars: Uint8Array)            -> Uint8Array PB + 1 (flag)
//   mulVarBatch(curveId, points, scalars[, out])     -> Uint8Array n * (PB + 1)  (points then flags; `out`: reuse the caller's array)
//   mulBaseBatch(curveId, scalars)                   -> Uint8Array n * (PB + 1)
//   ed25519VerifyBatch(sigs, pks, ks, zip215: bool)  -> Uint8Array n (0 / 1)
//   x25519(kind, scalars | null, rows)               -> Uint8Array n * 33 (32-byte results, then ok flags); kind 0 scalarMult
//                                                       (scalars: n rows, or ONE row used for every u), 1 getPublicKey, 2 toMontgomery
//   secpSign(kind, keys, flags | mode[, data, lens, extra]) -> secp256k1 public keys (kind 0), ECDSA signatures with RFC 6979 nonces
//       (kind 1) and BIP-340 signatures (kind 2) on packed rows; see SecpSign
//   ed25519Sign(kind, keys[, flags, dom, msgs, lens]) -> kind 0 getPublicKey (keys: n x 32) -> Uint8Array n * 32; kind 1 sign (keys: n rows
//                                                       or ONE, flags: 4 = prehash, dom, msgs back to back, lens: n LE uint32) ->
//                                                       Uint8Array n * 65 (64-byte signatures, then ok flags)
//   ed448(kind, a | null, b, c)                      -> kind 0 x448.scalarMult (a scalars: n rows or ONE, b u rows), 1 x448.getPublicKey (b):
//                                                       Uint8Array n * 57 (56-byte results, then ok flags); 2 ed448 verify (a signatures,
//                                                       b public keys, c challenges) -> Uint8Array n (0 / 1)
//   oprf(op, mode, flags, a, b, c, d)             -> the ristretto255 OPRF on packed rows (ncg_oprf_*): see Oprf below
//   ristretto(mode, a, b | null)                   -> ristretto255 on packed rows; mode 0 decode (a: n x 32) -> n x 64 points + n ok flags,
//                                                       1 encode (a: n x 64) -> n x 32, 2 equals (a, b: n x 64) -> n flags,
//                                                       3 deriveToCurve (a: n x 64) -> n x 32, 4 multiply (a: n x 32 encodings, b: n or ONE
//                                                       scalar row) -> n x 32 + n ok flags, 5 BASE.multiply (a: n x 32 scalars) -> n x 32,
//                                                       6 msm (a: encodings, b: scalars) -> 32 bytes; throws naming a bad index
//   decaf448(mode, a, b | null)                    -> decaf448 on packed rows; mode 0 decode (a: n x 56) -> n x 112 points + n ok flags,
//                                                       1 encode (a: n x 112) -> n x 56, 2 equals (a, b: n x 112) -> n flags,
//                                                       3 deriveToCurve (a: n x 112) -> n x 56, 4 multiply (a: n x 56 encodings, b: n or ONE
//                                                       scalar row) -> n x 56 + n ok flags, 5 BASE.multiply (a: n x 56 scalars) -> n x 56
//   decodePoints(curveId, encoded, zip215: bool)     -> Uint8Array n * (PB + 2)  (points, ok flags, inf flags)
//   encodePoints(curveId, points)                    -> Uint8Array n * (EB + 1)  (encodings, ok flags)
//   aggregateEncoded(curveId, encoded, zip215)       -> Uint8Array PB + 1 (flag); throws naming a bad index
//   ntt(log2n, omega: Uint8Array 32, data, flags, field = 0) -> Uint8Array (same length); field: NCG_FIELD_* of ncg.h
//   poly(kind, field, a, b, small, i1, i2)           -> Uint8Array; the ncg_poly_* family on packed 32-byte elements (see Poly below)
//   mapToCurve(curveId, count, u)                    -> Uint8Array n * (PB + 1)
//   pointBytes(curveId) / version()
// Buffers use the wire format of include/ncg.h.  Build: make -C addon  (g++ + /usr/include/node).
#include <node_api.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../include/ncg.h"

static ncg_ctx* g_ctx = nullptr;

#define NAPI_OK(call)                                             \
  do {                                                            \
    if ((call) != napi_ok) {                                      \
      napi_throw_error(env, nullptr, "noble-gpu: N-API failure"); \
      return nullptr;                                             \
    }                                                             \
  } while (0)

static napi_value throw_native(napi_env env) {
  const char* m = ncg_last_error(g_ctx);
  napi_throw_error(env, nullptr, (m && *m) ? m : "noble-gpu: native call failed");
  return nullptr;
}

static bool get_u8(napi_env env, napi_value v, uint8_t** data, size_t* len) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return false;
  napi_typedarray_type t;
  napi_value ab;
  size_t off;
  void* p;
  if (napi_get_typedarray_info(env, v, &t, len, &p, &ab, &off) != napi_ok || t != napi_uint8_array) return false;
  *data = (uint8_t*)p;
  return true;
}

static napi_value make_u8(napi_env env, size_t n, uint8_t** out) {
  napi_value ab, arr;
  void* p;
  if (napi_create_arraybuffer(env, n, &p, &ab) != napi_ok) return nullptr;
  if (napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &arr) != napi_ok) return nullptr;
  *out = (uint8_t*)p;
  return arr;
}

static napi_value Init(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t dev = 0;
  if (argc >= 1) napi_get_value_int32(env, argv[0], &dev);
  if (!g_ctx && ncg_init(dev, &g_ctx) != 0) {
    napi_throw_error(env, nullptr, ncg_last_error(nullptr));
    return nullptr;
  }
  return nullptr;
}

// initMulti([deviceIds]): one process, several GPUs (include/ncg.h "multi-GPU MSM" (2)).  The context of the
// first device serves the single-GPU entry points; msm() shards over the whole set.
static ncg_multi* g_multi = nullptr;
static napi_value InitMulti(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  bool is_arr = false;
  uint32_t n = 0;
  if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, argv[0], &n) != napi_ok ||
      n == 0 || n > 64) {
    napi_throw_type_error(env, nullptr, "noble-gpu: initMulti([deviceId, ...])");
    return nullptr;
  }
  if (g_ctx || g_multi) {
    napi_throw_error(env, nullptr, "noble-gpu: already initialised");
    return nullptr;
  }
  int ids[64];
  for (uint32_t i = 0; i < n; i++) {
    napi_value e;
    int32_t v = 0;
    if (napi_get_element(env, argv[0], i, &e) != napi_ok || napi_get_value_int32(env, e, &v) != napi_ok) {
      napi_throw_type_error(env, nullptr, "noble-gpu: initMulti: device ids must be integers");
      return nullptr;
    }
    ids[i] = v;
  }
  if (ncg_multi_init(ids, (int)n, &g_multi) != 0) {
    napi_throw_error(env, nullptr, ncg_last_error(nullptr));
    return nullptr;
  }
  g_ctx = ncg_multi_ctx(g_multi, 0);
  napi_value r;
  napi_create_uint32(env, (uint32_t)ncg_multi_devices(g_multi), &r);
  return r;
}

static bool need_ctx(napi_env env) {
  if (g_ctx) return true;
  napi_throw_error(env, nullptr, "noble-gpu: call init() first");
  return false;
}

static napi_value Msm(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve;
  uint8_t *pts, *sc, *out;
  size_t pl, sl;
  if (argc < 3 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || !get_u8(env, argv[1], &pts, &pl) ||
      !get_u8(env, argv[2], &sc, &sl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: msm(curveId, Uint8Array, Uint8Array)");
    return nullptr;
  }
  int pb = ncg_point_bytes(curve);
  if (pb == 0 || sl % 32 || pl != (sl / 32) * (size_t)pb) {
    napi_throw_error(env, nullptr, "arrays of points and scalars must have equal length");
    return nullptr;
  }
  napi_value res = make_u8(env, pb + 1, &out);
  if (!res) return nullptr;
  if (g_multi) {  // shard over the device set
    if (ncg_msm_multi(g_multi, curve, sl / 32, pts, sc, out, out + pb) != 0) {
      napi_throw_error(env, nullptr, ncg_multi_last_error(g_multi));
      return nullptr;
    }
    return res;
  }
  if (ncg_msm(g_ctx, curve, sl / 32, pts, sc, out, out + pb) != 0) return throw_native(env);
  return res;
}

// mulVarBatch(curveId, points, scalars[, out]): with `out` (a Uint8Array of n * (PB + 1) bytes the caller keeps - and may pin once
// with hostRegister) the results land there and `out` is returned; without it a fresh array is made per call, which at 2^20 items is
// 68 MB of first-touch page faults and a per-call page lock before the first result byte can be written.
static napi_value MulVarBatch(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve;
  uint8_t *pts, *sc, *out;
  size_t pl, sl;
  if (argc < 3 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || !get_u8(env, argv[1], &pts, &pl) ||
      !get_u8(env, argv[2], &sc, &sl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: mulVarBatch(curveId, Uint8Array, Uint8Array[, Uint8Array out])");
    return nullptr;
  }
  int pb = ncg_point_bytes(curve);
  size_t n = sl / 32;
  if (pb == 0 || sl % 32 || pl != n * (size_t)pb) {
    napi_throw_error(env, nullptr, "arrays of points and scalars must have equal length");
    return nullptr;
  }
  napi_value res;
  napi_valuetype vt = napi_undefined;
  if (argc >= 4) napi_typeof(env, argv[3], &vt);
  if (argc >= 4 && vt != napi_undefined && vt != napi_null) {
    size_t ol;
    if (!get_u8(env, argv[3], &out, &ol) || ol != n * (size_t)(pb + 1)) {
      napi_throw_error(env, nullptr, "noble-gpu: mulVarBatch: out must be a Uint8Array of n * (point bytes + 1) bytes");
      return nullptr;
    }
    res = argv[3];
  } else {
    res = make_u8(env, n * (pb + 1), &out);
    if (!res) return nullptr;
  }
  if (n && ncg_mul_var_batch(g_ctx, curve, n, pts, sc, out, out + n * pb) != 0) return throw_native(env);
  return res;
}

static napi_value MulBaseBatch(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve;
  uint8_t *sc, *out;
  size_t sl;
  if (argc < 2 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || !get_u8(env, argv[1], &sc, &sl) || sl % 32) {
    napi_throw_type_error(env, nullptr, "noble-gpu: mulBaseBatch(curveId, Uint8Array)");
    return nullptr;
  }
  int pb = ncg_point_bytes(curve);
  size_t n = sl / 32;
  napi_value res = make_u8(env, n * (pb + 1), &out);
  if (!res) return nullptr;
  if (n && ncg_mul_base_batch(g_ctx, curve, n, sc, out, out + n * pb) != 0) return throw_native(env);
  return res;
}

static napi_value Ed25519VerifyBatch(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  uint8_t *sig, *pk, *k, *out;
  size_t sgl, pkl, kl;
  bool zip215 = true;
  if (argc < 3 || !get_u8(env, argv[0], &sig, &sgl) || !get_u8(env, argv[1], &pk, &pkl) || !get_u8(env, argv[2], &k, &kl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ed25519VerifyBatch(sigs, pks, ks, zip215)");
    return nullptr;
  }
  if (argc >= 4) napi_get_value_bool(env, argv[3], &zip215);
  size_t n = sgl / 64;
  if (sgl % 64 || pkl != n * 32 || kl != n * 32) {
    napi_throw_error(env, nullptr, "arrays of signatures, public keys and challenges must have equal length");
    return nullptr;
  }
  napi_value res = make_u8(env, n, &out);
  if (!res) return nullptr;
  if (n && ncg_ed25519_verify_batch(g_ctx, n, sig, pk, k, zip215 ? 1 : 0, out) != 0) return throw_native(env);
  return res;
}

// X25519 and ed25519.utils.toMontgomery on packed 32-byte rows (ncg_x25519_batch, ncg_x25519_base_batch,
// ncg_ed25519_to_montgomery_batch): kind 0 (scalars, us) - one scalar row against n > 1 rows of u selects NCG_X25519_ONE_SCALAR -
// kind 1 (null, secret keys), kind 2 (null, Ed25519 public keys).  Result: n x 32 bytes, then n ok flags (a refused row is zero).
static napi_value X25519(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t kind;
  uint8_t *sc = nullptr, *rows, *out;
  size_t sl = 0, rl;
  if (argc < 3 || napi_get_value_int32(env, argv[0], &kind) != napi_ok || kind < 0 || kind > 2 || !get_u8(env, argv[2], &rows, &rl) ||
      rl % 32 || (kind == 0 && (!get_u8(env, argv[1], &sc, &sl) || (sl != rl && sl != 32)))) {
    napi_throw_type_error(env, nullptr, "noble-gpu: x25519(kind, scalars | null, rows of 32 bytes)");
    return nullptr;
  }
  const size_t n = rl / 32;
  napi_value res = make_u8(env, n * 33, &out);
  if (!res) return nullptr;
  int rc = 0;
  if (n && kind == 0) rc = ncg_x25519_batch(g_ctx, n, sc, rows, sl != rl ? NCG_X25519_ONE_SCALAR : 0, out, out + n * 32);
  else if (n && kind == 1) rc = ncg_x25519_base_batch(g_ctx, n, rows, out, out + n * 32);
  else if (n) rc = ncg_ed25519_to_montgomery_batch(g_ctx, n, rows, out, out + n * 32);
  if (rc != 0) return throw_native(env);
  return res;
}

// Ed448 signing and verification from messages on packed rows (ncg_ed448_public_key_batch, ncg_ed448_sign_batch,
// ncg_ed448_verify_batch_msgs).  kind 0 (secret keys n x 57) -> n x 57 public keys.  kind 1 (keys, flags, dom, msgs, lens): keys n x 57 -
// or ONE row, which selects NCG_ED448_SIGN_ONE_KEY; flags: the PREHASH bit; dom: the domain prefix; msgs: the messages back to back;
// lens: n message lengths as LE uint32 -> n x 114 signatures, then n ok flags (a refused row is zero).  kind 2 (sigs n x 114, flags, dom,
// msgs, lens, publicKeys n x 57) -> n verdicts, the challenge hashed on the device.
static napi_value Ed448Sign(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t kind, flags = 0;
  uint8_t *keys, *dom = nullptr, *msgs = nullptr, *lens = nullptr, *pks = nullptr, *out;
  size_t kl, dl = 0, ml = 0, ll = 0, pl = 0;
  if (argc < 2 || napi_get_value_int32(env, argv[0], &kind) != napi_ok || kind < 0 || kind > 2 || !get_u8(env, argv[1], &keys, &kl) ||
      kl % (kind == 2 ? 114 : 57) ||
      (kind >= 1 && (argc < 6 || napi_get_value_int32(env, argv[2], &flags) != napi_ok || !get_u8(env, argv[3], &dom, &dl) ||
                     !get_u8(env, argv[4], &msgs, &ml) || !get_u8(env, argv[5], &lens, &ll) || ll % 4)) ||
      (kind == 2 && (argc < 7 || !get_u8(env, argv[6], &pks, &pl)))) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ed448Sign(kind, keys of 57 bytes | signatures of 114[, flags, dom, msgs, lens[, publicKeys]])");
    return nullptr;
  }
  if (kind == 0) {
    const size_t n = kl / 57;
    napi_value res = make_u8(env, n * 57, &out);
    if (!res) return nullptr;
    if (n && ncg_ed448_public_key_batch(g_ctx, n, keys, out) != 0) return throw_native(env);
    return res;
  }
  const size_t n = ll / 4;
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    uint32_t len;
    memcpy(&len, lens + 4 * i, 4);
    off[i + 1] = off[i] + len;
  }
  if (flags & ~NCG_ED448_PREHASH) {
    napi_throw_error(env, nullptr, "noble-gpu: ed448Sign: flags may hold the prehash bit (4) only");
    return nullptr;
  }
  if (kind == 2) {
    if (off[n] != ml || kl != 114 * n || pl != 57 * n) {
      napi_throw_error(env, nullptr, "arrays of signatures, messages and public keys must have equal length");
      return nullptr;
    }
    napi_value res = make_u8(env, n, &out);
    if (!res) return nullptr;
    if (n && ncg_ed448_verify_batch_msgs(g_ctx, n, keys, pks, flags, dl ? dom : nullptr, dl, ml ? msgs : nullptr, off.data(), out) != 0)
      return throw_native(env);
    return res;
  }
  if (off[n] != ml || (kl != 57 * n && kl != 57)) {
    napi_throw_error(env, nullptr, "arrays of messages and secret keys must have equal length");
    return nullptr;
  }
  napi_value res = make_u8(env, n * 115, &out);
  if (!res) return nullptr;
  if (kl != 57 * n) flags |= NCG_ED448_SIGN_ONE_KEY;
  if (n && ncg_ed448_sign_batch(g_ctx, n, keys, flags, dl ? dom : nullptr, dl, ml ? msgs : nullptr, off.data(), out, out + n * 114) != 0)
    return throw_native(env);
  return res;
}

// Ed25519 signing on packed rows (ncg_ed25519_public_key_batch, ncg_ed25519_sign_batch).  kind 0 (secret keys n x 32) -> n x 32 public
// keys.  kind 1 (keys, flags, dom, msgs, lens): keys n x 32 - or ONE row, which selects NCG_ED25519_SIGN_ONE_KEY; flags: the PREHASH bit;
// dom: the domain prefix (may be empty); msgs: the messages back to back; lens: n message lengths as LE uint32 -> n x 64 signatures,
// then n ok flags (a refused row is zero).
static napi_value Ed25519Sign(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t kind, flags = 0;
  uint8_t *keys, *dom = nullptr, *msgs = nullptr, *lens = nullptr, *out;
  size_t kl, dl = 0, ml = 0, ll = 0;
  if (argc < 2 || napi_get_value_int32(env, argv[0], &kind) != napi_ok || kind < 0 || kind > 1 || !get_u8(env, argv[1], &keys, &kl) || kl % 32 ||
      (kind == 1 && (argc < 6 || napi_get_value_int32(env, argv[2], &flags) != napi_ok || !get_u8(env, argv[3], &dom, &dl) ||
                     !get_u8(env, argv[4], &msgs, &ml) || !get_u8(env, argv[5], &lens, &ll) || ll % 4))) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ed25519Sign(kind, keys of 32 bytes[, flags, dom, msgs, lens])");
    return nullptr;
  }
  if (kind == 0) {
    const size_t n = kl / 32;
    napi_value res = make_u8(env, n * 32, &out);
    if (!res) return nullptr;
    if (n && ncg_ed25519_public_key_batch(g_ctx, n, keys, out) != 0) return throw_native(env);
    return res;
  }
  const size_t n = ll / 4;
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    uint32_t len;
    memcpy(&len, lens + 4 * i, 4);
    off[i + 1] = off[i] + len;
  }
  if (flags & ~NCG_ED25519_SIGN_PREHASH) {
    napi_throw_error(env, nullptr, "noble-gpu: ed25519Sign: flags may hold the prehash bit (4) only");
    return nullptr;
  }
  if (off[n] != ml || (kl != 32 * n && kl != 32)) {
    napi_throw_error(env, nullptr, "arrays of messages and secret keys must have equal length");
    return nullptr;
  }
  napi_value res = make_u8(env, n * 65, &out);
  if (!res) return nullptr;
  if (kl != 32 * n) flags |= NCG_ED25519_SIGN_ONE_KEY;
  if (n && ncg_ed25519_sign_batch(g_ctx, n, keys, flags, dl ? dom : nullptr, dl, ml ? msgs : nullptr, off.data(), out, out + n * 64) != 0)
    return throw_native(env);
  return res;
}

// secp256k1 signing on packed rows (ncg_secp256k1_public_key_batch, ncg_ecdsa_sign_batch[_msgs], ncg_schnorr_sign_batch).  Keys are n x 32
// big-endian bytes; ONE key row against n > 1 messages selects NCG_SECP_SIGN_ONE_KEY.  An empty Uint8Array stands for "not given".
//   kind 0 (keys, mode)                       -> n public keys of 33 / 65 / 32 bytes (mode 0 / 1 / 2), then n ok flags
//   kind 1 (keys, flags, data, lens, extra)   ECDSA: lens empty: data = n x 32 hashes (prehash false); else data = the messages back to
//                                             back and lens = n lengths as LE uint32; extra: empty or n x 32; flags: the lowS bit
//                                             -> n x 64 signatures, n recovery ids, n ok flags
//   kind 2 (keys, 0, msgs, lens, aux)         BIP-340: aux n x 32 -> n x 64 signatures, n ok flags
// A refused row is zero.
static napi_value SecpSign(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t kind, flags = 0;
  uint8_t *keys, *data = nullptr, *lens = nullptr, *extra = nullptr, *out;
  size_t kl, dl = 0, ll = 0, xl = 0;
  if (argc < 3 || napi_get_value_int32(env, argv[0], &kind) != napi_ok || kind < 0 || kind > 2 || !get_u8(env, argv[1], &keys, &kl) || kl % 32 ||
      napi_get_value_int32(env, argv[2], &flags) != napi_ok ||
      (kind > 0 && (argc < 6 || !get_u8(env, argv[3], &data, &dl) || !get_u8(env, argv[4], &lens, &ll) || ll % 4 || !get_u8(env, argv[5], &extra, &xl)))) {
    napi_throw_type_error(env, nullptr, "noble-gpu: secpSign(kind, keys of 32 bytes, flags | mode[, data, lens, extra | aux])");
    return nullptr;
  }
  if (kind == 0) {
    const size_t n = kl / 32, w = flags == NCG_SECP_PK_UNCOMPRESSED ? 65 : flags == NCG_SECP_PK_XONLY ? 32 : 33;
    napi_value res = make_u8(env, n * (w + 1), &out);
    if (!res) return nullptr;
    if (n && ncg_secp256k1_public_key_batch(g_ctx, n, keys, flags, out, out + n * w) != 0) return throw_native(env);
    return res;
  }
  const bool hashes = kind == 1 && ll == 0 && dl != 0;
  const size_t n = hashes ? dl / 32 : ll / 4;
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n && !hashes; i++) {
    uint32_t len;
    memcpy(&len, lens + 4 * i, 4);
    off[i + 1] = off[i] + len;
  }
  if ((hashes ? dl != 32 * n : off[n] != dl) || (kl != 32 * n && kl != 32) || (kind == 2 ? xl != 32 * n : (xl != 0 && xl != 32 * n)) ||
      (flags & ~NCG_ECDSA_LOW_S)) {
    napi_throw_error(env, nullptr, "noble-gpu: secpSign: arrays of messages, secret keys and extra rows must have matching lengths");
    return nullptr;
  }
  if (kl != 32 * n) flags |= NCG_SECP_SIGN_ONE_KEY;
  napi_value res = make_u8(env, n * (kind == 1 ? 66 : 65), &out);
  if (!res) return nullptr;
  int rc = 0;
  if (n && kind == 2) rc = ncg_schnorr_sign_batch(g_ctx, n, keys, extra, dl ? data : nullptr, off.data(), flags, out, out + n * 64);
  else if (n && hashes) rc = ncg_ecdsa_sign_batch(g_ctx, NCG_SECP256K1, n, keys, data, xl ? extra : nullptr, flags, out, out + n * 64, out + n * 65);
  else if (n)
    rc = ncg_ecdsa_sign_batch_msgs(g_ctx, NCG_SECP256K1, n, keys, dl ? data : nullptr, off.data(), xl ? extra : nullptr, flags, out, out + n * 64,
                                   out + n * 65);
  if (rc != 0) return throw_native(env);
  return res;
}

// X448 and Ed448 on packed rows (ncg_x448_batch, ncg_x448_base_batch, ncg_ed448_verify_batch): kind 0 (scalars, us) - one 56-byte scalar
// row against n > 1 rows of u selects NCG_X448_ONE_SCALAR - and kind 1 (null, secret keys): n x 56 bytes, then n ok flags (a refused row
// is zero); kind 2 (signatures n x 114, public keys n x 57, challenges n x 56) -> n verdicts (0 / 1).
static napi_value Ed448(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t kind;
  uint8_t *a = nullptr, *b = nullptr, *c = nullptr, *out;
  size_t al = 0, bl = 0, cl = 0;
  bool good = argc >= 3 && napi_get_value_int32(env, argv[0], &kind) == napi_ok && kind >= 0 && kind <= 2 && get_u8(env, argv[2], &b, &bl);
  if (good && kind == 0) good = bl % 56 == 0 && get_u8(env, argv[1], &a, &al) && (al == bl || al == 56);
  if (good && kind == 1) good = bl % 56 == 0;
  if (good && kind == 2)
    good = argc >= 4 && get_u8(env, argv[1], &a, &al) && get_u8(env, argv[3], &c, &cl) && al % 114 == 0 && bl == al / 114 * 57 && cl == al / 114 * 56;
  if (!good) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ed448(kind, scalars | signatures | null, rows, challenges)");
    return nullptr;
  }
  const size_t n = kind == 2 ? al / 114 : bl / 56;
  napi_value res = make_u8(env, kind == 2 ? n : n * 57, &out);
  if (!res) return nullptr;
  int rc = 0;
  if (n && kind == 0) rc = ncg_x448_batch(g_ctx, n, a, b, al != bl ? NCG_X448_ONE_SCALAR : 0, out, out + n * 56);
  else if (n && kind == 1) rc = ncg_x448_base_batch(g_ctx, n, b, out, out + n * 56);
  else if (n) rc = ncg_ed448_verify_batch(g_ctx, n, a, b, c, out);
  if (rc != 0) return throw_native(env);
  return res;
}

// ristretto255 on packed rows (ncg_ristretto_*): one entry, the operation chosen by `mode` (see the list at the top of this file).
static napi_value Ristretto(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  static const size_t in_row[7] = {32, 64, 64, 64, 32, 32, 32}, out_row[7] = {65, 32, 1, 32, 33, 32, 0};
  int32_t mode;
  uint8_t *a, *b = nullptr, *out;
  size_t al, bl = 0;
  bool ok = argc >= 3 && napi_get_value_int32(env, argv[0], &mode) == napi_ok && mode >= 0 && mode <= 6 && get_u8(env, argv[1], &a, &al) &&
            al % in_row[mode] == 0;
  const bool two = ok && (mode == 2 || mode == 4 || mode == 6);
  if (two) ok = get_u8(env, argv[2], &b, &bl);
  const size_t n = ok ? al / in_row[mode] : 0;
  if (ok && mode == 2) ok = bl == al;
  if (ok && mode == 4) ok = bl == al || bl == 32;
  if (ok && mode == 6) ok = bl == al;
  if (!ok) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ristretto(mode, rows, rows | null)");
    return nullptr;
  }
  napi_value res = make_u8(env, mode == 6 ? 32 : n * out_row[mode], &out);
  if (!res) return nullptr;
  int rc = 0;
  if (mode == 6) rc = ncg_ristretto_msm(g_ctx, n, a, b, out, nullptr);
  else if (n == 0) rc = 0;
  else if (mode == 0) rc = ncg_ristretto_decode_batch(g_ctx, n, a, out, out + n * 64);
  else if (mode == 1) rc = ncg_ristretto_encode_batch(g_ctx, n, a, out);
  else if (mode == 2) rc = ncg_ristretto_equals_batch(g_ctx, n, a, b, out);
  else if (mode == 3) rc = ncg_ristretto_from_uniform_batch(g_ctx, n, a, out, nullptr);
  else if (mode == 4) rc = ncg_ristretto_mul_batch(g_ctx, n, a, b, bl != al ? NCG_RISTRETTO_ONE_SCALAR : 0, out, out + n * 32);
  else rc = ncg_ristretto_mul_base_batch(g_ctx, n, a, out);
  if (rc != 0) return throw_native(env);
  return res;
}

// The ristretto255 OPRF on packed rows (ncg_oprf_*, ncg_ristretto_hash_to_scalar_batch): oprf(op, mode, flags, a, b, c, d), an empty
// Uint8Array standing for "not given".  Messages travel back to back with n lengths as LE uint32; a refused row is zero with its status.
//   op 0 blind     (a: inputs, b: lens, c: blinds n x 32)                              -> n x 32 blinded, then n statuses
//   op 1 mul       (a: elements n x 32, b: scalars n x 32 or ONE row; flags: INVERT)   -> n x 32, then n statuses
//   op 2 finalize  (a: inputs, b: lens, c: blinds n x 32 then evaluated n x 32, d: info) -> n x 64, then n statuses
//   op 3 evaluate  (a: inputs, b: lens, c: the scalar, d: info; flags: INVERT)         -> n x 64, then n statuses
//   op 4 proof     (a: k || B || r, b: C n x 32, c: D n x 32)                          -> 64 bytes c || s
//   op 5 verify    (a: B || proof, b: C, c: D)                                         -> 1 byte
//   op 6 hashToScalar (a: msgs, b: lens, c: DST)                                       -> n x 32
static napi_value Oprf(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t op, mode, flags;
  uint8_t *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr, *out;
  size_t al = 0, bl = 0, cl = 0, dl = 0;
  if (argc < 7 || napi_get_value_int32(env, argv[0], &op) != napi_ok || op < 0 || op > 6 || napi_get_value_int32(env, argv[1], &mode) != napi_ok ||
      napi_get_value_int32(env, argv[2], &flags) != napi_ok || !get_u8(env, argv[3], &a, &al) || !get_u8(env, argv[4], &b, &bl) ||
      !get_u8(env, argv[5], &c, &cl) || !get_u8(env, argv[6], &d, &dl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: oprf(op, mode, flags, a, b, c, d)");
    return nullptr;
  }
  const int suite = NCG_OPRF_RISTRETTO255_SHA512;
  const bool msgs = op == 0 || op == 2 || op == 3 || op == 6;
  size_t n = msgs ? bl / 4 : (op == 1 ? al / 32 : bl / 32);
  std::vector<uint64_t> off(n + 1, 0);
  bool good = true;
  if (msgs) {
    good = bl % 4 == 0;
    for (size_t i = 0; good && i < n; i++) {
      uint32_t len;
      memcpy(&len, b + 4 * i, 4);
      off[i + 1] = off[i] + len;
    }
    good = good && off[n] == al;
  }
  if (op == 0) good = good && cl == 32 * n;
  if (op == 1) good = al % 32 == 0 && (bl == al || bl == 32);
  if (op == 2) good = good && cl == 64 * n;
  if (op == 3) good = good && cl == 32;
  if (op == 4) good = al == 96 && bl % 32 == 0 && cl == bl && n > 0;
  if (op == 5) good = al == 96 && bl % 32 == 0 && cl == bl && n > 0;
  if (!good) {
    napi_throw_error(env, nullptr, "noble-gpu: oprf: the rows do not match");
    return nullptr;
  }
  static const size_t per_row[7] = {33, 33, 65, 65, 0, 0, 32};
  napi_value res = make_u8(env, op == 4 ? 64 : (op == 5 ? 1 : n * per_row[op]), &out);
  if (!res) return nullptr;
  const void* inf = mode == 2 ? (dl ? (const void*)d : (const void*)"") : nullptr;
  int rc = 0;
  if (n == 0) rc = 0;
  else if (op == 0) rc = ncg_oprf_blind_batch(g_ctx, suite, mode, n, al ? a : nullptr, off.data(), c, out, out + n * 32);
  else if (op == 1) rc = ncg_oprf_mul_batch(g_ctx, suite, n, a, b, flags | (bl != al ? NCG_OPRF_ONE_SCALAR : 0), out, out + n * 32);
  else if (op == 2) rc = ncg_oprf_finalize_batch(g_ctx, suite, mode, n, al ? a : nullptr, off.data(), inf, mode == 2 ? dl : 0, c, c + 32 * n, out, out + n * 64);
  else if (op == 3)
    rc = ncg_oprf_evaluate_batch(g_ctx, suite, mode, n, al ? a : nullptr, off.data(), inf, mode == 2 ? dl : 0, c, flags | NCG_OPRF_ONE_SCALAR, out, out + n * 64);
  else if (op == 4) rc = ncg_oprf_generate_proof(g_ctx, suite, mode, n, a, a + 32, b, c, a + 64, out);
  else if (op == 5) rc = ncg_oprf_verify_proof(g_ctx, suite, mode, n, a, b, c, a + 32, out);
  else rc = ncg_ristretto_hash_to_scalar_batch(g_ctx, n, al ? a : nullptr, off.data(), c, cl, out);
  if (rc != 0) return throw_native(env);
  return res;
}

// RFC 9380 for secp256k1 and edwards25519 (ncg_h2c_*): h2c(op, suite, count, msgs, lens, dst).  Messages travel back to back with n
// lengths as LE uint32, as for oprf(); dst is 1..255 bytes (the shim hashes an oversize one).
//   op 0 hashToCurve (count 2) / encodeToCurve (count 1)  -> n x 64 affine wire bytes of the suite's curve, then n ZERO flags
//   op 1 hashToScalar (count ignored)                     -> n x 32 little-endian
static napi_value H2c(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t op, suite, count;
  uint8_t *a = nullptr, *b = nullptr, *c = nullptr, *out;
  size_t al = 0, bl = 0, cl = 0;
  if (argc < 6 || napi_get_value_int32(env, argv[0], &op) != napi_ok || (op != 0 && op != 1) || napi_get_value_int32(env, argv[1], &suite) != napi_ok ||
      napi_get_value_int32(env, argv[2], &count) != napi_ok || !get_u8(env, argv[3], &a, &al) || !get_u8(env, argv[4], &b, &bl) ||
      !get_u8(env, argv[5], &c, &cl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: h2c(op, suite, count, msgs, lens, dst)");
    return nullptr;
  }
  const size_t n = bl / 4;
  std::vector<uint64_t> off(n + 1, 0);
  bool good = bl % 4 == 0;
  for (size_t i = 0; good && i < n; i++) {
    uint32_t len;
    memcpy(&len, b + 4 * i, 4);
    off[i + 1] = off[i] + len;
  }
  if (!good || off[n] != al) {
    napi_throw_error(env, nullptr, "noble-gpu: h2c: the rows do not match");
    return nullptr;
  }
  napi_value res = make_u8(env, n * (op == 0 ? 65 : 32), &out);
  if (!res) return nullptr;
  int rc = 0;
  if (n == 0) rc = 0;
  else if (op == 0) rc = ncg_h2c_hash_batch(g_ctx, suite, n, count, al ? a : nullptr, off.data(), c, cl, out, out + n * 64);
  else rc = ncg_h2c_hash_to_scalar_batch(g_ctx, suite, n, al ? a : nullptr, off.data(), c, cl, out);
  if (rc != 0) return throw_native(env);
  return res;
}

// RFC 9380 for edwards448 and the hash side of decaf448 (ncg_ed448_h2c_*, ncg_decaf448_hash_to_*): h2c448(op, count, msgs, lens, dst).
// Messages travel as for h2c(); dst is 1..255 bytes (the shim compresses an oversize one).
//   op 0 ed448 hashToCurve (count 2) / encodeToCurve (count 1)  -> n x 112 bytes, affine x || y little-endian, ZERO as (0, 1)
//   op 1 ed448 hashToScalar   op 2 decaf448 hashToCurve (the encoded element)   op 3 decaf448 hashToScalar   -> n x 56 (count ignored)
static napi_value H2c448(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t op, count;
  uint8_t *a = nullptr, *b = nullptr, *c = nullptr, *out;
  size_t al = 0, bl = 0, cl = 0;
  if (argc < 5 || napi_get_value_int32(env, argv[0], &op) != napi_ok || op < 0 || op > 3 || napi_get_value_int32(env, argv[1], &count) != napi_ok ||
      !get_u8(env, argv[2], &a, &al) || !get_u8(env, argv[3], &b, &bl) || !get_u8(env, argv[4], &c, &cl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: h2c448(op, count, msgs, lens, dst)");
    return nullptr;
  }
  const size_t n = bl / 4;
  std::vector<uint64_t> off(n + 1, 0);
  bool good = bl % 4 == 0;
  for (size_t i = 0; good && i < n; i++) {
    uint32_t len;
    memcpy(&len, b + 4 * i, 4);
    off[i + 1] = off[i] + len;
  }
  if (!good || off[n] != al) {
    napi_throw_error(env, nullptr, "noble-gpu: h2c448: the rows do not match");
    return nullptr;
  }
  napi_value res = make_u8(env, n * (op == 0 ? 112 : 56), &out);
  if (!res) return nullptr;
  const void* msgs = al ? a : nullptr;
  int rc = 0;
  if (n == 0) rc = 0;
  else if (op == 0) rc = ncg_ed448_h2c_hash_batch(g_ctx, n, count, msgs, off.data(), c, cl, out);
  else if (op == 1) rc = ncg_ed448_h2c_hash_to_scalar_batch(g_ctx, n, msgs, off.data(), c, cl, out);
  else if (op == 2) rc = ncg_decaf448_hash_to_group_batch(g_ctx, n, msgs, off.data(), c, cl, out);
  else rc = ncg_decaf448_hash_to_scalar_batch(g_ctx, n, msgs, off.data(), c, cl, out);
  if (rc != 0) return throw_native(env);
  return res;
}

// decaf448 on packed rows (ncg_decaf448_*): one entry, the operation chosen by `mode` (see the list at the top of this file).
static napi_value Decaf448(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  static const size_t in_row[6] = {56, 112, 112, 112, 56, 56}, out_row[6] = {113, 56, 1, 56, 57, 56};
  int32_t mode;
  uint8_t *a, *b = nullptr, *out;
  size_t al, bl = 0;
  bool ok = argc >= 3 && napi_get_value_int32(env, argv[0], &mode) == napi_ok && mode >= 0 && mode <= 5 && get_u8(env, argv[1], &a, &al) &&
            al % in_row[mode] == 0;
  const bool two = ok && (mode == 2 || mode == 4);
  if (two) ok = get_u8(env, argv[2], &b, &bl);
  const size_t n = ok ? al / in_row[mode] : 0;
  if (ok && mode == 2) ok = bl == al;
  if (ok && mode == 4) ok = bl == al || bl == 56;
  if (!ok) {
    napi_throw_type_error(env, nullptr, "noble-gpu: decaf448(mode, rows, rows | null)");
    return nullptr;
  }
  napi_value res = make_u8(env, n * out_row[mode], &out);
  if (!res) return nullptr;
  int rc = 0;
  if (n == 0) rc = 0;
  else if (mode == 0) rc = ncg_decaf448_decode_batch(g_ctx, n, a, out, out + n * 112);
  else if (mode == 1) rc = ncg_decaf448_encode_batch(g_ctx, n, a, out);
  else if (mode == 2) rc = ncg_decaf448_equals_batch(g_ctx, n, a, b, out);
  else if (mode == 3) rc = ncg_decaf448_from_uniform_batch(g_ctx, n, a, out);
  else if (mode == 4) rc = ncg_decaf448_mul_batch(g_ctx, n, a, b, bl != al ? NCG_DECAF448_ONE_SCALAR : 0, out, out + n * 56);
  else rc = ncg_decaf448_mul_base_batch(g_ctx, n, a, out);
  if (rc != 0) return throw_native(env);
  return res;
}

// bls12-381 pairings on packed rows.  bls(0, g1 rows (96 B), g2 rows (192 B), offsets (n_groups + 1 little-endian uint32), flags)
// -> n_groups GT elements (576 B each) followed by n_groups is_one bytes (ncg_pairing_batch);
// bls(1, pk rows, sig rows, u rows, scheme) -> n verdict bytes (ncg_bls_verify_batch; scheme 0: 48 / 96 / 192 B, scheme 1: 96 / 48 / 96 B).
static napi_value Bls(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t mode, last;
  uint8_t *a, *b, *c, *out;
  size_t al, bl, cl;
  if (argc < 5 || napi_get_value_int32(env, argv[0], &mode) != napi_ok || (mode != 0 && mode != 1) || !get_u8(env, argv[1], &a, &al) ||
      !get_u8(env, argv[2], &b, &bl) || !get_u8(env, argv[3], &c, &cl) || napi_get_value_int32(env, argv[4], &last) != napi_ok) {
    napi_throw_type_error(env, nullptr, "noble-gpu: bls(mode, rows, rows, rows, flags | scheme)");
    return nullptr;
  }
  if (mode == 0) {
    const size_t n = al / 96, ng = cl >= 4 ? cl / 4 - 1 : 0;
    if (al % 96 || bl != n * 192 || cl % 4 || cl < 4) {
      napi_throw_error(env, nullptr, "arrays of G1 points, G2 points and group offsets must have matching lengths");
      return nullptr;
    }
    std::vector<uint32_t> off(ng + 1);
    memcpy(off.data(), c, (ng + 1) * 4);
    napi_value res = make_u8(env, ng * 577, &out);
    if (!res) return nullptr;
    if (ncg_pairing_batch(g_ctx, n, a, b, ng, off.data(), last, out, out + ng * 576, nullptr) != 0) return throw_native(env);
    return res;
  }
  const size_t pw = last == 0 ? 48 : 96, sw = last == 0 ? 96 : 48, uw = last == 0 ? 192 : 96, n = al / pw;
  if ((last != 0 && last != 1) || al % pw || bl != n * sw || cl != n * uw) {
    napi_throw_error(env, nullptr, "arrays of keys, signatures and messages must have matching lengths");
    return nullptr;
  }
  napi_value res = make_u8(env, n, &out);
  if (!res) return nullptr;
  if (n && ncg_bls_verify_batch(g_ctx, last, n, a, b, c, out) != 0) return throw_native(env);
  return res;
}

// eddsa.verify from (sig, msg, pk): the challenge hash runs on the device too.  msgs = all messages back to
// back, offs = Float64Array / BigUint64Array-free: a Uint8Array holding n + 1 little-endian uint64 offsets.
static napi_value Ed25519VerifyMsgs(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  uint8_t *sig, *pk, *msgs, *offs, *out;
  size_t sgl, pkl, ml, ol;
  bool zip215 = true;
  if (argc < 4 || !get_u8(env, argv[0], &sig, &sgl) || !get_u8(env, argv[1], &pk, &pkl) || !get_u8(env, argv[2], &msgs, &ml) ||
      !get_u8(env, argv[3], &offs, &ol)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ed25519VerifyMsgs(sigs, pks, msgs, offsets, zip215)");
    return nullptr;
  }
  if (argc >= 5) napi_get_value_bool(env, argv[4], &zip215);
  const size_t n = sgl / 64;
  if (sgl % 64 || pkl != n * 32 || ol != (n + 1) * 8) {
    napi_throw_error(env, nullptr, "arrays of signatures, public keys and message offsets must have matching lengths");
    return nullptr;
  }
  std::vector<uint64_t> off(n + 1);
  memcpy(off.data(), offs, ol);
  if (off[n] > ml) {
    napi_throw_error(env, nullptr, "noble-gpu: message offsets run past the message buffer");
    return nullptr;
  }
  napi_value res = make_u8(env, n, &out);
  if (!res) return nullptr;
  if (n && ncg_ed25519_verify_batch_msgs(g_ctx, n, sig, pk, msgs, off.data(), zip215 ? 1 : 0, out) != 0) return throw_native(env);
  return res;
}

// ecdsaVerify(sigs [n*64: r || s big-endian], hashes [n*32], keys [n*33 SEC1 compressed], lowS) -> Uint8Array verdicts
static napi_value EcdsaVerify(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  uint8_t *sig, *hs, *pk, *out;
  size_t sgl, hl, pkl;
  bool low_s = true;
  if (argc < 3 || !get_u8(env, argv[0], &sig, &sgl) || !get_u8(env, argv[1], &hs, &hl) || !get_u8(env, argv[2], &pk, &pkl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ecdsaVerify(sigs, hashes, keys, lowS)");
    return nullptr;
  }
  if (argc >= 4) napi_get_value_bool(env, argv[3], &low_s);
  const size_t n = sgl / 64;
  if (sgl % 64 || hl != n * 32 || pkl != n * 33) {
    napi_throw_error(env, nullptr, "arrays of signatures, message hashes and public keys must have matching lengths");
    return nullptr;
  }
  napi_value res = make_u8(env, n, &out);
  if (!res) return nullptr;
  if (n && ncg_ecdsa_verify_batch(g_ctx, NCG_SECP256K1, n, sig, hs, pk, low_s ? NCG_ECDSA_LOW_S : 0, out) != 0) return throw_native(env);
  return res;
}

// secpVerifyMsgs(kind, sigs [n*64], keys [n*33 | n*65 | n*32], msgs, offsets [(n+1)*8 LE], lowS) -> Uint8Array verdicts
// kind 0: ECDSA with prehash (SHA-256 on the device), keys compressed (33 B) or uncompressed (65 B) rows;
// kind 1: BIP-340 Schnorr, x-only keys (32 B), tagged challenge hash on the device
static napi_value SecpVerifyMsgs(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t kind = 0;
  uint8_t *sig, *pk, *msgs, *offs, *out;
  size_t sgl, pkl, ml, ol;
  bool low_s = true;
  if (argc < 5 || napi_get_value_int32(env, argv[0], &kind) != napi_ok || !get_u8(env, argv[1], &sig, &sgl) || !get_u8(env, argv[2], &pk, &pkl) ||
      !get_u8(env, argv[3], &msgs, &ml) || !get_u8(env, argv[4], &offs, &ol)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: secpVerifyMsgs(kind, sigs, keys, msgs, offsets, lowS)");
    return nullptr;
  }
  if (argc >= 6) napi_get_value_bool(env, argv[5], &low_s);
  const size_t n = sgl / 64;
  const size_t kb = n ? pkl / n : 0;
  if (sgl % 64 || ol != (n + 1) * 8 || (n && (pkl % n || (kind == 1 ? kb != 32 : (kb != 33 && kb != 65))))) {
    napi_throw_error(env, nullptr, "arrays of signatures, public keys and message offsets must have matching lengths");
    return nullptr;
  }
  std::vector<uint64_t> off(n + 1);
  memcpy(off.data(), offs, ol);
  if (off[n] > ml) {
    napi_throw_error(env, nullptr, "noble-gpu: message offsets run past the message buffer");
    return nullptr;
  }
  napi_value res = make_u8(env, n, &out);
  if (!res) return nullptr;
  int rc = 0;
  if (n && kind == 0)
    rc = ncg_ecdsa_verify_batch_msgs(g_ctx, NCG_SECP256K1, n, sig, msgs, off.data(), pk,
                                     (low_s ? NCG_ECDSA_LOW_S : 0) | (kb == 65 ? NCG_ECDSA_PUB_UNCOMPRESSED : 0), out);
  else if (n)
    rc = ncg_schnorr_verify_batch_msgs(g_ctx, n, sig, msgs, off.data(), pk, out);
  if (rc != 0) return throw_native(env);
  return res;
}
// ecdsaRecover(sigs65 [n*65: recid || r || s], hashes [n*32]) -> Uint8Array(n*33 compressed keys || n ok flags)
static napi_value EcdsaRecover(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  uint8_t *sig, *hs, *out;
  size_t sgl, hl;
  if (argc < 2 || !get_u8(env, argv[0], &sig, &sgl) || !get_u8(env, argv[1], &hs, &hl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ecdsaRecover(sigs65, hashes)");
    return nullptr;
  }
  const size_t n = sgl / 65;
  if (sgl % 65 || hl != n * 32) {
    napi_throw_error(env, nullptr, "arrays of signatures and message hashes must have matching lengths");
    return nullptr;
  }
  napi_value res = make_u8(env, n * 34, &out);
  if (!res) return nullptr;
  if (n) {
    std::vector<uint8_t> aff(n * 64), ok(n), eok(n);
    if (ncg_ecdsa_recover_batch(g_ctx, NCG_SECP256K1, n, sig, hs, aff.data(), ok.data()) != 0) return throw_native(env);
    if (ncg_encode_points_batch(g_ctx, NCG_SECP256K1, n, aff.data(), out, eok.data()) != 0) return throw_native(env);
    for (size_t i = 0; i < n; i++) out[n * 33 + i] = (ok[i] && eok[i]) ? 1 : 0;
  }
  return res;
}

static int encoded_bytes(int curve);
// ---- resident point sets: upload once (affine wire points or compressed encodings), then MSMs / batch
// multiplies with only the scalars crossing.  Handles are small integers; `scalars` may be a Uint8Array
// of packed 32-byte LE values (no marshalling at all) or an Array of BigInt (read with
// napi_get_value_bigint_words - no hex strings).
static std::vector<ncg_points*> g_sets;

static bool get_scalars(napi_env env, napi_value v, size_t n, std::vector<uint8_t>& store, uint8_t** data) {
  size_t len = 0;
  if (get_u8(env, v, data, &len)) return len == n * 32;
  bool is_arr = false;
  if (napi_is_array(env, v, &is_arr) != napi_ok || !is_arr) return false;
  uint32_t m = 0;
  if (napi_get_array_length(env, v, &m) != napi_ok || m != n) return false;
  store.assign(n * 32, 0);
  for (uint32_t i = 0; i < m; i++) {
    napi_value e;
    if (napi_get_element(env, v, i, &e) != napi_ok) return false;
    int sign = 0;
    size_t words = 4;
    uint64_t w[4] = {0, 0, 0, 0};
    if (napi_get_value_bigint_words(env, e, &sign, &words, w) != napi_ok || sign != 0 || words > 4) return false;
    memcpy(store.data() + (size_t)i * 32, w, 32);  // little-endian host
  }
  *data = store.data();
  return true;
}

// packBigInts(values: BigInt[], byteLen) -> Uint8Array(values.length * byteLen), little-endian: the marshalling of
// coordinates / scalars without hex strings (napi_get_value_bigint_words); negative or too wide values throw
static napi_value PackBigInts(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  bool is_arr = false;
  uint32_t m = 0, blen = 0;
  if (argc < 2 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, argv[0], &m) != napi_ok ||
      napi_get_value_uint32(env, argv[1], &blen) != napi_ok || blen == 0 || blen > 64 || blen % 8) {
    napi_throw_type_error(env, nullptr, "noble-gpu: packBigInts(BigInt[], byteLen multiple of 8, <= 64)");
    return nullptr;
  }
  uint8_t* out;
  napi_value res = make_u8(env, (size_t)m * blen, &out);
  if (!res) return nullptr;
  const size_t maxw = blen / 8;
  napi_handle_scope scope = nullptr;
  for (uint32_t i = 0; i < m; i++) {
    // the element handles of a million-entry array would otherwise all live until the call returns: a fresh
    // handle scope every 4096 elements keeps the handle stack bounded (no speed-up measured: the ~100 ns per value
    // are napi_get_element + napi_get_value_bigint_words themselves)
    if ((i & 4095u) == 0) {
      if (scope) (void)napi_close_handle_scope(env, scope);
      scope = nullptr;
      if (napi_open_handle_scope(env, &scope) != napi_ok) scope = nullptr;
    }
    napi_value e;
    int sign = 0;
    size_t words = 8;
    uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (napi_get_element(env, argv[0], i, &e) != napi_ok || napi_get_value_bigint_words(env, e, &sign, &words, w) != napi_ok) {
      if (scope) (void)napi_close_handle_scope(env, scope);
      napi_throw_type_error(env, nullptr, "noble-gpu: packBigInts: expected bigint");
      return nullptr;
    }
    // `words` comes back as the count the value NEEDS (it may exceed the 8 fetched): a canonical BigInt with more
    // words than the field holds is never zero (e.g. 1n << 512n has eight zero low words), and -0n does not exist
    if (sign != 0 || words > maxw) {
      if (scope) (void)napi_close_handle_scope(env, scope);
      napi_throw_range_error(env, nullptr, "noble-gpu: packBigInts: value out of range");
      return nullptr;
    }
    memcpy(out + (size_t)i * blen, w, blen);  // little-endian host
  }
  if (scope) (void)napi_close_handle_scope(env, scope);
  return res;
}

// unpackBigInts(bytes: Uint8Array, byteLen) -> BigInt[]: little-endian fields of byteLen bytes each
static napi_value UnpackBigInts(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  uint8_t* buf;
  size_t len;
  uint32_t blen = 0;
  if (argc < 2 || !get_u8(env, argv[0], &buf, &len) || napi_get_value_uint32(env, argv[1], &blen) != napi_ok || blen == 0 || blen > 64 ||
      blen % 8 || len % blen) {
    napi_throw_type_error(env, nullptr, "noble-gpu: unpackBigInts(Uint8Array, byteLen multiple of 8, <= 64)");
    return nullptr;
  }
  const size_t m = len / blen;
  napi_value arr;
  NAPI_OK(napi_create_array_with_length(env, m, &arr));
  for (size_t i = 0; i < m; i++) {
    uint64_t w[8];
    memcpy(w, buf + i * blen, blen);
    napi_value v;
    NAPI_OK(napi_create_bigint_words(env, 0, blen / 8, w, &v));
    NAPI_OK(napi_set_element(env, arr, (uint32_t)i, v));
  }
  return arr;
}

static napi_value UploadPoints(napi_env env, napi_callback_info info) {  // (curveId, Uint8Array affine | encoded, encoded?, zip215?)
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve;
  uint8_t* buf;
  size_t len;
  bool encoded = false, zip215 = false;
  if (argc < 2 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || !get_u8(env, argv[1], &buf, &len)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: uploadPoints(curveId, Uint8Array, encoded, zip215)");
    return nullptr;
  }
  if (argc >= 3) napi_get_value_bool(env, argv[2], &encoded);
  if (argc >= 4) napi_get_value_bool(env, argv[3], &zip215);
  const int unit = encoded ? encoded_bytes(curve) : ncg_point_bytes(curve);
  if (unit == 0 || len % unit) {
    napi_throw_error(env, nullptr, "noble-gpu: uploadPoints: buffer is not a whole number of points");
    return nullptr;
  }
  ncg_points* h = nullptr;
  int64_t bad = -1;
  int rc = encoded ? ncg_points_from_encoded(g_ctx, curve, len / unit, buf, zip215 ? 1 : 0, &h, &bad)
                   : ncg_points_upload(g_ctx, curve, len / unit, buf, &h);
  if (rc != 0) return throw_native(env);
  size_t slot = g_sets.size();
  for (size_t i = 0; i < g_sets.size(); i++)
    if (!g_sets[i]) { slot = i; break; }
  if (slot == g_sets.size()) g_sets.push_back(nullptr);
  g_sets[slot] = h;
  napi_value r;
  napi_create_uint32(env, (uint32_t)slot, &r);
  return r;
}

static ncg_points* get_set(napi_env env, napi_value v) {
  uint32_t id = 0;
  if (napi_get_value_uint32(env, v, &id) != napi_ok || id >= g_sets.size() || !g_sets[id]) {
    napi_throw_error(env, nullptr, "noble-gpu: unknown point-set handle");
    return nullptr;
  }
  return g_sets[id];
}

static napi_value FreePoints(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  uint32_t id = 0;
  if (argc >= 1 && napi_get_value_uint32(env, argv[0], &id) == napi_ok && id < g_sets.size() && g_sets[id]) {
    ncg_points_free(g_sets[id]);
    g_sets[id] = nullptr;
  }
  return nullptr;
}

// (handle) -> -1 if every point lies in the prime-order subgroup (the set then takes the endomorphism MSM),
// else the index of the first point outside it (the set keeps the generic path); bls12-381 only
static napi_value VerifySubgroup(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  ncg_points* h = argc >= 1 ? get_set(env, argv[0]) : nullptr;
  if (!h) return nullptr;
  int64_t bad = -1;
  if (ncg_points_verify_subgroup(g_ctx, h, &bad) != NCG_OK) {
    napi_throw_error(env, nullptr, ncg_last_error(g_ctx));
    return nullptr;
  }
  napi_value r;
  NAPI_OK(napi_create_int64(env, bad, &r));
  return r;
}
// precomputePoints(handle) -> boolean: interleavedMSMUnsafe's per-point tables in device form (ncg_points_precompute)
static napi_value PrecomputePoints(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  ncg_points* h = argc >= 1 ? get_set(env, argv[0]) : nullptr;
  if (!h) return nullptr;
  if (ncg_points_precompute(g_ctx, h) != NCG_OK) {
    napi_throw_error(env, nullptr, ncg_last_error(g_ctx));
    return nullptr;
  }
  napi_value r;
  NAPI_OK(napi_get_boolean(env, ncg_points_precomputed(h) != 0, &r));
  return r;
}
static napi_value InSubgroup(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  ncg_points* h = argc >= 1 ? get_set(env, argv[0]) : nullptr;
  if (!h) return nullptr;
  napi_value r;
  NAPI_OK(napi_get_boolean(env, ncg_points_in_subgroup(h) != 0, &r));
  return r;
}

static napi_value MsmResident(napi_env env, napi_callback_info info) {  // (handle, scalars) -> affine || inf
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  ncg_points* h = argc >= 1 ? get_set(env, argv[0]) : nullptr;
  if (!h) return nullptr;
  const size_t n = ncg_points_count(h);
  std::vector<uint8_t> store;
  uint8_t *sc = nullptr, *out;
  if (argc < 2 || !get_scalars(env, argv[1], n, store, &sc)) {
    napi_throw_error(env, nullptr, "arrays of points and scalars must have equal length");
    return nullptr;
  }
  const int pb = ncg_point_bytes(ncg_points_curve(h));
  napi_value res = make_u8(env, pb + 1, &out);
  if (!res) return nullptr;
  if (ncg_msm_resident(g_ctx, h, sc, out, out + pb) != 0) return throw_native(env);
  return res;
}

static napi_value MulVarResident(napi_env env, napi_callback_info info) {  // (handle, scalars) -> n x (affine) || n x inf
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  ncg_points* h = argc >= 1 ? get_set(env, argv[0]) : nullptr;
  if (!h) return nullptr;
  const size_t n = ncg_points_count(h);
  std::vector<uint8_t> store;
  uint8_t *sc = nullptr, *out;
  if (argc < 2 || !get_scalars(env, argv[1], n, store, &sc)) {
    napi_throw_error(env, nullptr, "arrays of points and scalars must have equal length");
    return nullptr;
  }
  const int pb = ncg_point_bytes(ncg_points_curve(h));
  napi_value res = make_u8(env, n * (pb + 1), &out);
  if (!res) return nullptr;
  if (n && ncg_mul_var_batch_resident(g_ctx, h, sc, out, out + n * pb) != 0) return throw_native(env);
  return res;
}

static int encoded_bytes(int curve) { return curve == 0 ? 33 : curve == 1 ? 32 : curve == 2 ? 48 : curve == 3 ? 96 : 0; }

static napi_value DecodePoints(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve;
  uint8_t *enc, *out;
  size_t el;
  bool zip215 = false;
  if (argc < 2 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || !get_u8(env, argv[1], &enc, &el)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: decodePoints(curveId, Uint8Array, zip215)");
    return nullptr;
  }
  if (argc >= 3) napi_get_value_bool(env, argv[2], &zip215);
  int eb = encoded_bytes(curve), pb = ncg_point_bytes(curve);
  if (!eb || el % eb) {
    napi_throw_error(env, nullptr, "noble-gpu: decodePoints: bad curve or length");
    return nullptr;
  }
  size_t n = el / eb;
  napi_value res = make_u8(env, n * (pb + 2), &out);
  if (!res) return nullptr;
  if (n && ncg_decode_points_batch(g_ctx, curve, n, enc, zip215 ? NCG_DECODE_ZIP215 : 0, out, out + n * pb, out + n * pb + n) != 0)
    return throw_native(env);
  return res;
}

static napi_value AggregateEncoded(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve;
  uint8_t *enc, *out;
  size_t el;
  bool zip215 = false;
  if (argc < 2 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || !get_u8(env, argv[1], &enc, &el)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: aggregateEncoded(curveId, Uint8Array, zip215)");
    return nullptr;
  }
  if (argc >= 3) napi_get_value_bool(env, argv[2], &zip215);
  int eb = encoded_bytes(curve), pb = ncg_point_bytes(curve);
  if (!eb || el % eb) {
    napi_throw_error(env, nullptr, "noble-gpu: aggregateEncoded: bad curve or length");
    return nullptr;
  }
  napi_value res = make_u8(env, pb + 1, &out);
  if (!res) return nullptr;
  int64_t bad = -1;
  if (ncg_aggregate_encoded(g_ctx, curve, el / eb, enc, zip215 ? NCG_DECODE_ZIP215 : 0, out, out + pb, &bad) != 0)
    return throw_native(env);
  return res;
}

static napi_value EncodePoints(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve;
  uint8_t *pts, *out;
  size_t pl;
  if (argc < 2 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || !get_u8(env, argv[1], &pts, &pl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: encodePoints(curveId, Uint8Array)");
    return nullptr;
  }
  int eb = encoded_bytes(curve), pb = ncg_point_bytes(curve);
  if (!eb || pl % pb) {
    napi_throw_error(env, nullptr, "noble-gpu: encodePoints: bad curve or length");
    return nullptr;
  }
  size_t n = pl / pb;
  napi_value res = make_u8(env, n * (eb + 1), &out);
  if (!res) return nullptr;
  if (n && ncg_encode_points_batch(g_ctx, curve, n, pts, out, out + n * eb) != 0) return throw_native(env);
  return res;
}

static napi_value Ntt(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t log2n, flags = 0, field = NCG_FIELD_BLS12_381_FR;
  uint8_t *om, *data, *out;
  size_t ol, dl;
  if (argc < 3 || napi_get_value_int32(env, argv[0], &log2n) != napi_ok || !get_u8(env, argv[1], &om, &ol) || ol != 32 ||
      !get_u8(env, argv[2], &data, &dl)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: ntt(log2n, omega32, data, flags, field)");
    return nullptr;
  }
  if (argc >= 4) napi_get_value_int32(env, argv[3], &flags);
  if (argc >= 5) napi_get_value_int32(env, argv[4], &field);
  if (log2n < 0 || log2n > NCG_NTT_MAX_LOG2N || dl % ((size_t)32 << log2n)) {
    napi_throw_error(env, nullptr, "FFT: Polynomial size should be power of two");
    return nullptr;
  }
  napi_value res = make_u8(env, dl, &out);
  if (!res) return nullptr;
  size_t batch = dl / ((size_t)32 << log2n);
  if (batch && ncg_ntt(g_ctx, field, log2n, batch, om, data, out, flags) != 0) return throw_native(env);
  return res;
}

// poly(kind, field, a, b, small, i1, i2): one entry for the polynomial operations of include/ncg.h.  a, b: packed 32-byte
// little-endian elements (or null); small: the host operands; returns the packed result.
//   kind 0 pointwise   i1 = NCG_POLY_ADD | SUB | DOT                              -> n elements
//        1 scale       small = scalar (32 bytes), i1 = powers (0: a[i] s, 1: a[i] s^i) -> n elements
//        2 eval        sum a[i] b[i]                                              -> 1 element
//        3 evalMonomial small = m points (m * 32 bytes)                           -> m elements
//        4 lagrangeBasis small = omega || x (64 bytes), i1 = log2n, i2 = brp      -> 2^log2n elements
//        5 mul         small = omega (32 bytes), i1 = log2n; a, b at most 2^log2n elements each -> 2^log2n elements
static napi_value Poly(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t kind = -1, field = 0, i1 = 0, i2 = 0;
  uint8_t *a = nullptr, *b = nullptr, *sm = nullptr, *out = nullptr;
  size_t al = 0, bl = 0, sl = 0;
  bool ok = argc >= 5 && napi_get_value_int32(env, argv[0], &kind) == napi_ok && napi_get_value_int32(env, argv[1], &field) == napi_ok;
  if (ok) {
    get_u8(env, argv[2], &a, &al);   // null / undefined leave the operand empty
    get_u8(env, argv[3], &b, &bl);
    get_u8(env, argv[4], &sm, &sl);
    if (argc >= 6) napi_get_value_int32(env, argv[5], &i1);
    if (argc >= 7) napi_get_value_int32(env, argv[6], &i2);
    ok = al % 32 == 0 && bl % 32 == 0 && sl % 32 == 0;
  }
  const size_t n = al / 32;
  const bool bits_ok = i1 >= 0 && i1 <= NCG_NTT_MAX_LOG2N;
  switch (ok ? kind : -1) {
    case 0: ok = bl == al; break;
    case 1: ok = sl == 32; break;
    case 2: ok = bl == al; break;
    case 3: ok = sl >= 32 && sl <= 32 * NCG_POLY_MAX_POINTS; break;
    case 4: ok = sl == 64 && bits_ok; break;
    case 5: ok = sl == 32 && bits_ok && n <= ((size_t)1 << i1) && bl / 32 <= ((size_t)1 << i1); break;
    default: ok = false;
  }
  if (!ok) {
    napi_throw_type_error(env, nullptr, "noble-gpu: poly(kind, field, a, b, small, i1, i2)");
    return nullptr;
  }
  const size_t out_elems = kind <= 1 ? n : kind == 2 ? 1 : kind == 3 ? sl / 32 : (size_t)1 << i1;
  napi_value res = make_u8(env, out_elems * 32, &out);
  if (!res) return nullptr;
  int rc = 0;
  switch (kind) {
    case 0: rc = ncg_poly_pointwise(g_ctx, field, i1, n, a, b, out); break;
    case 1: rc = ncg_poly_scale(g_ctx, field, n, a, sm, i1, out); break;
    case 2: rc = ncg_poly_eval(g_ctx, field, n, a, b, out); break;
    case 3: rc = ncg_poly_eval_monomial(g_ctx, field, n, a, (int)(sl / 32), sm, out); break;
    case 4: rc = ncg_poly_lagrange_basis(g_ctx, field, i1, sm, sm + 32, i2, out); break;
    default: rc = ncg_poly_mul(g_ctx, field, i1, sm, n, a, bl / 32, b, out); break;
  }
  if (rc != 0) return throw_native(env);
  return res;
}

static napi_value MapToCurve(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!need_ctx(env)) return nullptr;
  int32_t curve, count;
  uint8_t *u, *out;
  size_t ul;
  if (argc < 3 || napi_get_value_int32(env, argv[0], &curve) != napi_ok || napi_get_value_int32(env, argv[1], &count) != napi_ok ||
      !get_u8(env, argv[2], &u, &ul)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: mapToCurve(curveId, count, Uint8Array)");
    return nullptr;
  }
  int pb = ncg_point_bytes(curve);
  size_t per = (size_t)count * (pb / 2);
  if ((curve != NCG_BLS12_381_G1 && curve != NCG_BLS12_381_G2) || (count != 1 && count != 2) || ul % per) {
    napi_throw_error(env, nullptr, "noble-gpu: mapToCurve: bad curve, count or length");
    return nullptr;
  }
  size_t n = ul / per;
  napi_value res = make_u8(env, n * (pb + 1), &out);
  if (!res) return nullptr;
  if (n && ncg_map_to_curve_batch(g_ctx, curve, n, count, u, out, out + n * pb) != 0) return throw_native(env);
  return res;
}

static napi_value PointBytes(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], r;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t curve = -1;
  if (argc >= 1) napi_get_value_int32(env, argv[0], &curve);
  NAPI_OK(napi_create_int32(env, ncg_point_bytes(curve), &r));
  return r;
}

// hostRegister(Uint8Array) / hostUnregister(Uint8Array): pin a long-lived input / output buffer ONCE (ncg_host_register),
// so that every later call on it moves by DMA at PCIe speed with no per-call page locking
// A registered array must outlive its registration: a strong reference is held from hostRegister until hostUnregister, so the
// backing store cannot be collected (and its address range handed to another allocation) while HIP still has it pinned.
// The map is process-wide (ncg_host_register is) while a napi_ref belongs to ONE env: worker_threads each load the addon, so the
// map is guarded by a mutex and an entry remembers the env that made it; only that env may delete its reference.
struct Registered { napi_env env; napi_ref ref; size_t len; };
static std::map<uintptr_t, Registered> g_registered;
static std::mutex g_registered_mu;
static napi_value HostRegister(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  uint8_t* p;
  size_t len;
  if (argc < 1 || !get_u8(env, argv[0], &p, &len)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: hostRegister(Uint8Array)");
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(g_registered_mu);
  auto have = g_registered.find((uintptr_t)p);
  if (have != g_registered.end()) {
    if (have->second.len >= len) return nullptr;   // already registered through this addon, at least this long
    // the same base with a LARGER length: silently succeeding would leave the tail unpinned
    napi_throw_error(env, nullptr, "noble-gpu: hostRegister: this buffer is already registered with a smaller length - hostUnregister it first");
    return nullptr;
  }
  if (ncg_host_register(p, len) != 0) return throw_native(env);
  napi_ref ref = nullptr;
  if (napi_create_reference(env, argv[0], 1, &ref) != napi_ok) {
    (void)ncg_host_unregister(p);
    napi_throw_error(env, nullptr, "noble-gpu: hostRegister: cannot hold a reference to the array");
    return nullptr;
  }
  g_registered[(uintptr_t)p] = Registered{env, ref, len};
  return nullptr;
}
static napi_value HostUnregister(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  uint8_t* p;
  size_t len;
  if (argc < 1 || !get_u8(env, argv[0], &p, &len)) {
    napi_throw_type_error(env, nullptr, "noble-gpu: hostUnregister(Uint8Array)");
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(g_registered_mu);
  auto it = g_registered.find((uintptr_t)p);
  if (it != g_registered.end() && it->second.env != env) {
    napi_throw_error(env, nullptr, "noble-gpu: hostUnregister: this buffer was registered from another thread's environment");
    return nullptr;
  }
  (void)ncg_host_unregister(p);
  if (it != g_registered.end()) {
    (void)napi_delete_reference(env, it->second.ref);
    g_registered.erase(it);
  }
  return nullptr;
}

static napi_value Version(napi_env env, napi_callback_info) {
  napi_value r;
  NAPI_OK(napi_create_string_utf8(env, ncg_version(), NAPI_AUTO_LENGTH, &r));
  return r;
}

NAPI_MODULE_INIT() {
  struct {
    const char* name;
    napi_callback fn;
  } fns[] = {{"init", Init},           {"initMulti", InitMulti}, {"msm", Msm},
             {"mulVarBatch", MulVarBatch}, {"mulBaseBatch", MulBaseBatch},
             {"ed25519VerifyBatch", Ed25519VerifyBatch}, {"x25519", X25519}, {"ed25519Sign", Ed25519Sign}, {"secpSign", SecpSign}, {"ed448", Ed448}, {"ed448Sign", Ed448Sign}, {"ristretto", Ristretto}, {"oprf", Oprf}, {"h2c", H2c}, {"h2c448", H2c448}, {"decaf448", Decaf448},{"bls", Bls}, {"pointBytes", PointBytes},
             {"decodePoints", DecodePoints}, {"encodePoints", EncodePoints},
             {"aggregateEncoded", AggregateEncoded},
             {"ntt", Ntt},               {"poly", Poly},             {"mapToCurve", MapToCurve},
             {"packBigInts", PackBigInts}, {"unpackBigInts", UnpackBigInts}, {"uploadPoints", UploadPoints}, {"freePoints", FreePoints}, {"verifySubgroup", VerifySubgroup}, {"precomputePoints", PrecomputePoints}, {"inSubgroup", InSubgroup},
             {"msmResident", MsmResident}, {"mulVarResident", MulVarResident},
             {"ed25519VerifyMsgs", Ed25519VerifyMsgs}, {"ecdsaVerify", EcdsaVerify}, {"secpVerifyMsgs", SecpVerifyMsgs}, {"ecdsaRecover", EcdsaRecover},
             {"hostRegister", HostRegister}, {"hostUnregister", HostUnregister},
             {"version", Version}};
  for (auto& f : fns) {
    napi_value v;
    if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &v) != napi_ok) return exports;
    napi_set_named_property(env, exports, f.name, v);
  }
  return exports;
}
