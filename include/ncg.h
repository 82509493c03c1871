/* ncg.h - C ABI of the MI355X batch elliptic-curve engine ("noble-curves GPU").
 *
 * This is the drop-in boundary for the hot path of paulmillr/noble-curves.  The reference
 * has no FFI seam - the seam is its public TypeScript surface - so each entry point below
 * names the reference function whose *result* it reproduces for a whole batch.  A thin
 * N-API addon or the Python host mirror (noble-curves_amd/) binds these.
 *
 * Wire format:
 *   - field elements: canonical residues (NOT Montgomery), little-endian bytes, fixed width:
 *       secp256k1 / ed25519 / bn254 Fp: 32 bytes;  bls12-381 Fp: 48 bytes;  Fp2 = c0 || c1 (96 bytes)
 *   - affine points: x || y.  Infinity is (0,0) on Weierstrass curves
 *       (reference src/abstract/weierstrass.ts:716 fromAffine, :966 toAffine) and (0,1) on
 *       Edwards (src/abstract/edwards.ts:606); outputs also carry a separate is_inf byte.
 *   - scalars: 32 bytes little-endian, 0 <= k < 2^256 (range rules of the reference are
 *       enforced by the host shim before crossing: weierstrass.ts:904,920; curve.ts:398-404).
 *
 * Conventions: every function returns 0 on success or a negative ncg_status; no C++ type,
 * exception or torch type crosses this boundary.  Pointers suffixed _dev are device (HBM)
 * addresses valid on the context's GPU; all others are host pointers.  `stream` is a
 * hipStream_t passed as void* (NULL = the context's own stream); *_dev calls are
 * asynchronous on that stream, host-pointer calls return after the result is in host memory.
 * Device buffers must be 16-byte aligned (any hipMalloc / torch allocation is, and so is any whole-record
 * offset into one: records are 32 bytes or more); the kernels read and write them with 16-byte accesses.
 *
 * Threading and memory: a context is not thread-safe - use it from one host thread at a time (the
 * reference is single-threaded); several contexts per process are fine.  The context
 * owns its device workspaces (grown on demand, reused across calls, released by ncg_destroy): the
 * batch multiplies keep a Jacobian scratch plus a per-item window table (secp256k1 1.6 KB, ed25519
 * 1.1 KB, bls12-381 G1 1.5 KB / G2 3.0 KB per item), the MSM about 650 B per point at 2^20, the NTT
 * a twiddle table of N elements per transform size, the pairing 672 B per pair (its Miller value) plus 4 B per group, BLS verification
 * about 1.1 KB per row on top of its two pairs.
 * Because these buffers are shared, *_dev calls
 * on one context must be issued in stream order (same stream, or externally ordered); growing a
 * workspace synchronises the stream it was used on.
 */
#ifndef NCG_H
#define NCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ncg_ctx ncg_ctx;

enum ncg_curve {
  NCG_SECP256K1 = 0,     /* src/secp256k1.ts:48-64   */
  NCG_ED25519 = 1,       /* src/ed25519.ts:49-65     */
  NCG_BLS12_381_G1 = 2,  /* src/bls12-381.ts:134-148 */
  NCG_BLS12_381_G2 = 3,  /* src/bls12-381.ts:321-345 */
  NCG_BN254_G1 = 5       /* src/bn254.ts G1 (alt_bn128, EIP-196); id 4 is unassigned */
};

enum ncg_status {
  NCG_OK = 0,
  NCG_ERR_INVALID_ARG = -1,
  NCG_ERR_HIP = -2,
  NCG_ERR_NO_DEVICE = -3,
  NCG_ERR_UNSUPPORTED = -4,
  NCG_ERR_NOMEM = -5,
  NCG_ERR_RCCL = -6
};

/* ---- context ------------------------------------------------------------------------- */
/* One context per GPU.  Multi-GPU: see the "multi-GPU MSM" section below (per-process
 * communicators for one-process-per-GPU launches, ncg_multi for one process driving several GPUs). */
int ncg_init(int device_id, ncg_ctx** out_ctx);
void ncg_destroy(ncg_ctx* ctx);
const char* ncg_last_error(ncg_ctx* ctx); /* ctx may be NULL: last process-wide error */
int ncg_sync(ncg_ctx* ctx);               /* waits for the context's own stream */
const char* ncg_version(void);
/* bytes per affine point / per field element for a curve (0 if unknown) */
int ncg_point_bytes(int curve);
int ncg_field_bytes(int curve);

/* Pin a long-lived HOST buffer once (hipHostRegister): the host-pointer entry points then move it by DMA at PCIe speed
 * with no per-call page locking - what a binding does for buffers it reuses (the N-API addon's input / output Buffers).
 * Unpinned buffers stay correct: large ones are registered for the duration of each call. */
int ncg_host_register(void* host_ptr, size_t bytes);
int ncg_host_unregister(void* host_ptr);

/* ---- batch variable-base scalar multiplication ---------------------------------------
 * out[i] = scalars[i] * points[i].  Replaces, batch-wise, Point.multiplyUnsafe(k)
 * (src/abstract/weierstrass.ts:915-928; GLV path :660-671 on secp256k1) and the value of
 * Point.multiply(k) (:900-907); on ed25519 Point.multiplyUnsafe / multiply
 * (src/abstract/edwards.ts:555-577), exact integer multiples also for points with a torsion
 * component.  k = 0 or P = infinity gives infinity.  All four curves.  out_is_inf may be NULL
 * in the host-pointer variant. */
int ncg_mul_var_batch(ncg_ctx* ctx, int curve, size_t n, const void* points_affine,
                      const void* scalars, void* out_affine, uint8_t* out_is_inf);
int ncg_mul_var_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* points_affine_dev,
                          const void* scalars_dev, void* out_affine_dev,
                          uint8_t* out_is_inf_dev, void* stream);

/* ---- batch normalisation of projective points -----------------------------------------------
 * (X, Y, Z) -> affine (x, y) = (X/Z, Y/Z) for a batch with one field inversion per 8 points:
 * normalizeZ(c, points) / FpInvertBatch (src/abstract/curve.ts:311-326,
 * src/abstract/modular.ts:728-760, toAffine(invZ) src/abstract/weierstrass.ts:951-969; the same
 * map on Edwards extended points, src/abstract/edwards.ts:595-609).  Input wire: X || Y || Z,
 * canonical residues (3 field elements per point).  Z = 0 (Weierstrass identity) gives (0,0)
 * and out_is_inf = 1.  All four curves. */
int ncg_normalize_batch(ncg_ctx* ctx, int curve, size_t n, const void* points_proj, void* out_affine,
                        uint8_t* out_is_inf);
int ncg_normalize_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* points_proj_dev,
                            void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream);

/* ---- batch point decoding (decompression + validity checks) ---------------------------------
 * out[i] = Point.fromBytes(encoded[i]) as an affine wire point, out_ok[i] = 0 where the reference
 * throws.  Encodings (fixed size per curve):
 *   NCG_SECP256K1     33 bytes SEC1 compressed (src/abstract/weierstrass.ts:566-605,
 *                     sqrt src/secp256k1.ts:73-95)
 *   NCG_BLS12_381_G1  48 bytes compressed with flag bits (src/bls12-381.ts:377-459); includes
 *                     the prime-order-subgroup check of assertValidity (:567-577); the
 *                     canonical infinity encoding gives out_is_inf = 1
 *   NCG_BLS12_381_G2  96 bytes compressed, x.c1 || x.c0 (src/bls12-381.ts:354-368, Fp2.sqrt
 *                     src/abstract/tower.ts:476-500) + the psi subgroup check (:599-601)
 *   NCG_ED25519       32 bytes (src/abstract/edwards.ts:405-436); flags bit 0 = zip215
 * out_is_inf may be NULL in the host-pointer variant. */
#define NCG_DECODE_ZIP215 1
int ncg_decode_points_batch(ncg_ctx* ctx, int curve, size_t n, const void* encoded, int flags,
                            void* out_affine, uint8_t* out_ok, uint8_t* out_is_inf);
int ncg_decode_points_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* encoded_dev, int flags,
                                void* out_affine_dev, uint8_t* out_ok_dev, uint8_t* out_is_inf_dev,
                                void* stream);

/* ---- pairwise point addition -------------------------------------------------------------------
 * out[i] = a[i] + b[i] (subtract != 0: a[i] - b[i]) on affine wire points: Point.add / subtract of the
 * reference for a batch of pairs, incl. P = Q, P = -Q and ZERO operands (src/abstract/weierstrass.ts:
 * 834-891, src/abstract/edwards.ts:526-545).  With two batch multiplies this is Point.mulAddUnsafe
 * (a*P + b*Q, weierstrass.ts:937-944 - the ECDSA-verification shape). */
int ncg_add_pairs_batch(ncg_ctx* ctx, int curve, size_t n, const void* a, const void* b, int subtract,
                        void* out_affine, uint8_t* out_is_inf);
int ncg_add_pairs_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* a_dev, const void* b_dev,
                            int subtract, void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream);

/* ---- aggregation of encoded points -----------------------------------------------------------
 * out = sum_i Point.fromBytes(encoded[i]): the group operation of bls.aggregatePublicKeys /
 * aggregateSignatures on encoded inputs (src/abstract/bls.ts:857-873: normPub / fromBytes +
 * assertValidity, then the running sum).  Decoding (incl. the subgroup checks) and the sum - an MSM
 * with unit scalars - run on the device; only the encodings go up.  An entry the reference would
 * reject makes the call fail with NCG_ERR_INVALID_ARG and *out_bad_index = its position (else -1).
 * Encodings and `flags` as in ncg_decode_points_batch. */
int ncg_aggregate_encoded(ncg_ctx* ctx, int curve, size_t n, const void* encoded, int flags,
                          void* out_affine, uint8_t* out_is_inf, int64_t* out_bad_index);

/* ---- batch point encoding (Point.toBytes, compressed form) -----------------------------------
 * encoded[i] = affine wire point i in the encodings listed above (secp256k1 pointToBytes
 * src/abstract/weierstrass.ts:541-564; bls12-381 coder.encode src/bls12-381.ts:400-410; ed25519
 * src/abstract/edwards.ts:620-628).  out_ok[i] = 0 where the reference throws (secp256k1 ZERO). */
int ncg_encode_points_batch(ncg_ctx* ctx, int curve, size_t n, const void* affine, void* out_encoded,
                            uint8_t* out_ok);
int ncg_encode_points_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* affine_dev,
                                void* out_encoded_dev, uint8_t* out_ok_dev, void* stream);

/* ---- batch map-to-curve (hash-to-curve without the byte hashing) ------------------------------
 * out[i] = clearCofactor( sum_j mapToCurve(u[i][j]) ), j < count, for NCG_BLS12_381_G1 / _G2:
 * count = 2 is createHasher(...).hashToCurve after hash_to_field, count = 1 is encodeToCurve /
 * mapToCurve (src/abstract/hash-to-curve.ts:441-548; SWU :652-717, isogeny :381-410; suite
 * constants and clearCofactor src/bls12-381.ts:560-619, :668-862).  The byte-level
 * hash_to_field / expand_message_xmd (:189-228, :312-378) is done by the host shim.
 * u: n * count field elements, each one Fp (48 bytes LE) for G1 or Fp2 (c0 then c1, 96 bytes)
 * for G2, any value below 2^384 (reduced mod p like Fp.create).  ZERO gives out_is_inf = 1 and
 * (0, 0).  out_is_inf may be NULL in the host-pointer variant. */
int ncg_map_to_curve_batch(ncg_ctx* ctx, int curve, size_t n, int count, const void* u,
                           void* out_affine, uint8_t* out_is_inf);
int ncg_map_to_curve_batch_dev(ncg_ctx* ctx, int curve, size_t n, int count, const void* u_dev,
                               void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream);

/* ---- number-theoretic transform over a scalar field ------------------------------------------
 * out = FFT(roots, Fr).direct(in, brpInput, brpOutput) / .inverse(...) of the reference
 * (src/abstract/fft.ts:518-577 over FFTCore :422-480; tables rootsOfUnity :230-312) for `batch`
 * polynomials of N = 2^log2n coefficients each, stored back to back.  Elements: canonical
 * residues, 32 bytes little-endian.  `omega` (HOST pointer, 32 bytes, canonical) is the primitive
 * N-th root roots.omega(log2n) = G^((r-1)/N); the table roots(log2n) is built on the device at
 * first use and cached per size.  The inverse transform walks the reversed table
 * (roots.inverse, :296-304) and scales by 1/N (:568-570).  in and out may alias.
 * field: NCG_FIELD_BLS12_381_FR (bls12_381.fields.Fr) or NCG_FIELD_BN254_FR (bn254.fields.Fr, r =
 * 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001; the number is that of NCG_BN254_G1, whose
 * scalars it holds).  bn254 Fr has 2-adicity 28 = NCG_NTT_MAX_LOG2N; the reference's generator for it is 5
 * (findGenerator) or the 7 its tests pass.  The twiddle tables are cached per (field, log2n); a root of the other
 * field is refused as not primitive.  Every other field id returns NCG_ERR_UNSUPPORTED. */
#define NCG_FIELD_BLS12_381_FR 0
#define NCG_FIELD_BN254_FR 5
#define NCG_NTT_INVERSE 1
#define NCG_NTT_BRP_INPUT 2
#define NCG_NTT_BRP_OUTPUT 4
#define NCG_NTT_MAX_LOG2N 28
int ncg_ntt(ncg_ctx* ctx, int field, int log2n, size_t batch, const void* omega, const void* in,
            void* out, int flags);
int ncg_ntt_dev(ncg_ctx* ctx, int field, int log2n, size_t batch, const void* omega,
                const void* in_dev, void* out_dev, int flags, void* stream);

/* ---- polynomial arithmetic on vectors of scalar-field elements ------------------------------------
 * The device side of the reference's poly(field, roots, create?, fft?, length?) (src/abstract/fft.ts:583-926)
 * for the two fields of the NTT (NCG_FIELD_BLS12_381_FR, NCG_FIELD_BN254_FR; every other field id returns
 * NCG_ERR_UNSUPPORTED).  Elements: canonical residues, 32 bytes little-endian, in and out.  Every operation
 * has a host-pointer form and a _dev form on resident, 16-byte aligned buffers with a trailing stream; the
 * small operands (scalar, xs, x, omega) are HOST pointers in both forms, as omega is for ncg_ntt_dev.  The
 * _dev forms share one workspace per context: one call at a time per context, and nothing synchronises
 * with the host.
 *   pointwise       out[i] = a[i] + b[i] | a[i] - b[i] | a[i] * b[i]  (add / sub / dot, :789-806); out may
 *                   alias a or b.
 *   scale           powers = 0: out[i] = a[i] * s  (mul by a scalar, :826-830);
 *                   powers = 1: out[i] = a[i] * s^i  (shift, :838-850; 0^0 = 1).  out may alias a.
 *   eval            out32 = sum a[i] * basis[i]  (:857-862).
 *   eval_monomial   out[k] = sum a[i] * xs[k]^i for m <= NCG_POLY_MAX_POINTS points in one pass over a
 *                   (monomial.eval, :873-879).
 *   lagrange_basis  out[i] = L_i(x) over the N = 2^log2n roots of unity roots(log2n) of `omega` (the table of
 *                   ncg_ntt, cached the same way; bit-reversed order when brp is set), :882-901.  If x is
 *                   itself root i the result is the Kronecker delta at i (the reference's shortcut).
 *   mul             out = inverse(direct(a, brpOutput) .* direct(b, brpOutput), brpInput) of length N =
 *                   2^log2n: the cyclic product mod x^N - 1 (mul with an FFT, :810-814).  a and b hold
 *                   na, nb <= N coefficients and are zero-extended on the device, so na + nb - 1 <= N gives
 *                   convolve (:832-837).  na = 0 or nb = 0 gives the zero polynomial.  out may alias a or b.
 * n = 0: the vector operations return NCG_OK and touch nothing; the two evaluations write zero, so their
 * output is required even then. */
#define NCG_POLY_ADD 0
#define NCG_POLY_SUB 1
#define NCG_POLY_DOT 2
#define NCG_POLY_MAX_POINTS 8
int ncg_poly_pointwise(ncg_ctx* ctx, int field, int op, size_t n, const void* a, const void* b, void* out);
int ncg_poly_pointwise_dev(ncg_ctx* ctx, int field, int op, size_t n, const void* a_dev, const void* b_dev,
                           void* out_dev, void* stream);
int ncg_poly_scale(ncg_ctx* ctx, int field, size_t n, const void* a, const void* scalar, int powers, void* out);
int ncg_poly_scale_dev(ncg_ctx* ctx, int field, size_t n, const void* a_dev, const void* scalar, int powers,
                       void* out_dev, void* stream);
int ncg_poly_eval(ncg_ctx* ctx, int field, size_t n, const void* a, const void* basis, void* out32);
int ncg_poly_eval_dev(ncg_ctx* ctx, int field, size_t n, const void* a_dev, const void* basis_dev,
                      void* out32_dev, void* stream);
int ncg_poly_eval_monomial(ncg_ctx* ctx, int field, size_t n, const void* a, int m, const void* xs, void* out);
int ncg_poly_eval_monomial_dev(ncg_ctx* ctx, int field, size_t n, const void* a_dev, int m, const void* xs,
                               void* out_dev, void* stream);
int ncg_poly_lagrange_basis(ncg_ctx* ctx, int field, int log2n, const void* omega, const void* x, int brp,
                            void* out);
int ncg_poly_lagrange_basis_dev(ncg_ctx* ctx, int field, int log2n, const void* omega, const void* x, int brp,
                                void* out_dev, void* stream);
int ncg_poly_mul(ncg_ctx* ctx, int field, int log2n, const void* omega, size_t na, const void* a, size_t nb,
                 const void* b, void* out);
int ncg_poly_mul_dev(ncg_ctx* ctx, int field, int log2n, const void* omega, size_t na, const void* a_dev,
                     size_t nb, const void* b_dev, void* out_dev, void* stream);

/* ---- batch fixed-base scalar multiplication -----------------------------------------------
 * out[i] = scalars[i] * BASE.  Replaces, batch-wise, Point.BASE.multiply(k) / multiplyUnsafe(k)
 * through the cached window table (ScalarMultiplier.wnafCachedCT, src/abstract/curve.ts:588-606;
 * table :560-577) - e.g. getPublicKey.  k = 0 gives infinity.  The table (33 x 128 window
 * multiples of BASE) is built on the device at first use and cached in the context. */
int ncg_mul_base_batch(ncg_ctx* ctx, int curve, size_t n, const void* scalars, void* out_affine,
                       uint8_t* out_is_inf);
int ncg_mul_base_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* scalars_dev,
                           void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream);

/* ---- multi-scalar multiplication ---------------------------------------------------------
 * out = sum_i scalars[i] * points[i].  Replaces pippenger(c, points, scalars)
 * (src/abstract/curve.ts:863-905) on all four curves; n = 0 gives infinity (:878); scalar 0 and
 * infinity points are allowed.  The result (one affine point, canonical residues) is written to HOST memory
 * in both variants: the last step (Horner over <= 272 window/level sums + one inversion) runs
 * on the host, so the call returns after synchronising the stream. */
int ncg_msm(ncg_ctx* ctx, int curve, size_t n, const void* points_affine, const void* scalars,
            void* out_affine, uint8_t* out_is_inf);
/* The window plan the MSM entry points use for n points (measurement / diagnostics): out4 = {window bits c,
 * windows, buckets per window 2^(c-1) (signed digits), grouped window sums per window handed to the host finish}. */
int ncg_msm_plan_info(int curve, size_t n, int* out4);
int ncg_msm_dev(ncg_ctx* ctx, int curve, size_t n, const void* points_affine_dev,
                const void* scalars_dev, void* out_affine, uint8_t* out_is_inf, void* stream);
/* Diagnostics of the MSM pipeline on one context.  ncg_msm_set_tuning overrides two internals that decide HOW buckets are
 * cut, never the result: `seg` = sorted entries per accumulate lane (lane boundaries cut buckets into pieces), `run_serial`
 * = how many following pieces the owner of a cut bucket adds itself before the run goes to the long-run work list
 * (k_msm_fixup_long); seg <= 0 / run_serial < 0 restore the measured defaults.  ncg_msm_last_plan reports what the last MSM
 * launch on the context ran with: out8 = {window bits c, windows run, buckets per window, first window, windows of the whole
 * plan, seg, run_serial, runs that went to the work list}; it synchronises the device.  (tests/test_gpu_msm.py uses the pair
 * to cut buckets in every possible way and to prove that the requested cut was the one executed.) */
int ncg_msm_set_tuning(ncg_ctx* ctx, int seg, int run_serial);
int ncg_msm_last_plan(ncg_ctx* ctx, int* out8);

/* ---- resident point sets --------------------------------------------------------------------
 * Upload a point set once, multiply many times with only the scalars crossing - the usage pattern of
 * the reference's interleavedMSMUnsafe closure (src/abstract/curve.ts:907-959: precompute for a fixed
 * point set, call with scalars), and the answer to SURVEY 8a gotcha 8 (marshalling dominates an
 * end-to-end call).  ncg_points_from_encoded takes the points in their compressed wire encodings
 * (sizes as for ncg_decode_points_batch) and decodes / validates them on the device; an entry the
 * reference's fromBytes would reject fails the call and is named in *out_bad_index.  A handle
 * belongs to the context it was made on; free it before the context. */
typedef struct ncg_points ncg_points;
int ncg_points_upload(ncg_ctx* ctx, int curve, size_t n, const void* points_affine, ncg_points** out);
int ncg_points_from_encoded(ncg_ctx* ctx, int curve, size_t n, const void* encoded, int flags,
                            ncg_points** out, int64_t* out_bad_index);
void ncg_points_free(ncg_points* pts);
size_t ncg_points_count(const ncg_points* pts);
int ncg_points_curve(const ncg_points* pts);
const void* ncg_points_dev(const ncg_points* pts); /* device address of the affine wire points */
/* bls12-381 G1 / G2 sets whose points all lie in the prime-order subgroup get a faster ncg_msm_resident: the
 * scalars are split along the curve endomorphism (G1: k = k1 + k2 z^2 with phi, the map of the reference's own
 * subgroup test bls12-381.ts:567-577; G2: k = sum d_e z^e with psi, :599-601), which halves / quarters the
 * window count for the same group element.  pippenger itself (curve.ts:863-905) takes arbitrary curve points,
 * so this is never assumed: sets from ncg_points_from_encoded qualify automatically (the decoder runs the
 * reference's subgroup test on every point); for uploaded affine points ncg_points_verify_subgroup runs the
 * test once - every point P must satisfy [z^2]P = -phi(P) resp. [z]P = -psi(P) - and enables the path only if
 * all pass.  A failing set is not an error: *out_bad_index names the first point outside the subgroup and the
 * set keeps using the generic path.  ncg_points_in_subgroup: 1 if the fast path is active.  A verified set also
 * makes ncg_mul_var_batch_resident* use the endomorphism ladders (G1: two 128-bit half-scalars, half the doublings;
 * G2: four 64-bit streams along psi, a quarter of the doublings) - same group elements as the generic ladder. */
int ncg_points_verify_subgroup(ncg_ctx* ctx, ncg_points* pts, int64_t* out_bad_index);
/* The precomputation of interleavedMSMUnsafe (src/abstract/curve.ts:907-959: per-point tables built ONCE for a
 * fixed point set) in device form: window-shifted copies 2^(16 w) P of every point (or of every endomorphism image
 * of a verified set - call ncg_points_verify_subgroup first to get those), 16 / 8 / 4 copies of the set in device
 * memory.  ncg_msm_resident* then adds every window into ONE bucket set: the bucket fold runs once instead of once
 * per window and the serial combine across windows (curve.ts:901-902) disappears.  Same group element, bit for bit.
 * Weierstrass curves, sets of >= 4096 points; otherwise (and when memory is short) the call succeeds and changes
 * nothing.  ncg_points_precomputed: 1 if the shared-bucket path is active. */
int ncg_points_precompute(ncg_ctx* ctx, ncg_points* pts);
int ncg_points_precomputed(const ncg_points* pts);
int ncg_points_in_subgroup(const ncg_points* pts);
/* pippenger(c, <resident points>, scalars) and the batch multiplyUnsafe on them; scalars: host */
int ncg_msm_resident(ncg_ctx* ctx, const ncg_points* pts, const void* scalars, void* out_affine,
                     uint8_t* out_is_inf);
int ncg_msm_resident_dev(ncg_ctx* ctx, const ncg_points* pts, const void* scalars_dev, void* out_affine,
                         uint8_t* out_is_inf, void* stream); /* scalars: device, 32 B LE each */
int ncg_mul_var_batch_resident(ncg_ctx* ctx, const ncg_points* pts, const void* scalars,
                               void* out_affine, uint8_t* out_is_inf);
/* the same with scalars (32 B LE each), results and infinity flags (all required) in device memory */
int ncg_mul_var_batch_resident_dev(ncg_ctx* ctx, const ncg_points* pts, const void* scalars_dev,
                                   void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream);

/* ---- multi-GPU MSM ---------------------------------------------------------------------
 * pippenger is a sum over points (src/abstract/curve.ts:863-905; its last step is the chain
 * `sum = sum.add(resI)` :895-902), so the points are sharded: each GPU runs the single-GPU pipeline on
 * its slice up to the grouped window sums (~18 KB for G1), ONE ncclAllGather over xGMI exchanges those,
 * a small kernel adds the G arrays (pairwise tree, log2 G additions deep) and the usual finish follows.  No
 * bucket-sized data moves and nothing but the final point reaches the host.  All four curves
 * (BASELINE configs[3] G1 and configs[4] G2).  SURVEY 8(b): "one RCCL communicator for the device
 * set, all hidden behind the call"; RCCL (librccl.so) is loaded on first use.
 *
 * (1) One process per GPU (torch.distributed, MPI, bench.py): rank 0 calls ncg_comm_unique_id and
 *     ships the 128 bytes to the other ranks by any means; every rank calls ncg_comm_init on its own
 *     context (collective).  ncg_msm_sharded_dev is then a collective: every rank passes ITS points
 *     (n_local of them, device memory) and n_max = the largest n_local of any rank (it fixes the
 *     window plan, which must agree on all ranks; pass 0 only if all ranks hold n_local points); every
 *     rank receives the same sum in host memory.  Without a communicator it is ncg_msm_dev.
 *     Every rank posts a slot of the same fixed size (ncg_msm_shard_slot_bytes) whatever plan it derived;
 *     ranks whose plans disagree get NCG_ERR_INVALID_ARG after the gather, never a mismatched collective. */
#define NCG_COMM_ID_BYTES 128
int ncg_comm_unique_id(uint8_t* out_id128);
int ncg_comm_init(ncg_ctx* ctx, int nranks, int rank, const uint8_t* id128);
int ncg_comm_destroy(ncg_ctx* ctx); /* also done by ncg_destroy */
int ncg_comm_size(ncg_ctx* ctx);
int ncg_comm_rank(ncg_ctx* ctx);
/* the communicator's OWN answer (ncclCommCount / ncclCommUserRank); *out_ranks = 0 when the context has none */
int ncg_comm_count(ncg_ctx* ctx, int* out_ranks, int* out_rank);
int ncg_msm_sharded_dev(ncg_ctx* ctx, int curve, size_t n_local, size_t n_max,
                        const void* points_affine_dev, const void* scalars_dev, void* out_affine,
                        uint8_t* out_is_inf, void* stream);
/* The same sharded MSM with a HOST-STAGED exchange, for transports other than RCCL (gloo, MPI, sockets; also how
 * two ranks sharing one GPU are tested): ncg_msm_shard_local_dev runs this rank's per-shard phase and writes its
 * slot - a 32-byte header (window plan, window range, mode, scalar-range verdict) + the grouped window sums,
 * ncg_msm_shard_slot_bytes(curve) bytes, zero padded - to host memory; a scalar outside the group order does NOT fail
 * this call: the verdict travels in the header and fails ncg_msm_shard_combine on EVERY rank (so no rank leaves the
 * exchange early); the caller gathers the slots of all ranks (rank order) and any rank calls
 * ncg_msm_shard_combine on the concatenation: upload, header check, adding kernel, finish - the code
 * ncg_msm_sharded_dev runs after its all-gather.  n_max as above (the same value on every rank and in combine). */
size_t ncg_msm_shard_slot_bytes(int curve);
int ncg_msm_shard_local_dev(ncg_ctx* ctx, int curve, size_t n_local, size_t n_max, const void* points_affine_dev,
                            const void* scalars_dev, void* slot_out, void* stream);
int ncg_msm_shard_combine(ncg_ctx* ctx, int curve, size_t n_max, int nparts, const void* slots, void* out_affine,
                          uint8_t* out_is_inf, void* stream);
/* WINDOW-sharded mode (strong scaling of ONE MSM; round 4).  pippenger's windows are independent until its final
 * double-and-add chain (src/abstract/curve.ts:886-902), so when every rank holds ALL n points and scalars - a replicated
 * array, or a resident set uploaded on every GPU (the fixed bases of a prover) - rank r of G runs only a contiguous range of
 * the windows (2 of 16 at G = 8 for 2^20 bls12-381 G1 points): digits, sort, accumulate and the throughput part of the
 * bucket fold all divide by G, where point sharding leaves every rank the full fold and tail.  The slots hold the ranks'
 * grouped window sums; they are CONCATENATED (no group additions) and every rank runs the Horner chain.  On a
 * precomputed resident set (ncg_points_precompute) the rank's windows add into ONE bucket set and the slots are added.
 * Pass points_affine_dev (n points, device) or `resident` (then curve / n / points_affine_dev are ignored); scalars_dev:
 * all n scalars.  Collective over the context's communicator like ncg_msm_sharded_dev; without one it is a single-GPU MSM.
 * Host-staged twin: ncg_msm_shard_windows_local_dev (part r of nparts) -> any all-gather -> ncg_msm_shard_combine (which
 * reads the mode from the slot headers). */
int ncg_msm_sharded_windows_dev(ncg_ctx* ctx, int curve, size_t n, const void* points_affine_dev, const ncg_points* resident,
                                const void* scalars_dev, void* out_affine, uint8_t* out_is_inf, void* stream);
int ncg_msm_shard_windows_local_dev(ncg_ctx* ctx, int curve, size_t n, int part, int nparts, const void* points_affine_dev,
                                    const ncg_points* resident, const void* scalars_dev, void* slot_out, void* stream);
/* the window-sharded pipeline on ONE GPU: the parts run in turn, then the same concatenation / finish */
int ncg_msm_split_windows_dev(ncg_ctx* ctx, int curve, size_t n, int parts, const void* points_affine_dev,
                              const ncg_points* resident, const void* scalars_dev, void* out_affine, uint8_t* out_is_inf,
                              void* stream);
/* Several MSMs in flight (round 4).  A context has ncg_msm_async_lanes() lanes; each owns a stream, a workspace and a
 * pinned landing area.  ncg_msm_async_submit enqueues one MSM on a lane and returns at once (`stream`, if given, is the
 * stream the inputs were produced on; the lane waits for it); ncg_msm_async_collect waits for that MSM, runs the host
 * finish and frees the lane.  Used in turn, the lanes overlap the dependent tail of one MSM (narrow fold levels, per-window
 * tail, D2H, host Horner: latency, not throughput) with the sort / accumulate kernels of the next - the steady-state time
 * per MSM is the throughput part alone.  Points: device array or `resident` (as above).  flags: NCG_MSM_ASYNC_WINDOWS =
 * window-sharded over the context's communicator (collective: all ranks submit / collect the same lanes in the same order).
 * Errors of the MSM itself (scalar outside the group order, plans that disagree) are reported by collect. */
#define NCG_MSM_ASYNC_WINDOWS 1
/* ONE part of a window-sharded MSM on a lane (part p of P, no communicator): its slot comes back through
 * ncg_msm_async_collect_slot and goes, with the other parts' slots, to ncg_msm_shard_combine.  This is the host-staged
 * exchange with several parts in flight - and how one GPU measures a rank's share of a G-GPU MSM (bench.py). */
#define NCG_MSM_ASYNC_PART_FLAG 2
#define NCG_MSM_ASYNC_PART(p, P) (NCG_MSM_ASYNC_PART_FLAG | ((p) << 8) | ((P) << 20))
int ncg_msm_async_collect_slot(ncg_ctx* ctx, int lane, void* slot_out);
int ncg_msm_async_lanes(void);
int ncg_msm_async_submit(ncg_ctx* ctx, int lane, int curve, size_t n, const void* points_affine_dev, const ncg_points* resident,
                         const void* scalars_dev, int flags, void* stream);
int ncg_msm_async_collect(ncg_ctx* ctx, int lane, void* out_affine, uint8_t* out_is_inf);
/* The sharded pipeline on ONE GPU (self-check, shard-plan A/B): the points are cut into `parts` slices,
 * each runs the per-shard phase in turn, the slices' window sums go through the multi-GPU combine kernel
 * and finish - everything of ncg_msm_sharded_dev except the all-gather. */
int ncg_msm_split_dev(ncg_ctx* ctx, int curve, size_t n, int parts, const void* points_affine_dev,
                      const void* scalars_dev, void* out_affine, uint8_t* out_is_inf, void* stream);
/* (2) One process, several GPUs (the shape of the N-API addon: Node runs one thread).  ncg_multi_init
 *     opens a context per device and one communicator over the set (ncclCommInitAll); ncg_msm_multi
 *     takes HOST arrays like ncg_msm, uploads slice g to device g, and returns the sum. */
typedef struct ncg_multi ncg_multi;
int ncg_multi_init(const int* device_ids, int n_dev, ncg_multi** out);
void ncg_multi_destroy(ncg_multi* m);
int ncg_multi_devices(ncg_multi* m);
ncg_ctx* ncg_multi_ctx(ncg_multi* m, int i); /* context of device i (for the single-GPU entry points) */
const char* ncg_multi_last_error(ncg_multi* m);
int ncg_msm_multi(ncg_multi* m, int curve, size_t n, const void* points_affine, const void* scalars,
                  void* out_affine, uint8_t* out_is_inf);

/* ---- ed25519 batch signature verification -------------------------------------------------
 * out_ok[i] = eddsa.verify(sig[i], msg[i], pk[i], {zip215}) of the reference
 * (src/abstract/edwards.ts:942-989) given the already-hashed challenge
 * k32[i] = SHA-512(R || A || M) mod L as 32 bytes LE (edwards.ts:984, :900-906; the hash is in
 * @noble/hashes and is computed by the host shim).  sig64 = R (32 B) || s (32 B) as on the wire;
 * pk32 = compressed public key.  zip215 != 0 selects the reference's default (ZIP-215) decoding
 * rules, 0 the strict RFC 8032 rules (edwards.ts:405-436, :980).  Decoding failures and
 * s >= L give 0, exactly where the reference returns false (:967-975). */
int ncg_ed25519_verify_batch(ncg_ctx* ctx, size_t n, const void* sig64, const void* pk32,
                             const void* k32, int zip215, uint8_t* out_ok);
int ncg_ed25519_verify_batch_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev,
                                 const void* pk32_dev, const void* k32_dev, int zip215,
                                 uint8_t* out_ok_dev, void* stream);

/* The same from the MESSAGES: the challenge k = SHA-512(R || A || M) mod L (edwards.ts:984, :900-906,
 * modN_LE :866-868; SHA-512 is @noble/hashes in the reference) is computed on the device, one lane per
 * signature, so nothing but (signature, key, message) crosses - SURVEY 8(b) `k32* | (msgs*, msg_off*)`.
 * msgs: the messages back to back; msg_off: n + 1 byte offsets, message i = msgs[msg_off[i] .. msg_off[i+1]).
 * ncg_ed25519_challenge_batch_dev exposes the hash step alone (out: n x 32 bytes LE). */
int ncg_ed25519_verify_batch_msgs(ncg_ctx* ctx, size_t n, const void* sig64, const void* pk32,
                                  const void* msgs, const uint64_t* msg_off, int zip215, uint8_t* out_ok);
int ncg_ed25519_verify_batch_msgs_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* pk32_dev,
                                      const void* msgs_dev, const uint64_t* msg_off_dev, int zip215,
                                      uint8_t* out_ok_dev, void* stream);
int ncg_ed25519_challenge_batch_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* pk32_dev,
                                    const void* msgs_dev, const uint64_t* msg_off_dev, void* out_k32_dev,
                                    void* stream);

/* ---- Ed25519 signing: eddsa.getPublicKey, getExtendedPublicKey and sign (edwards.ts:870-930, ed25519.ts:146-223) ----------
 * seed32: the 32-byte secret keys.  An expanded key row is 96 bytes: scalar (32 bytes LE, the clamped head of SHA-512(seed)
 * reduced mod L) || prefix (the second half of the hash) || A (the public key); ncg_ed25519_expand_key_batch writes such rows
 * for repeated use with NCG_ED25519_SIGN_EXPANDED.  Key rows, public keys and signatures are read and written as 32-bit words:
 * device pointers to them must be 4-byte aligned.
 *
 * ncg_ed25519_sign_batch: out_sig64[i] = R || S of message i under key i (or under the one key row, NCG_ED25519_SIGN_ONE_KEY)
 * and out_ok[i] = 1; 64 zero bytes and out_ok[i] = 0 where the nonce r is 0 mod L and the reference throws.  msgs / msg_off
 * as for ncg_ed25519_verify_batch_msgs.  dom: the domain prefix of both hashes, dom_len <= NCG_ED25519_DOM_MAX bytes, a HOST
 * pointer in both forms (it is the same for the whole call; NULL only with dom_len 0): empty for ed25519,
 * "SigEd25519 no Ed25519 collisions" || phflag || len(ctx) || ctx for ed25519ctx (phflag 0) and ed25519ph (phflag 1).
 * NCG_ED25519_SIGN_PREHASH signs SHA-512(M) in place of M (ed25519ph).  The secret scalars never select an address or a branch
 * (a table walk that reads every entry); this is not a constant-time claim.  Device and staging memory
 * that held keys, prefixes or nonces is cleared on the call's stream before the call returns.
 * Unknown flag bits, dom_len above the maximum, a NULL required buffer: NCG_ERR_INVALID_ARG; n = 0 returns NCG_OK. */
#define NCG_ED25519_SIGN_EXPANDED 1   /* keys are 96-byte expanded rows, not 32-byte seeds */
#define NCG_ED25519_SIGN_ONE_KEY  2   /* one key row serves all n messages */
#define NCG_ED25519_SIGN_PREHASH  4   /* hash each message with SHA-512 first (ed25519ph) */
#define NCG_ED25519_DOM_MAX 289       /* 32 + 2 + 255 */
int ncg_ed25519_public_key_batch(ncg_ctx* ctx, size_t n, const void* seed32, void* out_pk32);
int ncg_ed25519_public_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed32_dev, void* out_pk32_dev, void* stream);
int ncg_ed25519_expand_key_batch(ncg_ctx* ctx, size_t n, const void* seed32, void* out_key96);
int ncg_ed25519_expand_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed32_dev, void* out_key96_dev, void* stream);
int ncg_ed25519_sign_batch(ncg_ctx* ctx, size_t n, const void* keys, int flags, const void* dom, size_t dom_len, const void* msgs,
                           const uint64_t* msg_off, void* out_sig64, uint8_t* out_ok);
int ncg_ed25519_sign_batch_dev(ncg_ctx* ctx, size_t n, const void* keys_dev, int flags, const void* dom, size_t dom_len,
                               const void* msgs_dev, const uint64_t* msg_off_dev, void* out_sig64_dev, uint8_t* out_ok_dev, void* stream);

/* ---- X25519 (RFC 7748) and the Ed25519 -> Curve25519 key conversion ---------------------------------
 * Every row is 32 bytes as on the wire (little-endian), 4-byte aligned; out32[i] is the 32-byte result and out_ok[i] = 1,
 * or 32 zero bytes and out_ok[i] = 0 where the reference throws.  n = 0 returns NCG_OK and touches nothing.
 *
 * ncg_x25519_batch: out32[i] = x25519.scalarMult(scalars[i], u[i]) = x25519.getSharedSecret(secret, peer)
 * (src/abstract/montgomery.ts:314-331).  The scalar bytes are RAW: the call clamps them (adjustScalarBytes: b[0] &= 248,
 * b[31] &= 127, b[31] |= 64).  Bit 255 of u is ignored and u is reduced mod p = 2^255 - 19, so the non-canonical encodings
 * 2^255 - 19 .. 2^255 - 1 are accepted (RFC 7748 section 5).  The five u of low order - 0, 1, p - 1 and the two of order 8,
 * in any encoding (p and p + 1 included) - give out_ok = 0 ('invalid private or public key received'), as would a zero
 * result.  flags: NCG_X25519_ONE_SCALAR = `scalars` holds ONE 32-byte secret used for every row (a server's static key
 * against n peer keys); any other bit returns NCG_ERR_INVALID_ARG.
 *
 * ncg_x25519_base_batch: out32[i] = x25519.getPublicKey(scalars[i]) = scalarMult(scalars[i], 9), computed like the
 * reference's own hook (src/ed25519.ts:281-290): [k]B on the fixed-base Edwards table, then u = (Z + Y) / (Z - Y).
 *
 * ncg_ed25519_to_montgomery_batch: out32[i] = ed25519.utils.toMontgomery(pk32[i]) = (1 + y) / (1 - y) of
 * Point.fromBytes(pk32[i]) under the strict rules (zip215 = false: y < p, a point of the curve, no sign bit on x = 0);
 * out_ok = 0 where the decoding fails and for y = 1 (the identity: the reference's inversion of zero throws).
 *
 * Each lane runs the same instructions whatever its scalar (the ladder swaps by selects, nothing branches or indexes on
 * a scalar bit), but the library makes no constant-time claim. */
#define NCG_X25519_ONE_SCALAR 1
int ncg_x25519_batch(ncg_ctx* ctx, size_t n, const void* scalars, const void* u, int flags, void* out32, uint8_t* out_ok);
int ncg_x25519_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, const void* u_dev, int flags, void* out32_dev,
                         uint8_t* out_ok_dev, void* stream);
int ncg_x25519_base_batch(ncg_ctx* ctx, size_t n, const void* scalars, void* out32, uint8_t* out_ok);
int ncg_x25519_base_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, void* out32_dev, uint8_t* out_ok_dev,
                              void* stream);
int ncg_ed25519_to_montgomery_batch(ncg_ctx* ctx, size_t n, const void* pk32, void* out32, uint8_t* out_ok);
int ncg_ed25519_to_montgomery_batch_dev(ncg_ctx* ctx, size_t n, const void* pk32_dev, void* out32_dev, uint8_t* out_ok_dev,
                                        void* stream);

/* ---- ristretto255 (RFC 9496): codecs, equals, hash-to-group, multiply and MSM ---------------------------
 * The prime-order group over curve25519: _RistrettoPoint and ristretto255_hasher of src/ed25519.ts:443-668.  An element crosses
 * as its 32-byte encoding; on the device it is an ed25519 wire point (x || y, 64 bytes), its Edwards REPRESENTATIVE.  A
 * representative is one of four (P + the points of order 1, 2, 4 encode alike), so it may be fed to every NCG_ED25519 entry
 * point - MSM, resident sets, add pairs, multiplies - but two elements are compared only through ncg_ristretto_equals_batch or
 * their encodings, never through their coordinates.  Rows are 32 bytes (64 for uniform input and for wire points), 4-byte
 * aligned; n = 0 returns NCG_OK and touches nothing (ncg_ristretto_msm excepted, below).
 *
 * ncg_ristretto_decode_batch: out_affine[i] = the representative of RistrettoPoint.fromBytes(enc[i]) (:510-533), out_ok[i] = 1;
 * a zero row and out_ok[i] = 0 where the reference throws: s >= p - bit 255 set included, the opposite of the rule the map's
 * parser has - or s odd ('invalid ristretto255 encoding 1'); no square root, t odd or y = 0 ('... encoding 2').
 * ncg_ristretto_encode_batch: out32[i] = toBytes() (:548-572) of the wire point i.  Any point of the curve is accepted, as in
 * the reference's fromAffine; the result for a pair that is not on the curve is unspecified.
 * ncg_ristretto_equals_batch: out_eq[i] = a[i].equals(b[i]) (:578-586) on wire points: x1 y2 == y1 x2 or y1 y2 == x1 x2.
 * ncg_ristretto_from_uniform_batch: out32[i] = ristretto255_hasher.deriveToCurve(bytes64[i]).toBytes() (:658-666; the Elligator
 * map :443-461 on each half, bit 255 of a half masked and the rest reduced mod p, then one addition).  out_affine may be
 * NULL; otherwise it also receives the representative R1 + R2.  hashToCurve is this after expand_message_xmd(msg, DST, 64,
 * SHA-512), which the host shim computes.
 * ncg_ristretto_mul_batch: out32[i] = fromBytes(enc[i]).multiply(k[i]).toBytes(): decode, the ed25519 variable-base multiply,
 * encode, all on the device - only bytes cross.  flags: NCG_RISTRETTO_ONE_SCALAR = `scalars` holds ONE 32-byte scalar used for
 * every row (broadcast on the device: an OPRF server's blindEvaluate); any other bit returns NCG_ERR_INVALID_ARG.  A rejected
 * encoding gives out_ok[i] = 0 and a zero row (its lane multiplies the identity).  Scalars as for ncg_mul_var_batch on
 * NCG_ED25519: any k below 2^256, exact integer multiples, k = 0 gives the identity (32 zero bytes); the reference's range
 * 1 <= k < L is the host shim's to enforce.
 * ncg_ristretto_mul_base_batch: out32[i] = BASE.multiply(k[i]).toBytes() on the fixed-base Edwards table of
 * ncg_mul_base_batch, encoded from the projective result without the inversion of an affine conversion.
 * ncg_ristretto_msm: out32 = toBytes(sum_i k[i] fromBytes(enc[i])): decode, then the NCG_ED25519 path of ncg_msm on the decoded
 * points where they lie, then the encoding of the one result.  out32 is HOST memory in both forms.  Scalars and their error
 * as for ncg_msm (below the group order).  An encoding the reference rejects fails the call with NCG_ERR_INVALID_ARG and
 * *out_bad_index = its position (else -1), as ncg_aggregate_encoded does.  A zero sum gives 32 zero bytes - the identity is a
 * valid element.  n = 0 does what ncg_msm does: it WRITES the identity (32 zero bytes) and therefore requires out32.
 * The library makes no constant-time claim. */
#define NCG_RISTRETTO_ONE_SCALAR 1
int ncg_ristretto_decode_batch(ncg_ctx* ctx, size_t n, const void* enc, void* out_affine, uint8_t* out_ok);
int ncg_ristretto_decode_batch_dev(ncg_ctx* ctx, size_t n, const void* enc_dev, void* out_affine_dev, uint8_t* out_ok_dev,
                                   void* stream);
int ncg_ristretto_encode_batch(ncg_ctx* ctx, size_t n, const void* affine, void* out32);
int ncg_ristretto_encode_batch_dev(ncg_ctx* ctx, size_t n, const void* affine_dev, void* out32_dev, void* stream);
int ncg_ristretto_equals_batch(ncg_ctx* ctx, size_t n, const void* a, const void* b, uint8_t* out_eq);
int ncg_ristretto_equals_batch_dev(ncg_ctx* ctx, size_t n, const void* a_dev, const void* b_dev, uint8_t* out_eq_dev,
                                   void* stream);
int ncg_ristretto_from_uniform_batch(ncg_ctx* ctx, size_t n, const void* bytes64, void* out32, void* out_affine);
int ncg_ristretto_from_uniform_batch_dev(ncg_ctx* ctx, size_t n, const void* bytes64_dev, void* out32_dev,
                                         void* out_affine_dev, void* stream);
int ncg_ristretto_mul_batch(ncg_ctx* ctx, size_t n, const void* enc, const void* scalars, int flags, void* out32,
                            uint8_t* out_ok);
int ncg_ristretto_mul_batch_dev(ncg_ctx* ctx, size_t n, const void* enc_dev, const void* scalars_dev, int flags,
                                void* out32_dev, uint8_t* out_ok_dev, void* stream);
int ncg_ristretto_mul_base_batch(ncg_ctx* ctx, size_t n, const void* scalars, void* out32);
int ncg_ristretto_mul_base_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars_dev, void* out32_dev, void* stream);
int ncg_ristretto_msm(ncg_ctx* ctx, size_t n, const void* enc, const void* scalars, void* out32, int64_t* out_bad_index);
int ncg_ristretto_msm_dev(ncg_ctx* ctx, size_t n, const void* enc_dev, const void* scalars_dev, void* out32,
                          int64_t* out_bad_index, void* stream);

/* ---- OPRF over ristretto255 (RFC 9497): OPRF, VOPRF and POPRF -------------------------------------------------
 * ristretto255_oprf of src/ed25519.ts:682, built by createOPRF (src/abstract/oprf.ts).  suite: NCG_OPRF_RISTRETTO255_SHA512, any
 * other id returns NCG_ERR_UNSUPPORTED; mode: 0 OPRF, 1 VOPRF, 2 POPRF.  Elements and scalars are rows of 32 bytes read as 8 LE
 * words (a DEVICE pointer to them must be 4-byte aligned); messages are one blob with n + 1 ascending offsets, as in
 * ncg_ed25519_sign_batch; dst, info, and in the proof calls k32, r32, B32, proof64 and the outputs are HOST pointers in both forms.
 * n = 0 returns NCG_OK and touches nothing.
 *
 * Every scalar argument is a secret: the multiply doubles, always adds and keeps by mask, the inversion is the Fermat chain for
 * L - 2, and no table is indexed by a digit.  The workspace and the staged copy of the scalars of a host form are cleared on the
 * call's stream before the call returns.  The key and the nonce of ncg_oprf_generate_proof reach the device as a kernel argument:
 * the library's copy of it is wiped, the HIP runtime's own argument buffer is beyond its reach and keeps them until it is reused.
 * This is not a constant-time claim.  n above 2^31 - 256 is refused ("batch too large").
 *
 * out_status[i]: 0 ok; 1 the element does not decode; 2 the element is the identity (exactly 32 zero bytes); 3 the scalar is zero
 * or not below L.  The element is looked at before the scalar.  A rejected row writes zero bytes and never stops the call.
 *
 * ncg_xmd_sha512_batch: out[i] = expand_message_xmd(msg i, dst, out_len) over SHA-512 (RFC 9380 section 5.3.1), out_len bytes per
 *   row, 1 <= out_len <= 256, 1 <= dst_len <= 255 (an oversize DST is hashed by the caller).
 * ncg_ristretto_hash_to_group_batch: out32[i] = ristretto255_hasher.hashToCurve(msg i, {DST: dst}).toBytes(); out_affine (may
 *   be NULL): the Edwards representative, 64 bytes.
 * ncg_ristretto_hash_to_scalar_batch: out32[i] = ristretto255_hasher.hashToScalar(msg i, {DST: dst}).
 * ncg_oprf_blind_batch: out_blinded32[i] = hashToGroup(input i) * blind i (oprf.ts:595-606).  Inputs are at most 65535 bytes
 *   (checked in the host form; the caller's promise in the _dev form).
 * ncg_oprf_mul_batch: out32[i] = element i * scalar i, or * 1 / scalar i with NCG_OPRF_INVERT; NCG_OPRF_ONE_SCALAR: scalars32 is
 *   one row used for every element (with INVERT it is inverted once).  blindEvaluate, and the unblinding of finalize.
 * ncg_oprf_finalize_batch: out64[i] = Hash(len || input i || [len || info] || 0x0020 || evaluated i / blind i || "Finalize").
 * ncg_oprf_evaluate_batch: out64[i] = the same hash of hashToGroup(input i) * scalar [1 / scalar with NCG_OPRF_INVERT] (oprf.ts:607-618;
 *   POPRF passes t = skS + m and NCG_OPRF_INVERT).  flags as ncg_oprf_mul_batch.
 *   info is read only in mode 2 and must be NULL with info_len 0 otherwise (at most 65535 bytes).
 * ncg_oprf_composite_scalars_batch: out32[i] = the d_i of getTranscripts (oprf.ts:502-513) for the public key B32 (host); C_i and
 *   D_i are hashed as given, a row where either is refused reports C's status first.  n <= 65535.
 * ncg_oprf_generate_proof: out_proof64 = c || s of generateProof(k, B, C, D) with the nonce r (oprf.ts:542-550): M by
 *   ncg_ristretto_msm, Z = k M, t3 = r M and t2 = r G by the secret multiplies.  ncg_oprf_verify_proof: *out_ok = 1 iff
 *   verifyProof accepts (oprf.ts:552-562); a c or s not below L gives 0.  Both fail with NCG_ERR_INVALID_ARG on the first
 *   refused row of C or D, on a refused B, and (generate) on k or r zero or not below L; n <= 65535; they synchronise. */
enum { NCG_OPRF_RISTRETTO255_SHA512 = 0 };
enum { NCG_OPRF_ONE_SCALAR = 1, NCG_OPRF_INVERT = 2 };
int ncg_xmd_sha512_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                         size_t out_len, void* out);
int ncg_xmd_sha512_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                             size_t dst_len, size_t out_len, void* out_dev, void* stream);
int ncg_ristretto_hash_to_group_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst,
                                      size_t dst_len, void* out32, void* out_affine);
int ncg_ristretto_hash_to_group_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                          size_t dst_len, void* out32_dev, void* out_affine_dev, void* stream);
int ncg_ristretto_hash_to_scalar_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst,
                                       size_t dst_len, void* out32);
int ncg_ristretto_hash_to_scalar_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                           size_t dst_len, void* out32_dev, void* stream);
int ncg_oprf_blind_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs, const uint64_t* off, const void* blinds32,
                         void* out_blinded32, uint8_t* out_status);
int ncg_oprf_blind_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs_dev, const uint64_t* off_dev,
                             const void* blinds32_dev, void* out_blinded32_dev, uint8_t* out_status_dev, void* stream);
int ncg_oprf_mul_batch(ncg_ctx* ctx, int suite, size_t n, const void* elements32, const void* scalars32, int flags, void* out32,
                       uint8_t* out_status);
int ncg_oprf_mul_batch_dev(ncg_ctx* ctx, int suite, size_t n, const void* elements32_dev, const void* scalars32_dev, int flags,
                           void* out32_dev, uint8_t* out_status_dev, void* stream);
int ncg_oprf_finalize_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs, const uint64_t* off, const void* info,
                            size_t info_len, const void* blinds32, const void* evaluated32, void* out64, uint8_t* out_status);
int ncg_oprf_finalize_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs_dev, const uint64_t* off_dev,
                                const void* info, size_t info_len, const void* blinds32_dev, const void* evaluated32_dev,
                                void* out64_dev, uint8_t* out_status_dev, void* stream);
int ncg_oprf_evaluate_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs, const uint64_t* off, const void* info,
                            size_t info_len, const void* scalar32, int flags, void* out64, uint8_t* out_status);
int ncg_oprf_evaluate_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* inputs_dev, const uint64_t* off_dev,
                                const void* info, size_t info_len, const void* scalar32_dev, int flags, void* out64_dev,
                                uint8_t* out_status_dev, void* stream);
int ncg_oprf_composite_scalars_batch(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32, const void* D32,
                                     void* out32, uint8_t* out_status);
int ncg_oprf_composite_scalars_batch_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32_dev,
                                         const void* D32_dev, void* out32_dev, uint8_t* out_status_dev, void* stream);
int ncg_oprf_generate_proof(ncg_ctx* ctx, int suite, int mode, size_t n, const void* k32, const void* B32, const void* C32,
                            const void* D32, const void* r32, void* out_proof64);
int ncg_oprf_generate_proof_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* k32, const void* B32, const void* C32_dev,
                                const void* D32_dev, const void* r32, void* out_proof64, void* stream);
int ncg_oprf_verify_proof(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32, const void* D32,
                          const void* proof64, uint8_t* out_ok);
int ncg_oprf_verify_proof_dev(ncg_ctx* ctx, int suite, int mode, size_t n, const void* B32, const void* C32_dev, const void* D32_dev,
                              const void* proof64, uint8_t* out_ok, void* stream);
/* The lane code of csrc/oprf.hpp on n rows of RAW uint32 words, bit for bit with its CPU twin.  Words per row (a, b, out), per op:
 *   0  a b mod L                  (8, 8, 8)    a, b below L
 *   1  1 / a mod L                (8, 8, 8)    0 < a < L; b not read
 *   2  [b] a, secret multiply     (16, 8, 8)   a = an ed25519 wire point (x, y), b below 2^253; out = the ristretto255 encoding
 *   3  one xmd                    (8, 8, 16)   a = 32 message bytes, b = DST' = DST || len(DST) in its first `variant` bytes
 *                                              (2 <= variant <= 32); out = 64 bytes
 *   4  a + b mod L   5  a - b mod L   (8, 8, 8)   a, b below L
 * b is required (non-NULL) even where it is not read.  An op nobody defines, or op 3 with a variant out of range, reads nothing and
 * leaves out zero (rows of 8 words).  n above 2^24 is refused. */
int ncg_oprf_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out);

/* ---- RFC 9380 hash-to-curve for secp256k1 and edwards25519 ----------------------------------------------------
 * secp256k1_hasher (src/secp256k1.ts:345-428: expand_message_xmd over SHA-256, simplified SWU on E', the 3-isogeny) and
 * ed25519_hasher (src/ed25519.ts:294-405: xmd over SHA-512, Elligator 2, the map to Edwards form, the cofactor 8) under
 * createHasher (src/abstract/hash-to-curve.ts:441-530), hashing included.  suite: one of NCG_H2C_*, any other id returns
 * NCG_ERR_UNSUPPORTED (ncg_map_to_curve_batch keeps refusing both curves: these are dedicated entry points).  count: NCG_H2C_RO
 * (2, hashToCurve: two field elements per row, their images added) or NCG_H2C_NU (1, encodeToCurve / mapToCurve); anything else is
 * NCG_ERR_INVALID_ARG.  Messages are one blob with n + 1 ascending offsets, as in ncg_xmd_sha512_batch; dst is a HOST pointer in
 * both forms, 1 <= dst_len <= 255 (an oversize DST is hashed by the caller: H("H2C-OVERSIZE-DST-" || DST)).  Outputs are affine
 * wire points of NCG_SECP256K1 / NCG_ED25519 (64 bytes) and one is_inf byte per row, exactly what ncg_mul_var_batch, ncg_msm and
 * ncg_encode_points_batch take; ZERO is written as (0, 0) on secp256k1 and (0, 1) on ed25519 with the byte set, as
 * ncg_mul_var_batch reports it.  Rows of words (u48, out_u, out32, the points) behind a DEVICE pointer must be 4-byte aligned.
 * n = 0 returns NCG_OK and touches nothing; n above 2^31 - 256 is refused ("batch too large").  Nothing here is secret.
 * DST' and every hand-off of a call (the uniform bytes, the reduced elements, the mapped points) live in one workspace of the context:
 * one call at a time per context, whatever streams the _dev forms are given - a second call on another stream would overwrite them.
 *
 * ncg_h2c_hash_batch: out[i] = hasher.hashToCurve(msg i, {DST: dst}) (count 2) or hasher.encodeToCurve(msg i, {DST: dst}) (count 1).
 * ncg_h2c_map_batch: u48 holds count values per row, 48 bytes little-endian each, any value below 2^384, reduced mod p like
 *   Fp.create; out[i] = hasher.mapToCurve(u) for count 1, and the cleared sum of the two images for count 2 - the way to reach
 *   Q0 = +-Q1 (a doubling, or ZERO).
 * ncg_h2c_hash_to_field_batch: out_u[i] = hash_to_field(msg i, count, {DST: dst, m: 1, k: 128}) as count reduced elements of 32
 *   bytes little-endian: the hash half of ncg_h2c_hash_batch on its own.
 * ncg_h2c_hash_to_scalar_batch: out32[i] = hasher.hashToScalar(msg i, {DST: dst}): one 48-byte chunk mod n (secp256k1) or mod L
 *   (ed25519), 32 bytes little-endian.
 * ncg_xmd_sha256_batch: out[i] = expand_message_xmd(msg i, dst, out_len) over SHA-256, out_len bytes per row, 1 <= out_len <= 256. */
enum { NCG_H2C_SECP256K1_XMD_SHA256_SSWU = 0, NCG_H2C_EDWARDS25519_XMD_SHA512_ELL2 = 1 };
enum { NCG_H2C_RO = 2, NCG_H2C_NU = 1 };
int ncg_h2c_hash_batch(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs, const uint64_t* msg_off, const void* dst,
                       size_t dst_len, void* out_affine, uint8_t* out_is_inf);
int ncg_h2c_hash_batch_dev(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev,
                           const void* dst, size_t dst_len, void* out_affine_dev, uint8_t* out_is_inf_dev, void* stream);
int ncg_h2c_map_batch(ncg_ctx* ctx, int suite, size_t n, int count, const void* u48, void* out_affine, uint8_t* out_is_inf);
int ncg_h2c_map_batch_dev(ncg_ctx* ctx, int suite, size_t n, int count, const void* u48_dev, void* out_affine_dev,
                          uint8_t* out_is_inf_dev, void* stream);
int ncg_h2c_hash_to_scalar_batch(ncg_ctx* ctx, int suite, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst,
                                 size_t dst_len, void* out32);
int ncg_h2c_hash_to_scalar_batch_dev(ncg_ctx* ctx, int suite, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev,
                                     const void* dst, size_t dst_len, void* out32_dev, void* stream);
int ncg_h2c_hash_to_field_batch(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs, const uint64_t* msg_off,
                                const void* dst, size_t dst_len, void* out_u);
int ncg_h2c_hash_to_field_batch_dev(ncg_ctx* ctx, int suite, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev,
                                    const void* dst, size_t dst_len, void* out_u_dev, void* stream);
int ncg_xmd_sha256_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                         size_t out_len, void* out);
int ncg_xmd_sha256_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                             size_t dst_len, size_t out_len, void* out_dev, void* stream);
/* The lane code of csrc/h2c_suites.hpp on n rows of RAW uint32 words, bit for bit with its CPU twin: 24 words per row of a and of
 * out, words an op does not use are not read / left zero.  Its own entry point: the table of ncg_field_check is closed.
 *   0 / 1  a[0..12) mod p of secp256k1 / ed25519 -> out[0..8)          2 / 3  a[0..12) mod n of secp256k1 / mod L -> out[0..8)
 *   4      SWU on E' of u = a[0..12): out = x, xd, y (8 words each), the point being (x / xd, y)
 *   5      the 3-isogeny at the affine point (x', y') = a[0..8), a[8..16) of E': out = X, Y, Z of the Jacobian image, Z = 0 for ZERO
 *   6      the edwards25519 map of u = a[0..12) before the cofactor: out = X, Y, Z with (x, y) = (X / Z, Y / Z)
 * An op nobody defines reads nothing and leaves out zero.  n above 2^24 is refused. */
int ncg_h2c_check(ncg_ctx* ctx, int op, size_t n, const void* a, void* out);

/* ---- X448 (RFC 7748) and Ed448-Goldilocks (RFC 8032): the reference's src/ed448.ts -------------------------------
 * The curve has no ncg_curve id and no ncg_field_check field: these are dedicated entry points, bytes in and bytes out.
 * Field elements and scalars are 56 bytes little-endian, read as 14 words: a DEVICE pointer to such rows (scalars56, u56, out56,
 * k56, the affine points x || y of 112 bytes) must be 4-byte aligned and is refused, not dereferenced, otherwise.  Encoded
 * points (57 bytes) and signatures (114 bytes) are packed rows and may sit at any address.  Host pointers may sit at any address.
 * Rejected rows come back as zero rows with out_ok[i] = 0.  n = 0 returns NCG_OK and touches nothing; n >= 2^31 is refused
 * ("too large") before any buffer is read; unknown flag bits return NCG_ERR_INVALID_ARG.
 *
 * ncg_x448_batch: out56[i] = x448.scalarMult(scalars56[i], u56[i]) = getSharedSecret (src/abstract/montgomery.ts:314-331 with
 * the ladder of :352-393, a24 = 39081, 448 steps).  The scalar bytes are RAW: the call clamps them (ed448.ts:122-130:
 * b[0] &= 252, b[55] |= 128).  u has no masked bit (montgomery.ts:277-287) and is reduced mod p = 2^448 - 2^224 - 1, so the
 * encodings p .. 2^448 - 1 are accepted.  The low-order u 0, 1, p - 1 in any encoding (p and p + 1 included) give out_ok = 0
 * ('invalid private or public key received', :303-325), as does a zero result (:329).  flags: NCG_X448_ONE_SCALAR =
 * `scalars56` holds ONE secret used for every row.
 * ncg_x448_base_batch: out56[i] = x448.getPublicKey(scalars56[i]) = scalarMult(scalars56[i], 5); the reference's Edwards hook
 * (ed448.ts:299-309) gives the same bytes.
 *
 * ncg_ed448_decode_batch: Point.fromBytes(enc57[i]) under the strict rules (src/abstract/edwards.ts:405-436, zip215 = false,
 * uvRatio of ed448.ts:135-153) -> x || y, 56 bytes each, canonical.  Refused: y >= p (any bit of byte 56 but bit 7), a y with
 * no x, x = 0 with the sign bit.
 * ncg_ed448_encode_batch: Point.toBytes (edwards.ts:620-628) of affine points: y, then the parity of x in bit 7 of byte 56.
 * ncg_ed448_add_pairs_batch: Point.add (subtract != 0: Point.subtract) of affine points by the complete a = 1 formulas: the
 * identity, the points of order 2 and 4, P = Q and P = -Q need no care by the caller.  The inputs are not validated.
 * ncg_ed448_mul_batch: out57[i] = fromBytes(enc57[i]).multiplyUnsafe(k56[i]).toBytes(), k any value below 2^448 (the exact
 * integer multiple, k = 0 gives the identity).  flags: NCG_ED448_ONE_SCALAR = one k for every row.
 * ncg_ed448_mul_base_batch: out57[i] = BASE.multiplyUnsafe(k56[i]).toBytes().
 * ncg_ed448_to_montgomery_batch: ed448.utils.toMontgomery (ed448.ts:171-179): u = y^2 / x^2 of the strictly decoded key;
 * out_ok = 0 where decoding fails and for x = 0.
 * ncg_ed448_verify_batch: eddsa.verify (edwards.ts:942-989) per row with the challenge given: sig114 = R || s, pk57 = A,
 * k56 = the challenge (any value below 2^448; the caller hashes: k = SHAKE256(dom4(phflag, context) || R || A || PH(M), 114)
 * mod n, ed448.ts:190-201).  A and R are decoded strictly, s >= n is refused, a small-order A (the four points of order 1, 2, 4)
 * is refused even where the equation holds, and the row is accepted iff [4]([s]B - [k]A - R) is the identity - cofactored: an R
 * with a torsion component is accepted when the equation holds.
 *
 * Nothing in the ladder branches or indexes on a scalar bit, but the library makes no constant-time claim; the Edwards
 * multiplications are multiplyUnsafe and the verification works on public data. */
#define NCG_X448_ONE_SCALAR 1
#define NCG_ED448_ONE_SCALAR 1
int ncg_x448_batch(ncg_ctx* ctx, size_t n, const void* scalars56, const void* u56, int flags, void* out56, uint8_t* out_ok);
int ncg_x448_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars56_dev, const void* u56_dev, int flags, void* out56_dev,
                       uint8_t* out_ok_dev, void* stream);
int ncg_x448_base_batch(ncg_ctx* ctx, size_t n, const void* scalars56, void* out56, uint8_t* out_ok);
int ncg_x448_base_batch_dev(ncg_ctx* ctx, size_t n, const void* scalars56_dev, void* out56_dev, uint8_t* out_ok_dev, void* stream);
int ncg_ed448_decode_batch(ncg_ctx* ctx, size_t n, const void* enc57, void* out_affine112, uint8_t* out_ok);
int ncg_ed448_decode_batch_dev(ncg_ctx* ctx, size_t n, const void* enc57_dev, void* out_affine112_dev, uint8_t* out_ok_dev,
                               void* stream);
int ncg_ed448_encode_batch(ncg_ctx* ctx, size_t n, const void* affine112, void* out57);
int ncg_ed448_encode_batch_dev(ncg_ctx* ctx, size_t n, const void* affine112_dev, void* out57_dev, void* stream);
int ncg_ed448_add_pairs_batch(ncg_ctx* ctx, size_t n, const void* a112, const void* b112, int subtract, void* out112);
int ncg_ed448_add_pairs_batch_dev(ncg_ctx* ctx, size_t n, const void* a112_dev, const void* b112_dev, int subtract,
                                  void* out112_dev, void* stream);
int ncg_ed448_mul_batch(ncg_ctx* ctx, size_t n, const void* enc57, const void* k56, int flags, void* out57, uint8_t* out_ok);
int ncg_ed448_mul_batch_dev(ncg_ctx* ctx, size_t n, const void* enc57_dev, const void* k56_dev, int flags, void* out57_dev,
                            uint8_t* out_ok_dev, void* stream);
int ncg_ed448_mul_base_batch(ncg_ctx* ctx, size_t n, const void* k56, void* out57);
int ncg_ed448_mul_base_batch_dev(ncg_ctx* ctx, size_t n, const void* k56_dev, void* out57_dev, void* stream);
int ncg_ed448_to_montgomery_batch(ncg_ctx* ctx, size_t n, const void* pk57, void* out56, uint8_t* out_ok);
int ncg_ed448_to_montgomery_batch_dev(ncg_ctx* ctx, size_t n, const void* pk57_dev, void* out56_dev, uint8_t* out_ok_dev,
                                      void* stream);
int ncg_ed448_verify_batch(ncg_ctx* ctx, size_t n, const void* sig114, const void* pk57, const void* k56, uint8_t* out_ok);
int ncg_ed448_verify_batch_dev(ncg_ctx* ctx, size_t n, const void* sig114_dev, const void* pk57_dev, const void* k56_dev,
                               uint8_t* out_ok_dev, void* stream);

/* ---- SHAKE256, Ed448 signing and Ed448 verification from messages ----------------------------------------------------------
 * eddsa.getPublicKey / getExtendedPublicKey / sign / verify of ed448 and ed448ph (src/ed448.ts:190-246 over
 * src/abstract/edwards.ts:866-989) with every hash on the device (Keccak-f[1600], one message per lane):
 *   h = SHAKE256(seed57, 114); scalar = clamp(h[0..57)) mod n; prefix = h[57..114); A = [scalar]B
 *   r = SHAKE256(dom || prefix || PH(M), 114) mod n; R = [r]B; k = SHAKE256(dom || R || A || PH(M), 114) mod n; S = r + k scalar mod n
 * msgs / msg_off are as for ncg_ed25519_verify_batch_msgs: n + 1 byte offsets into one blob; the offsets must not decrease; msgs
 * may be NULL when every message is empty.  dom is the domain prefix "SigEd448" || phflag || len(ctx) || ctx that the CALLER
 * builds, a HOST pointer in both forms, NULL only with dom_len 0, at most NCG_ED448_DOM_MAX bytes; the library hashes whatever
 * it is given.  Packed rows of 57 (seeds, public keys) and 114 bytes (signatures) may sit at any address; expanded key rows
 * (NCG_ED448_KEY_BYTES) and out_k56 are read and written as words: a DEVICE pointer to them must be 4-byte aligned and is refused
 * otherwise.  Unknown flag bits, dom_len above the maximum and out_len outside 1 .. 65535 return NCG_ERR_INVALID_ARG; n = 0 returns
 * NCG_OK and touches nothing; n >= 2^31 is refused ("too large") before any buffer is read.
 *
 * ncg_shake256_batch: out[i] = SHAKE256(message i, out_len), rows of out_len bytes.
 * ncg_ed448_challenge_batch_dev: out_k56[i] = k of row i, reduced mod n (56 bytes).  flags: NCG_ED448_PREHASH.
 * ncg_ed448_verify_batch_msgs: ncg_ed448_challenge_batch_dev, then ncg_ed448_verify_batch_dev, on one stream.
 * ncg_ed448_public_key_batch: out_pk57[i] = getPublicKey(seed57[i]).
 * ncg_ed448_expand_key_batch: out_key172[i] = scalar (56 bytes LE, below n) || prefix (57) || A (57) || 2 zero bytes, the row that
 * ncg_ed448_sign_batch takes with NCG_ED448_SIGN_EXPANDED.
 * ncg_ed448_sign_batch: out_sig114[i] = R || S of message i under key i (or under the one key row, NCG_ED448_SIGN_ONE_KEY).
 * out_ok[i] = 0 with 114 zero bytes where r = 0 mod n, the one case in which the reference throws (edwards.ts:920-924); the scalar
 * of a key is never 0 mod n.  The secret scalars never select an address or a branch (double, always add, select), but the library
 * makes no constant-time claim.  The workspace and the staged keys of a host form are cleared on the call's stream before the call
 * returns.
 *
 * ncg_ed448_sign_check: the lane code of csrc/keccak.hpp and csrc/ed448_sign.hpp on n rows of RAW uint32 words, in the style of
 * ncg_fe448_check.  Words per row (a, b, out), per op:
 *   0  keccak_f1600                (50,  0, 50)   the 25 lanes as 50 LE words
 *   1  x mod n                     (29,  0, 14)   x below 2^912: word 28 is taken below 2^16
 *   2  (r + k s) mod n             (28, 14, 14)   a = r || k, b = s, all below n
 *   3  sign with the nonce GIVEN   (43, 30, 30)   a = an expanded key row, b = r (14 words, below n) || a 64-byte message;
 *                                                 out = R || S, 2 zero bytes, ok as one word; ed448, empty context
 * `variant` is not read.  b is required (non-NULL) even where its width is 0.  An op nobody defines reads nothing and leaves out
 * zero (rows of 16 words).  n above 2^24 is refused. */
#define NCG_ED448_SIGN_EXPANDED 1   /* keys are NCG_ED448_KEY_BYTES rows, not 57-byte seeds */
#define NCG_ED448_SIGN_ONE_KEY  2   /* one key row serves all n messages */
#define NCG_ED448_PREHASH       4   /* hash each message with SHAKE256(M, 64) first (ed448ph); sign, challenge and verify_msgs */
#define NCG_ED448_DOM_MAX   265     /* "SigEd448" || phflag || len(ctx) || ctx: 10 + 255 */
#define NCG_ED448_KEY_BYTES 172     /* scalar (56 LE, < n) || prefix (57) || A (57) || 2 zero bytes; 4-byte aligned on the device */
int ncg_shake256_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, size_t out_len, void* out);
int ncg_shake256_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, size_t out_len, void* out_dev,
                           void* stream);
int ncg_ed448_challenge_batch_dev(ncg_ctx* ctx, size_t n, const void* sig114_dev, const void* pk57_dev, int flags, const void* dom,
                                  size_t dom_len, const void* msgs_dev, const uint64_t* msg_off_dev, void* out_k56_dev, void* stream);
int ncg_ed448_verify_batch_msgs(ncg_ctx* ctx, size_t n, const void* sig114, const void* pk57, int flags, const void* dom, size_t dom_len,
                                const void* msgs, const uint64_t* msg_off, uint8_t* out_ok);
int ncg_ed448_verify_batch_msgs_dev(ncg_ctx* ctx, size_t n, const void* sig114_dev, const void* pk57_dev, int flags, const void* dom,
                                    size_t dom_len, const void* msgs_dev, const uint64_t* msg_off_dev, uint8_t* out_ok_dev, void* stream);
int ncg_ed448_public_key_batch(ncg_ctx* ctx, size_t n, const void* seed57, void* out_pk57);
int ncg_ed448_public_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed57_dev, void* out_pk57_dev, void* stream);
int ncg_ed448_expand_key_batch(ncg_ctx* ctx, size_t n, const void* seed57, void* out_key172);
int ncg_ed448_expand_key_batch_dev(ncg_ctx* ctx, size_t n, const void* seed57_dev, void* out_key172_dev, void* stream);
int ncg_ed448_sign_batch(ncg_ctx* ctx, size_t n, const void* keys, int flags, const void* dom, size_t dom_len, const void* msgs,
                         const uint64_t* msg_off, void* out_sig114, uint8_t* out_ok);
int ncg_ed448_sign_batch_dev(ncg_ctx* ctx, size_t n, const void* keys_dev, int flags, const void* dom, size_t dom_len,
                             const void* msgs_dev, const uint64_t* msg_off_dev, void* out_sig114_dev, uint8_t* out_ok_dev, void* stream);
int ncg_ed448_sign_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out);

/* ---- decaf448 (RFC 9496 section 5): _DecafPoint and decaf448_hasher of the reference's src/ed448.ts ---------------------
 * The prime-order group over edwards448.  An element is handled through an Edwards representative: an Ed448 affine point x || y,
 * 56 canonical little-endian bytes each, the format ncg_ed448_add_pairs_batch and ncg_ed448_encode_batch take.  Encodings, scalars,
 * representatives and uniform input are all made of 56-byte values read as 14 words: a DEVICE pointer to any of them must be
 * 4-byte aligned and is refused, not dereferenced, otherwise; host pointers may sit at any address.  n = 0 returns NCG_OK and
 * touches nothing; n >= 2^31 is refused; unknown flag bits return NCG_ERR_INVALID_ARG.
 *
 * ncg_decaf448_decode_batch: DecafPoint.fromBytes (ed448.ts:569-595) -> the affine representative of steps 5-7.  out_ok = 0 and a
 * zero row where the reference throws: s >= p or s odd ('invalid decaf448 encoding 1'), the ratio not a square ('encoding 2').
 * ncg_decaf448_encode_batch: toBytes (:610-621) of ANY point of the curve given affine: P and P + (0, -1) give the same 56 bytes
 * (as in the reference, a translate by a point of order 4 does not: the identity and (0, -1) encode to zero, (+-1, 0) to p - 1).
 * The input is not validated.
 * ncg_decaf448_equals_batch: equals (:627-633): out_eq[i] = (x1 y2 == y1 x2).
 * ncg_decaf448_from_uniform_batch: decaf448_hasher.deriveToCurve (:689-700) of 112 uniform bytes, ENCODED: each 56-byte half is
 * reduced mod p (no bit is masked, p .. 2^448 - 1 are accepted), mapped (calcElligatorDecafMap, :474-510), and the two points added.
 * ncg_decaf448_mul_batch: out56[i] = fromBytes(enc56[i]).multiplyUnsafe(k56[i]).toBytes(), k any value below 2^448: the exact
 * integer multiple of the decoded representative, k = 0 gives 56 zero bytes.  Decode, multiply and encode run in one kernel.
 * flags: NCG_DECAF448_ONE_SCALAR = one k for every row.  A refused encoding gives a zero row and out_ok = 0.
 * ncg_decaf448_mul_base_batch: out56[i] = DecafPoint.BASE.multiplyUnsafe(k56[i]).toBytes(); BASE is twice the Ed448 base (:515-520).
 * The multiplications are multiplyUnsafe; the library makes no constant-time claim. */
#define NCG_DECAF448_ONE_SCALAR 1
int ncg_decaf448_decode_batch(ncg_ctx* ctx, size_t n, const void* enc56, void* out_affine112, uint8_t* out_ok);
int ncg_decaf448_decode_batch_dev(ncg_ctx* ctx, size_t n, const void* enc56_dev, void* out_affine112_dev, uint8_t* out_ok_dev,
                                  void* stream);
int ncg_decaf448_encode_batch(ncg_ctx* ctx, size_t n, const void* affine112, void* out56);
int ncg_decaf448_encode_batch_dev(ncg_ctx* ctx, size_t n, const void* affine112_dev, void* out56_dev, void* stream);
int ncg_decaf448_equals_batch(ncg_ctx* ctx, size_t n, const void* a112, const void* b112, uint8_t* out_eq);
int ncg_decaf448_equals_batch_dev(ncg_ctx* ctx, size_t n, const void* a112_dev, const void* b112_dev, uint8_t* out_eq_dev,
                                  void* stream);
int ncg_decaf448_from_uniform_batch(ncg_ctx* ctx, size_t n, const void* uniform112, void* out56);
int ncg_decaf448_from_uniform_batch_dev(ncg_ctx* ctx, size_t n, const void* uniform112_dev, void* out56_dev, void* stream);
int ncg_decaf448_mul_batch(ncg_ctx* ctx, size_t n, const void* enc56, const void* k56, int flags, void* out56, uint8_t* out_ok);
int ncg_decaf448_mul_batch_dev(ncg_ctx* ctx, size_t n, const void* enc56_dev, const void* k56_dev, int flags, void* out56_dev,
                               uint8_t* out_ok_dev, void* stream);
int ncg_decaf448_mul_base_batch(ncg_ctx* ctx, size_t n, const void* k56, void* out56);
int ncg_decaf448_mul_base_batch_dev(ncg_ctx* ctx, size_t n, const void* k56_dev, void* out56_dev, void* stream);

/* ---- RFC 9380 for edwards448 and decaf448: ed448_hasher (src/ed448.ts:313-417) and the hash side of decaf448_hasher (:662-701) ----
 * edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_: m = 1, k = 224, L = 84, expand_message_xof over SHAKE256 (hash-to-curve.ts:252-286), all of
 * it on the device.  Messages are one blob with n + 1 non-decreasing offsets (msgs may be NULL only when every message is empty).
 * dst is a HOST pointer in both forms, 1 <= dst_len <= 255, anything else returns NCG_ERR_INVALID_ARG: the caller compresses an
 * oversize DST (SHAKE256("H2C-OVERSIZE-DST-" || DST, ceil(2 k / 8)): 56 bytes for k = 224, 64 for decaf448's hashToScalar, k = 256).
 * count: NCG_H2C_RO (2, hashToCurve) or NCG_H2C_NU (1, encodeToCurve / mapToCurve); anything else returns NCG_ERR_INVALID_ARG.
 * Rows of words (u56, out_u56, out56, out_affine112) are read and written as 32-bit words: a DEVICE pointer to them must be 4-byte
 * aligned and is refused, not dereferenced, otherwise; host pointers may sit at any address.  n = 0 returns NCG_OK and touches
 * nothing; n >= 2^31 is refused before any buffer is read.  Nothing here is secret.  The hand-offs of a call (the staged DST, the
 * uniform bytes, the reduced elements) live in a workspace of the context: ONE CALL AT A TIME per context, on whatever stream.
 *
 * ncg_xof_shake256_batch: out[i] = expand_message_xof(msg i, dst, out_len) over SHAKE256 =
 *   SHAKE256(msg || I2OSP(out_len, 2) || dst || I2OSP(dst_len, 1), out_len), out_len bytes per row, 1 <= out_len <= 65535.
 * ncg_ed448_h2c_hash_batch: hashToCurve (count 2) / encodeToCurve (count 1) from messages: hash_to_field, the Elligator 2 map to
 *   curve448 and on to edwards448 (ed448.ts:320-394), the sum of the images, the cofactor 4, the canonical affine x || y, 56
 *   little-endian bytes each.  The identity is written as (0, 1); there is no flag byte (as ncg_ed448_add_pairs_batch).
 * ncg_ed448_h2c_map_batch: the same from count field elements per row, 56 little-endian bytes each, any value below 2^448, reduced
 *   mod p.
 * ncg_ed448_h2c_hash_to_field_batch: hash_to_field alone: count reduced elements of 56 little-endian bytes per row.
 * ncg_ed448_h2c_hash_to_scalar_batch: createHasher's hashToScalar (hash-to-curve.ts:520-528): 84 bytes big-endian mod the group
 *   order n, 56 little-endian bytes.
 * ncg_decaf448_hash_to_group_batch: decaf448_hasher.hashToCurve: expand_message_xof(112 bytes, k = 224) then deriveToCurve, the
 *   ENCODED element (the 56 bytes ncg_decaf448_from_uniform_batch gives for the same uniform bytes).
 * ncg_decaf448_hash_to_scalar_batch: decaf448_hasher.hashToScalar: expand_message_xof(64 bytes) little-endian mod n. */
int ncg_xof_shake256_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst, size_t dst_len,
                           size_t out_len, void* out);
int ncg_xof_shake256_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                               size_t dst_len, size_t out_len, void* out_dev, void* stream);
int ncg_ed448_h2c_hash_batch(ncg_ctx* ctx, size_t n, int count, const void* msgs, const uint64_t* msg_off, const void* dst,
                             size_t dst_len, void* out_affine112);
int ncg_ed448_h2c_hash_batch_dev(ncg_ctx* ctx, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                 size_t dst_len, void* out_affine112_dev, void* stream);
int ncg_ed448_h2c_map_batch(ncg_ctx* ctx, size_t n, int count, const void* u56, void* out_affine112);
int ncg_ed448_h2c_map_batch_dev(ncg_ctx* ctx, size_t n, int count, const void* u56_dev, void* out_affine112_dev, void* stream);
int ncg_ed448_h2c_hash_to_field_batch(ncg_ctx* ctx, size_t n, int count, const void* msgs, const uint64_t* msg_off, const void* dst,
                                      size_t dst_len, void* out_u56);
int ncg_ed448_h2c_hash_to_field_batch_dev(ncg_ctx* ctx, size_t n, int count, const void* msgs_dev, const uint64_t* msg_off_dev,
                                          const void* dst, size_t dst_len, void* out_u56_dev, void* stream);
int ncg_ed448_h2c_hash_to_scalar_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst,
                                       size_t dst_len, void* out56);
int ncg_ed448_h2c_hash_to_scalar_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                           size_t dst_len, void* out56_dev, void* stream);
int ncg_decaf448_hash_to_group_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst,
                                     size_t dst_len, void* out56);
int ncg_decaf448_hash_to_group_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                         size_t dst_len, void* out56_dev, void* stream);
int ncg_decaf448_hash_to_scalar_batch(ncg_ctx* ctx, size_t n, const void* msgs, const uint64_t* msg_off, const void* dst,
                                      size_t dst_len, void* out56);
int ncg_decaf448_hash_to_scalar_batch_dev(ncg_ctx* ctx, size_t n, const void* msgs_dev, const uint64_t* msg_off_dev, const void* dst,
                                          size_t dst_len, void* out56_dev, void* stream);
/* The lane code of csrc/h2c448.hpp on n <= 2^24 rows of RAW uint32 words (host pointers), 42 words per row of a and of out; an op
 * reads and writes only its own width, an undefined op reads nothing and leaves out zero.  Every output element is 14 LE words,
 * canonical.  0: the 84-byte value as 21 LE words, mod p.  1: the same value mod n.  2: 16 LE words (the 64-byte form) mod n.
 * 3: map_to_curve_elligator2_curve448 of u (14 words, any value below 2^448): xn, xd, y.  4: map_to_curve_elligator2_edwards448
 * of u before the cofactor: X, Y, Z of the projective point (xEn yEd : yEn xEd : xEd yEd). */
int ncg_h2c448_check(ncg_ctx* ctx, int op, size_t n, const void* a, void* out);

/* ---- measurement helpers (not on the product path) ------------------------------------ */
/* ---- secp256k1 ECDSA batch verification --------------------------------------------------------
 * out_ok[i] = ecdsa.verify(sig[i], msgHash[i], publicKey[i], { prehash: false, format: 'compact', lowS })
 * (src/abstract/weierstrass.ts:1571-1620; the caller above Point.mulAddUnsafe, :1609).  sig: r || s, 32
 * big-endian bytes each (Signature.fromBytes 'compact': both in [1, n), else false); msgHash: 32 bytes, taken as
 * h = bits2int_modN; publicKey: 33-byte SEC1 compressed, or 65-byte uncompressed rows with NCG_ECDSA_PUB_UNCOMPRESSED
 * (Point.fromBytes; a key the reference rejects or the identity gives false).  flags: NCG_ECDSA_LOW_S = the reference's default lowS rule (s <= n/2).  Everything -
 * key decompression, s^-1 mod n (one inversion per 16 signatures), u1 G + u2 P, R.x mod n == r - runs on the
 * device.  NCG_SECP256K1 only. */
#define NCG_ECDSA_LOW_S 1
#define NCG_ECDSA_PUB_UNCOMPRESSED 2 /* public keys are 65-byte uncompressed SEC1 rows (04 || x || y): prefix, range and
                                        curve-equation checks on the device (weierstrass.ts:589-597), no square root */
int ncg_ecdsa_verify_batch(ncg_ctx* ctx, int curve, size_t n, const void* sig64, const void* hash32,
                           const void* pub33, int flags, uint8_t* out_ok);
int ncg_ecdsa_verify_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* sig64_dev,
                               const void* hash32_dev, const void* pub33_dev, int flags,
                               uint8_t* out_ok_dev, void* stream);

/* Public-key recovery for a batch: out[i] = Signature.fromBytes(sig65[i], 'recovered').recoverPublicKey(msgHash[i])
 * (src/abstract/weierstrass.ts:1391-1407) as an affine wire point.  sig65: recovery id (0..3) || r || s, 32 big-endian
 * bytes each; out_ok[i] = 0 where the reference throws (recid > 3, r or s outside [1, n), r + n >= p for recid 2 / 3,
 * no point with that x, Q = O) and the point is then zeroed.  NCG_SECP256K1 only. */
int ncg_ecdsa_recover_batch(ncg_ctx* ctx, int curve, size_t n, const void* sig65, const void* hash32,
                            void* out_affine, uint8_t* out_ok);
int ncg_ecdsa_recover_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* sig65_dev,
                                const void* hash32_dev, void* out_affine_dev, uint8_t* out_ok_dev, void* stream);

/* ---- secp256k1 BIP-340 Schnorr batch verification ----------------------------------------------
 * out_ok[i] = schnorr.verify(sig[i], msg[i], publicKey[i]) (src/secp256k1.ts:228-258) given the challenge
 * e[i] = int(taggedHash('BIP0340/challenge', r || pk || msg)) mod n as 32 big-endian bytes (:176-178; the host
 * shim hashes, like the reference's host sha256).  sig: r || s big-endian (r in [1, p), s in [1, n), else false);
 * publicKey: 32-byte x-only, P = lift_x (:158-170: the even root; no root / x >= p gives false).  On the device:
 * the range checks, lift_x, R = s G + (n - e) P, and R != O, even y(R), x(R) == r. */
int ncg_schnorr_verify_batch(ncg_ctx* ctx, size_t n, const void* sig64, const void* e32, const void* pkx32,
                             uint8_t* out_ok);
int ncg_schnorr_verify_batch_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* e32_dev,
                                 const void* pkx32_dev, uint8_t* out_ok_dev, void* stream);

/* ---- the two verifications from MESSAGES (hash on the device, csrc/sha256.hpp) -------------------------------
 * ncg_ecdsa_verify_batch_msgs: ecdsa.verify(sig, msg, publicKey, { prehash: true, ... }) - SHA-256(msg) is the message
 * representative (weierstrass.ts:1465-1470); ncg_schnorr_verify_batch_msgs: schnorr.verify(sig, msg, pk) with the tagged
 * challenge hash (src/secp256k1.ts:129-137, :176-178).  msgs = all messages back to back, msg_off = n + 1 byte
 * offsets (message i = msgs[msg_off[i] .. msg_off[i+1])); everything else as in the entry points above. */
int ncg_ecdsa_verify_batch_msgs(ncg_ctx* ctx, int curve, size_t n, const void* sig64, const void* msgs,
                                const uint64_t* msg_off, const void* pub, int flags, uint8_t* out_ok);
int ncg_ecdsa_verify_batch_msgs_dev(ncg_ctx* ctx, int curve, size_t n, const void* sig64_dev, const void* msgs_dev,
                                    const uint64_t* msg_off_dev, const void* pub_dev, int flags,
                                    uint8_t* out_ok_dev, void* stream);
int ncg_schnorr_verify_batch_msgs(ncg_ctx* ctx, size_t n, const void* sig64, const void* msgs,
                                  const uint64_t* msg_off, const void* pkx32, uint8_t* out_ok);
int ncg_schnorr_verify_batch_msgs_dev(ncg_ctx* ctx, size_t n, const void* sig64_dev, const void* msgs_dev,
                                      const uint64_t* msg_off_dev, const void* pkx32_dev, uint8_t* out_ok_dev,
                                      void* stream);

/* ---- secp256k1 signing: secp256k1.getPublicKey / sign and schnorr.getPublicKey / sign ----------------------------------------
 * (src/abstract/weierstrass.ts:1480-1568 with the HMAC-DRBG of src/utils.ts:755-813; src/secp256k1.ts:147-221).
 * sk32, hash32, extra32 and aux32 are rows of 32 big-endian bytes, read byte by byte (no alignment rule); signatures are rows of
 * 64 bytes.  Every row gets out_ok[i] = 1 and its result, or out_ok[i] = 0 and a row of zero bytes where the reference throws: a
 * key outside [1, n), the DRBG's cap of 1000 candidates (ECDSA), k' = 0 (BIP-340).  A refused row does not disturb its neighbours.
 *
 * ncg_secp256k1_public_key_batch: out[i] = the public key of sk32[i] as flags says - NCG_SECP_PK_COMPRESSED (0, the default,
 *   33 bytes), NCG_SECP_PK_UNCOMPRESSED (65 bytes 04 || x || y) or NCG_SECP_PK_XONLY (32 bytes, schnorr.getPublicKey).
 * ncg_ecdsa_sign_batch: out_sig64[i] = r || s of sign(hash32[i], sk32[i], { prehash: false, lowS, extraEntropy }) with RFC 6979
 *   nonces; out_recid[i] (the array may be NULL) = (y(R) odd) | (x(R) >= n) << 1, bit 0 flipped where lowS replaced s by n - s.
 *   hash32: 32 bytes taken as h1 = bits2int_modN.  extra32: NULL, or 32 bytes PER ROW that join the DRBG's seed (RFC 6979 3.6) -
 *   n rows also with NCG_SECP_SIGN_ONE_KEY, any other length of extra entropy is not offered.  The reference's blinding of the
 *   inversion changes no output bit and is not reproduced.
 * ncg_ecdsa_sign_batch_msgs: the same with hash32[i] = SHA-256(message i) computed on the device ({ prehash: true }); msgs /
 *   msg_off as for ncg_ecdsa_verify_batch_msgs.
 *   flags of both: NCG_ECDSA_LOW_S, NCG_SECP_SIGN_ONE_KEY (sk32 is ONE row used for all n rows); curve: NCG_SECP256K1 only.
 * ncg_schnorr_sign_batch: out_sig64[i] = schnorr.sign(message i, sk32[i], aux32[i]) without its self-verification (run
 *   ncg_schnorr_verify_batch_msgs over the output for that).  aux32: n rows, required.  flags: NCG_SECP_SIGN_ONE_KEY.
 * The secret scalars never select an address or a branch of a multiplication (a table walk that reads every entry, DESIGN.md
 * section 8); this is not a constant-time claim.  Device and staging memory that held keys, nonces or DRBG state is cleared on
 * the call's stream before the call returns.  Unknown flag bits, a NULL required buffer: NCG_ERR_INVALID_ARG; n = 0 returns NCG_OK. */
#define NCG_SECP_PK_COMPRESSED   0
#define NCG_SECP_PK_UNCOMPRESSED 1
#define NCG_SECP_PK_XONLY        2
#define NCG_SECP_SIGN_ONE_KEY    4   /* beside NCG_ECDSA_LOW_S (1); bit 1 is the verify forms' NCG_ECDSA_PUB_UNCOMPRESSED */
int ncg_secp256k1_public_key_batch(ncg_ctx* ctx, size_t n, const void* sk32, int flags, void* out, uint8_t* out_ok);
int ncg_secp256k1_public_key_batch_dev(ncg_ctx* ctx, size_t n, const void* sk32_dev, int flags, void* out_dev, uint8_t* out_ok_dev,
                                       void* stream);
int ncg_ecdsa_sign_batch(ncg_ctx* ctx, int curve, size_t n, const void* sk32, const void* hash32, const void* extra32, int flags,
                         void* out_sig64, uint8_t* out_recid, uint8_t* out_ok);
int ncg_ecdsa_sign_batch_dev(ncg_ctx* ctx, int curve, size_t n, const void* sk32_dev, const void* hash32_dev, const void* extra32_dev,
                             int flags, void* out_sig64_dev, uint8_t* out_recid_dev, uint8_t* out_ok_dev, void* stream);
int ncg_ecdsa_sign_batch_msgs(ncg_ctx* ctx, int curve, size_t n, const void* sk32, const void* msgs, const uint64_t* msg_off,
                              const void* extra32, int flags, void* out_sig64, uint8_t* out_recid, uint8_t* out_ok);
int ncg_ecdsa_sign_batch_msgs_dev(ncg_ctx* ctx, int curve, size_t n, const void* sk32_dev, const void* msgs_dev,
                                  const uint64_t* msg_off_dev, const void* extra32_dev, int flags, void* out_sig64_dev,
                                  uint8_t* out_recid_dev, uint8_t* out_ok_dev, void* stream);
int ncg_schnorr_sign_batch(ncg_ctx* ctx, size_t n, const void* sk32, const void* aux32, const void* msgs, const uint64_t* msg_off,
                           int flags, void* out_sig64, uint8_t* out_ok);
int ncg_schnorr_sign_batch_dev(ncg_ctx* ctx, size_t n, const void* sk32_dev, const void* aux32_dev, const void* msgs_dev,
                               const uint64_t* msg_off_dev, int flags, void* out_sig64_dev, uint8_t* out_ok_dev, void* stream);
/* The pieces of csrc/secp256k1_sign.hpp on raw 32-bit words, one row per lane (host pointers; n <= 2^24): the branches of the
 * signing code that real inputs reach with probability about 2^-128 can only be tested by feeding them directly.  An op nobody
 * defines reads nothing and leaves rows of 16 zero words.  Words per row (a, b, out):
 *   0  candidate j = variant >> 1 (j <= 3) of the HMAC-SHA256 DRBG from the 96 seed bytes a, as they lie in memory (the last 32
 *      only when variant & 1: extra entropy): the candidate's 32 bytes                                            24, 1, 8
 *   1  the uniform-scan multiply: x || y of a G, canonical, 8 + 8 little-endian words                              8, 1, 16
 *   2  the ECDSA finish: a = k || x(R) || m || d (8 LE words each), b = (y(R) odd) | lowS << 1:
 *      r || s || recid || accepted                                                                                32, 1, 18
 *   3  the BIP-340 scalar half: a = k' || e || d, b = y(R) odd: s = (k + e d) mod n                               24, 1, 8
 *   4  one whole ECDSA row with the DRBG's candidates below variant >> 1 (<= 3) refused (variant & 1: extra entropy):
 *      a = sk || hash || extra as bytes, b = lowS: sig64 as bytes || recid || ok                                  24, 1, 18 */
int ncg_secp256k1_sign_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out);

/* Runs instruction-rate / field-multiply micro-benchmark `kind` (see csrc/ubench.hip) and
 * returns the kernel time in milliseconds. */
int ncg_ubench(ncg_ctx* ctx, int kind, int blocks, int threads, int iters, float* out_ms);
/* Field-level self-check: out[i] = op(a[i], b[i]) computed by the device field code, one lane per element
 * (host buffers; csrc/selfcheck.hpp lists the fields and the words per row of a, b and out, csrc/selfcheck.hip holds the
 * kernels).  field 0 / 1 = secp256k1 / ed25519 base field in the radix-2^29 lazy form (fe9.hpp): a, b
 * are 9 RAW 32-bit limbs per element, `variant` = 10 A + B names the operand bound types; out = 8 canonical
 * LE words (variants 11 12 17 71 23 32 22 15 33 77 46; any other leaves out zero).  op: 0 mul, 1 sqr (of the normalised
 * operand when A > 2), 2 add, 3 sub, 4 neg, 5 inv, 6 normalise, 10 double; 7 out[0] = is-zero-mod-p, 8 out[0] = the largest
 * limb of the normalised a, 9 out[0] = the largest output limb of the product.  An op the bounds do not admit leaves out
 * zero.  field 2 = bls12-381 Fp: 12-word canonical operands and results, ops 0-5 of the same list.
 * field 3 = bls12-381 Fp on RAW radix-2^29 limbs (fe29.hpp, Montgomery R = 2^406): a = [a, c], b = [b, d], 14 limbs
 * each, values up to the top of the lazy bounds (a, c < 4096 p; b, d < 4096 p for op 0, 2048 p for op 6);
 * field 4 = the lane-paired Fp2 form: every element c0 then c1 (28 limbs), a, c < 4096 p (2048 p for op 1), b, d <
 * 2048 p (op 0) / 1024 p (op 6).  ops 0 a*b, 1 a^2, 6 a*b - c*d (the fused reduction); out = canonical wire words
 * of the result taken out of Montgomery form (12, or 12 + 12 for Fp2).
 * field 5 / 6 = the fused Fe9 expressions (fe9.hpp) over secp256k1 / ed25519 p: a = [a, c], b = [b, d], 9 RAW limbs
 * each (18 words); ops 0 a*b + c*d, 1 a*b + c^2, 2 a*b + c, 3 a^2 + c, 4 a/2; `variant` = decimal A B C D bound digits
 * (1111 1322 3211 2311 1123 3121 1327 7171 1771 2171; a combination the op does not admit leaves out zero); out = 9 RAW
 * limbs of the result.
 * field 7 = the secp256k1 ladder pieces, RAW limbs in and out: a = 27 words, b = 18 words, out = 27 words.  op 0
 * jac_dbl_neg(P), op 1 jac_madd_neg(P, qx, qy) (ec_sw.hpp) with P = a (X, Y, Z at bound 2), qx = b[0..9) at bound 2,
 * qy = b[9..18) at bound 3: out = X, Y, Z; op 2 secp_glv_split + secp_glv_make_odd (scalar.hpp) of the scalar in
 * a[0..8): out[0..12) = k1[5] k2[5] k1neg k2neg; op 3 secp_glv_split + secp_glv_make_k1_odd (the split of the fused ladder),
 * the same layout.  Any other op leaves out zero.
 * field 8 = fr29.hpp, the bls12-381 Fr form of the NTT butterflies, RAW limbs in and out: a, b, out = 9 words each.
 * ops 0 mont(a, b), 1 a + b, 2 a + 3 r - b, 3 weak(a), 4 reduce256(a), 5 cond_sub(a), 6 from_words(a[0..8)),
 * 7 to_words(a) (8 words, then 0), 8 one fold (fr29_fold255).  `variant` 0 = bls12-381 Fr, 1 = bn254 Fr (the same
 * ops with that field's constants; its fold is at 2^254); any other variant leaves out zero.
 * field 9 = the bn254 base field (fe9m.hpp: radix 2^29, Montgomery R = 2^261), RAW limbs in and out: a, b, out = 9 words
 * each, `variant` = 10 A + B names the operand bound types (11 12 22 23 32 17 71 33 77; a bound-B element has limbs below
 * B 2^29 and a value below 2 B p).  ops 0 a*b, 1 a^2, 2 a + b, 3 a - b, 4 -a, 5 1/a, 6 weak normalisation, 7 to wire
 * (8 canonical LE words of a / R, then 0), 8 from wire (a[0..8) canonical LE words -> a R).  An op the bounds do not admit
 * leaves out zero.
 * fields 3 / 4, op 7 = the zero test f_eqz (fe29.hpp) of the element a of the row (the row widths stay; c and b are ignored) taken
 * as Fe29<A> / the lane-paired Fe29x2P<A>, `variant` = A, one of the bounds the group law instantiates it at: 4 (xyzz_add: the
 * difference of two products), 66 (xyzz_madd: a product minus a stored coordinate), 128 (CoopXyzz::add: two values read back
 * as stored coordinates).  out[0] = 1 when the value is j p with j < A (both halves, on field 4), else 0; any other A leaves
 * out zero.
 * fields 10-14 = the group law the MSM runs on its buckets, on STORED words (csrc/group_check.hpp): 10 MsmGroup<CurveSecp>
 * (Fe9, FW = 9 words per coordinate), 11 MsmGroup<CurveEd> (extended accumulators / affine Niels inputs, FW = 9), 12
 * MsmGroup<CurveG1> (Fe29, FW = 14), 13 MsmGroup<CurveG2P> (lane-paired Fp2, FW = 28: c0 then c1, two lanes per row), 14
 * MsmGroup<CurveBn254> (Fe9 Montgomery, FW = 9).  Every row of a, b and out is ACC_WORDS = 4 FW raw words in the layout of
 * acc_load / acc_store - X Y ZZ ZZZ (ed25519: X Y Z T), Montgomery form included, nothing converted; an all-zero row is the
 * identity.  For ops 0 / 1 the row of b starts with a stored input point in aff_load's layout (x y: 2 FW words; ed25519:
 * y + x, y - x, 2 d x y: 3 FW words) and the rest of it is ignored.  ops 0 madd(a, b, false), 1 madd(a, b, true) (a - b),
 * 2 add(a, b), 3 dbl(a).  Fields 12 / 13 also take the four-lane form of msm_coop.hpp (device only; one group of four items per
 * row, blocks of 64 lanes): 8 CoopXyzz::add(a, b) -> out, 9 the same with out aliasing a (the row is copied to out, then added
 * in place), 10 with out aliasing b, 11 CoopXyzz::dbl(a) -> out, 12 dbl in place, 13 CoopXyzz::copy; on the other fields ops
 * 8-13 leave out zero, as does any other op.  `variant` is ignored.
 * field 16 = the X25519 ladder pieces (csrc/x25519.hpp), RAW words in and out: a = 36 words, b = 9 words, out = 36 words
 * (field 15 is unassigned and refused).  op 0 one x25519_step with the swap bit `variant` & 1: a = x2 z2 x3 z3, b = x1, 9 raw
 * limbs each at the bound the ladder stores them at (1: limbs below 2^29 + 2^19); out = x2 z2 x3 z3, 9 limbs each, again
 * below that bound.  op 1 decodeU and the low-order test: a[0..8) = the LE words of an encoded u; out[0..8) = the canonical
 * residue, out[8] = 0 for the five low-order values, else 1.  op 2 adjustScalarBytes: a[0..8) -> out[0..8).  Any other op
 * leaves out zero.
 * field 17 = the ristretto255 pieces (csrc/ristretto.hpp), RAW words in and out: a = 36 words, b = 9 words, out = 36 words,
 * every input a field element of 9 raw limbs below 2^29 + 2^19.  op 0 SQRT_RATIO_M1(u, v) (uvRatio, src/ed25519.ts:107-125):
 * a[0..9) = u, b = v; out[0..9) = the raw limbs of the value (the non-negative root of u / v, or of sqrt(-1) u / v where u / v
 * is no square), out[9] = 1 if u / v is a square.  op 1 the encoder: a = X Y Z T of an extended point; out[0..8) = the LE
 * words of its encoding.  op 2 the Elligator map: a[0..9) = r0; out = X Y Z T of the extended representative, 9 raw limbs
 * each.  Any other op leaves out zero.  `variant` is ignored.
 * bn254 G1 (NCG_BN254_G1) takes the MSM (every entry point, resident / precomputed / async / split / sharded), the batch
 * variable-base multiply, the pairwise add and normalize_batch; the reference has no byte format for it, so decode /
 * encode / points_from_encoded / aggregate_encoded return NCG_ERR_UNSUPPORTED, as do mul_base_batch, map_to_curve_batch
 * and points_verify_subgroup. */
int ncg_field_check(ncg_ctx* ctx, int field, int op, int variant, size_t n, const void* a, const void* b, void* out);

/* The lane code of csrc/fe448.hpp and csrc/ed448.hpp (GF(2^448 - 2^224 - 1), X448, Ed448) on n rows of RAW uint32 words.  It is
 * an entry point of its own because the table of ncg_field_check is closed.  A field element is 16 limbs in radix 2^28; "at
 * bound B" means every limb below B * (2^28 + 2^10).  Words per row (a, b, out) and the input bounds, per op:
 *   0  a * b                       (16, 16, 16)   a at 3, b at 2; out at 1
 *   1  a^2                         (16,  0, 16)   a at 2; out at 1
 *   2  a + b, a - b, -a            (16, 16, 48)   both at 1; out at 2, 3, 1
 *   3  a + 39081 b                 (16, 16, 16)   a at 3, b at 2; out at 1
 *   4  the canonical store         (16,  0, 14)   a at 8; out = the 14 LE words of the residue
 *   5  the 56-byte load            (14,  0, 16)   a = 14 LE words of any value below 2^448; out at 1, the same integer
 *   6  a^((p - 3) / 4)             (16,  0, 16)   a at 1; out at 1
 *   7  1 / a                       (16,  0, 16)   a at 1; out at 1 (0 -> 0)
 *   8  one X448 ladder step        (64, 16, 64)   a = x2 z2 x3 z3, b = x1, all at 1, swap bit = variant & 1; out at 1
 *   9  one Edwards addition        (48, 48, 48)   a, b = X Y Z projective, all at 1; out at 1
 *  10  one Edwards doubling        (48,  0, 48)   a = X Y Z; out at 1
 * b is required (non-NULL) even where its width is 0.  An op nobody defines reads nothing and leaves out zero (rows of 16
 * words).  n above 2^24 is refused. */
int ncg_fe448_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out);

/* The lane code of csrc/decaf448.hpp on n rows of RAW uint32 words, in the style of ncg_fe448_check (whose op table is closed as
 * well).  Field elements are 16 limbs in radix 2^28; every input element is at bound 1 (every limb below 2^28 + 2^10, the value
 * any representative), every output element at bound 1.  Words per row (a, b, out), per op:
 *   0  SQRT_RATIO_M1(u, v)         (16, 16, 17)   a = u, b = v; out[0..16) = the value, non-negative; out[16] = 1 iff v value^2 = u
 *   1  encode_ext                  (64,  0, 14)   a = X Y Z T; out = the 14 LE words of the encoding
 *   2  the Elligator map           (16,  0, 64)   a = r0; out = X Y Z T of the extended representative
 * `variant` is not read.  b is required (non-NULL) even where its width is 0.  An op nobody defines reads nothing and leaves out
 * zero (rows of 16 words).  n above 2^24 is refused. */
int ncg_decaf448_check(ncg_ctx* ctx, int op, int variant, size_t n, const void* a, const void* b, void* out);

/* ---- bls12-381 pairings: batch pairing products and GT arithmetic ------------------------------------------
 * A GT (Fp12) element crosses as 576 bytes: the 12 Fp coefficients in tower order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..,
 * c1.c2.c1 - the order of Fp12.toBytes - each 48 bytes little-endian and canonical like every field element here.
 *
 * ncg_pairing_batch: bls.pairingBatch (src/abstract/bls.ts:670-693) for n_groups groups at once.  g1_affine / g2_affine
 * are n_pairs affine wire points (96 / 192 bytes); group_offsets is a HOST array (in both forms) of n_groups + 1
 * ascending pair offsets, the first 0 and the last n_pairs; out_gt[g] = finalExponentiate(product of the Miller values
 * of the pairs of group g) and out_is_one[g] = 1 where that is Fp12.ONE.  Groups of one give bls.pairing per row, one
 * group gives one pairing check, an empty group gives ONE.  out_gt may be NULL when only the booleans are wanted.
 * Like the reference the call refuses a ZERO operand ("pairing is not available for ZERO point", bls.ts:685) and an
 * operand that fails assertValidity - a coordinate not below p or a point off its curve ("bad point: equation left !=
 * right") - with NCG_ERR_INVALID_ARG: *out_bad_index (optional) is the first such pair, ncg_last_error carries the
 * message, the outputs are untouched.  Membership of the prime-order subgroups - the last part of assertValidity, "bad
 * point: not in prime-order subgroup" - is checked only under NCG_PAIRING_CHECK_SUBGROUP (the endomorphism tests of the
 * decoders, about two more ladders per pair): points from ncg_decode_points_batch, ncg_map_to_curve_batch and the
 * multiplies of subgroup points are members already.
 * There is no un-exponentiated output: a Miller value is only defined up to factors the final exponentiation removes.
 * Both forms return after the result is complete (the refusal needs the device's verdict); n_groups = 0 returns NCG_OK. */
#define NCG_PAIRING_CHECK_SUBGROUP 1
int ncg_pairing_batch(ncg_ctx* ctx, size_t n_pairs, const void* g1_affine, const void* g2_affine, size_t n_groups,
                      const uint32_t* group_offsets, int flags, void* out_gt, uint8_t* out_is_one, int64_t* out_bad_index);
int ncg_pairing_batch_dev(ncg_ctx* ctx, size_t n_pairs, const void* g1_affine_dev, const void* g2_affine_dev, size_t n_groups,
                          const uint32_t* group_offsets, int flags, void* out_gt_dev, uint8_t* out_is_one_dev,
                          int64_t* out_bad_index, void* stream);

/* ncg_fp12_batch: bls12_381.fields.Fp12 for a batch, out[i] = op(a[i], b[i]) on GT wire elements (any Fp12 element,
 * not only members of GT).  b is read by NCG_FP12_MUL (an Fp12) and NCG_FP12_MUL014 (o0 || o1 || o4, three Fp2 = 288
 * bytes: the sparse product by o0 + o1 v + o4 v w of the line function, bls.ts:476-519) and may be NULL otherwise;
 * out is n Fp12 elements, for NCG_FP12_IS_ONE n bytes (Fp12.eql(a, ONE)); out may be a (and b): a row is read before it is written.  NCG_FP12_CYCLOTOMIC_SQR is
 * Fp12._cyclotomicSquare (the square only for members of the cyclotomic subgroup), NCG_FP12_INV of 0 gives 0. */
enum ncg_fp12_op {
  NCG_FP12_MUL = 0,
  NCG_FP12_SQR = 1,
  NCG_FP12_INV = 2,
  NCG_FP12_CONJUGATE = 3,
  NCG_FP12_FROBENIUS1 = 4,
  NCG_FP12_FROBENIUS2 = 5,
  NCG_FP12_FROBENIUS3 = 6,
  NCG_FP12_CYCLOTOMIC_SQR = 7,
  NCG_FP12_MUL014 = 8,
  NCG_FP12_FINAL_EXP = 9,
  NCG_FP12_IS_ONE = 10
};
int ncg_fp12_batch(ncg_ctx* ctx, int op, size_t n, const void* a, const void* b, void* out);
int ncg_fp12_batch_dev(ncg_ctx* ctx, int op, size_t n, const void* a_dev, const void* b_dev, void* out_dev, void* stream);


/* ncg_bls_verify_batch: verify of bls.longSignatures (scheme 0: pk 48 bytes in G1, sig 96 bytes in G2) or bls.shortSignatures
 * (scheme 1: pk 96 bytes, sig 48 bytes) for n independent rows (src/abstract/bls.ts:795-818).  pk_enc / sig_enc are the compressed
 * encodings, u the hash_to_field output of each message with count 2 as ncg_map_to_curve_batch takes it (scheme 0: 192 bytes,
 * scheme 1: 96 bytes per row).  On the device, in order: both sets are decoded with the subgroup checks, the messages mapped,
 * e(-pk, H(m)) e(G1, sig) - scheme 1: e(H(m), -pk) e(sig, G2) - formed and taken through the pairing path as groups of two,
 * out_ok[i] = is_one.  out_ok[i] = 0 wherever the reference's verify returns false or its fromBytes throws: an undecodable, ZERO
 * or out-of-subgroup key or signature included.  The call itself fails only on bad arguments.  Workspace: about 1.1 KB per row
 * beside the pairing's 2 x 672 B.  Both forms return after the result is complete. */
int ncg_bls_verify_batch(ncg_ctx* ctx, int scheme, size_t n, const void* pk_enc, const void* sig_enc, const void* u, uint8_t* out_ok);
int ncg_bls_verify_batch_dev(ncg_ctx* ctx, int scheme, size_t n, const void* pk_enc_dev, const void* sig_enc_dev, const void* u_dev,
                             uint8_t* out_ok_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NCG_H */
