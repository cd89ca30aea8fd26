/* C ABI of the MI355X MSM engine (libmsm_hip.so).
 *
 * This is the drop-in boundary for the reference's MSM path: the coarse `Curve.Parallel.*` surface
 * that callers use (reference src/parallel.ts:135-145, 251-259) expressed over plain pointers and
 * sizes, plus a few fine-grained operators of the wasm export table (src/field-msm.ts:86-123,
 * src/scalar-glv.ts:41-51) exposed as GPU test kernels.  INTEGRATION.md shows the N-API / ctypes
 * stubs that bind it.
 *
 * Wire formats are the reference's (`pointsFromBytes` / `scalarsFromBytes`, src/parallel.ts:97-133):
 *   BLS12-377 G1 point : 96 bytes  = x || y, each 48-byte little-endian canonical integer (non-Montgomery)
 *   Ed-on-BLS12-377    : 64 bytes  = x || y, each 32-byte little-endian
 *   scalar             : 32 bytes little-endian
 * The all-zero point encoding denotes the identity (the reference's byte format cannot express it;
 * its object form has `isZero`, scripts/zprize23/submission-bls377.ts:83).
 *
 * Ownership: the caller owns every buffer it passes; the library owns all device memory.  Calls on
 * one context are serialised by the caller; distinct contexts are independent.  Every function
 * returns MSM_OK or an error code; msm_last_error() gives the message of the last failure.
 */
#ifndef MSM_HIP_H
#define MSM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MSM_OK = 0,
  MSM_ERR_ARG = 1,         /* null pointer, bad length, bad window size, unknown curve */
  MSM_ERR_HIP = 2,         /* HIP runtime failure (message has the HIP error string) */
  MSM_ERR_POINT = 3,       /* coordinate >= p, point not on the curve or outside the subgroup (when validation is requested),
                              undecodable compressed point */
  MSM_ERR_NO_POINTS = 4,   /* msm called before msm_set_points, or with n > resident points */
  MSM_ERR_NO_DEVICE = 5,   /* no usable GPU: there is no CPU fallback */
  MSM_ERR_SCALAR = 6,      /* a scalar >= the group order q and msm_opts.strict was set (default: reduced mod q); a scalar outside
                              the range a narrow call declared (msm_run_narrow) */
  MSM_ERR_INTERNAL = 7     /* host allocation failure or another unexpected condition; no C++ exception crosses this ABI */
};

enum {
  MSM_CURVE_BLS12_377_G1 = 0,     /* Weierstrass + GLV, batched-affine path: src/msm-batched-affine.ts */
  MSM_CURVE_ED_ON_BLS12_377 = 1,  /* twisted Edwards, generic path: src/msm-basic.ts */
  MSM_CURVE_BLS12_381_G1 = 2,     /* Weierstrass + GLV, batched-affine path; src/concrete/bls12-381.params.ts */
  MSM_CURVE_PALLAS = 3,           /* same path on 9 limbs / 8 packed words, src/concrete/pasta.params.ts (the reference sizes
                                   * limbs per field, src/parallel.ts:53-57): coordinates at this ABI -- wire points, test
                                   * operands, the used part of msm_result.x / .y -- are 32-byte little-endian integers, as for
                                   * the Edwards curve; window sums stay 144-byte (X, Y, Z) records for every curve */
  /* The two curve cycles of recursive provers, not in the reference: the Pallas path (9 limbs / 8 words, 32-byte coordinates,
   * GLV, cofactor 1) with their own constants.  New enum values only: MSM_ABI_VERSION and the struct sizes are unchanged, a
   * binding detects them by msm_ctx_create not answering MSM_ERR_ARG. */
  MSM_CURVE_BN254_G1 = 4,         /* alt_bn128 (EIP-196): y^2 = x^3 + 3, generator (1, 2) */
  MSM_CURVE_GRUMPKIN = 5,         /* BN254's cycle partner: y^2 = x^3 - 17 over BN254's scalar field, of order BN254's p */
  MSM_CURVE_VESTA = 6             /* Pallas' cycle partner: y^2 = x^3 + 5 over Pallas' scalar field, generator (-1, 2) */
};

/* Layout version of this header.  The symbol names do not change when a struct grows or an argument changes meaning, so a
 * binding built against another version of the header would misread memory silently: msm_abi_version() returns the version the
 * LIBRARY was built with, msm_abi_struct_bytes(0 / 1) its sizeof(msm_opts) / sizeof(msm_result).  The Python loader and the N-API
 * addon compare both at load time and refuse a mismatch.  History: 3 = round 3 (msm_generate_scalars writes to a caller-owned
 * buffer; msm_opts.point_lo / by_window); 4 = msm_result.n_pairs_algo; 5 = window tables (msm_opts.no_tables, msm_result.tables,
 * msm_precompute / msm_tables_info / msm_set_tables_limit), msm_reserve, msm_opts.bucket_shard / bucket_shards; 6 = window tables
 * over a range of the points (msm_opts.merged_sums, msm_precompute with point_lo, msm_tables_range); 7 = msm_run_batch;
 * 8 = compressed points and subgroup validation (msm_set_points_ex, msm_validate_points, msm_get_points_ex).
 * Narrow scalars (msm_run_narrow, msm_run_batch_narrow, msm_plan_narrow, msm_scalar_bits) came WITHOUT a new version: they are
 * new symbols only, msm_opts / msm_result keep their size and fields, so a binding of version 8 reads the same memory as
 * before.  A binding detects the feature by the presence of the symbol msm_run_narrow.
 * The indexed (sparse) MSM (msm_run_indexed, msm_run_indexed_narrow) came the same way: two new symbols, version 8 and both struct
 * sizes unchanged.  A binding detects the feature by the presence of the symbol msm_run_indexed.
 * Point-set linear combinations (msm_points_lincomb, msm_pointset_size) came the same way: two new symbols, version 8 and both
 * struct sizes unchanged.  A binding detects the feature by the presence of the symbol msm_points_lincomb.
 * The resident scalar-vector operations (msm_scalars_lincomb, msm_scalars_mul, msm_scalars_inner, msm_scalars_powers) and
 * msm_device_download came the same way: five new symbols, version 8 and both struct sizes unchanged.  A binding detects the
 * feature by the presence of the symbol msm_scalars_lincomb.
 * Per-row scalar multiplication of point sets (msm_points_mul, msm_points_mul_base) came the same way: two new symbols, version 8
 * and both struct sizes unchanged.  A binding detects the feature by the presence of the symbol msm_points_mul.
 * The transform over point sets (msm_points_ntt) came the same way: one new symbol, version 8 and both struct sizes unchanged.  A
 * binding detects the feature by the presence of the symbol msm_points_ntt. */
#define MSM_ABI_VERSION 8
uint32_t msm_abi_version(void);
uint32_t msm_abi_struct_bytes(int which);

typedef struct msm_ctx msm_ctx;

/* Options of one msm call; mirrors `{c, useSafeAdditions}` of src/msm-batched-affine.ts:74-77.
 * Zero-initialise for defaults. */
typedef struct msm_opts {
  int32_t c;            /* window size in bits, 0 = pick from N (windowSize, src/msm-common.ts:8-41, retuned).  The number of
                           windows is the reference's K = ceil((b + 1) / c) (src/msm-batched-affine.ts:90) with one exception:
                           for c >= 18, a top window that would hold the carry bit of the signed recoding alone
                           (b + 1 = (K - 1) c + 1; BLS12-377: c = 18, 21) is folded into the window below -- K - 1 windows,
                           window k still weighs 2^(c k).  msm_plan / msm_result.K report the K in use; every rank of a
                           sharded run gets the same one from the same c */
  int32_t unsafe;       /* accepted for API parity with msmUnsafe (src/curve-affine.ts:463-522) and ignored: there is one tree
                           kernel and it always handles the edge cases -- the equal-x detection the unsafe variant would drop is
                           19 of its 3 171 instructions per pair addition (0.6 %), and the identity operands it also ignores are
                           structural here (bucket padding) */
  int32_t k_lo, k_hi;   /* window shard [k_lo, k_hi) for msm_window_sums; 0,0 = all windows */
  int32_t serial;       /* != 0: run the window groups one after the other on one stream (no overlap): phase_ms then
                           hold exclusive kernel times -- used for roofline measurements.  Every tree launch then has the
                           chip to itself and takes the launch geometry of a lone window (128 instead of 512 pairs per
                           lane and batch), which is what such a launch would ship with */
  int32_t no_glv;       /* != 0 (Weierstrass curves): no endomorphism split -- digits of the full scalar, K = ceil((b + 1) / c)
                           with b = bit length of q: the window structure of msmProjective / msmBasic
                           (src/parallel.ts:69-87, src/msm-basic.ts:56-91).  Same group element, 2x the additions */
  int32_t strict;       /* != 0: a scalar >= q fails the call with MSM_ERR_SCALAR.  Default: such scalars are reduced mod q
                           (the reference specifies inputs < q, src/curve-random.ts:151-194, and does not check) */
  uint32_t point_lo;    /* the call covers the resident points [point_lo, point_lo + n): scalars[i] belongs to point
                           point_lo + i.  The points-split shard of a multi-GPU run: rank g runs all K windows
                           on its n / G points, msm_combine_groups adds the G partial sums of every window */
  int32_t by_window;    /* multi-device contexts (msm_ctx_create_multi): != 0 shards an MSM by scalar window, every device then
                           needs all n scalars; default 0: by points, device d gets the scalars of its n / G points only */
  int32_t no_tables;    /* != 0: do not use (and do not build) window tables for this call -- the plain path over the resident
                           rows, K windows of buckets and a Horner step, as in rounds 1-4 (see msm_precompute) */
  int32_t bucket_shard, bucket_shards;   /* bucket_shards = G > 1: the call covers only the buckets [L g / G, L (g + 1) / G) of every
                           window, g = bucket_shard (L = buckets per window): the bucket-range shard of a multi-GPU run -- rank g
                           slices ALL scalars into all K windows but sorts and adds an eighth of the entries, K stays the
                           single-GPU plan's (the reference splits every window's buckets across its threads the same way,
                           src/msm-common.ts:72-172).  The partial sums keep the buckets' true weights: the G results of
                           msm_window_sums add up per window (msm_combine_groups), those of msm_run as points */
  int32_t merged_sums;  /* msm_window_sums, != 0: the caller only COMBINES the sums (msm_combine / msm_combine_groups), so the call may
                           hand them back merged -- slot 0 of its window range then carries sum_k 2^(c (k - k_lo)) P_k and the
                           other slots the identity, which the Horner step of either combine takes like one P_k per slot -- and
                           with that run on window tables: those of the whole point set, or of the range of the points the call
                           covers (the share of one rank of a points-split run; see msm_precompute).  Default 0: one P_k per
                           slot, the plain path */
  int32_t reserved_;
} msm_opts;

#define MSM_N_PHASES 8
/* phase_ms indices (HIP-event timings on the context's stream; the reference returns a tic/toc log,
 * src/msm-common.ts:176-214) */
enum {
  MSM_T_TOTAL = 0, MSM_T_UPLOAD = 1, MSM_T_DIGITS = 2, MSM_T_SORT = 3,
  MSM_T_ACCUMULATE = 4, MSM_T_REDUCE = 5, MSM_T_FINAL = 6, MSM_T_ACC_ROUND1 = 7
};

typedef struct msm_result {
  uint8_t x[48];        /* canonical affine result, little-endian (first 32 bytes used for Ed-on-BLS12-377) */
  uint8_t y[48];
  int32_t is_infinity;  /* Weierstrass only; twisted Edwards returns (0, 1) for the identity */
  int32_t c;            /* window size used */
  int32_t K;            /* number of windows */
  int32_t rounds;       /* accumulation tree rounds (k_batch_add launches) summed over all window groups */
  float phase_ms[MSM_N_PHASES];
  uint64_t n_pairs;     /* affine pair additions issued (all rounds, all windows), padding lanes of the tree included */
  uint64_t max_bucket;  /* largest bucket population seen */
  uint64_t n_pairs_algo; /* pair additions the bucket sums NEED: sum over the non-empty buckets of (population - 1); the
                            basis of roofline figures (n_pairs is ~2.5 % above it at 2^26) */
  int32_t tables;        /* != 0: the call ran on window tables (tables 2^(c j) P of the point set, one set of buckets per window group) */
  int32_t reserved_;
} msm_result;

/* Context: binds one curve to one GPU (device index as seen by HIP). Replaces
 * `Weierstraß.create(params)` / `TwistedEdwards.create(params)` (src/parallel.ts:40-66, 179-200). */
int msm_ctx_create(msm_ctx** out, int curve, int device);
/* The same over a device list ("create(curve id, device list)").  Every device holds the whole
 * point set; msm_run / msm_window_sums give every device a share of the POINTS (all windows over n / G points, the
 * default) or, with msm_opts.by_window, one contiguous shard of the window range (windows are independent until the
 * final sum, src/msm-batched-affine.ts:312-333), run the shards from one host thread per device and combine the
 * K x 144 bytes of partition sums per device on the host -- so a C or JS host can use a whole node without
 * torch.distributed.  Device scalars must live on devices[0]; the other devices copy their part peer-to-peer.
 * (bench.py --gpus N keeps the one-process-per-GPU RCCL form of the north star.) */
int msm_ctx_create_multi(msm_ctx** out, int curve, const int32_t* devices, int32_t n_devices);
int msm_ctx_device_count(const msm_ctx* ctx);
void msm_ctx_destroy(msm_ctx* ctx);
const char* msm_last_error(const msm_ctx* ctx);

/* Upload + convert the base points and keep them resident (pointsFromBytes, src/parallel.ts:97-116:
 * fromPackedBytes + toMontgomery; the endomorphism image beta*x is precomputed here once instead of
 * per call as in preparePointsAndScalars, src/msm-batched-affine.ts:350-421).
 * on_device != 0: `points` is a device pointer.  check_curve != 0: verify the curve equation. */
int msm_set_points(msm_ctx* ctx, const void* points, uint64_t n, int on_device, int check_curve);

/* Point formats and validation levels of msm_set_points_ex / msm_validate_points / msm_get_points_ex.
 * MSM_POINTS_UNCOMPRESSED is the x || y format of msm_set_points.  MSM_POINTS_COMPRESSED is one coordinate and flag bits:
 *   BLS12-381 G1 (ZCash / blst)   48 bytes, x BIG-endian; first byte: 0x80 compressed (must be set), 0x40 infinity,
 *                                 0x20 sign = y > (p-1)/2.  Identity: c0 00 .. 00
 *   BLS12-377 G1 (arkworks)       48 bytes, x little-endian; last byte: 0x80 sign = y > (p-1)/2, 0x40 infinity.
 *                                 Identity: last byte 0x40, every other byte 0
 *   Pallas, Vesta (pasta / halo2) 32 bytes, x little-endian; bit 255 sign = y odd.  Identity: 32 zero bytes
 *   BN254 G1, Grumpkin (arkworks) 32 bytes, x little-endian; last byte: 0x80 sign = y > (p-1)/2, 0x40 infinity (254-bit
 *                                 moduli leave both bits free).  Identity: last byte 0x40, every other byte 0
 *   Ed-on-BLS12-377 (arkworks)    32 bytes, y little-endian; bit 255 sign = x > (r-1)/2.  Identity: y = 1, sign 0
 * Decoding refuses a coordinate >= the modulus, invalid flags (a missing 0x80 on BLS12-381; infinity with any other bit set;
 * both flags on BLS12-377 / BN254 / Grumpkin; bits the layout does not use), an x (Edwards: y) without a curve point, and a sign bit set on a
 * root that is 0.  Validation: NONE; CURVE = the curve equation (a decoded point always satisfies it); SUBGROUP = the curve
 * equation and [q] P = O (Pallas, Vesta, BN254 G1, Grumpkin: cofactor 1, the curve equation is enough). */
enum { MSM_POINTS_UNCOMPRESSED = 0, MSM_POINTS_COMPRESSED = 1 };
enum { MSM_VALIDATE_NONE = 0, MSM_VALIDATE_CURVE = 1, MSM_VALIDATE_SUBGROUP = 2 };
/* msm_set_points with a format and a validation level.  UNCOMPRESSED + CURVE is msm_set_points(check_curve = 1), UNCOMPRESSED
 * + NONE msm_set_points(check_curve = 0).  Compressed points are decoded on the GPU (one square root per point, written
 * straight into the resident rows); SUBGROUP runs the subgroup check over the new rows.  A refused point fails the call with
 * MSM_ERR_POINT and a message that names its index and the reason ("coordinate >= p", "invalid flags", "no curve point",
 * "not on curve", "not in the prime-order subgroup"); *bad_index_out (may be NULL) gets that index -- the smallest bad one --
 * or UINT64_MAX when every point passed.  A failed call leaves the current point set as a failed msm_set_points does: empty,
 * its window tables dropped.  Host or device input, n < 2^30.  Device lists: every device decodes for itself, devices[0]
 * alone runs the subgroup check. */
int msm_set_points_ex(msm_ctx* ctx, const void* points, uint64_t n, int on_device, int format, int validate,
                      uint64_t* bad_index_out);
/* Checks the resident points [first, first + count) of the current set at `validate` and changes nothing: MSM_OK, or
 * MSM_ERR_POINT with the first bad index in the message and in *bad_index_out (UINT64_MAX when every point passed). */
int msm_validate_points(msm_ctx* ctx, uint64_t first, uint64_t count, int validate, uint64_t* bad_index_out);
/* msm_get_points in either format: count x (2 coordinates) or count x (1 coordinate) bytes.  The compressed encoding is the
 * inverse of the decoder of msm_set_points_ex. */
int msm_get_points_ex(msm_ctx* ctx, uint64_t first, uint64_t count, int format, uint8_t* out);

/* Window tables.  For a fixed point set (the bases of a prover: the reference's callers load their points once and run many
 * MSMs over them, scripts/msm-weierstrass.ts:19-35) the library can keep K tables instead of one: table k holds 2^(c k) P_i for
 * every point, so the digit of window k addresses a point that already carries the window's weight and all K windows share ONE
 * set of 2^(c-1) buckets -- K times fewer buckets to finish and reduce, no Horner step, same group element.  The reference has
 * no counterpart (its heap is 4 GiB).
 * Shared tables: a call that runs as two window groups (BLS12-377 and the other Weierstrass curves from 2^21 points, the
 * Edwards curve from 2^20) holds only T = ceil(K / 2) tables: both groups read tables 0 .. T - 1, each relative to its own first
 * window, and the host supplies the weight 2^(c T) between the two sums.  Three tables of 2^26 BLS12-377 points under the
 * six-window plan are 51.5 GB of the 288 GB of HBM, the plain rows included (six would be 103 GB).
 * msm_run builds them by itself on its first call over the WHOLE current point set with the default window (opts->c == 0)
 * when they fit the limit (default: 20 % of the device memory -- 57.6 GB: point sets of up to 2^26 BLS12-377 points; what they
 * buy shrinks from 6-10 % below 2^24 points to about 5 % at 2^26), and uses them whenever the call's plan is the one they were built
 * for; any other call -- another window size, a prefix or another range of the points, msm_window_sums without merged_sums, a bucket-range shard, a device-list context --
 * takes the plain path over table 0, which is always the plain row table.  msm_precompute builds them ahead of the first call
 * (also for an explicit opts->c); it is not an error if they do not fit: the plain path stays.  msm_set_points drops them.
 * Tables over a RANGE of the points (round 6): the rank of a points-split run works on its share [point_lo, point_lo + n) of
 * the resident points in every step; msm_precompute with opts->point_lo builds the tables of exactly that range (2^23 points x 4
 * shared tables for 7 windows = 8.6 GB, in a buffer of their own next to the plain rows), and msm_run / msm_window_sums (with msm_opts.merged_sums)
 * over that range run on them.  Without msm_precompute they are built when a call comes back for the same range a second
 * time in a row -- a caller that walks over several ranges on one GPU is spared a build per call.  The first call already runs
 * under the plan the tables will have (on the plain path: msm_result.tables = 0), so every call over one range reports the
 * (c, K) msm_plan gives for it, before and after the build.  A point set holds the tables
 * of ONE range (or of the whole set, which a range never replaces by itself): while the whole set's tables exist, a default-plan
 * call over a range runs -- and msm_plan reports -- the plain plan.
 * msm_precompute with opts->c == 0 builds for the plan a default-plan call over those points picks on tables: such a call then
 * runs on them from the first time on.
 * msm_tables_info: window size and window count K of the plan the tables present serve (0, 0: none) and the bytes they take --
 * those of the T tables held; msm_tables_range: the points they cover. */
int msm_precompute(msm_ctx* ctx, uint64_t n, const msm_opts* opts);
int msm_tables_info(const msm_ctx* ctx, int32_t* c_out, int32_t* K_out, uint64_t* bytes_out);
int msm_tables_range(const msm_ctx* ctx, uint64_t* point_lo_out, uint64_t* n_out);
int msm_set_tables_limit(msm_ctx* ctx, uint64_t bytes);   /* 0: never build tables */

/* Everything a later msm_run(ctx, <device scalars>, n, opts) allocates or builds -- the per-call workspace (device memory costs
 * ~40 ms per GB to get on this system: 3 s before the first 2^26 MSM) and the window tables -- taken out of that call: runs one
 * MSM over internally generated scalars and discards the result. */
int msm_reserve(msm_ctx* ctx, uint64_t n, const msm_opts* opts);

/* Point-set handles (the reference's `pointPtr`s are independent allocations, src/parallel.ts:97-116): a context starts
 * with point set 0; msm_pointset_create adds an empty one and makes it current, msm_pointset_select switches.
 * msm_set_points / msm_generate_points / msm_run / msm_get_points always act on the current set. */
int msm_pointset_create(msm_ctx* ctx, int32_t* id_out);
int msm_pointset_select(msm_ctx* ctx, int32_t id);
int msm_pointset_destroy(msm_ctx* ctx, int32_t id);

/* Device buffers for scalar handles (`scalarPtr`s are independent allocations too): owned by the context, freed by
 * msm_device_free or with the context.  On a multi-device context they live on devices[0]. */
int msm_device_alloc(msm_ctx* ctx, uint64_t bytes, void** dev_ptr_out);
int msm_device_free(msm_ctx* ctx, void* dev_ptr);
int msm_device_upload(msm_ctx* ctx, void* dev_ptr, const void* host, uint64_t bytes);
/* the way back: `bytes` bytes from device memory of the context's device (a buffer of msm_device_alloc or any allocation of the
 * caller, at any offset) into host memory; returns when they have arrived */
int msm_device_download(msm_ctx* ctx, void* host, const void* dev_ptr, uint64_t bytes);

/* Resident scalar-vector operations: arithmetic mod q -- the group order of the context's curve -- over vectors of scalars that
 * stay in device memory: the scalar half of a round of an inner-product argument (the fold a' = u a_lo + u^-1 a_hi, the inner
 * products <a_lo, b_hi> and <a_hi, b_lo>) beside msm_points_lincomb and msm_run, the powers (1, z, z^2, ...) of an evaluation
 * point, a polynomial evaluation <coeffs, powers(z)>, a random linear combination or the element-wise product of two columns.
 * The reference has no counterpart.  All seven curves.
 * Vectors: dst, a and b are device pointers on the context's device, n x 32 bytes each: from msm_device_alloc or any allocation
 *   of the caller, at any 32-byte offset inside one; aligned to 16 bytes, else MSM_ERR_ARG.  Elements are the 32-byte little-endian
 *   integers msm_run reads (no Montgomery form); an element >= q is taken as its residue, msm_run's rule without `strict`.  Every
 *   element written is canonical, in [0, q).  n < 2^30; n == 0 is valid, writes nothing, and msm_scalars_inner then returns 0.
 * Host scalars: x, y and s are 32 bytes little-endian; a value >= q fails with MSM_ERR_SCALAR (the rule of msm_points_lincomb).
 *   0 and 1 are ordinary input.
 * Aliasing: dst may be exactly a, exactly b, or disjoint from both -- lane i reads its inputs before its one store.  The in-place
 *   fold of a vector v of 2 h elements is dst = a = v, b = v + 32 h, n = h; the upper half is left as it was.  A dst range that
 *   overlaps a source range in part fails with MSM_ERR_ARG before anything is launched.  The sources may overlap each other freely.
 * Errors: null pointers with n > 0 (a null b of msm_scalars_lincomb is its one-term form), a null host scalar or `out`, a
 *   device-list context, n >= 2^30: MSM_ERR_ARG.  All checks run before anything is written; a failed call leaves the context
 *   usable.
 * Ordering: every call returns when its result is in place (it synchronises the context's stream, as msm_points_lincomb does):
 *   an msm_run over the same buffer needs no extra step.  No call touches point sets, window tables or the range-table candidate.
 * msm_scalars_inner returns the same bits whatever the launch geometry: field addition is exact. */
/* dst[i] = x * a[i] + y * b[i] mod q.  b == NULL: one term, dst[i] = x * a[i] (y is ignored) */
int msm_scalars_lincomb(msm_ctx* ctx, void* dst, const uint8_t* x /* 32 B LE */, const void* a, const uint8_t* y /* 32 B LE */,
                        const void* b, uint64_t n);
/* dst[i] = a[i] * b[i] mod q */
int msm_scalars_mul(msm_ctx* ctx, void* dst, const void* a, const void* b, uint64_t n);
/* out = sum_i a[i] * b[i] mod q, 32 bytes little-endian on the host */
int msm_scalars_inner(msm_ctx* ctx, const void* a, const void* b, uint64_t n, uint8_t* out);
/* dst[i] = s * x^i mod q, i < n */
int msm_scalars_powers(msm_ctx* ctx, void* dst, const uint8_t* s /* 32 B LE */, const uint8_t* x /* 32 B LE */, uint64_t n);

/* The resident number-theoretic transform over the same vectors: polynomials in evaluation form (PLONK / Halo2 columns, KZG,
 * Groth16's quotient) go to coefficients and back, on a domain or on a coset of it, without leaving the device; an msm_run over
 * dst needs no extra step.  A binding detects the feature by the presence of msm_scalars_ntt.  The reference has no counterpart.
 * B transforms of n = 2^log2n elements each, vectors back to back (vector b at element offset b n):
 *   forward:  dst[k] = sum_j a[j] (shift omega^k)^j  -- the polynomial with coefficients a on the coset shift <omega>
 *   inverse:  the exact inverse map (evaluations on that coset -> coefficients; the factors n^-1 and shift^-j included)
 *   natural order in and out, both directions.
 * Vectors: everything msm_scalars_* says above holds -- plain 32-byte little-endian integers, any value below 2^256 counts as
 *   its residue, every element written is canonical, 16-byte alignment at any 32-byte offset inside an allocation.  Single-device
 *   contexts only.  The call returns when the result is in place (it synchronises the context's stream) and touches no point set,
 *   window table or range-table candidate.
 * Aliasing: dst may be exactly a, or disjoint from it, over the whole B n range; a partial overlap is MSM_ERR_ARG.
 * omega: 32 bytes little-endian, a primitive n-th root of unity mod q of the caller's convention (arkworks, halo2), or NULL for
 *   the library's (msm_scalars_root_of_unity).  The host checks omega^(n/2) = q - 1 for n >= 2 -- which is "primitive n-th root" --
 *   and fails with MSM_ERR_ARG and a message about the order otherwise; a value >= q is MSM_ERR_SCALAR; for n = 1 omega is ignored.
 * shift: 32 bytes little-endian in [1, q), or NULL for 1.  0 is MSM_ERR_ARG (the inverse needs shift^-1), a value >= q is
 *   MSM_ERR_SCALAR.  The host computes shift^-1 and n^-1 once per call.  A forward transform without a shift multiplies nothing
 *   for it.
 * Limits: log2n above msm_scalars_ntt_max_log2n, B == 0 and B n >= 2^30 are MSM_ERR_ARG.  The two-adicity of q - 1 is 47 for
 *   BLS12-377, 32 for BLS12-381, Pallas and Vesta, 28 for BN254 and 1 for Grumpkin and Ed-on-BLS12-377: the last two accept
 *   log2n <= 1 and refuse the rest, which is the correct answer for those fields.
 * Errors: null pointers, misaligned pointers, a device-list context and the limits above: MSM_ERR_ARG.  All checks run before
 *   anything is written; a failed call leaves the context usable.
 * Device memory beyond the caller's vectors, owned by the context and freed with it (each grows to the largest call, plus 1/16):
 *   twiddle cache   64 (2^h + 2^(log2n - h) + 2^(g - 1)) bytes, h = log2n for log2n <= 10 and ceil(log2n / 2) above, g = min(log2n, 10):
 *                   two-level tables of omega and omega^-1 (3.0 MiB at 2^29, 1 MiB at 2^26).  It holds the tables of one
 *                   (log2n, omega) at a time; a second call with the same pair builds nothing.
 *   shift table     32 (2^h + 2^(log2n - h)) bytes, calls with a shift other than 1 only, rebuilt by each of them
 *   scratch vector  32 B n bytes when the transform takes more than one pass (log2n > 9), else none */
int msm_scalars_ntt(msm_ctx* ctx, void* dst, const void* a, uint32_t log2n, uint32_t B,
                    const uint8_t* omega /* 32 B LE, NULL = the library's root */,
                    const uint8_t* shift /* 32 B LE, NULL = 1 */, int inverse);
/* the library's primitive 2^log2n-th root of unity mod q: g^((q-1)/2^log2n), g = the smallest positive quadratic non-residue
 * (11 for BLS12-377, 3 for Grumpkin, 5 for the other five), so root(k)^2 = root(k - 1).  log2n above the two-adicity of q - 1:
 * MSM_ERR_ARG.  No device work. */
int msm_scalars_root_of_unity(const msm_ctx* ctx, uint32_t log2n, uint8_t* out /* 32 B LE */);
/* the largest log2n msm_scalars_ntt accepts on this context: min(two-adicity of q - 1, 29) */
int msm_scalars_ntt_max_log2n(const msm_ctx* ctx, uint32_t* out);

/* Resident scans over the same vectors: what carries a value from one element to the next.  Prefix sums and products (the grand
 * product z[i+1] = z[i] num[i] / den[i] of a PLONK / Halo2 permutation or lookup argument, the running sum of a log-derivative
 * lookup), the element-wise inverse they need (Montgomery's trick), and the division of a polynomial by X - z (the witness of a
 * KZG opening, with the evaluation a(z) as its remainder), without leaving the device; an msm_run over dst needs no extra step.
 * A binding detects the feature by the presence of msm_scalars_scan.  The reference has no counterpart.  All seven curves.
 * Vectors: everything msm_scalars_* says above holds -- plain 32-byte little-endian integers, any value below 2^256 counts as
 *   its residue, every element written is canonical, 16-byte alignment at any 32-byte offset inside an allocation.  n < 2^30.
 *   n == 0 is valid and writes nothing: total_out = init, n_zero_out = 0, rem_out = 0.
 * Host scalars: init and z are 32 bytes little-endian; a value >= q fails with MSM_ERR_SCALAR.  0 and 1 are ordinary input.
 * Aliasing: dst may be exactly a, or disjoint from it; a partial overlap is MSM_ERR_ARG before anything is launched.
 * Errors: null pointers with n > 0 (a null z always), misaligned pointers, a device-list context, n >= 2^30, an unknown op and
 *   unknown flag bits: MSM_ERR_ARG.  All checks run before anything is written; a failed call leaves the context usable.
 * Ordering: every call returns when its result is in place (it synchronises the context's stream) and touches no point set,
 *   window table or range-table candidate.
 * Results are the same bits whatever the tile geometry: the operators are exact.
 * Device memory beyond the caller's vectors, owned by the context and freed with it (it grows to the largest call, plus 1/16):
 *   tile aggregates 32 bytes per tile and level, and 32 for the total: a scan runs over tiles of 2^10 elements, the aggregates
 *                   of more than one tile are scanned the same way, so 32 (1 + ceil(n / 2^10) + ceil(n / 2^20)) bytes
 *                   (2.0 MiB at 2^26; none beyond the total up to 2^10 elements)
 *   zero counts     4 ceil(n / 2^11) bytes for msm_scalars_inverse, in the same buffer */
enum { MSM_SCAN_SUM = 0, MSM_SCAN_PRODUCT = 1 };
enum { MSM_SCAN_EXCLUSIVE = 1 }; /* flags; every other bit is MSM_ERR_ARG */
/* o = addition (MSM_SCAN_SUM) or multiplication (MSM_SCAN_PRODUCT) mod q
 *   inclusive: dst[i] = init o a[0] o ... o a[i]
 *   exclusive: dst[i] = init o a[0] o ... o a[i-1]   (dst[0] = init)
 * *total_out (32 B LE on the host, may be NULL) = init o a[0] o ... o a[n-1]
 * init: 32 B LE below q, NULL = the operator's neutral element (0 / 1) */
int msm_scalars_scan(msm_ctx* ctx, void* dst, const void* a, uint64_t n, int op, uint32_t flags,
                     const uint8_t* init, uint8_t* total_out);
/* dst[i] = a[i]^-1 mod q.  An element whose residue is 0 gives 0 (the rule of arkworks' and halo2's batch inversion): that is
 * 0, q, and every other multiple of q below 2^256.  *n_zero_out (may be NULL) = how many such elements there were */
int msm_scalars_inverse(msm_ctx* ctx, void* dst, const void* a, uint64_t n, uint64_t* n_zero_out);
/* a = the n coefficients of a polynomial, a[0] the constant term: dst[j] = q_j for j < n - 1 and dst[n-1] = 0, where
 * a(X) = (X - z) q(X) + a(z); *rem_out (32 B LE, may be NULL) = a(z).  z: 32 B LE below q; 0 is ordinary input.
 * n == 1: dst[0] = 0, rem = a[0] mod q */
int msm_scalars_div_linear(msm_ctx* ctx, void* dst, const void* a, uint64_t n, const uint8_t* z, uint8_t* rem_out);

/* Resident sumcheck over the same vectors: the scalar work of the provers on the curve cycles (Nova / Spartan, HyperPlonk, Jolt,
 * GKR) is not the NTT but the sumcheck over multilinear tables.  Three operators run a whole sumcheck with d + 1 scalars leaving
 * the device per round and one challenge entering it: the round polynomial of a product of tables, the binding of one variable
 * to the challenge, and the table eq(r, .) that every multilinear evaluation f(r) = <eq(r), f> and every Spartan-style round
 * needs; an msm_run over a bound or eq-weighted vector needs no extra step.  A binding detects the feature by the presence of
 * msm_scalars_sumcheck_round.  The reference has no counterpart.  All seven curves.
 * Tables: a vector of n = 2^log2n elements is a multilinear table, log2n = 1 .. 29.  VARIABLE j IS BIT j OF THE INDEX: variable 0
 *   is the least significant bit, which is arkworks' and HyperPlonk's order.  A caller with the most-significant-first convention
 *   (Spartan) reverses its point.  For a variable var < log2n, h = n / 2 and a pair index i < h the two rows of pair i are
 *     lo(i) = ((i >> var) << (var + 1)) | (i & (2^var - 1))      hi(i) = lo(i) + 2^var
 *   so var = log2n - 1 pairs row i with row i + h (the halves of the table), and var = 0 pairs neighbours.
 * Vectors: everything msm_scalars_* says above holds -- plain 32-byte little-endian integers, any value below 2^256 counts as
 *   its residue, every element written is canonical, 16-byte alignment at any 32-byte offset inside an allocation.
 * Host scalars: r and s are 32 bytes little-endian each; a value >= q fails with MSM_ERR_SCALAR.  0 and 1 are ordinary input.
 * Errors: log2n outside 1 .. 29 (v above 29), var >= log2n, m out of range, an unknown shape, null or misaligned pointers -- a
 *   null entry of a pointer array included --, a device-list context: MSM_ERR_ARG.  All checks run before anything is written; a
 *   failed call leaves its outputs and the context as they were.
 * Ordering: every call returns when its result is in place (it synchronises the context's stream) and touches no point set,
 *   window table or range-table candidate.
 * msm_scalars_sumcheck_round returns the same bits whatever the launch geometry: field addition is exact.
 * Device memory beyond the caller's vectors, owned by the context and freed with it:
 *   round partials  32 bytes per block and value and the d + 1 results: at most 32 * 5 * 1025 bytes
 *   eq half-tables  32 (2^ceil(v / 2) + 2^floor(v / 2)) bytes (1.5 MiB at v = 29), rebuilt by every msm_scalars_eq */
enum { MSM_SUMCHECK_PROD = 0, MSM_SUMCHECK_R1CS = 1 };
/* The round polynomial s of the sum over all pairs, at t = 0 .. d:
 *   evals_out[t] = sum_{i<h} g(f_0(i,t), .., f_(m-1)(i,t)),    f_j(i,t) = a_j[lo(i)] + t (a_j[hi(i)] - a_j[lo(i)])
 * a_j = vecs[j], m device vectors of n elements; evals_out: (d + 1) x 32 bytes little-endian on the host.
 *   MSM_SUMCHECK_PROD   g = prod_j f_j, 1 <= m <= 4, d = m.  m = 1 is the plain sum.
 *   MSM_SUMCHECK_R1CS   g = f_0 (f_1 f_2 - f_3), m = 4 exactly, d = 3: the outer sumcheck of Spartan / Nova, f_0 = eq(tau, .)
 * All d + 1 values come back, s(1) included: s(0) + s(1) is the claim of the round, which a prover asserts.
 * The vectors are only read; the same pointer may appear several times and vectors may overlap freely.
 * A general sum of products sum_c c prod_j f_(c,j) is deliberately not a shape: the round polynomial is linear in g, so a caller
 * runs one call per product and combines the d + 1 scalars of each on the host. */
int msm_scalars_sumcheck_round(msm_ctx* ctx, const void* const* vecs, uint32_t m, uint32_t log2n, uint32_t var, int shape,
                               uint8_t* evals_out /* (d+1) x 32 B LE, host */);
/* Binds variable var of m tables (1 <= m <= 8) to r in one launch, one multiplication per output:
 *   dst[j][i] = a[j][lo(i)] + r (a[j][hi(i)] - a[j][lo(i)]),  i < h: a table of log2n - 1 variables, the variables above var
 *   moving down by one.
 * Aliasing: every dst range (h x 32 bytes) is disjoint from every other dst range and from every source range (n x 32 bytes),
 *   with one exception: dst[j] == a[j] exactly when var == log2n - 1 -- lane i then reads rows i and i + h and writes row i, and
 *   the upper half is left as it was.  Anything else is MSM_ERR_ARG before a launch.  Sources may overlap each other. */
int msm_scalars_bind(msm_ctx* ctx, void* const* dst, const void* const* a, uint32_t m, uint32_t log2n, uint32_t var,
                     const uint8_t* r /* 32 B LE, < q */);
/* dst[i] = s prod_{j<v} (bit_j(i) ? r_j : 1 - r_j), i < 2^v: the table eq(r, .) scaled by s.  0 <= v <= 29; v = 0 writes
 * dst[0] = s.  r: v x 32 bytes little-endian on the host (may be NULL with v = 0); s: 32 bytes, NULL = 1.
 * Built from two half-tables, eq(r, i) = T_hi[i >> k] T_lo[i & (2^k - 1)] with k = ceil(v / 2): one multiplication and one store
 * per element. */
int msm_scalars_eq(msm_ctx* ctx, void* dst, const uint8_t* r /* v x 32 B LE, host */, uint32_t v,
                   const uint8_t* s /* 32 B LE, NULL = 1 */);

/* Resident sparse matrices and matrix-vector products over the same vectors: dst = alpha M x (+ dst) mod q.  The tables of the
 * R1CS shape above are A z, B z and C z -- the circuit's sparse matrices times the resident witness --, Spartan's second sumcheck
 * needs the transposed product M^T eq(r_x, .), and with every coefficient 1 the product is the gather y[i] = T[idx[i]] of a lookup
 * or permutation argument and the row sum.  A matrix is a HANDLE as a point set is, not per-call pointers: a circuit's matrices
 * are fixed across thousands of proofs, so validation, the conversion of the coefficients and the load-balancing plan are paid
 * once, at creation.  A binding detects the feature by the presence of msm_scalars_matvec.  The reference has no counterpart.
 * All seven curves.
 * Format: CSR.  row_ptr holds rows + 1 32-bit words, col holds nnz 32-bit column indices, val holds nnz x 32-byte little-endian
 *   scalars in the vectors' format (any value below 2^256 counts as its residue).  val == NULL: every coefficient is 1 -- no
 *   multiplication, and no value bytes stored or read.  Within a row the entries may come in any order and may repeat a column:
 *   the product sums the multiset; an empty row gives 0.  rows, cols < 2^30 and nnz < 2^31; rows == 0 or nnz == 0 is valid.
 *   on_device covers all three arrays; device arrays are aligned to 4 bytes, val to 16.
 * Ownership: the context copies everything into memory it owns -- the sole-ownership rule of point sets --, so the caller's
 *   buffers may be freed or overwritten as soon as msm_matrix_create returns.  A matrix is freed by msm_matrix_destroy or with the
 *   context.  Ids behave as msm_pointset_* ids do: small positive integers, a destroyed one may be handed out again.
 * Validation, at creation and before any index is ever used as an address: row_ptr[0] == 0, row_ptr non-decreasing,
 *   row_ptr[rows] == nnz, every col[j] < cols.  A defect is MSM_ERR_ARG and the message names the smallest bad position and its
 *   value ("col[j] = v but cols = c"); row_ptr defects are reported before col defects.  Host input is checked on the host before
 *   the upload, device input by kernels that read only the arrays inside their stated lengths, col only after row_ptr has passed.
 *   A refused creation leaves no matrix, no leaked memory and a usable context; *id_out is untouched.
 * MSM_MATRIX_TRANSPOSE stores M^T of what is given, so the handle is cols x rows: a stable counting sort over the columns on the
 *   host -- within a transposed row the entries keep the order of the original rows.  Host input only (with on_device: MSM_ERR_ARG).
 * Errors: unknown flag bits, sizes beyond the limits, null pointers with a non-empty range, misaligned device pointers, an unknown
 *   or destroyed id, a device-list context (on every entry point here): MSM_ERR_ARG.  alpha >= q: MSM_ERR_SCALAR.
 * Device memory of a matrix (msm_matrix_info): 4 (rows + 1) + 4 nnz + 32 nnz bytes (4 nnz without coefficients), plus 12 bytes per
 *   part, 8 per long row and 32 per part of partial sums for the rows above short_max, each array rounded up by a sixteenth. */
enum { MSM_MATRIX_TRANSPOSE = 1 };   /* create flags; every other bit is MSM_ERR_ARG */
int msm_matrix_create(msm_ctx* ctx, uint64_t rows, uint64_t cols, uint64_t nnz, const uint32_t* row_ptr,
                      const uint32_t* col, const void* val, int on_device, uint32_t flags, int32_t* id_out);
int msm_matrix_destroy(msm_ctx* ctx, int32_t id);
/* Sizes of matrix `id` as it is held (transposed, if it was created so) and the device bytes it takes; every out may be NULL. */
int msm_matrix_info(const msm_ctx* ctx, int32_t id, uint64_t* rows_out, uint64_t* cols_out, uint64_t* nnz_out,
                    uint64_t* bytes_out);
/* dst[r] = alpha sum_{j in row r} val[j] x[col[j]] mod q; with MSM_MATVEC_ACCUMULATE the old dst[r] is added (taken as its
 * residue, as every vector element is).  dst: rows x 32 bytes, x: cols x 32 bytes, device pointers aligned to 16 bytes; every
 * element written is canonical.  dst must be DISJOINT from x, because a row reads arbitrary entries of x: an exact or partial
 * overlap is MSM_ERR_ARG before a launch.  alpha: 32 bytes little-endian below q, NULL = 1; 0 and 1 are ordinary input.  x may be
 * NULL when the matrix has no entry.  One launch, three when a row is longer than short_max.  The call returns when the result
 * is in place and touches no point set, window table or range-table candidate.
 * THE RESULT IS THE SAME BITS WHATEVER THE LAUNCH GEOMETRY: field addition is exact and no atomic touches a field element. */
enum { MSM_MATVEC_ACCUMULATE = 1 };  /* flags; every other bit is MSM_ERR_ARG */
int msm_scalars_matvec(msm_ctx* ctx, int32_t id, void* dst, const void* x, const uint8_t* alpha /* 32 B LE, NULL = 1 */,
                       uint32_t flags);

/* Device memory the working buffers of one call may take (digits, sort records, tree nodes: the reference sizes them per call
 * in wasm memory, src/msm-batched-affine.ts:96-130).  0 = automatic: 85 % of what the device has free when a big call starts.
 * Windows run in as many groups as fit, and a window whose buffers would not fit at all runs over ranges of the points, one
 * range after the other, its sums added on the host -- so a limit (a GPU shared with other work) or an input of 2^29 points
 * costs time, not an error.  Multi-device contexts apply the limit per device. */
int msm_set_workspace_limit(msm_ctx* ctx, uint64_t bytes);

/* sum_i scalars[i] * points[i] over the first n resident points
 * (msm / msmUnsafe, src/msm-batched-affine.ts:69-340, 587-598; for the Edwards curve msmBasic,
 * src/msm-basic.ts:45-164).  on_device != 0: `scalars` already sits in HBM. */
int msm_run(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, msm_result* out);

/* B MSMs over the same resident points [point_lo, point_lo + n) of the current point set:
 * out[b] = sum_i scalars[b][i] * P_(point_lo + i).  scalars[b] is n x 32 bytes, host or device (on_device).
 * Result by result, equal to B calls of msm_run(ctx, scalars[b], n, on_device, opts, &out[b]): out[b].x / .y / .is_infinity are
 * bit-identical to what msm_run returns for element b.  Where one MSM is mostly fixed latency (single-device contexts, window
 * plans of the one-level sort: below 2^20 points on the Weierstrass curves, 2^22 on the Edwards curve) the elements share the
 * same launches -- element b's window k is window b K + k of one window group -- and the call never builds or uses window
 * tables; elsewhere it runs element by element through msm_run.  out[b].c / .K report the plan that ran; phase_ms, rounds,
 * n_pairs, n_pairs_algo and max_bucket describe the whole batched call and are written identically into every element.
 * Options: c, no_glv, strict (one scalar >= q anywhere fails the whole call), point_lo, serial and no_tables are honoured,
 * unsafe is ignored as in msm_run; k_lo / k_hi, bucket_shards > 1, merged_sums and by_window fail with MSM_ERR_ARG, as do
 * B == 0, a null `out` and a null scalars[b] when n > 0.  n == 0 returns B identities. */
int msm_run_batch(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, int on_device, const msm_opts* opts,
                  msm_result* out /* B entries */);

/* Narrow scalars: the MSM of a column whose values are known to be small -- machine words, bits, small signed values -- without
 * the endomorphism split, which would spread a 64-bit scalar over two halves of ~126 bits: one entry per point and
 * K = ceil((bits + 1) / c) windows (msm_plan_narrow), e.g. 4 windows of 17 bits for 64-bit scalars instead of 6 x 21 bits over
 * 2 n entries.  The reference has no counterpart.
 * width_bytes: 1, 2, 4, 8, 16 (little-endian integers, n x width_bytes, naturally aligned) or 32 (field elements, as msm_run).
 *   DEVICE scalars must be aligned to min(width_bytes, 16) bytes -- the 16- and 32-byte forms are loaded 16 bytes at a time,
 *   also by msm_scalar_bits -- or the call fails with MSM_ERR_ARG; host buffers may sit anywhere.
 * bits: magnitude bits, 1 .. 128; 0 = all the width gives (8 w unsigned, 8 w - 1 signed; not allowed with width 32).
 * is_signed = 0: values in [0, 2^bits).  is_signed = 1: values in [-2^bits, 2^bits), so that a two's-complement word of
 *   8 w bits is covered by bits = 8 w - 1; widths 1 .. 16 are two's complement, width 32 holds v >= 0 as v and v < 0 as q - |v|.
 * A value outside the declared range ALWAYS fails the call with MSM_ERR_SCALAR (never a silently wrong sum).
 * out->x / y / is_infinity are bit-identical to msm_run over the same values written as 32-byte scalars (negatives as q - |v|);
 * out->c / K report the plan that ran, phase_ms, n_pairs, n_pairs_algo and max_bucket are those of msm_run.
 * Options: c (2 .. 24, at most 64 windows), point_lo and serial are honoured; no_glv is implied, unsafe ignored, strict has nothing
 * to add; k_lo / k_hi, bucket_shards > 1, merged_sums and by_window fail with MSM_ERR_ARG, as do a device-list context, a bad
 * width, bits beyond the width or beyond 128, B == 0 and null pointers.  n == 0 returns the identity.
 * A narrow call takes the plain path over table 0: it neither builds, uses nor drops the window tables of the point set.  Host
 * scalars are uploaded whole before the run.  msm_run_batch_narrow is msm_run_batch over narrow elements: fused where
 * msm_run_batch fuses (up to 64 elements per group; without opts->c it then picks a window of the one-level sort, at most 13
 * bits, where a single call would take 17), element by element through msm_run_narrow elsewhere -- bigger inputs, an explicit
 * c > 16, 1- or 2-byte device elements that do not start on a 4-byte boundary. */
int msm_run_narrow(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, int32_t width_bytes, int32_t bits, int32_t is_signed,
                   const msm_opts* opts, msm_result* out);
int msm_run_batch_narrow(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, int on_device, int32_t width_bytes,
                         int32_t bits, int32_t is_signed, const msm_opts* opts, msm_result* out /* B entries */);
/* the plan of msm_run_narrow over n points and scalars of `bits` magnitude bits (opts->c forces the window) */
int msm_plan_narrow(const msm_ctx* ctx, uint64_t n, int32_t bits, const msm_opts* opts, int32_t* c_out, int32_t* K_out);
/* smallest `bits` under which msm_run_narrow(width 32) accepts these 32-byte scalars, unsigned and signed
 * (0 for all-zero input; 255 when a scalar needs more than 128 bits or is >= q). */
int msm_scalar_bits(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, int32_t* unsigned_bits_out, int32_t* signed_bits_out);

/* Indexed (sparse) MSM: out = sum_j scalars[j] * P[indices[j]], j < m, over the current point set -- a sparse witness or error
 * column, lookup multiplicities scattered over a big table -- without the dense vector of mostly zeros the other entry points
 * need.  The call pays for its m entries, not for the resident count: digits, sort and pairing run over the m positions, and the
 * payloads are rewritten to name the resident rows before round 1 of the tree gathers them.  The reference has no counterpart.
 * Indices: m 32-bit unsigned positions in the current point set, each < the resident count, in any order and with repeats --
 *   the sum is over the multiset: the same point several times, or a point under a scalar and under its negative, are ordinary
 *   input.  m may be smaller or larger than the resident count, m < 2^30; m == 0 returns the identity.  on_device covers BOTH
 *   buffers; device indices must be aligned to 4 bytes.  Host buffers are uploaded whole before the run.
 * An index >= the resident count ALWAYS fails the call with MSM_ERR_ARG; the message names the smallest bad position j and its
 *   value ("indices[j] = v but n resident points").  The check runs on the GPU before anything is gathered: no row outside the
 *   table is ever read.  A failed call leaves the context usable and the point set untouched.  A call before any points are
 *   set fails with MSM_ERR_NO_POINTS.
 * Result: out->x / y / is_infinity are bit-identical to msm_run over the dense equivalent, the vector t of resident length with
 *   t[i] = sum of scalars[j] over indices[j] == i, mod q.  out->c / K report the plan that ran; phase_ms (MSM_T_UPLOAD: indices
 *   and host scalars into HBM and the index check), n_pairs, n_pairs_algo, max_bucket and rounds are as for msm_run.
 * Plan: the window is picked from m, not from the resident count -- the plain-path plan msm_plan(ctx, m, {no_tables}) reports
 *   (narrow: msm_plan_narrow(ctx, m, bits)); opts->c forces it.
 * Window tables: the call takes the plain path over table 0.  It neither builds, uses nor drops the window tables of the point
 *   set and does not count as a call over a range for the automatic range-table build.
 * Options: c, no_glv, strict and serial are honoured, unsafe is ignored as elsewhere; point_lo != 0, k_lo / k_hi,
 *   bucket_shards > 1, merged_sums and by_window fail with MSM_ERR_ARG, as do a device-list context and null pointers with m > 0.
 *   Scalars >= q under strict fail with MSM_ERR_SCALAR as in msm_run.
 * An input too big for the workspace runs over ranges of the ENTRIES as the dense path runs over ranges of the points: scalars
 *   and indices of a range are sliced together.
 * msm_run_indexed_narrow is the same over narrow scalars: width_bytes / bits / is_signed exactly as msm_run_narrow, which also
 *   says what it refuses (a bad width, bits beyond the width, misaligned device scalars) and that a value outside the declared
 *   range fails with MSM_ERR_SCALAR; equal to msm_run_narrow over the dense equivalent where that fits the declared range. */
int msm_run_indexed(msm_ctx* ctx, const void* scalars, const uint32_t* indices, uint64_t m, int on_device, const msm_opts* opts,
                    msm_result* out);
int msm_run_indexed_narrow(msm_ctx* ctx, const void* scalars, const uint32_t* indices, uint64_t m, int on_device, int32_t width_bytes,
                           int32_t bits, int32_t is_signed, const msm_opts* opts, msm_result* out);

/* Point-set linear combinations: D[i] = a * A[a_lo + i] + b * B[b_lo + i], i < count, written as the rows [0, count) of point set
 * `dst`, which then holds exactly `count` points -- resident points made from resident points, on the GPU.  With a = 1 or
 * a = u^-1, b = u over the two halves of one set it is the generator fold between two rounds of an inner-product argument
 * (Halo2, Bulletproofs); with one term it scales, copies or negates a set; with a = b = 1 it adds two sets element-wise.  The
 * reference has no counterpart.
 * Operands: src_a, src_b and dst are point-set ids of this context (msm_pointset_create; 0 = the default set), any mix of equal
 *   and different ids.  src_b < 0: no second term, D[i] = a * A[a_lo + i] (b and b_lo are ignored).  The CURRENT set
 *   (msm_pointset_select) is not changed by the call.
 * Scalars: a and b are host values, 32 bytes little-endian, < q.  A value >= q fails with MSM_ERR_SCALAR: there is no silent
 *   reduction, which on the curves with a cofactor would change the result for points outside the subgroup.  Both scalars are
 *   the same for every point, so the host recodes them once into a short program of doublings and additions that every lane
 *   walks (Weierstrass curves: the endomorphism split and non-adjacent forms, at most 128 doublings; the Edwards curve: up to
 *   251).  The scalars 0, 1 and q - 1 are ordinary input and cost no multiplication: 0 drops the term, 1 adds the row as it is,
 *   q - 1 adds its negative.  a = 1 with src_b < 0 is a copy; a = b = 0 gives `count` identity rows.
 * Result rows are bit-identical to what msm_set_points writes for the same affine points (canonical Montgomery x and y, and the
 *   beta x line on the Weierstrass curves); the identity takes the identity row of msm_set_points (the Edwards curve: the row of
 *   (0, 1)).  Every later call on dst works unchanged: msm_run with and without the endomorphism, msm_get_points(_ex),
 *   msm_validate_points, msm_precompute.
 * Every input is handled: source rows that are the identity, A[i] and B[i] equal or opposite, a sum that is the identity, an
 *   accumulator that passes through the identity or meets its addend on the way -- next to ordinary points in one wave.
 * Points outside the prime-order subgroup: the Weierstrass path uses the endomorphism, and 1 and q - 1 are taken as +-1 on every
 *   curve, so -- as for msm_run with the endomorphism -- the result is a * A + b * B only for points of the subgroup
 *   (phi(T) != lambda T for a torsion point T).
 * Replacement: dst is replaced as by msm_set_points -- its window tables are dropped, the range-table candidate is reset, its
 *   size becomes `count`.  Window tables of OTHER sets, the sources included, are untouched.
 * In place: dst may be one of the sources.  A source range inside dst must then be either its rows [0, count) -- lane i reads
 *   and writes row i only -- or lie entirely at or above row `count`, disjoint from the rows written; both at once is the fold
 *   (src_a = src_b = dst, a_lo = 0, b_lo = count).  Any other overlap fails with MSM_ERR_ARG.  No new row buffer is allocated
 *   in place (a 2^26-point set is 17 GB): the set is truncated to `count`.  A dst that is not a source gets room for `count`
 *   rows as msm_set_points gives it.
 * Errors: all checks run before anything is written, so a failed call leaves every set as it was and the context usable.
 *   MSM_ERR_ARG: an id that does not name a live set, a null `a`, a null `b` with src_b >= 0, a device-list context,
 *   count >= 2^30, a forbidden overlap.  MSM_ERR_NO_POINTS: a source range that ends beyond its set's size.  MSM_ERR_SCALAR:
 *   a scalar >= q.  count == 0 is valid and leaves dst empty.  The call returns when the rows are written. */
int msm_points_lincomb(msm_ctx* ctx, int32_t src_a, uint64_t a_lo, const uint8_t* a /* 32 B LE */, int32_t src_b, uint64_t b_lo,
                       const uint8_t* b /* 32 B LE; ignored when src_b < 0 */, uint64_t count, int32_t dst);
/* number of resident points of a point set (ids as msm_pointset_create returns them; 0 = the default set) */
int msm_pointset_size(const msm_ctx* ctx, int32_t id, uint64_t* n_out);

/* Per-row scalar multiplication: D[i] = s[i] * A[a_lo + i] for i < count, written as the rows [0, count) of point set `dst` --
 * every row under its OWN scalar, where msm_points_lincomb takes one scalar for the whole set.  With the vectors of
 * msm_scalars_powers / msm_scalars_inverse it makes a commitment key [tau^i] G, the re-weighted generators y^-i H_i of
 * Bulletproofs, batched ElGamal / Pedersen terms r_i G and r_i P_i, or re-randomises a set row by row, without the scalars or the
 * points leaving the device.  The contract is that of msm_points_lincomb wherever this text does not say otherwise: point-set
 * ids, dst replaced as by msm_set_points (window tables dropped, size `count`), the current set not switched, all checks before
 * anything is written, the call returning when the rows are in place, count == 0 valid.
 * Scalars: `count` x 32-byte little-endian integers in host memory (on_device = 0) or in device memory aligned to 16 bytes
 *   (on_device = 1), the vectors msm_run and msm_scalars_* read.  A value >= q is taken as its residue (msm_run's rule without
 *   msm_opts.strict).  0 gives the identity row, q - 1 the negative of the row.
 * Result rows are bit-identical to what msm_set_points writes for the same affine points, the beta x line included; the identity
 *   takes the identity row (the Edwards curve: the row of (0, 1)).  Every later call works on dst: msm_run with and without the
 *   endomorphism, msm_get_points(_ex), msm_validate_points, msm_precompute, msm_points_lincomb.
 * In place: dst == src is allowed with a_lo == 0 (a lane reads row i and its scalar before its one store of row i; the set is
 *   truncated to `count`) and with a_lo >= count.  Any other overlap is MSM_ERR_ARG.
 * Points outside the prime-order subgroup: the Weierstrass path uses the endomorphism, so -- as for msm_points_lincomb -- the
 *   result is s * P only for points of the subgroup.  A torsion row neither faults nor disturbs its neighbours.
 * How: one lane per row on a fixed grid; the lane reduces and splits its scalar (glv_decompose), recodes both halves into signed
 *   4-bit windows, builds the table 1 P .. 8 P of its row in a device workspace (about 200 MB on BLS12-377 for the default grid
 *   of one round of resident blocks, whatever `count`; it counts against msm_set_workspace_limit, under which the grid shrinks
 *   down to one block) and walks the
 *   windows from the top: 4 doublings and two table additions per window.
 * Errors: MSM_ERR_ARG -- an id that does not name a live set, null `scalars` with count > 0, device scalars not aligned to 16
 *   bytes, a device-list context, count >= 2^30, a forbidden overlap.  MSM_ERR_NO_POINTS -- a source range that ends beyond its
 *   set.  A failed call leaves every set as it was. */
int msm_points_mul(msm_ctx* ctx, int32_t src, uint64_t a_lo, const void* scalars, int on_device, uint64_t count, int32_t dst);
/* The same for ONE base point: D[i] = s[i] * P.  base_xy is x || y in the wire format of msm_set_points (NULL: the curve's
 * generator); it is checked on the host -- a coordinate >= p or a point off the curve is MSM_ERR_POINT -- and the all-zero
 * encoding is the identity, which gives `count` identity rows.  The context keeps one table of rows j 2^(10 k) P (j = 1 .. 512,
 * k over the 13 windows of a scalar half: 1.7 MB on BLS12-377), built by the variable-base kernel itself and cached with the base's
 * bytes: a lane then adds one table row per window and half, no doubling.  A call with another base rebuilds the table;
 * msm_ctx_destroy frees it.  A short call (under 2^10 rows) with a base that is not cached does not build the table and runs
 * the variable-base kernel over a broadcast row instead. */
int msm_points_mul_base(msm_ctx* ctx, const uint8_t* base_xy, const void* scalars, int on_device, uint64_t count, int32_t dst);

/* The number-theoretic transform over POINTS: with n = 2^log2n and A = the rows [a_lo, a_lo + n) of point set `src`,
 *   forward:  D[k] = sum_j (shift omega^k)^j A[j]
 *   inverse:  the exact inverse map (the factors n^-1 and shift^-j included)
 * natural order in and out, written as the rows [0, n) of point set `dst`, which then holds exactly n points.  inverse = 1 over
 * the monomial commitment key [tau^j] G gives the key in the Lagrange basis, [L_k(tau)] G on <omega> (PLONK / Halo2's
 * g_lagrange, gnark's ToLagrangeG1, EIP-4844's setup) -- tau is unknown, so the transform has to run over the group elements --
 * and an msm_run over EVALUATIONS on that key commits to the polynomial msm_scalars_ntt would interpolate.  On a coset the two
 * maps part: the evaluations are M f with M[k][j] = (shift omega^k)^j, the key that commits to them is the TRANSPOSE inverse
 * (M^T)^-1 A, and M is symmetric only for shift = 1.  The Lagrange key of the coset shift <omega> is therefore n^-1 times the
 * FORWARD transform under omega^-1 and shift^-1 -- row k = n^-1 sum_j (shift omega^k)^-j A[j] = [L_k(tau)] G -- the factor n^-1
 * being one msm_points_lincomb; inverse = 1 with a shift is the inverse of the forward map, which is what a round trip needs.
 * The reference has no counterpart.  The contract is that of msm_points_mul and msm_scalars_ntt wherever this text does not say
 * otherwise: point-set ids, dst replaced as by msm_set_points (window tables dropped, range candidate reset, size n), the
 * current set not switched, all checks before anything is written, the call returning when the rows are in place.
 * Single-device contexts only.
 * omega, shift: the rules of msm_scalars_ntt.  omega NULL is the library's root (msm_scalars_root_of_unity); the host checks
 *   omega^(n/2) = q - 1 for n >= 2 and fails with MSM_ERR_ARG and a message about the order otherwise; a value >= q is
 *   MSM_ERR_SCALAR; a shift of 0 is MSM_ERR_ARG.  For n = 1 omega is ignored and the call is a copy.
 * Limits: log2n above msm_scalars_ntt_max_log2n is MSM_ERR_ARG: Grumpkin and Ed-on-BLS12-377 accept log2n <= 1 only, which is
 *   the correct answer for those fields.  A source range that ends beyond its set is MSM_ERR_NO_POINTS.
 * In place: dst == src is allowed with a_lo == 0 (the set is truncated to n) and with a_lo >= n; any other overlap is
 *   MSM_ERR_ARG.  The in-place form allocates no second row buffer.
 * Result rows are bit-identical to what msm_set_points writes for the same affine points, the beta x line included; the identity
 *   takes the identity row.  Every later call works on dst: msm_run with and without the endomorphism, msm_precompute,
 *   msm_get_points(_ex), msm_points_*.  Identity rows, equal rows and a butterfly whose two terms are equal or opposite are
 *   ordinary input.
 * Points outside the prime-order subgroup: the Weierstrass path uses the endomorphism, so the result is the transform only for
 *   rows of the subgroup.  A torsion row neither faults nor disturbs the rows of other butterflies; it does spread to every
 *   output, as the mathematics says.
 * How: radix 2, decimation in time, in place in dst: a bit reversal of the rows (a gather, or pairwise swaps in place), then one
 *   launch per stage of n / 2 butterflies (A, B) -> (A + w B, A - w B) on the fixed grid of msm_points_mul.  A lane computes w B
 *   with that call's walk (in its per-lane table workspace, which counts against msm_set_workspace_limit), adds the affine row A
 *   onto +-(w B) and takes both sums to affine with one inversion.  Butterflies with w = 1 skip the walk: stage 1 has no
 *   multiplication, and an unshifted forward transform does (n / 2)(log2n - 2) + 1 of them in all.  A forward shift other than 1
 *   costs one msm_points_mul pass over the powers of shift before the stages, the inverse one over n^-1 shift^-j after them.
 * Device memory beyond the rows, owned by the context and freed with it: the vector omega^j (inverse: omega^-j), j < n / 2, 16 n
 *   bytes, of one (log2n, omega, direction) at a time -- a second call with the same triple builds nothing -- and, for a coset or
 *   an inverse, 32 n bytes of scalars. */
int msm_points_ntt(msm_ctx* ctx, int32_t src, uint64_t a_lo, uint32_t log2n,
                   const uint8_t* omega /* 32 B LE, NULL = the library's root */,
                   const uint8_t* shift /* 32 B LE, NULL = 1 */, int inverse, int32_t dst);

/* Window-sharded form for multi-GPU runs: computes the partition sums P_k for k in [k_lo, k_hi)
 * only (src/msm-batched-affine.ts:42 "P_k = sum_l l * B_(k,l)") and writes them as
 * (k_hi - k_lo) x 144 bytes: X || Y || Z homogeneous projective, 48-byte little-endian canonical
 * integers (twisted Edwards: the extended point without T, which msm_combine rebuilds from T Z = X Y).
 * Ranks exchange these with one all-gather; msm_combine finishes.  With msm_opts.merged_sums the slots may come back merged
 * (first slot: sum_k 2^(c (k - k_lo)) P_k, the others the identity), which either combine takes unchanged, and the call may run
 * on window tables (msm_result.tables says whether it did).
 * k_lo == k_hi == 0 asks for all K windows: partials_out then takes K x 144 bytes, K as msm_plan reports it for the same n and
 * opts (merged_sums and point_lo included) in the same state of the context; a shard [k_lo, k_hi) is cut from that K too.
 * With opts->c == 0 a merged_sums call runs under that plan whether the tables it names exist yet or not: the call that comes
 * before the build takes the plain path under the tables' window, so msm_result.c / K never differ from msm_plan's answer and
 * do not change from one call over a range to the next. */
int msm_window_sums(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts,
                    uint8_t* partials_out, msm_result* stats);

/* msm_run on a multi-device context with the scalars already PLACED: dev_scalars[d] is a device pointer on devices[d]
 * holding the n_d x 32 bytes of that device's points [n d / G, n (d + 1) / G) (points split), so no peer copy happens
 * inside the call.  On a single-device context dev_scalars[0] is the whole scalar array. */
int msm_run_placed(msm_ctx* ctx, const void* const* dev_scalars, uint64_t n, const msm_opts* opts, msm_result* out);

/* S = sum_k 2^(c k) P_k over all K windows, then to affine (src/msm-batched-affine.ts:322-333,
 * src/curve-projective.ts:335-349).  Host arithmetic only: `ctx` may be NULL. */
int msm_combine(msm_ctx* ctx, const uint8_t* partials, int32_t K, int32_t c, msm_result* out);
/* The same without a context: `curve` names the constants.  No GPU is touched. */
int msm_combine_curve(int curve, const uint8_t* partials, int32_t K, int32_t c, msm_result* out);
/* Points-split runs: `partials` holds G groups of K window sums (group g = the sums of the g-th share of the points, as
 * msm_window_sums wrote them); P_k = sum over the groups, then as msm_combine_curve. */
int msm_combine_groups(int curve, const uint8_t* partials, int32_t G, int32_t K, int32_t c, msm_result* out);

/* Window plan for n points: the c the library would pick (opts->c forces one) and the resulting K (see msm_opts.c).  It is the
 * plan of msm_run over DEVICE-RESIDENT scalars: over the whole current point set that is the plan on window tables where they
 * exist or would be built (opts->no_tables: the plain plan, which msm_window_sums without merged_sums and bucket-range shards run;
 * opts->merged_sums: the plan of msm_window_sums(merged_sums) -- and of msm_run -- over the range [point_lo, point_lo + n), on its
 * tables where they fit).  The answer is the plan of the very next such call and of every call after it: it does not depend on
 * whether the tables have been built yet.  Only a change of the context's state moves it -- new points or another point set,
 * msm_set_tables_limit, msm_precompute, or tables of the whole set taking the place of a range's (see msm_precompute).
 * Host scalars of 2^24 points and more cross PCIe behind the computation: msm_run then runs whole MSMs over growing ranges of
 * the points, each under the plan of ITS size, and msm_result reports the plan of the last, biggest range. */
int msm_plan(const msm_ctx* ctx, uint64_t n, const msm_opts* opts, int32_t* c_out, int32_t* K_out);

/* Synthetic inputs generated on the GPU (randomPointsFast / randomScalars, src/curve-random.ts):
 * n resident points P_i = a_i * G and, if `a_out` is non-null, the n scalars a_i (32-byte LE) so a
 * caller can verify sum s_i P_i = (sum s_i a_i) G in O(n). */
int msm_generate_points(msm_ctx* ctx, uint64_t n, uint64_t seed, uint8_t* a_out);
/* n uniformly random scalars < q (`randomScalars`, src/curve-random.ts:151-194) into `dev_dst`, a caller-owned device buffer
 * of n * 32 bytes (msm_device_alloc, or any device allocation of the caller), and / or into `host_out` (n * 32 bytes).
 * Either may be NULL, not both. */
int msm_generate_scalars(msm_ctx* ctx, uint64_t n, uint64_t seed, void* dev_dst, uint8_t* host_out);

/* Read resident points [first, first + count) back in wire format (tests, CPU-baseline sampling). */
int msm_get_points(msm_ctx* ctx, uint64_t first, uint64_t count, uint8_t* out_xy);

/* ---- fine-grained GPU operators for parity tests (debug surface) ----
 * Coordinates are the curve's ABI width: 48-byte little-endian integers for BLS12-377 / BLS12-381, 32-byte ones for Pallas and
 * Ed-on-BLS12-377 ("48-byte" / "96-byte" below stand for one / two coordinates of that width). */
enum { MSM_OP_MUL = 0, MSM_OP_SQR = 1, MSM_OP_ADD = 2, MSM_OP_SUB = 3, MSM_OP_INV = 4,
       MSM_OP_TO_MONT = 5, MSM_OP_FROM_MONT = 6,
       MSM_OP_INV_FERMAT = 7,   /* a^(p-2): the cross-check of MSM_OP_INV (division steps) */
       MSM_OP_INV_KALISKI = 8,  /* the reference's almost-inverse, src/wasm/inverse.ts:136-218 */
       MSM_OP_INV_WORDSLICED = 9 /* the reference's experimental word-sliced almost-inverse, src/inverse/faster-inverse-wasm.ts:133-343 */ };
/* element-wise base-field op on n operands, each a 48-byte (32 for Ed) little-endian word string;
 * MUL/SQR/ADD/SUB/INV act on Montgomery-form operands (radix 2^390 / 2^270) and return canonical
 * Montgomery-form values, i.e. `multiply`, `square`, `add`, `subtract`, `inverse` of
 * src/field-msm.ts:86-123. */
int msm_test_fp(msm_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, uint64_t n);
/* `batchInverse` (src/wasm/inverse.ts:220-271): n Montgomery-form elements (48-byte words, non-zero) inverted with
 * one field inversion per `per_lane` consecutive elements (Montgomery's trick). */
int msm_test_batch_inverse(msm_ctx* ctx, const uint8_t* xs, uint8_t* out, uint64_t n, uint32_t per_lane);
/* GLV `decompose` (src/wasm/glv.ts:68-169) of n 32-byte scalars: out = n x 40 bytes
 * |s0| (16 B LE) || |s1| (16 B LE) || neg0 (u32) || neg1 (u32). */
int msm_test_glv(msm_ctx* ctx, const uint8_t* scalars, uint8_t* out, uint64_t n);
/* affine pair additions G_i + H_i through the batched-affine kernel (batchAddNew,
 * src/curve-affine.ts:376-458): inputs n x 96-byte wire points, output n x 96 bytes.  Ed-on-BLS12-377: the
 * unified extended addition of the gather round (src/curve-twisted-edwards.ts:84-165), n x 64 bytes each way. */
int msm_test_batch_add(msm_ctx* ctx, const uint8_t* g, const uint8_t* h, uint8_t* out, uint64_t n);

/* ---- worst-case / operator-level surface (round 2) ---- */
/* fe_mul / fe_sqr on RAW register-form operands: n x NL 30-bit limbs as uint32 (NL = 13; Ed-on-BLS12-377: 9), exactly as
 * given -- unreduced values up to the documented 2^6 p, all-ones limbs -- and the result limbs as they leave the
 * multiplier (not reduced).  op = MSM_OP_MUL or MSM_OP_SQR.  Mirrors src/field.test.ts:27-155 on [0, 2p) and beyond. */
int msm_test_fp_raw(msm_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n);
/* curve operators, one per element: Weierstrass curves take and return homogeneous projective points n x (X || Y || Z),
 * 48-byte little-endian integers < p (any representative; Z = 0 is the identity); Ed-on-BLS12-377 extended points
 * n x (X || Y || Z || T) of 32 bytes.  op 0: general addition with every edge case (proj_add / te_add, 9M form),
 * 1: doubling of P, 2 (Weierstrass): mixed addition, Q affine with (0, 0) the identity.
 * src/curve-projective.test.ts:77-208, src/curve-twisted-edwards.test.ts:55-158. */
enum { MSM_CURVE_OP_ADD = 0, MSM_CURVE_OP_DOUBLE = 1, MSM_CURVE_OP_ADD_MIXED = 2 };
int msm_test_curve_op(msm_ctx* ctx, int op, const uint8_t* p, const uint8_t* q, uint8_t* out, uint64_t n);
/* msm_test_batch_add through the plane-reading modes of the tree kernel with a chosen number of pairs per lane (= per
 * shared inversion): mode 1 = regular rounds, 2 = tail rounds (operand descriptors; an all-zero H_e is passed as
 * "no second operand").  steps >= 1. */
int msm_test_batch_add_mode(msm_ctx* ctx, const uint8_t* g, const uint8_t* h, uint8_t* out, uint64_t n, int mode, uint32_t steps);
/* Bucket reduction alone (Weierstrass curves): buckets = K x L affine points (x || y, 48-byte LE; (0, 0) = empty bucket),
 * bucket l of window k at index k L + l - 1; L a power of two.  Writes P_k = sum_l l B_(k,l) as K x 144 bytes (X || Y || Z)
 * and the device time of the reduction in *ms_out.
 *   mode 0: as the MSM does it -- bucket finish, then projective row / triangle sums per chunk of buckets and bit-sliced weights
 *           (reduceBucketsColumnProjective, src/msm-batched-affine.ts:556-583);
 *   mode 1: the all-affine reduction of the reference's single-thread MSM (reduceBucketsAffine,
 *           src/msm-batched-affine-single-thread.ts:522-667, doc/zprize22.md:317-358) out of in-place batched-affine
 *           additions and doublings; 2^c0 = buckets per chunk of its linear part.  SURVEY section 8(f)-3. */
int msm_test_bucket_reduce(msm_ctx* ctx, const uint8_t* buckets, int32_t K, uint32_t L, int mode, int c0, uint8_t* partials_out,
                           float* ms_out);
/* The end of every MSM on buckets of the caller, all curves: the bucket finish (k_finish_hist / k_finish_perm, k_bucket_finish or
 * k_te_bucket_finish) as the accumulation tree runs it, then the bucket reduction of the pipeline on its output.
 *   pool   n_pool affine wire points (x || y, one coordinate width each); (0, 0) is the identity on the Weierstrass curves,
 *          (0, 1) on the Edwards curve
 *   off    K L + 1 ascending offsets, off[0] = 0; elems: off[K L] pool indices.  Bucket l (1-based) of window k holds the
 *          elements elems[off[k L + l - 1]] .. elems[off[k L + l] - 1]; L a power of two
 *   merged, stride   as a full MSM asks for them: merged != 0 lets the call hand back sum_k 2^(stride k) P_k in slot 0 and the
 *          identity in the other slots (the contract is that sum_k 2^(stride k) slot_k is that sum); stride = bits a window
 *          advances by, 0 = log2(L) + 1; stride = log2(L) is the plan with a folded top window
 *   tc     buckets per lane of the reduction: 0 = the library's rule, else a power of two in 2 .. 32
 * Writes K x 144 bytes (X || Y || Z; Z = 0: the identity of a Weierstrass curve), without merged P_k = sum_l l B_(k,l).
 * perm_out (may be NULL): K L words, the order in which the finish took the buckets -- descending by element count, counts
 * from 63 up alike -- or 0, 1, 2, ... where it did not order them (fewer than 4096 buckets). */
int msm_test_bucket_sums(msm_ctx* ctx, const uint8_t* pool, uint64_t n_pool, const uint32_t* off, const uint32_t* elems, int32_t K,
                         uint32_t L, int merged, int stride, uint32_t tc, uint8_t* sums_out, uint32_t* perm_out);
/* The sort path of a window group -- which of the forms of the sort and of round 1 of the accumulation tree it took:
 *   ONE_LEVEL  a window's counters fit the LDS and the input is small
 *   RADIX      the radix split (an input whose largest bucket is `heavy` still takes the one-level scatter as its last pass)
 *   SLOTS      the bin split, round 1 over bucket-ordered padded slots (k_bin_slots), results as planes
 *   PAIRS      the bin split, round 1 over the tile-ordered pairs of k_bin_pairs, results as 64-byte element records that
 *              round 2 reads back ("pair form") */
enum { MSM_SORT_ONE_LEVEL = 0, MSM_SORT_RADIX = 1, MSM_SORT_SLOTS = 2, MSM_SORT_PAIRS = 3 };
/* The pair form is taken by big windows (c >= 18, buckets deep enough for two index-free rounds) over MORE than 2^log2_rows
 * rows of the point table or of the window tables a group reads.  The default, 23, is a measured break-even; this entry moves
 * it for the context, so that tests reach the pair form -- through the pipeline's own host code -- at sizes of a few seconds.
 * log2_rows: 1 .. 40, or 0 to restore the default.  Results do not depend on it.  Refused on a device-list context. */
int msm_test_set_chunk_rows_log(msm_ctx* ctx, int32_t log2_rows);
/* The sort paths (MSM_SORT_*) of the window groups of the last msm_run, msm_run_narrow, msm_run_indexed(_narrow), msm_run_placed
 * or msm_window_sums on this context, one per group in the order of the call's schedule; none (count 0) after a call that failed or a fused batch: writes
 * min(count, cap) of them to `out` (may be NULL with cap = 0) and returns the count, or -1 for a null or device-list context. */
int msm_test_last_sort_paths(msm_ctx* ctx, int32_t* out, int cap);
/* msm_scalars_ntt cuts its log2n stages into ceil(log2n / tile_log) passes of at most tile_log stages, one launch each.  This
 * entry moves tile_log for the context, so that tests reach plans of several passes, ragged ones included, at n <= 2^12 through
 * the library's own host code.  tile_log: 1 .. 10 (the kernel's maximum), or 0 to restore the default (9).  Results do not depend
 * on it.  Refused on a device-list context. */
int msm_test_set_ntt_tile_log(msm_ctx* ctx, int32_t tile_log);
/* The stages per pass of the last msm_scalars_ntt on this context, in the order the passes ran; none (count 0) after a call that
 * failed or a transform of one element: writes min(count, cap) of them to `stages_out` (may be NULL with cap = 0) and returns
 * the count, or -1 for a null or device-list context. */
int msm_test_last_ntt_plan(msm_ctx* ctx, int32_t* stages_out, int cap);
/* msm_scalars_scan and msm_scalars_div_linear run over tiles of 2^tile_log elements and scan the tiles' aggregates the same way,
 * level by level.  This entry moves tile_log for the context, so that tests reach plans of three levels at 65 537 elements through
 * the library's own host code.  tile_log: 8 (one element per lane) .. 10 (the default), or 0 to restore the default.  Results do
 * not depend on it.  Refused on a device-list context. */
/* msm_points_mul runs on a fixed grid of 256-lane blocks with a grid-stride loop over the rows.  This entry sets the number of
 * blocks for the context (0: the default, as many as stay resident at once and no more than the rows need), so that 321 rows under one block
 * make every lane take two rows and rebuild its table slots.  Results do not depend on it.  Refused on a device-list context. */
int msm_test_set_points_mul_grid(msm_ctx* ctx, int32_t blocks);
/* The path of msm_points_mul_base: 0 = automatic, 1 = always the table, 2 = always the broadcast row through the variable-base
 * kernel.  Results do not depend on it.  Refused on a device-list context. */
int msm_test_set_points_mul_base_path(msm_ctx* ctx, int32_t path);
/* The shape of the last msm_points_mul / msm_points_mul_base of the context, four words: blocks of the grid that wrote the rows
 * (0: no launch), window bits, path (0 = msm_points_mul, 1 = table, 2 = broadcast) and rows of the fixed-base table used (0:
 * none).  Writes min(4, cap) of them and returns 4, or -1 for a null or device-list context. */
int msm_test_last_points_mul(msm_ctx* ctx, int32_t* out, int cap);
/* The stages of msm_points_ntt run on a fixed grid of 256-lane blocks with a grid-stride loop over the butterflies.  This entry
 * sets the number of blocks for the context (0: the default, as many as stay resident at once and no more than the butterflies
 * need), so that 512 butterflies under one block make every lane take two and rebuild its table slots.  Results do not depend on
 * it.  Refused on a device-list context. */
int msm_test_set_points_ntt_grid(msm_ctx* ctx, int32_t blocks);
/* The plan of the last msm_points_ntt of the context, seven words: log2n, butterfly launches, blocks of their grid, how many of
 * those launches were multiplication-free, whether a pass of pre-scaling (a forward shift) ran, whether a pass of post-scaling
 * (the inverse's n^-1 shift^-j) ran, and the butterflies planned with a twiddle other than 1 (capped at 2^31 - 1); all 0 after
 * a refused call.  Writes min(7, cap) of them and returns 7, or -1 for a null or device-list context. */
int msm_test_last_points_ntt(msm_ctx* ctx, int32_t* out, int cap);
int msm_test_set_scan_tile_log(msm_ctx* ctx, int32_t tile_log);
/* The tiles per level of the last msm_scalars_scan or msm_scalars_div_linear on this context, bottom level first (the last entry
 * is 1); none (count 0) after a call that was refused or had n == 0: writes min(count, cap) of them to `tiles_out` (may be NULL
 * with cap = 0) and returns the count, or -1 for a null or device-list context. */
int msm_test_last_scan_plan(msm_ctx* ctx, int32_t* tiles_out, int cap);
/* msm_scalars_sumcheck_round runs on a grid of 256-lane blocks with a grid-stride loop over the pairs, one partial per block and
 * value.  This entry sets the number of blocks for the context (1 .. 1024, or 0: the default, one lane per pair up to 1024
 * blocks), so that 2^11 elements under one block give every lane four pairs and under three blocks a ragged second stride.
 * Results do not depend on it.  Refused on a device-list context. */
int msm_test_set_sumcheck_grid(msm_ctx* ctx, int32_t blocks);
/* The shape of the last sumcheck calls of the context, four words: blocks of the last round's grid, its pairs, its values d + 1
 * (all 0 before the first round and after a refused one), and the split k of the last msm_scalars_eq (the variables of its low
 * half-table; -1 before the first and after a refused one).  Writes min(4, cap) of them and returns 4, or -1 for a null or
 * device-list context. */
int msm_test_last_sumcheck(msm_ctx* ctx, int32_t* out, int cap);
/* msm_matrix_create splits the rows of a matrix by two thresholds: a row of at most short_max entries is summed by one lane, a
 * longer one is cut into parts of at most part_len entries, one wave each.  This entry sets both for the matrices the context
 * creates AFTERWARDS (0: the default of that threshold), so that a ladder of row lengths crosses them at small sizes.  Results do
 * not depend on them.  Refused on a device-list context. */
int msm_test_set_matvec_geometry(msm_ctx* ctx, uint32_t short_max, uint32_t part_len);
/* The shape of the last msm_scalars_matvec of the context, five words: short_max and part_len of its matrix, its long rows, their
 * parts, and the launches of the call (all 0 after a refused one).  Writes min(5, cap) of them and returns 5, or -1 for a null or
 * device-list context. */
int msm_test_last_matvec(msm_ctx* ctx, int32_t* out, int cap);
/* The device buffers the library holds in this process, over all contexts: how many are live and their bytes as allocated (a
 * buffer is allocated with some slack over what was asked of it).  Every one belongs to a context, a point set, a matrix or a
 * running call and goes back with its owner, so the two figures return to what they were when a context is destroyed and
 * after a call that failed: (0, 0) in a process without a context.  Takes no context; MSM_ERR_ARG, and nothing written, if either
 * pointer is null. */
int msm_test_live_buffers(uint64_t* count_out, uint64_t* bytes_out);
/* The first step of every MSM alone: the window digits of a call's scalars, from the digit kernel the call would launch
 * (k_digits, k_te_digits, k_digits_narrow<W>, k_te_digits_narrow<W>; B >= 2: their _batch forms), through the pipeline's own
 * launch code and geometry, and nothing behind it -- nothing sorts the digits, so a wrong one is a wrong word in digits_out and
 * never a bucket index.  Needs no resident points.
 *   scalars   B host arrays of n_array scalars each; the call's scalars are the elements [first, first + n) (what a range of
 *             the points of a bigger call sees: a narrow range may start inside the dword a lane loads)
 *   width_bytes, bits, is_signed   the narrow format of msm_run_narrow, bits resolved the same way; width_bytes = 0: 32-byte
 *             scalars (bits and is_signed are then ignored)
 *   opts      c, no_glv, strict, bucket_shard, bucket_shards as msm_window_sums reads them.  A narrow call and a batch refuse
 *             shard options as msm_run_narrow and msm_run_batch do (MSM_ERR_ARG): bucket shards, and k_lo / k_hi of opts, which
 *             a call of 32-byte scalars does not read
 *   k_lo, k_hi   the windows [k_lo, k_hi) of the plan's K; 0, 0 = all
 *   B >= 2    the fused batch of msm_run_batch(_narrow): host elements staged 16 bytes apart as there; opts->c must be set,
 *             first = 0, n_array = n, all windows, no shard; at most 16 elements, 64 narrow ones.  Unlike the real call, which
 *             fuses only under the one-level sort, any window the plan accepts is run, a folded plan included.
 * digits_out = NULL: only the plan is made and reported (c_out, K_out, fold_out), from which a caller sizes digits_out.
 * digits_out: (k_hi - k_lo) rows of 2 n words (Ed-on-BLS12-377: n words) -- on a Weierstrass curve word 2 i is the digit of
 * scalar i (with the endomorphism: of its first half), word 2 i + 1 that of the second half or 0; a word is magnitude |
 * sign << 31, 0 = no entry.  B >= 2: B K rows, row b K + k = window k of element b.
 * c_out, K_out, fold_out (may be NULL): the plan; fold = the top window is c + 1 bits wide (msm_plan).
 * Returns MSM_ERR_ARG where the real call refuses the plan or the format.  Otherwise MSM_OK with the digits, and in
 * *flags_rc_out what the real call returns for the error word the kernel left: MSM_OK, MSM_ERR_SCALAR (a scalar >= q under
 * opts->strict, a narrow value outside its range -- such a value counts as 0) or MSM_ERR_INTERNAL (a folded top window had to
 * be clamped). */
int msm_test_digits(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, uint64_t n_array, uint64_t first,
                    int32_t width_bytes, int32_t bits, int32_t is_signed, const msm_opts* opts, int32_t k_lo, int32_t k_hi,
                    uint32_t* digits_out, int32_t* c_out, int32_t* K_out, int32_t* fold_out, int32_t* flags_rc_out);
/* The stage between "sorted" and "finished" on buckets of the caller, all curves: the scans behind the sort (k_bucket_max,
 * k_pscan_partial / _top / _final), the host's round plan and every round of the accumulation tree in their real order on the
 * real buffers (accumulate_window_group itself: gather round 1 over padded slots, regular rounds, k_tail_desc and the search
 * rounds, the bucket finish), then the bucket reduction.  Runs on workspace 0; the resident points are not touched.
 *   pool, off, elems, K, L   as msm_test_bucket_sums (L = 1 allowed)
 *   flags  one byte per element, or NULL: bit 0 negates the point, bit 1 takes the beta x line of its row (the endomorphism
 *          image, of discrete log lambda d).  Every Weierstrass curve of this library carries that line; the Edwards curve has
 *          none and refuses bit 1.
 *   c      selects the threshold class only: FINISH_MAX and the smallest tail round worth a launch, as the tree derives them
 *          from the plan's window (c >= 18 or below); 1 .. 24
 *   logG   buckets are padded to multiples of 2^logG slots and take logG regular rounds; 1 .. 10, what the sort can ask for
 *   reported_max   0: k_bucket_max finds the largest bucket.  Otherwise a value >= the largest bucket that stands in its place,
 *          as the count pass of the pair form over-reports it: RT grows, the sums do not change.
 * Writes K x 144 bytes to sums_out (X || Y || Z as msm_test_bucket_sums, never merged) and the plan that ran:
 *   plan_out      8 words: RT, r_stop (tail rounds run), total padded slots, the largest bucket as reported, rounds and n_pairs
 *                 as msm_result counts them, launched rounds, 0
 *   cursor_out    (may be NULL) K L + 1 words: the slot every bucket starts at, [K L] = the total
 *   tail_off_out  (may be NULL) min(RT + 1, tail_tables_cap) tables of K L + 1 words: table r = offsets of the elements every
 *                 bucket holds after r tail rounds
 *   round_log_out (may be NULL with round_log_cap = 0) per launched round, at most round_log_cap: mode (0 gather, 1 regular,
 *                 2 search), n_out, steps (pairs per lane)
 * The slots are written on the host from the device's cursor.  Scans whose total or cursor would leave the padded slots end the
 * call with MSM_ERR_INTERNAL before any round runs (plan_out[0], [2], [3] and the two tables are written by then).
 * MSM_ERR_ARG, the context staying usable: a device-list context, offsets that do not start at 0 or do not ascend, an element
 * outside the pool, a flag the curve has no line for, logG or c outside their range, reported_max below the largest bucket,
 * 2^31 padded slots or more, and the sizes msm_test_bucket_sums refuses. */
int msm_test_tree_sums(msm_ctx* ctx, const uint8_t* pool, uint64_t n_pool, const uint32_t* off, const uint32_t* elems,
                       const uint8_t* flags, int32_t K, uint32_t L, int32_t c, uint32_t logG, uint32_t reported_max, uint8_t* sums_out,
                       uint64_t* plan_out, uint32_t* cursor_out, uint32_t* tail_off_out, uint32_t tail_tables_cap,
                       uint64_t* round_log_out, uint32_t round_log_cap);

#ifdef __cplusplus
}
#endif
#endif /* MSM_HIP_H */
