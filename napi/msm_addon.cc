// Node N-API shim over the C ABI of libmsm_hip.so (include/msm_hip.h).
//
// This is the "thin Node N-API C-ABI shim into HIP" that replaces the reference's wasm backend for
// the MSM path: the JS facade in js/montgomery-hip.js rebuilds the reference's
// `Curve.Parallel.{pointsFromBytes, scalarsFromBytes, msm, msmUnsafe}` (src/parallel.ts:135-145) and
// `compute_msm` (scripts/zprize23/submission-bls377.ts:20-65) on top of the functions exported here.
// Plain N-API (C), version 8 as shipped with the image's node 12; no node-addon-api / node-gyp.
//
// Exports: createContext(curve, device | [devices]) -> external handle, destroyContext(h), setPoints(h, Buffer, pointBytes, check),
//          pointsetCreate(h) -> id, pointsetSelect(h, id), pointsetDestroy(h, id),
//          msm(h, Buffer scalars, c, coordBytes, noGlv, unsafe) -> {x: Buffer, y: Buffer, isZero, c, K, phaseMs: number[8], nPairs},
//          deviceAlloc(h, bytes) -> device buffer handle, deviceUpload(h, dbuf, Buffer), deviceFree(h, dbuf),
//          msmDevice(h, dbuf, n, c, noGlv, unsafe) -> as msm: the scalars already sit in HBM (the reference keeps them in the
//          memory its kernels compute in, src/parallel.ts:119-133, scripts/msm-weierstrass.ts:29-32),
//          msmBatch(h, [Buffer scalars], c, noGlv, unsafe) / msmBatchDevice(h, [dbuf], n, c, noGlv, unsafe) -> array of results as
//          msm's: many MSMs over the same points in one call (msm_run_batch),
//          msmNarrow(h, Buffer scalars, width, bits, signed, c) -> as msm: narrow scalars (msm_run_narrow) -- width 1, 2, 4, 8, 16
//          bytes per scalar, or 32 for field elements holding small values; bits 0 = all the width gives,
//          msmBatchNarrow(h, [Buffer], width, bits, signed, c) -> array of results (msm_run_batch_narrow),
//          scalarBits(h, Buffer of n x 32 bytes) -> {unsigned, signed} (msm_scalar_bits),
//          msmIndexed(h, Buffer scalars of m x 32 bytes, Buffer indices of m x 4 bytes (uint32 LE), c, noGlv) -> as msm:
//          sum_j scalars[j] * P[indices[j]] (msm_run_indexed); an index >= the resident count throws (msm error 1, the position
//          in the message), msmIndexedNarrow(h, Buffer scalars, Buffer indices, width, bits, signed, c) (msm_run_indexed_narrow),
//          pointsMul(h, src, aLo, scalars, sOff, count, dst) -> count: rows [0, count) of point set dst = s[i] * A[aLo + i]
//          (msm_points_mul); scalars: a Buffer of >= count x 32 host bytes (sOff ignored) or a device buffer whose elements
//          [sOff, sOff + count) are the scalars; pointsMulBase(h, Buffer base (x || y) | null, scalars, sOff, count, dst) -> count
//          (msm_points_mul_base; null: the generator),
//          pointsNtt(h, src, aLo, log2n, omega | null, shift | null, inverse, dst) -> n: rows [0, n) of point set dst = the transform
//          of the n = 2^log2n rows [aLo, aLo + n) of point set src (msm_points_ntt; omega, shift: Buffers of 32 bytes),
//          pointsLincomb(h, srcA, aLo, Buffer a of 32 bytes, srcB (-1: no second term), bLo, Buffer b | null, count, dst) -> count:
//          rows [0, count) of point set dst = a * A[aLo + i] + b * B[bLo + i] (msm_points_lincomb), pointsetSize(h, id) -> n,
//          resident scalar vectors (msm_scalars_*): a vector is a device buffer and an offset in elements of 32 bytes --
//          deviceDownload(h, dbuf, byteOffset, bytes) -> Buffer, scalarsLincomb(h, dst, dstOff, Buffer x, a, aOff, Buffer y | null,
//          b | null, bOff, n): dst[i] = x a[i] + y b[i] mod q, scalarsMul(h, dst, dstOff, a, aOff, b, bOff, n),
//          scalarsInner(h, a, aOff, b, bOff, n) -> Buffer of 32 bytes, scalarsPowers(h, dst, dstOff, Buffer s, Buffer x, n),
//          scalarsNtt(h, dst, dstOff, a, aOff, log2n, batch, Buffer omega | null, Buffer shift | null, inverse) (msm_scalars_ntt),
//          scalarsRootOfUnity(h, log2n) -> Buffer of 32 bytes, scalarsNttMaxLog2n(h) -> number,
//          scalarsScan(h, dst, dstOff, a, aOff, n, op, exclusive, Buffer init | null) -> Buffer total (msm_scalars_scan),
//          scalarsInverse(h, dst, dstOff, a, aOff, n) -> number of zero residues, scalarsDivLinear(h, dst, dstOff, a, aOff, n, z) -> Buffer,
//          the resident sumcheck: a table is a device buffer and an offset in elements --
//          scalarsSumcheckRound(h, [bufs], [offs], log2n, var, shape) -> Buffer of (d + 1) x 32 bytes (msm_scalars_sumcheck_round),
//          scalarsBind(h, [dstBufs], [dstOffs], [srcBufs], [srcOffs], log2n, var, Buffer r) (msm_scalars_bind),
//          scalarsEq(h, dst, dstOff, Buffer r of v x 32 bytes, Buffer s | null) (msm_scalars_eq),
//          resident sparse matrices: matrixCreate(h, rows, cols, Buffer rowPtr, Buffer col, Buffer val | null, flags) -> id (CSR from
//          the host, uint32 LE words and 32-byte coefficients; flags 1: the transposed matrix), matrixDestroy(h, id), matrixInfo(h, id)
//          -> {rows, cols, nnz, bytes}, scalarsMatvec(h, id, dst, dstOff, x | null, xOff, Buffer alpha | null, flags): dst = alpha M x,
//          flags 1: plus the old dst (msm_scalars_matvec); testSetMatvecGeometry(h, shortMax, partLen), testLastMatvec(h) -> [5],
//          plan(h, n, c) -> {c, K}, generatePoints(h, n, seed) -> n, generateScalars(h, n, seed[, dbuf]) -> Buffer | n
//          the fine operator table of the reference's wasm exports (src/field-msm.ts:86-123,190-243, src/scalar-glv.ts:41-51,105-128)
//          over Buffers instead of wasm pointers: fieldOp(h, op, a, b) -> Buffer (msm_test_fp: multiply / square / add / subtract /
//          inverse / toMontgomery / fromMontgomery on n = a.length / coordBytes elements), batchInverse(h, xs, perLane) -> Buffer,
//          glvDecompose(h, scalars) -> Buffer of n x 40 bytes (|s0|, |s1|: 16 bytes each, neg0, neg1: 4 bytes each),
//          batchAdd(h, G, H) -> Buffer of n affine sums (wire points, (0, 0) = identity)
//          setPointsEx(h, Buffer, format, validate) -> n, getPointsEx(h, first, count, format) -> Buffer: compressed points and
//          subgroup validation (msm_set_points_ex / msm_get_points_ex; constants POINTS_* and VALIDATE_*); a refused point
//          throws an Error with its index in the message and in `badIndex`
// The addon is built against include/msm_hip.h and checks at load that the library it found was too (msm_abi_version).
#include <node_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "msm_hip.h"

#define NAPI_OK(call)                                                      \
  do {                                                                     \
    if ((call) != napi_ok) {                                               \
      napi_throw_error(env, NULL, "N-API call failed: " #call);            \
      return NULL;                                                         \
    }                                                                      \
  } while (0)

static napi_value throw_msm(napi_env env, msm_ctx* ctx, int rc, const char* what) {
  char buf[640];
  snprintf(buf, sizeof buf, "%s: msm error %d: %s", what, rc, ctx ? msm_last_error(ctx) : "no context (no usable GPU? there is no CPU fallback)");
  napi_throw_error(env, NULL, buf);
  return NULL;
}

// What a JS context handle points at: the sizes of the curve's wire format are derived here, never taken from JS
// (a wrong size from the caller would make the library read past the Buffer or this shim read past res.x).
typedef struct {
  msm_ctx* ctx;      /* NULL after destroyContext: a second destroy or any later call throws instead of double-freeing */
  int32_t curve;
  size_t coord_bytes, point_bytes;
  uint32_t refs;     /* the JS handle + every live device-buffer handle: the struct outlives whichever is collected last */
} js_ctx;

/* a device buffer of the context (msm_device_alloc): one per scalar pointer of the JS facade */
typedef struct {
  js_ctx* owner;
  void* dev;         /* NULL after deviceFree */
  uint64_t bytes;
} js_dbuf;

static void ctx_unref(js_ctx* h) {
  if (--h->refs == 0) free(h);
}

static js_ctx* get_handle(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, NULL, "expected a context handle from createContext()");
    return NULL;
  }
  js_ctx* h = (js_ctx*)p;
  if (!h->ctx) {
    napi_throw_error(env, NULL, "this context has been destroyed");
    return NULL;
  }
  return h;
}
static msm_ctx* get_ctx(napi_env env, napi_value v) {
  js_ctx* h = get_handle(env, v);
  return h ? h->ctx : NULL;
}
static void finalize_handle(napi_env env, void* data, void* hint) {
  (void)env; (void)hint;
  js_ctx* h = (js_ctx*)data;
  if (h->ctx) msm_ctx_destroy(h->ctx);   /* frees every device buffer the context still holds */
  h->ctx = NULL;
  ctx_unref(h);
}
/* a collected scalar pointer gives its device memory back (if its context is still alive and nobody freed it by hand) */
static void finalize_dbuf(napi_env env, void* data, void* hint) {
  (void)hint;
  js_dbuf* b = (js_dbuf*)data;
  if (b->dev && b->owner->ctx) {
    msm_device_free(b->owner->ctx, b->dev);
    int64_t adj;
    napi_adjust_external_memory(env, -(int64_t)b->bytes, &adj);
  }
  ctx_unref(b->owner);
  free(b);
}
static js_dbuf* get_dbuf(napi_env env, js_ctx* h, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, NULL, "expected a device buffer from deviceAlloc()");
    return NULL;
  }
  js_dbuf* b = (js_dbuf*)p;
  if (b->owner != h || !b->dev) {
    napi_throw_error(env, NULL, b->owner != h ? "this device buffer belongs to another context" : "this device buffer has been freed");
    return NULL;
  }
  return b;
}

static napi_value CreateContext(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t curve = 0, device = 0;
  if (argc > 0) napi_get_value_int32(env, argv[0], &curve);
  msm_ctx* ctx = NULL;
  int rc;
  bool is_array = false;
  if (argc > 1) napi_is_array(env, argv[1], &is_array);
  if (is_array) {   // a device list: one context over several GPUs of the node (msm_ctx_create_multi)
    uint32_t nd = 0;
    NAPI_OK(napi_get_array_length(env, argv[1], &nd));
    if (nd == 0 || nd > 64) {
      napi_throw_range_error(env, NULL, "device list must hold 1..64 device indices");
      return NULL;
    }
    int32_t devs[64];
    for (uint32_t i = 0; i < nd; i++) {
      napi_value e;
      NAPI_OK(napi_get_element(env, argv[1], i, &e));
      NAPI_OK(napi_get_value_int32(env, e, &devs[i]));
    }
    rc = msm_ctx_create_multi(&ctx, curve, devs, (int32_t)nd);
  } else {
    if (argc > 1) napi_get_value_int32(env, argv[1], &device);
    rc = msm_ctx_create(&ctx, curve, device);
  }
  if (rc != MSM_OK) return throw_msm(env, NULL, rc, "createContext");
  js_ctx* h = (js_ctx*)calloc(1, sizeof(js_ctx));
  if (!h) {
    msm_ctx_destroy(ctx);
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  h->ctx = ctx;
  h->refs = 1;
  h->curve = curve;
  h->coord_bytes = (curve == MSM_CURVE_BLS12_377_G1 || curve == MSM_CURVE_BLS12_381_G1) ? 48 : 32;   /* per field */
  h->point_bytes = 2 * h->coord_bytes;
  napi_value out;
  NAPI_OK(napi_create_external(env, h, finalize_handle, NULL, &out));
  return out;
}

static napi_value DestroyContext(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);   // throws on a handle that was destroyed before
  if (h) {
    msm_ctx_destroy(h->ctx);
    h->ctx = NULL;
  }
  return NULL;
}

static napi_value SetPoints(napi_env env, napi_callback_info info) {  // pointsFromBytes, src/parallel.ts:97-116
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  msm_ctx* ctx = h->ctx;
  void* data;
  size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &data, &len));
  int32_t point_bytes = (int32_t)h->point_bytes, check = 0;
  if (argc > 2) napi_get_value_int32(env, argv[2], &point_bytes);
  if (argc > 3) napi_get_value_int32(env, argv[3], &check);
  if ((size_t)point_bytes != h->point_bytes || len % h->point_bytes) {   // the C ABI reads n x point_bytes of this curve
    napi_throw_range_error(env, NULL, "point buffer: expected a multiple of the curve's point size (96 bytes for BLS12-377 / BLS12-381; 64 for the 32-byte curves: Ed-on-BLS12-377, Pallas, Vesta, BN254, Grumpkin)");
    return NULL;
  }
  int rc = msm_set_points(ctx, data, len / point_bytes, 0, check);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "setPoints");
  napi_value n;
  NAPI_OK(napi_create_uint32(env, (uint32_t)(len / point_bytes), &n));
  return n;
}

// setPointsEx(h, Buffer, format, validate) -> n: msm_set_points_ex over host bytes (format MSM_POINTS_*, validate
// MSM_VALIDATE_*).  A refused point throws an Error whose message names its index and whose `badIndex` property holds it.
static napi_value SetPointsEx(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  void* data;
  size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &data, &len));
  int32_t format = MSM_POINTS_UNCOMPRESSED, validate = MSM_VALIDATE_NONE;
  if (argc > 2) napi_get_value_int32(env, argv[2], &format);
  if (argc > 3) napi_get_value_int32(env, argv[3], &validate);
  const size_t step = format == MSM_POINTS_COMPRESSED ? h->coord_bytes : h->point_bytes;
  if (len % step) {
    napi_throw_range_error(env, NULL, "point buffer: expected a multiple of the curve's point size in this format");
    return NULL;
  }
  uint64_t bad = UINT64_MAX;
  int rc = msm_set_points_ex(h->ctx, data, len / step, 0, format, validate, &bad);
  if (rc != MSM_OK) {
    char buf[640];
    snprintf(buf, sizeof buf, "setPointsEx: msm error %d: %s", rc, msm_last_error(h->ctx));
    napi_value msg, err, idx;
    NAPI_OK(napi_create_string_utf8(env, buf, NAPI_AUTO_LENGTH, &msg));
    NAPI_OK(napi_create_error(env, NULL, msg, &err));
    if (bad != UINT64_MAX) {
      NAPI_OK(napi_create_double(env, (double)bad, &idx));
      NAPI_OK(napi_set_named_property(env, err, "badIndex", idx));
    }
    napi_throw(env, err);
    return NULL;
  }
  napi_value n;
  NAPI_OK(napi_create_uint32(env, (uint32_t)(len / step), &n));
  return n;
}

// getPointsEx(h, first, count, format) -> Buffer: resident points read back as x || y or compressed (msm_get_points_ex)
static napi_value GetPointsEx(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t first = 0, count = 0;
  int32_t format = MSM_POINTS_UNCOMPRESSED;
  if (argc > 1) napi_get_value_int64(env, argv[1], &first);
  if (argc > 2) napi_get_value_int64(env, argv[2], &count);
  if (argc > 3) napi_get_value_int32(env, argv[3], &format);
  if (first < 0 || count < 0) {
    napi_throw_range_error(env, NULL, "getPointsEx: negative range");
    return NULL;
  }
  const size_t step = format == MSM_POINTS_COMPRESSED ? h->coord_bytes : h->point_bytes;
  void* out;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, (size_t)count * step + (count ? 0 : 1), &out, &buf));
  int rc = msm_get_points_ex(h->ctx, (uint64_t)first, (uint64_t)count, format, (uint8_t*)out);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "getPointsEx");
  return buf;
}

static napi_value result_object(napi_env env, const js_ctx* h, const msm_result* res) {
  const size_t coord = h->coord_bytes;   // of the context's curve, never taken from JS
  napi_value out, x, y, v, ph;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_create_buffer_copy(env, coord, res->x, NULL, &x));
  NAPI_OK(napi_create_buffer_copy(env, coord, res->y, NULL, &y));
  NAPI_OK(napi_set_named_property(env, out, "x", x));
  NAPI_OK(napi_set_named_property(env, out, "y", y));
  NAPI_OK(napi_get_boolean(env, res->is_infinity != 0, &v));
  NAPI_OK(napi_set_named_property(env, out, "isZero", v));
  NAPI_OK(napi_create_int32(env, res->c, &v));
  NAPI_OK(napi_set_named_property(env, out, "c", v));
  NAPI_OK(napi_create_int32(env, res->K, &v));
  NAPI_OK(napi_set_named_property(env, out, "K", v));
  NAPI_OK(napi_create_double(env, (double)res->n_pairs_algo, &v));
  NAPI_OK(napi_set_named_property(env, out, "nPairs", v));
  NAPI_OK(napi_create_array_with_length(env, MSM_N_PHASES, &ph));
  for (uint32_t i = 0; i < MSM_N_PHASES; i++) {
    NAPI_OK(napi_create_double(env, res->phase_ms[i], &v));
    NAPI_OK(napi_set_element(env, ph, i, v));
  }
  NAPI_OK(napi_set_named_property(env, out, "phaseMs", ph));
  return out;
}

static napi_value Msm(napi_env env, napi_callback_info info) {  // msm / msmUnsafe, src/msm-batched-affine.ts:69-340
  size_t argc = 6;   // (ctx, scalars, c, coordBytes, noGlv, unsafe)
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  msm_ctx* ctx = h->ctx;
  void* data;
  size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &data, &len));
  if (len % 32) {
    napi_throw_range_error(env, NULL, "scalar buffer length is not a multiple of 32");
    return NULL;
  }
  msm_opts opts;
  memset(&opts, 0, sizeof opts);
  if (argc > 2) napi_get_value_int32(env, argv[2], &opts.c);   // (the fourth argument, coordBytes, is accepted and ignored)
  if (argc > 4) napi_get_value_int32(env, argv[4], &opts.no_glv);   // msmProjective, src/parallel.ts:69-87
  if (argc > 5) napi_get_value_int32(env, argv[5], &opts.unsafe);   // msmUnsafe, src/msm-batched-affine.ts:587-598
  msm_result res;
  int rc = msm_run(ctx, data, len / 32, 0, &opts, &res);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "msm");
  return result_object(env, h, &res);
}

// device buffers: the scalars of a scalar pointer live in HBM from scalarsFromBytes / randomScalars on, as the reference's
// live in wasm memory (src/parallel.ts:119-133); msm() then crosses no PCIe
static napi_value DeviceAlloc(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  double bytes = 0;
  NAPI_OK(napi_get_value_double(env, argv[1], &bytes));
  if (!(bytes >= 0) || bytes > 9.0e15) {
    napi_throw_range_error(env, NULL, "deviceAlloc: bad size");
    return NULL;
  }
  js_dbuf* b = (js_dbuf*)calloc(1, sizeof(js_dbuf));
  if (!b) {
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  b->bytes = (uint64_t)bytes < 32 ? 32 : (uint64_t)bytes;
  int rc = msm_device_alloc(h->ctx, b->bytes, &b->dev);
  if (rc != MSM_OK) {
    free(b);
    return throw_msm(env, h->ctx, rc, "deviceAlloc");
  }
  b->owner = h;
  h->refs++;
  napi_value out;
  if (napi_create_external(env, b, finalize_dbuf, NULL, &out) != napi_ok) {
    msm_device_free(h->ctx, b->dev);
    h->refs--;
    free(b);
    napi_throw_error(env, NULL, "N-API call failed: napi_create_external");
    return NULL;
  }
  int64_t adj;
  napi_adjust_external_memory(env, (int64_t)b->bytes, &adj);   // lets the collector see what a dropped handle holds
  return out;
}

static napi_value DeviceUpload(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  js_dbuf* b = get_dbuf(env, h, argv[1]);
  if (!b) return NULL;
  void* data;
  size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[2], &data, &len));
  if (len > b->bytes) {
    napi_throw_range_error(env, NULL, "deviceUpload: the Buffer is larger than the device buffer");
    return NULL;
  }
  int rc = msm_device_upload(h->ctx, b->dev, data, len);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "deviceUpload");
  return NULL;
}

static napi_value DeviceFree(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  js_dbuf* b = get_dbuf(env, h, argv[1]);   // throws on a buffer that was freed before
  if (!b) return NULL;
  int rc = msm_device_free(h->ctx, b->dev);
  b->dev = NULL;
  int64_t adj;
  napi_adjust_external_memory(env, -(int64_t)b->bytes, &adj);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "deviceFree");
  return NULL;
}

static napi_value MsmDevice(napi_env env, napi_callback_info info) {  // msm over scalars resident in HBM
  size_t argc = 6;   // (ctx, dbuf, n, c, noGlv, unsafe)
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  js_dbuf* b = get_dbuf(env, h, argv[1]);
  if (!b) return NULL;
  uint32_t n = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[2], &n));
  if ((uint64_t)n * 32 > b->bytes) {
    napi_throw_range_error(env, NULL, "msmDevice: more scalars than the device buffer holds");
    return NULL;
  }
  msm_opts opts;
  memset(&opts, 0, sizeof opts);
  if (argc > 3) napi_get_value_int32(env, argv[3], &opts.c);
  if (argc > 4) napi_get_value_int32(env, argv[4], &opts.no_glv);
  if (argc > 5) napi_get_value_int32(env, argv[5], &opts.unsafe);
  msm_result res;
  int rc = msm_run(h->ctx, b->dev, n, 1, &opts, &res);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "msmDevice");
  return result_object(env, h, &res);
}

// many MSMs over one point set in one call (msm_run_batch): argv[1] is an array of B scalar Buffers (msmBatch) or of B device
// buffers holding n scalars each (msmBatchDevice); returns an array of B result objects, each as msm's
static napi_value batch_common(napi_env env, napi_callback_info info, int on_device) {
  size_t argc = 6;   // (ctx, array, c, noGlv, unsafe) or (ctx, array, n, c, noGlv, unsafe)
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const char* who = on_device ? "msmBatchDevice" : "msmBatch";
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  bool is_array = false;
  if (argc > 1) napi_is_array(env, argv[1], &is_array);
  if (!is_array) {
    napi_throw_type_error(env, NULL, "expected an array of scalar buffers");
    return NULL;
  }
  uint32_t B = 0;
  NAPI_OK(napi_get_array_length(env, argv[1], &B));
  if (B == 0) {
    napi_throw_range_error(env, NULL, "empty batch");
    return NULL;
  }
  uint64_t n = 0;
  size_t o = 2;   // first option argument
  if (on_device) {
    uint32_t nn = 0;
    if (argc > 2) NAPI_OK(napi_get_value_uint32(env, argv[2], &nn));
    n = nn;
    o = 3;
  }
  msm_opts opts;
  memset(&opts, 0, sizeof opts);
  if (argc > o) napi_get_value_int32(env, argv[o], &opts.c);
  if (argc > o + 1) napi_get_value_int32(env, argv[o + 1], &opts.no_glv);
  if (argc > o + 2) napi_get_value_int32(env, argv[o + 2], &opts.unsafe);
  const void** ptrs = (const void**)calloc(B, sizeof(void*));
  msm_result* res = (msm_result*)calloc(B, sizeof(msm_result));
  if (!ptrs || !res) {
    free(ptrs);
    free(res);
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  const char* bad = NULL;
  for (uint32_t b = 0; b < B && !bad; b++) {
    napi_value e;
    if (napi_get_element(env, argv[1], b, &e) != napi_ok) { bad = "N-API call failed: napi_get_element"; break; }
    if (on_device) {
      js_dbuf* d = get_dbuf(env, h, e);
      if (!d) { free(ptrs); free(res); return NULL; }
      if (n * 32 > d->bytes) bad = "more scalars than a device buffer holds";
      ptrs[b] = d->dev;
    } else {
      void* data;
      size_t len;
      if (napi_get_buffer_info(env, e, &data, &len) != napi_ok) { bad = "expected an array of Buffers"; break; }
      if (len % 32) bad = "scalar buffer length is not a multiple of 32";
      else if (b == 0) n = len / 32;
      else if (len / 32 != n) bad = "the scalar buffers of a batch must have the same length";
      ptrs[b] = data;
    }
  }
  if (bad) {
    free(ptrs);
    free(res);
    napi_throw_range_error(env, NULL, bad);
    return NULL;
  }
  int rc = msm_run_batch(h->ctx, ptrs, B, n, on_device, &opts, res);
  free(ptrs);
  if (rc != MSM_OK) {
    free(res);
    return throw_msm(env, h->ctx, rc, who);
  }
  napi_value arr;
  if (napi_create_array_with_length(env, B, &arr) != napi_ok) {
    free(res);
    napi_throw_error(env, NULL, "N-API call failed: napi_create_array_with_length");
    return NULL;
  }
  for (uint32_t b = 0; b < B; b++) {
    napi_value r = result_object(env, h, &res[b]);
    if (!r || napi_set_element(env, arr, b, r) != napi_ok) {
      free(res);
      return NULL;
    }
  }
  free(res);
  return arr;
}
static napi_value MsmBatch(napi_env env, napi_callback_info info) { return batch_common(env, info, 0); }
static napi_value MsmBatchDevice(napi_env env, napi_callback_info info) { return batch_common(env, info, 1); }

// narrow scalars (msm_run_narrow / msm_run_batch_narrow / msm_scalar_bits): host Buffers of n x width bytes
static int narrow_args(napi_env env, size_t argc, napi_value* argv, int32_t* width, int32_t* bits, int32_t* is_signed, msm_opts* opts) {
  memset(opts, 0, sizeof *opts);
  *width = *bits = *is_signed = 0;
  if (argc > 2) napi_get_value_int32(env, argv[2], width);
  if (argc > 3) napi_get_value_int32(env, argv[3], bits);
  if (argc > 4) napi_get_value_int32(env, argv[4], is_signed);
  if (argc > 5) napi_get_value_int32(env, argv[5], &opts->c);
  if (*width != 1 && *width != 2 && *width != 4 && *width != 8 && *width != 16 && *width != 32) {
    napi_throw_range_error(env, NULL, "width must be 1, 2, 4, 8, 16 or 32 bytes");
    return 0;
  }
  return 1;
}

static napi_value MsmNarrow(napi_env env, napi_callback_info info) {
  size_t argc = 6;   // (ctx, scalars, width, bits, signed, c)
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  void* data;
  size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &data, &len));
  int32_t width, bits, is_signed;
  msm_opts opts;
  if (!narrow_args(env, argc, argv, &width, &bits, &is_signed, &opts)) return NULL;
  if (len % (size_t)width) {
    napi_throw_range_error(env, NULL, "scalar buffer length is not a multiple of the width");
    return NULL;
  }
  msm_result res;
  int rc = msm_run_narrow(h->ctx, data, len / (size_t)width, 0, width, bits, is_signed, &opts, &res);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "msmNarrow");
  return result_object(env, h, &res);
}

// indexed (sparse) MSM (msm_run_indexed / msm_run_indexed_narrow): host Buffers, the indices as m x 4 bytes (uint32, little-endian)
static int indexed_buffers(napi_env env, napi_value* argv, size_t width, void** sc, void** idx, size_t* m) {
  size_t slen, ilen;
  if (napi_get_buffer_info(env, argv[1], sc, &slen) != napi_ok || napi_get_buffer_info(env, argv[2], idx, &ilen) != napi_ok) {
    napi_throw_type_error(env, NULL, "scalars and indices must be Buffers");
    return 0;
  }
  if (slen % width || ilen % 4 || slen / width != ilen / 4) {
    napi_throw_range_error(env, NULL, "scalars and indices must hold the same number of entries (m x width and m x 4 bytes)");
    return 0;
  }
  *m = ilen / 4;
  return 1;
}

static napi_value MsmIndexed(napi_env env, napi_callback_info info) {
  size_t argc = 5;   // (ctx, scalars, indices, c, noGlv)
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "msmIndexed(ctx, scalars, indices[, c, noGlv])");
    return NULL;
  }
  void *sc, *idx;
  size_t m;
  if (!indexed_buffers(env, argv, 32, &sc, &idx, &m)) return NULL;
  msm_opts opts;
  memset(&opts, 0, sizeof opts);
  if (argc > 3) napi_get_value_int32(env, argv[3], &opts.c);
  if (argc > 4) napi_get_value_int32(env, argv[4], &opts.no_glv);
  msm_result res;
  int rc = msm_run_indexed(h->ctx, sc, (const uint32_t*)idx, m, 0, &opts, &res);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "msmIndexed");
  return result_object(env, h, &res);
}

static napi_value MsmIndexedNarrow(napi_env env, napi_callback_info info) {
  size_t argc = 7;   // (ctx, scalars, indices, width, bits, signed, c)
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  if (argc < 4) {
    napi_throw_type_error(env, NULL, "msmIndexedNarrow(ctx, scalars, indices, width[, bits, signed, c])");
    return NULL;
  }
  int32_t width, bits, is_signed;
  msm_opts opts;
  if (!narrow_args(env, argc - 1, argv + 1, &width, &bits, &is_signed, &opts)) return NULL;   // (the formats sit one argument later)
  void *sc, *idx;
  size_t m;
  if (!indexed_buffers(env, argv, (size_t)width, &sc, &idx, &m)) return NULL;
  msm_result res;
  int rc = msm_run_indexed_narrow(h->ctx, sc, (const uint32_t*)idx, m, 0, width, bits, is_signed, &opts, &res);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "msmIndexedNarrow");
  return result_object(env, h, &res);
}

static napi_value MsmBatchNarrow(napi_env env, napi_callback_info info) {
  size_t argc = 6;   // (ctx, [scalars], width, bits, signed, c)
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  bool is_array = false;
  if (argc > 1) napi_is_array(env, argv[1], &is_array);
  uint32_t B = 0;
  if (is_array) NAPI_OK(napi_get_array_length(env, argv[1], &B));
  if (!is_array || B == 0) {
    napi_throw_type_error(env, NULL, "expected a non-empty array of scalar Buffers");
    return NULL;
  }
  int32_t width, bits, is_signed;
  msm_opts opts;
  if (!narrow_args(env, argc, argv, &width, &bits, &is_signed, &opts)) return NULL;
  const void** ptrs = (const void**)calloc(B, sizeof(void*));
  msm_result* res = (msm_result*)calloc(B, sizeof(msm_result));
  if (!ptrs || !res) {
    free(ptrs);
    free(res);
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  uint64_t n = 0;
  const char* bad = NULL;
  for (uint32_t b = 0; b < B && !bad; b++) {
    napi_value e;
    void* data;
    size_t len;
    if (napi_get_element(env, argv[1], b, &e) != napi_ok || napi_get_buffer_info(env, e, &data, &len) != napi_ok) {
      bad = "expected an array of Buffers";
      break;
    }
    if (len % (size_t)width) bad = "scalar buffer length is not a multiple of the width";
    else if (b == 0) n = len / (size_t)width;
    else if (len / (size_t)width != n) bad = "the scalar buffers of a batch must have the same length";
    ptrs[b] = data;
  }
  if (bad) {
    free(ptrs);
    free(res);
    napi_throw_range_error(env, NULL, bad);
    return NULL;
  }
  int rc = msm_run_batch_narrow(h->ctx, ptrs, B, n, 0, width, bits, is_signed, &opts, res);
  free(ptrs);
  if (rc != MSM_OK) {
    free(res);
    return throw_msm(env, h->ctx, rc, "msmBatchNarrow");
  }
  napi_value arr;
  if (napi_create_array_with_length(env, B, &arr) != napi_ok) {
    free(res);
    napi_throw_error(env, NULL, "N-API call failed: napi_create_array_with_length");
    return NULL;
  }
  for (uint32_t b = 0; b < B; b++) {
    napi_value r = result_object(env, h, &res[b]);
    if (!r || napi_set_element(env, arr, b, r) != napi_ok) {
      free(res);
      return NULL;
    }
  }
  free(res);
  return arr;
}

static napi_value ScalarBits(napi_env env, napi_callback_info info) {
  size_t argc = 2;   // (ctx, scalars: n x 32 bytes)
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  void* data;
  size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &data, &len));
  if (len % 32) {
    napi_throw_range_error(env, NULL, "scalar buffer length is not a multiple of 32");
    return NULL;
  }
  int32_t ub = 0, sb = 0;
  int rc = msm_scalar_bits(h->ctx, data, len / 32, 0, &ub, &sb);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarBits");
  napi_value out, v;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_create_int32(env, ub, &v));
  NAPI_OK(napi_set_named_property(env, out, "unsigned", v));
  NAPI_OK(napi_create_int32(env, sb, &v));
  NAPI_OK(napi_set_named_property(env, out, "signed", v));
  return out;
}

static napi_value Plan(napi_env env, napi_callback_info info) {  // windowSize, src/msm-common.ts:8-41
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msm_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t n = 0;
  msm_opts opts;
  memset(&opts, 0, sizeof opts);
  napi_get_value_uint32(env, argv[1], &n);
  if (argc > 2) napi_get_value_int32(env, argv[2], &opts.c);
  int32_t c = 0, K = 0;
  int rc = msm_plan(ctx, n, &opts, &c, &K);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "plan");
  napi_value out, v;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_create_int32(env, c, &v));
  NAPI_OK(napi_set_named_property(env, out, "c", v));
  NAPI_OK(napi_create_int32(env, K, &v));
  NAPI_OK(napi_set_named_property(env, out, "K", v));
  return out;
}

// randomPointsFast, src/curve-random.ts:14-92: n resident points generated on the GPU
static napi_value GeneratePoints(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msm_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t n = 0, seed = 1;
  napi_get_value_uint32(env, argv[1], &n);
  if (argc > 2) napi_get_value_uint32(env, argv[2], &seed);
  int rc = msm_generate_points(ctx, n, seed, NULL);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "generatePoints");
  napi_value out;
  NAPI_OK(napi_create_uint32(env, n, &out));
  return out;
}

// randomScalars, src/curve-random.ts:151-194: n uniform scalars < q.  (h, n, seed) -> n x 32 little-endian bytes in a Buffer;
// (h, n, seed, dbuf) -> written to the device buffer, nothing crosses PCIe, returns n
static napi_value GenerateScalars(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  msm_ctx* ctx = h->ctx;
  uint32_t n = 0, seed = 1;
  napi_get_value_uint32(env, argv[1], &n);
  if (argc > 2) napi_get_value_uint32(env, argv[2], &seed);
  napi_valuetype t3 = napi_undefined;
  if (argc > 3) napi_typeof(env, argv[3], &t3);
  if (t3 == napi_external) {
    js_dbuf* b = get_dbuf(env, h, argv[3]);
    if (!b) return NULL;
    if ((uint64_t)n * 32 > b->bytes) {
      napi_throw_range_error(env, NULL, "generateScalars: the device buffer is too small");
      return NULL;
    }
    int rc = msm_generate_scalars(ctx, n, seed, b->dev, NULL);
    if (rc != MSM_OK) return throw_msm(env, ctx, rc, "generateScalars");
    napi_value out;
    NAPI_OK(napi_create_uint32(env, n, &out));
    return out;
  }
  void* data = NULL;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, (size_t)n * 32, &data, &buf));
  int rc = msm_generate_scalars(ctx, n, seed, NULL, (uint8_t*)data);   /* host copy only */
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "generateScalars");
  return buf;
}

// point-set handles: pointsetCreate(h) -> id (becomes current), pointsetSelect(h, id), pointsetDestroy(h, id)
static napi_value PointsetCreate(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msm_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int32_t id = 0;
  int rc = msm_pointset_create(ctx, &id);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "pointsetCreate");
  napi_value out;
  NAPI_OK(napi_create_int32(env, id, &out));
  return out;
}
static napi_value PointsetOp(napi_env env, napi_callback_info info, int destroy) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msm_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int32_t id = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &id));
  int rc = destroy ? msm_pointset_destroy(ctx, id) : msm_pointset_select(ctx, id);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, destroy ? "pointsetDestroy" : "pointsetSelect");
  return NULL;
}
static napi_value PointsetSelect(napi_env env, napi_callback_info info) { return PointsetOp(env, info, 0); }
static napi_value PointsetDestroy(napi_env env, napi_callback_info info) { return PointsetOp(env, info, 1); }

// point-set linear combinations (msm_points_lincomb): pointsLincomb(h, srcA, aLo, a, srcB, bLo, b, count, dst) -> count
static int scalar_arg(napi_env env, napi_value v, const uint8_t** out) {
  bool is_buf = false;
  void* p = NULL;
  size_t len = 0;
  if (napi_is_buffer(env, v, &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, v, &p, &len) != napi_ok || len != 32) {
    napi_throw_type_error(env, NULL, "pointsLincomb: a scalar is a Buffer of 32 bytes");
    return 0;
  }
  *out = (const uint8_t*)p;
  return 1;
}
static napi_value PointsLincomb(napi_env env, napi_callback_info info) {
  size_t argc = 9;
  napi_value argv[9];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 9) {
    napi_throw_type_error(env, NULL, "pointsLincomb(ctx, srcA, aLo, a, srcB, bLo, b, count, dst)");
    return NULL;
  }
  msm_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int32_t src_a = 0, src_b = -1, dst = 0;
  int64_t a_lo = 0, b_lo = 0, count = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &src_a));
  NAPI_OK(napi_get_value_int64(env, argv[2], &a_lo));
  NAPI_OK(napi_get_value_int32(env, argv[4], &src_b));
  NAPI_OK(napi_get_value_int64(env, argv[5], &b_lo));
  NAPI_OK(napi_get_value_int64(env, argv[7], &count));
  NAPI_OK(napi_get_value_int32(env, argv[8], &dst));
  if (a_lo < 0 || b_lo < 0 || count < 0) {
    napi_throw_range_error(env, NULL, "pointsLincomb: aLo, bLo and count must not be negative");
    return NULL;
  }
  const uint8_t *a = NULL, *b = NULL;
  if (!scalar_arg(env, argv[3], &a)) return NULL;
  if (src_b >= 0 && !scalar_arg(env, argv[6], &b)) return NULL;
  int rc = msm_points_lincomb(ctx, src_a, (uint64_t)a_lo, a, src_b, (uint64_t)b_lo, b, (uint64_t)count, dst);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "pointsLincomb");
  napi_value out;
  NAPI_OK(napi_create_int64(env, count, &out));
  return out;
}
static napi_value PointsetSize(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msm_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int32_t id = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &id));
  uint64_t n = 0;
  int rc = msm_pointset_size(ctx, id, &n);
  if (rc != MSM_OK) return throw_msm(env, ctx, rc, "pointsetSize");
  napi_value out;
  NAPI_OK(napi_create_int64(env, (int64_t)n, &out));
  return out;
}

// resident scalar vectors (msm_scalars_*): a vector argument is (device buffer, offset in elements); its n elements must lie
// inside the buffer -- the library cannot know where a caller's allocation ends
static int vec_arg(napi_env env, js_ctx* h, napi_value v_buf, napi_value v_off, int64_t n, const char* what, uint8_t** out) {
  js_dbuf* b = get_dbuf(env, h, v_buf);
  if (!b) return 0;
  int64_t off = 0;
  if (napi_get_value_int64(env, v_off, &off) != napi_ok || off < 0 || n < 0 || ((uint64_t)off + (uint64_t)n) * 32 > b->bytes) {
    char buf[160];
    snprintf(buf, sizeof buf, "%s: the elements lie outside the device buffer", what);
    napi_throw_range_error(env, NULL, buf);
    return 0;
  }
  *out = (uint8_t*)b->dev + (uint64_t)off * 32;
  return 1;
}
static int host_scalar_arg(napi_env env, napi_value v, const uint8_t** out) {
  bool is_buf = false;
  void* p = NULL;
  size_t len = 0;
  if (napi_is_buffer(env, v, &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, v, &p, &len) != napi_ok || len != 32) {
    napi_throw_type_error(env, NULL, "a host scalar is a Buffer of 32 bytes");
    return 0;
  }
  *out = (const uint8_t*)p;
  return 1;
}
static int is_nullish(napi_env env, napi_value v) {
  napi_valuetype t;
  return napi_typeof(env, v, &t) == napi_ok && (t == napi_undefined || t == napi_null);
}
// per-row scalar multiplication (msm_points_mul, msm_points_mul_base).  The scalars are host bytes (a Buffer holding at least
// count x 32 of them) or the elements [sOff, sOff + count) of a device buffer
static int scalars_arg(napi_env env, js_ctx* h, napi_value v, napi_value v_off, int64_t count, const char* what, const void** out, int* on_device) {
  bool is_buf = false;
  if (napi_is_buffer(env, v, &is_buf) == napi_ok && is_buf) {
    void* p = NULL;
    size_t len = 0;
    if (napi_get_buffer_info(env, v, &p, &len) != napi_ok || count < 0 || (uint64_t)count * 32 > len) {
      char buf[160];
      snprintf(buf, sizeof buf, "%s: the Buffer holds fewer than count x 32 bytes of scalars", what);
      napi_throw_range_error(env, NULL, buf);
      return 0;
    }
    *out = p;
    *on_device = 0;
    return 1;
  }
  uint8_t* d = NULL;
  if (!vec_arg(env, h, v, v_off, count, what, &d)) return 0;
  *out = d;
  *on_device = 1;
  return 1;
}
static napi_value PointsMul(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 7) {
    napi_throw_type_error(env, NULL, "pointsMul(ctx, src, aLo, scalars, sOff, count, dst)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int32_t src = 0, dst = 0;
  int64_t a_lo = 0, count = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &src));
  NAPI_OK(napi_get_value_int64(env, argv[2], &a_lo));
  NAPI_OK(napi_get_value_int64(env, argv[5], &count));
  NAPI_OK(napi_get_value_int32(env, argv[6], &dst));
  if (a_lo < 0 || count < 0) {
    napi_throw_range_error(env, NULL, "pointsMul: aLo and count must not be negative");
    return NULL;
  }
  const void* sc = NULL;
  int on_device = 0;
  if (!scalars_arg(env, h, argv[3], argv[4], count, "pointsMul", &sc, &on_device)) return NULL;
  int rc = msm_points_mul(h->ctx, src, (uint64_t)a_lo, sc, on_device, (uint64_t)count, dst);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "pointsMul");
  napi_value out;
  NAPI_OK(napi_create_int64(env, count, &out));
  return out;
}
static napi_value PointsMulBase(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) {
    napi_throw_type_error(env, NULL, "pointsMulBase(ctx, base, scalars, sOff, count, dst)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int32_t dst = 0;
  int64_t count = 0;
  NAPI_OK(napi_get_value_int64(env, argv[4], &count));
  NAPI_OK(napi_get_value_int32(env, argv[5], &dst));
  if (count < 0) {
    napi_throw_range_error(env, NULL, "pointsMulBase: count must not be negative");
    return NULL;
  }
  const uint8_t* base = NULL;
  if (!is_nullish(env, argv[1])) {
    bool is_buf = false;
    void* p = NULL;
    size_t len = 0;
    if (napi_is_buffer(env, argv[1], &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, argv[1], &p, &len) != napi_ok ||
        (len != 64 && len != 96)) {
      napi_throw_type_error(env, NULL, "pointsMulBase: the base is a Buffer of x || y in the curve's wire format, or null");
      return NULL;
    }
    base = (const uint8_t*)p;
  }
  const void* sc = NULL;
  int on_device = 0;
  if (!scalars_arg(env, h, argv[2], argv[3], count, "pointsMulBase", &sc, &on_device)) return NULL;
  int rc = msm_points_mul_base(h->ctx, base, sc, on_device, (uint64_t)count, dst);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "pointsMulBase");
  napi_value out;
  NAPI_OK(napi_create_int64(env, count, &out));
  return out;
}
// pointsNtt(ctx, src, aLo, log2n, omega: Buffer | null, shift: Buffer | null, inverse, dst) -> n = 2^log2n: rows [0, n) of point
// set dst = the transform of the rows [aLo, aLo + n) of point set src (msm_points_ntt)
static napi_value PointsNtt(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 8) {
    napi_throw_type_error(env, NULL, "pointsNtt(ctx, src, aLo, log2n, omega, shift, inverse, dst)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int32_t src = 0, dst = 0;
  int64_t a_lo = 0;
  uint32_t log2n = 0;
  bool inverse = false;
  NAPI_OK(napi_get_value_int32(env, argv[1], &src));
  NAPI_OK(napi_get_value_int64(env, argv[2], &a_lo));
  NAPI_OK(napi_get_value_uint32(env, argv[3], &log2n));
  NAPI_OK(napi_get_value_bool(env, argv[6], &inverse));
  NAPI_OK(napi_get_value_int32(env, argv[7], &dst));
  if (a_lo < 0 || log2n > 31) {
    napi_throw_range_error(env, NULL, "pointsNtt: aLo must not be negative and log2n must be below 32");
    return NULL;
  }
  const uint8_t *omega = NULL, *shift = NULL;
  if (!is_nullish(env, argv[4]) && !host_scalar_arg(env, argv[4], &omega)) return NULL;
  if (!is_nullish(env, argv[5]) && !host_scalar_arg(env, argv[5], &shift)) return NULL;
  int rc = msm_points_ntt(h->ctx, src, (uint64_t)a_lo, log2n, omega, shift, inverse ? 1 : 0, dst);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "pointsNtt");
  napi_value out;
  NAPI_OK(napi_create_int64(env, (int64_t)1 << log2n, &out));
  return out;
}
static napi_value DeviceDownload(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4) {
    napi_throw_type_error(env, NULL, "deviceDownload(ctx, dbuf, byteOffset, bytes)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  js_dbuf* b = get_dbuf(env, h, argv[1]);
  if (!b) return NULL;
  int64_t off = 0, bytes = 0;
  NAPI_OK(napi_get_value_int64(env, argv[2], &off));
  NAPI_OK(napi_get_value_int64(env, argv[3], &bytes));
  if (off < 0 || bytes < 0 || (uint64_t)off + (uint64_t)bytes > b->bytes) {
    napi_throw_range_error(env, NULL, "deviceDownload: the range lies outside the device buffer");
    return NULL;
  }
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, (size_t)bytes, &po, &out));
  if (bytes) {
    int rc = msm_device_download(h->ctx, po, (uint8_t*)b->dev + off, (uint64_t)bytes);
    if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "deviceDownload");
  }
  return out;
}
static napi_value ScalarsLincomb(napi_env env, napi_callback_info info) {
  size_t argc = 10;
  napi_value argv[10];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 10) {
    napi_throw_type_error(env, NULL, "scalarsLincomb(ctx, dst, dstOff, x, a, aOff, y, b, bOff, n)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t n = 0;
  NAPI_OK(napi_get_value_int64(env, argv[9], &n));
  uint8_t *dst = NULL, *a = NULL, *b = NULL;
  const uint8_t *x = NULL, *y = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsLincomb", &dst) || !vec_arg(env, h, argv[4], argv[5], n, "scalarsLincomb", &a)) return NULL;
  if (!host_scalar_arg(env, argv[3], &x)) return NULL;
  if (!is_nullish(env, argv[7])) {
    if (!vec_arg(env, h, argv[7], argv[8], n, "scalarsLincomb", &b) || !host_scalar_arg(env, argv[6], &y)) return NULL;
  }
  int rc = msm_scalars_lincomb(h->ctx, dst, x, a, y, b, (uint64_t)n);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsLincomb");
  return NULL;
}
static napi_value ScalarsMul(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 8) {
    napi_throw_type_error(env, NULL, "scalarsMul(ctx, dst, dstOff, a, aOff, b, bOff, n)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t n = 0;
  NAPI_OK(napi_get_value_int64(env, argv[7], &n));
  uint8_t *dst = NULL, *a = NULL, *b = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsMul", &dst) || !vec_arg(env, h, argv[3], argv[4], n, "scalarsMul", &a) ||
      !vec_arg(env, h, argv[5], argv[6], n, "scalarsMul", &b))
    return NULL;
  int rc = msm_scalars_mul(h->ctx, dst, a, b, (uint64_t)n);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsMul");
  return NULL;
}
static napi_value ScalarsInner(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) {
    napi_throw_type_error(env, NULL, "scalarsInner(ctx, a, aOff, b, bOff, n)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t n = 0;
  NAPI_OK(napi_get_value_int64(env, argv[5], &n));
  uint8_t *a = NULL, *b = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsInner", &a) || !vec_arg(env, h, argv[3], argv[4], n, "scalarsInner", &b)) return NULL;
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, 32, &po, &out));
  int rc = msm_scalars_inner(h->ctx, a, b, (uint64_t)n, (uint8_t*)po);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsInner");
  return out;
}
static napi_value ScalarsPowers(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) {
    napi_throw_type_error(env, NULL, "scalarsPowers(ctx, dst, dstOff, s, x, n)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t n = 0;
  NAPI_OK(napi_get_value_int64(env, argv[5], &n));
  uint8_t* dst = NULL;
  const uint8_t *s = NULL, *x = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsPowers", &dst)) return NULL;
  if (!host_scalar_arg(env, argv[3], &s) || !host_scalar_arg(env, argv[4], &x)) return NULL;
  int rc = msm_scalars_powers(h->ctx, dst, s, x, (uint64_t)n);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsPowers");
  return NULL;
}
// the resident NTT (msm_scalars_ntt): B vectors of 2^log2n elements back to back from (buffer, offset); omega, shift: Buffer | null
static napi_value ScalarsNtt(napi_env env, napi_callback_info info) {
  size_t argc = 10;
  napi_value argv[10];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 10) {
    napi_throw_type_error(env, NULL, "scalarsNtt(ctx, dst, dstOff, a, aOff, log2n, batch, omega, shift, inverse)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint32_t log2n = 0, batch = 0;
  bool inverse = false;
  NAPI_OK(napi_get_value_uint32(env, argv[5], &log2n));
  NAPI_OK(napi_get_value_uint32(env, argv[6], &batch));
  NAPI_OK(napi_get_value_bool(env, argv[9], &inverse));
  if (log2n > 31) {
    napi_throw_range_error(env, NULL, "scalarsNtt: log2n must be below 32");
    return NULL;
  }
  const int64_t n = (int64_t)batch << log2n;
  uint8_t *dst = NULL, *a = NULL;
  const uint8_t *omega = NULL, *shift = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsNtt", &dst) || !vec_arg(env, h, argv[3], argv[4], n, "scalarsNtt", &a)) return NULL;
  if (!is_nullish(env, argv[7]) && !host_scalar_arg(env, argv[7], &omega)) return NULL;
  if (!is_nullish(env, argv[8]) && !host_scalar_arg(env, argv[8], &shift)) return NULL;
  int rc = msm_scalars_ntt(h->ctx, dst, a, log2n, batch, omega, shift, inverse ? 1 : 0);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsNtt");
  return NULL;
}
// scalarsRootOfUnity(ctx, log2n) -> Buffer of 32 bytes; scalarsNttMaxLog2n(ctx) -> number
static napi_value ScalarsRootOfUnity(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) {
    napi_throw_type_error(env, NULL, "scalarsRootOfUnity(ctx, log2n)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint32_t log2n = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[1], &log2n));
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, 32, &po, &out));
  if (msm_scalars_root_of_unity(h->ctx, log2n, (uint8_t*)po) != MSM_OK) {
    napi_throw_range_error(env, NULL, "scalarsRootOfUnity: the group order minus one has no such power of two as a factor");
    return NULL;
  }
  return out;
}
static napi_value ScalarsNttMaxLog2n(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = argc ? get_handle(env, argv[0]) : NULL;
  if (!h) return NULL;
  uint32_t top = 0;
  int rc = msm_scalars_ntt_max_log2n(h->ctx, &top);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsNttMaxLog2n");
  napi_value out;
  NAPI_OK(napi_create_uint32(env, top, &out));
  return out;
}

// the resident scans (msm_scalars_scan, msm_scalars_inverse, msm_scalars_div_linear): n elements from (buffer, offset)
// scalarsScan(ctx, dst, dstOff, a, aOff, n, op, exclusive, init: Buffer | null) -> Buffer of 32 bytes, the total
static napi_value ScalarsScan(napi_env env, napi_callback_info info) {
  size_t argc = 9;
  napi_value argv[9];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 9) {
    napi_throw_type_error(env, NULL, "scalarsScan(ctx, dst, dstOff, a, aOff, n, op, exclusive, init)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t n = 0;
  int32_t op = 0;
  bool exclusive = false;
  NAPI_OK(napi_get_value_int64(env, argv[5], &n));
  NAPI_OK(napi_get_value_int32(env, argv[6], &op));
  NAPI_OK(napi_get_value_bool(env, argv[7], &exclusive));
  uint8_t *dst = NULL, *a = NULL;
  const uint8_t* init = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsScan", &dst) || !vec_arg(env, h, argv[3], argv[4], n, "scalarsScan", &a)) return NULL;
  if (!is_nullish(env, argv[8]) && !host_scalar_arg(env, argv[8], &init)) return NULL;
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, 32, &po, &out));
  int rc = msm_scalars_scan(h->ctx, dst, a, (uint64_t)n, op, exclusive ? MSM_SCAN_EXCLUSIVE : 0u, init, (uint8_t*)po);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsScan");
  return out;
}
// scalarsInverse(ctx, dst, dstOff, a, aOff, n) -> number of elements whose residue is 0
static napi_value ScalarsInverse(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) {
    napi_throw_type_error(env, NULL, "scalarsInverse(ctx, dst, dstOff, a, aOff, n)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t n = 0;
  NAPI_OK(napi_get_value_int64(env, argv[5], &n));
  uint8_t *dst = NULL, *a = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsInverse", &dst) || !vec_arg(env, h, argv[3], argv[4], n, "scalarsInverse", &a)) return NULL;
  uint64_t zeros = 0;
  int rc = msm_scalars_inverse(h->ctx, dst, a, (uint64_t)n, &zeros);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsInverse");
  napi_value out;
  NAPI_OK(napi_create_int64(env, (int64_t)zeros, &out));
  return out;
}
// scalarsDivLinear(ctx, dst, dstOff, a, aOff, n, z: Buffer) -> Buffer of 32 bytes, the remainder
static napi_value ScalarsDivLinear(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 7) {
    napi_throw_type_error(env, NULL, "scalarsDivLinear(ctx, dst, dstOff, a, aOff, n, z)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t n = 0;
  NAPI_OK(napi_get_value_int64(env, argv[5], &n));
  uint8_t *dst = NULL, *a = NULL;
  const uint8_t* z = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], n, "scalarsDivLinear", &dst) || !vec_arg(env, h, argv[3], argv[4], n, "scalarsDivLinear", &a)) return NULL;
  if (!host_scalar_arg(env, argv[6], &z)) return NULL;
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, 32, &po, &out));
  int rc = msm_scalars_div_linear(h->ctx, dst, a, (uint64_t)n, z, (uint8_t*)po);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsDivLinear");
  return out;
}

// the resident sumcheck (msm_scalars_sumcheck_round, msm_scalars_bind, msm_scalars_eq): a table is a device buffer and an offset in elements
// `count` tables of n elements from two arrays, device buffers and offsets; 0: a JS exception is pending
static int vec_array_arg(napi_env env, js_ctx* h, napi_value v_bufs, napi_value v_offs, uint32_t max, int64_t n, const char* what,
                         uint8_t** out, uint32_t* count) {
  bool is_a = false, is_b = false;
  uint32_t la = 0, lb = 0;
  if (napi_is_array(env, v_bufs, &is_a) != napi_ok || napi_is_array(env, v_offs, &is_b) != napi_ok || !is_a || !is_b ||
      napi_get_array_length(env, v_bufs, &la) != napi_ok || napi_get_array_length(env, v_offs, &lb) != napi_ok || la != lb || la < 1 ||
      la > max) {
    char buf[160];
    snprintf(buf, sizeof buf, "%s: tables are two arrays of equal length 1 .. %u, device buffers and element offsets", what, max);
    napi_throw_type_error(env, NULL, buf);
    return 0;
  }
  for (uint32_t j = 0; j < la; j++) {
    napi_value vb, vo;
    if (napi_get_element(env, v_bufs, j, &vb) != napi_ok || napi_get_element(env, v_offs, j, &vo) != napi_ok) return 0;
    if (!vec_arg(env, h, vb, vo, n, what, &out[j])) return 0;
  }
  *count = la;
  return 1;
}
// scalarsSumcheckRound(ctx, bufs, offs, log2n, var, shape) -> Buffer of (d + 1) x 32 bytes: s(0), .., s(d)
static napi_value ScalarsSumcheckRound(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) {
    napi_throw_type_error(env, NULL, "scalarsSumcheckRound(ctx, bufs, offs, log2n, var, shape)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint32_t log2n = 0, var = 0, m = 0;
  int32_t shape = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[3], &log2n));
  NAPI_OK(napi_get_value_uint32(env, argv[4], &var));
  NAPI_OK(napi_get_value_int32(env, argv[5], &shape));
  if (log2n < 1 || log2n > 29) {
    napi_throw_range_error(env, NULL, "scalarsSumcheckRound: log2n must be 1 .. 29");
    return NULL;
  }
  uint8_t* vecs[4] = {NULL, NULL, NULL, NULL};
  if (!vec_array_arg(env, h, argv[1], argv[2], 4, (int64_t)1 << log2n, "scalarsSumcheckRound", vecs, &m)) return NULL;
  uint8_t evals[5 * 32];
  int rc = msm_scalars_sumcheck_round(h->ctx, (const void* const*)vecs, m, log2n, var, shape, evals);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsSumcheckRound");
  const size_t values = (shape == MSM_SUMCHECK_R1CS ? 3 : m) + 1;
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer_copy(env, values * 32, evals, &po, &out));
  return out;
}
// scalarsBind(ctx, dstBufs, dstOffs, srcBufs, srcOffs, log2n, var, r: Buffer)
static napi_value ScalarsBind(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 8) {
    napi_throw_type_error(env, NULL, "scalarsBind(ctx, dstBufs, dstOffs, srcBufs, srcOffs, log2n, var, r)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint32_t log2n = 0, var = 0, m = 0, md = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[5], &log2n));
  NAPI_OK(napi_get_value_uint32(env, argv[6], &var));
  if (log2n < 1 || log2n > 29) {
    napi_throw_range_error(env, NULL, "scalarsBind: log2n must be 1 .. 29");
    return NULL;
  }
  uint8_t *dst[8] = {NULL}, *src[8] = {NULL};
  const uint8_t* r = NULL;
  if (!vec_array_arg(env, h, argv[3], argv[4], 8, (int64_t)1 << log2n, "scalarsBind", src, &m)) return NULL;
  if (!vec_array_arg(env, h, argv[1], argv[2], 8, (int64_t)1 << (log2n - 1), "scalarsBind", dst, &md)) return NULL;
  if (md != m) {
    napi_throw_type_error(env, NULL, "scalarsBind: as many destinations as tables");
    return NULL;
  }
  if (!host_scalar_arg(env, argv[7], &r)) return NULL;
  int rc = msm_scalars_bind(h->ctx, (void* const*)dst, (const void* const*)src, m, log2n, var, r);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsBind");
  return NULL;
}
// scalarsEq(ctx, dst, dstOff, r: Buffer of v x 32 bytes, s: Buffer | null): 2^v elements
static napi_value ScalarsEq(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 5) {
    napi_throw_type_error(env, NULL, "scalarsEq(ctx, dst, dstOff, r, s)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  bool is_buf = false;
  void* pr = NULL;
  size_t len = 0;
  if (napi_is_buffer(env, argv[3], &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, argv[3], &pr, &len) != napi_ok || len % 32 ||
      len / 32 > 29) {
    napi_throw_type_error(env, NULL, "scalarsEq: r is a Buffer of v x 32 bytes, v <= 29");
    return NULL;
  }
  const uint32_t v = (uint32_t)(len / 32);
  uint8_t* dst = NULL;
  const uint8_t* s = NULL;
  if (!vec_arg(env, h, argv[1], argv[2], (int64_t)1 << v, "scalarsEq", &dst)) return NULL;
  if (!is_nullish(env, argv[4]) && !host_scalar_arg(env, argv[4], &s)) return NULL;
  int rc = msm_scalars_eq(h->ctx, dst, (const uint8_t*)pr, v, s);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsEq");
  return NULL;
}

/* ---- resident sparse matrices (msm_matrix_*, msm_scalars_matvec) ------------------------------------------------------ */

// an array of 32-bit words as a Buffer (uint32 LE); *count = its words
static int u32_buffer_arg(napi_env env, napi_value v, const char* what, const uint32_t** out, uint64_t* count) {
  bool is_buf = false;
  void* p = NULL;
  size_t len = 0;
  if (napi_is_buffer(env, v, &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, v, &p, &len) != napi_ok || len % 4) {
    char buf[160];
    snprintf(buf, sizeof buf, "%s is a Buffer of 32-bit little-endian words", what);
    napi_throw_type_error(env, NULL, buf);
    return 0;
  }
  *out = (const uint32_t*)p;
  *count = len / 4;
  return 1;
}
// matrixCreate(ctx, rows, cols, rowPtr: Buffer of (rows + 1) x 4 bytes, col: Buffer of nnz x 4 bytes, val: Buffer of nnz x 32 bytes | null,
//              flags) -> id.  The lengths of the Buffers are checked here: the library reads rows + 1 and nnz entries of them.
static napi_value MatrixCreate(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 7) {
    napi_throw_type_error(env, NULL, "matrixCreate(ctx, rows, cols, rowPtr, col, val, flags)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int64_t rows = 0, cols = 0;
  uint32_t flags = 0;
  NAPI_OK(napi_get_value_int64(env, argv[1], &rows));
  NAPI_OK(napi_get_value_int64(env, argv[2], &cols));
  NAPI_OK(napi_get_value_uint32(env, argv[6], &flags));
  const uint32_t *rp = NULL, *col = NULL;
  uint64_t n_rp = 0, nnz = 0;
  if (!u32_buffer_arg(env, argv[3], "matrixCreate: rowPtr", &rp, &n_rp) || !u32_buffer_arg(env, argv[4], "matrixCreate: col", &col, &nnz)) return NULL;
  if (rows < 0 || cols < 0 || n_rp != (uint64_t)rows + 1) {
    napi_throw_range_error(env, NULL, "matrixCreate: rowPtr holds rows + 1 entries");
    return NULL;
  }
  const void* val = NULL;
  if (!is_nullish(env, argv[5])) {
    bool is_buf = false;
    void* p = NULL;
    size_t len = 0;
    if (napi_is_buffer(env, argv[5], &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, argv[5], &p, &len) != napi_ok || len != nnz * 32) {
      napi_throw_range_error(env, NULL, "matrixCreate: val is a Buffer of 32 bytes per column index, or null");
      return NULL;
    }
    val = nnz ? p : (const void*)"";   /* (no entry: any non-null address says "coefficients", none is read) */
  }
  int32_t id = -1;
  int rc = msm_matrix_create(h->ctx, (uint64_t)rows, (uint64_t)cols, nnz, rp, col, val, 0, flags, &id);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "matrixCreate");
  napi_value out;
  NAPI_OK(napi_create_int32(env, id, &out));
  return out;
}
static napi_value MatrixDestroy(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) {
    napi_throw_type_error(env, NULL, "matrixDestroy(ctx, id)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int32_t id = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &id));
  int rc = msm_matrix_destroy(h->ctx, id);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "matrixDestroy");
  return NULL;
}
// matrixInfo(ctx, id) -> {rows, cols, nnz, bytes}
static napi_value MatrixInfo(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) {
    napi_throw_type_error(env, NULL, "matrixInfo(ctx, id)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int32_t id = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &id));
  uint64_t w[4] = {0, 0, 0, 0};
  int rc = msm_matrix_info(h->ctx, id, &w[0], &w[1], &w[2], &w[3]);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "matrixInfo");
  static const char* const names[4] = {"rows", "cols", "nnz", "bytes"};
  napi_value out, v;
  NAPI_OK(napi_create_object(env, &out));
  for (int i = 0; i < 4; i++) {
    NAPI_OK(napi_create_double(env, (double)w[i], &v));
    NAPI_OK(napi_set_named_property(env, out, names[i], v));
  }
  return out;
}
// scalarsMatvec(ctx, id, dst, dstOff, x | null, xOff, alpha: Buffer | null, flags): the device buffers must hold rows and cols elements
static napi_value ScalarsMatvec(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 8) {
    napi_throw_type_error(env, NULL, "scalarsMatvec(ctx, id, dst, dstOff, x, xOff, alpha, flags)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int32_t id = 0;
  uint32_t flags = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &id));
  NAPI_OK(napi_get_value_uint32(env, argv[7], &flags));
  uint64_t rows = 0, cols = 0, nnz = 0;
  int rc = msm_matrix_info(h->ctx, id, &rows, &cols, &nnz, NULL);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsMatvec");
  uint8_t *dst = NULL, *x = NULL;
  const uint8_t* alpha = NULL;
  if (!vec_arg(env, h, argv[2], argv[3], (int64_t)rows, "scalarsMatvec", &dst)) return NULL;
  if (!is_nullish(env, argv[4]) && !vec_arg(env, h, argv[4], argv[5], nnz ? (int64_t)cols : 0, "scalarsMatvec", &x)) return NULL;
  if (!is_nullish(env, argv[6]) && !host_scalar_arg(env, argv[6], &alpha)) return NULL;
  rc = msm_scalars_matvec(h->ctx, id, dst, x, alpha, flags);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "scalarsMatvec");
  return NULL;
}
// testSetMatvecGeometry(ctx, shortMax, partLen): the thresholds of the matrices created afterwards (msm_test_set_matvec_geometry)
static napi_value TestSetMatvecGeometry(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "testSetMatvecGeometry(ctx, shortMax, partLen)");
    return NULL;
  }
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint32_t s = 0, p = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[1], &s));
  NAPI_OK(napi_get_value_uint32(env, argv[2], &p));
  int rc = msm_test_set_matvec_geometry(h->ctx, s, p);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "testSetMatvecGeometry");
  return NULL;
}
// testLastMatvec(ctx) -> [shortMax, partLen, longRows, parts, launches] of the last product (msm_test_last_matvec)
static napi_value TestLastMatvec(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = argc ? get_handle(env, argv[0]) : NULL;
  if (!h) return NULL;
  int32_t w[5] = {0, 0, 0, 0, 0};
  if (msm_test_last_matvec(h->ctx, w, 5) != 5) return throw_msm(env, h->ctx, MSM_ERR_ARG, "testLastMatvec");
  napi_value out, v;
  NAPI_OK(napi_create_array_with_length(env, 5, &out));
  for (uint32_t i = 0; i < 5; i++) {
    NAPI_OK(napi_create_int32(env, w[i], &v));
    NAPI_OK(napi_set_element(env, out, i, v));
  }
  return out;
}

/* ---- the fine operator table: element-wise field / GLV / curve operators over Buffers -------------------------------- */

static int buffer_arg(napi_env env, napi_value v, uint8_t** data, size_t* len) {
  bool is_buf = false;
  if (napi_is_buffer(env, v, &is_buf) != napi_ok || !is_buf) {
    napi_throw_type_error(env, NULL, "expected a Buffer");
    return 0;
  }
  void* p = NULL;
  if (napi_get_buffer_info(env, v, &p, len) != napi_ok) return 0;
  *data = (uint8_t*)p;
  return 1;
}

static napi_value FieldOp(napi_env env, napi_callback_info info) {  // Field.multiply / square / add / subtract / inverse ..., src/field-msm.ts:86-123
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  int32_t op = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &op));
  uint8_t *a = NULL, *b = NULL;
  size_t la = 0, lb = 0;
  if (!buffer_arg(env, argv[2], &a, &la)) return NULL;
  if (argc > 3) {
    napi_valuetype t;
    NAPI_OK(napi_typeof(env, argv[3], &t));
    if (t != napi_undefined && t != napi_null && !buffer_arg(env, argv[3], &b, &lb)) return NULL;
  }
  if (!b) { b = a; lb = la; }   /* one-operand operators read the second array too: hand them the first */
  if (la % h->coord_bytes || la != lb) {
    napi_throw_error(env, NULL, "fieldOp: operands must be equally long arrays of whole field elements");
    return NULL;
  }
  if (op < MSM_OP_MUL || op > MSM_OP_INV_WORDSLICED) {
    napi_throw_error(env, NULL, "fieldOp: unknown operator");
    return NULL;
  }
  const uint64_t n = la / h->coord_bytes;
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, la, &po, &out));
  if (n) {
    int rc = msm_test_fp(h->ctx, op, a, b, (uint8_t*)po, n);
    if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "fieldOp");
  }
  return out;
}

static napi_value BatchInverse(napi_env env, napi_callback_info info) {  // batchInverse, src/wasm/inverse.ts:220-271
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint8_t* xs = NULL;
  size_t len = 0;
  if (!buffer_arg(env, argv[1], &xs, &len)) return NULL;
  uint32_t per_lane = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[2], &per_lane));
  if (len % h->coord_bytes || per_lane == 0) {
    napi_throw_error(env, NULL, "batchInverse: an array of whole field elements and a batch length >= 1");
    return NULL;
  }
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, len, &po, &out));
  if (len) {
    int rc = msm_test_batch_inverse(h->ctx, xs, (uint8_t*)po, len / h->coord_bytes, per_lane);
    if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "batchInverse");
  }
  return out;
}

static napi_value GlvDecompose(napi_env env, napi_callback_info info) {  // Scalar.decompose, src/scalar-glv.ts:105-128
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint8_t* sc = NULL;
  size_t len = 0;
  if (!buffer_arg(env, argv[1], &sc, &len)) return NULL;
  if (len % 32) {
    napi_throw_error(env, NULL, "glvDecompose: scalars are 32 bytes each");
    return NULL;
  }
  const uint64_t n = len / 32;
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, n * 40, &po, &out));
  if (n) {
    int rc = msm_test_glv(h->ctx, sc, (uint8_t*)po, n);
    if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "glvDecompose");
  }
  return out;
}

static napi_value BatchAdd(napi_env env, napi_callback_info info) {  // Affine.batchAdd, src/curve-affine.ts:376-522
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  js_ctx* h = get_handle(env, argv[0]);
  if (!h) return NULL;
  uint8_t *g = NULL, *hh = NULL;
  size_t lg = 0, lh = 0;
  if (!buffer_arg(env, argv[1], &g, &lg) || !buffer_arg(env, argv[2], &hh, &lh)) return NULL;
  if (lg % h->point_bytes || lg != lh || lg == 0) {
    napi_throw_error(env, NULL, "batchAdd: two equally long, non-empty arrays of whole wire points");
    return NULL;
  }
  napi_value out;
  void* po = NULL;
  NAPI_OK(napi_create_buffer(env, lg, &po, &out));
  int rc = msm_test_batch_add(h->ctx, g, hh, (uint8_t*)po, lg / h->point_bytes);
  if (rc != MSM_OK) return throw_msm(env, h->ctx, rc, "batchAdd");
  return out;
}

NAPI_MODULE_INIT() {
  // the library found at run time must come from the header this addon was compiled against: same symbol names, other
  // struct layouts would otherwise be read wrongly without a word
  if (msm_abi_version() != MSM_ABI_VERSION || msm_abi_struct_bytes(0) != sizeof(msm_opts) || msm_abi_struct_bytes(1) != sizeof(msm_result)) {
    napi_throw_error(env, NULL, "msm_hip.node: libmsm_hip.so was built from another version of include/msm_hip.h (msm_abi_version); rebuild both");
    return NULL;
  }
  struct { const char* name; napi_callback fn; } fns[] = {
      {"createContext", CreateContext}, {"destroyContext", DestroyContext}, {"setPoints", SetPoints}, {"msm", Msm}, {"plan", Plan},
      {"setPointsEx", SetPointsEx}, {"getPointsEx", GetPointsEx},
      {"generatePoints", GeneratePoints}, {"generateScalars", GenerateScalars},
      {"deviceAlloc", DeviceAlloc}, {"deviceUpload", DeviceUpload}, {"deviceFree", DeviceFree}, {"msmDevice", MsmDevice},
      {"msmBatch", MsmBatch}, {"msmBatchDevice", MsmBatchDevice},
      {"msmNarrow", MsmNarrow}, {"msmBatchNarrow", MsmBatchNarrow}, {"scalarBits", ScalarBits},
      {"msmIndexed", MsmIndexed}, {"msmIndexedNarrow", MsmIndexedNarrow},
      {"pointsetCreate", PointsetCreate}, {"pointsetSelect", PointsetSelect}, {"pointsetDestroy", PointsetDestroy},
      {"pointsLincomb", PointsLincomb}, {"pointsetSize", PointsetSize},
      {"pointsMul", PointsMul}, {"pointsMulBase", PointsMulBase}, {"pointsNtt", PointsNtt},
      {"deviceDownload", DeviceDownload}, {"scalarsLincomb", ScalarsLincomb}, {"scalarsMul", ScalarsMul},
      {"scalarsInner", ScalarsInner}, {"scalarsPowers", ScalarsPowers},
      {"scalarsNtt", ScalarsNtt}, {"scalarsRootOfUnity", ScalarsRootOfUnity}, {"scalarsNttMaxLog2n", ScalarsNttMaxLog2n},
      {"scalarsScan", ScalarsScan}, {"scalarsInverse", ScalarsInverse}, {"scalarsDivLinear", ScalarsDivLinear},
      {"scalarsSumcheckRound", ScalarsSumcheckRound}, {"scalarsBind", ScalarsBind}, {"scalarsEq", ScalarsEq},
      {"matrixCreate", MatrixCreate}, {"matrixDestroy", MatrixDestroy}, {"matrixInfo", MatrixInfo}, {"scalarsMatvec", ScalarsMatvec},
      {"testSetMatvecGeometry", TestSetMatvecGeometry}, {"testLastMatvec", TestLastMatvec},
      {"fieldOp", FieldOp}, {"batchInverse", BatchInverse}, {"glvDecompose", GlvDecompose}, {"batchAdd", BatchAdd}};
  for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
    if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
  }
  napi_value v;
  struct { const char* name; int32_t val; } ops[] = {{"OP_MUL", MSM_OP_MUL}, {"OP_SQR", MSM_OP_SQR}, {"OP_ADD", MSM_OP_ADD}, {"OP_SUB", MSM_OP_SUB},
      {"OP_INV", MSM_OP_INV}, {"OP_TO_MONT", MSM_OP_TO_MONT}, {"OP_FROM_MONT", MSM_OP_FROM_MONT}, {"OP_INV_FERMAT", MSM_OP_INV_FERMAT},
      {"OP_INV_KALISKI", MSM_OP_INV_KALISKI}, {"OP_INV_WORDSLICED", MSM_OP_INV_WORDSLICED},
      {"POINTS_UNCOMPRESSED", MSM_POINTS_UNCOMPRESSED}, {"POINTS_COMPRESSED", MSM_POINTS_COMPRESSED},
      {"VALIDATE_NONE", MSM_VALIDATE_NONE}, {"VALIDATE_CURVE", MSM_VALIDATE_CURVE}, {"VALIDATE_SUBGROUP", MSM_VALIDATE_SUBGROUP}};
  for (size_t i = 0; i < sizeof ops / sizeof ops[0]; i++) {
    napi_create_int32(env, ops[i].val, &v);
    napi_set_named_property(env, exports, ops[i].name, v);
  }
  napi_create_int32(env, MSM_ABI_VERSION, &v);
  napi_set_named_property(env, exports, "ABI_VERSION", v);
  napi_create_int32(env, MSM_CURVE_BLS12_377_G1, &v);
  napi_set_named_property(env, exports, "CURVE_BLS12_377_G1", v);
  napi_create_int32(env, MSM_CURVE_ED_ON_BLS12_377, &v);
  napi_set_named_property(env, exports, "CURVE_ED_ON_BLS12_377", v);
  napi_create_int32(env, MSM_CURVE_BLS12_381_G1, &v);
  napi_set_named_property(env, exports, "CURVE_BLS12_381_G1", v);
  napi_create_int32(env, MSM_CURVE_PALLAS, &v);
  napi_set_named_property(env, exports, "CURVE_PALLAS", v);
  napi_create_int32(env, MSM_CURVE_BN254_G1, &v);
  napi_set_named_property(env, exports, "CURVE_BN254_G1", v);
  napi_create_int32(env, MSM_CURVE_GRUMPKIN, &v);
  napi_set_named_property(env, exports, "CURVE_GRUMPKIN", v);
  napi_create_int32(env, MSM_CURVE_VESTA, &v);
  napi_set_named_property(env, exports, "CURVE_VESTA", v);
  return exports;
}
