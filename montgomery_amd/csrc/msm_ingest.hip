// Point ingest of the C ABI: msm_set_points_ex (compressed points, subgroup validation, the index of the first bad point),
// msm_validate_points and msm_get_points_ex.  The kernels are in points_ingest.h; the plain uncompressed upload stays
// msm_set_points (msm_abi.hip), which msm_set_points_ex calls for that format.
#include "msm_internal.h"
#include "points_ingest.h"

using namespace msm;
using namespace msmi;

namespace {

constexpr uint64_t NO_BAD = ~0ull;

const char* reason_text(uint32_t r) {
  switch (r) {
    case ingest::R_COORD: return "coordinate >= p";
    case ingest::R_FLAGS: return "invalid flags";
    case ingest::R_NO_POINT: return "no curve point";
    case ingest::R_NOT_ON_CURVE: return "not on curve";
    case ingest::R_SUBGROUP: return "not in the prime-order subgroup";
  }
  return "bad point";
}

size_t compressed_bytes(const msm_ctx* ctx) { return ctx->coord_bytes(); }   // one coordinate and its flags

unsigned long long* err_word(msm_ctx* ctx) { return (unsigned long long*)((char*)ctx->errflag.p + 8); }

void err_reset(msm_ctx* ctx) { HIPCHK(hipMemsetAsync(err_word(ctx), 0xFF, 8, ctx->stream)); }

// reads the failure word back (synchronising the stream): NO_BAD or (index << 3) | reason
uint64_t err_read(msm_ctx* ctx) {
  HIPCHK(hipMemcpyAsync(ctx->h_info + 8, err_word(ctx), 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  uint64_t v;
  memcpy(&v, ctx->h_info + 8, 8);
  return v;
}

int fail_point(msm_ctx* ctx, const char* who, uint64_t code, uint64_t* bad_out) {
  if (bad_out) *bad_out = code >> 3;
  return fail(ctx, MSM_ERR_POINT, "%s: point %llu: %s", who, (unsigned long long)(code >> 3), reason_text((uint32_t)(code & 7)));
}

dim3 grid_of(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// curve (and with `subgroup` the prime-order subgroup) check of resident rows [first, first + count) of the current set, into the
// failure word as it stands (which may already hold what an earlier kernel of the call found)
void launch_validate(msm_ctx* ctx, uint64_t first, uint64_t count, int subgroup) {
  if (count) {
    const uint32_t* rows = (const uint32_t*)ctx->pts().rows.p;
    if (ctx->is_te())
      hipLaunchKernelGGL(ingest::k_te_points_validate, grid_of(count), dim3(256), 0, ctx->stream, rows, first, count, subgroup,
                         err_word(ctx));
    else
      W_LAUNCH(ctx, ingest::k_points_validate, grid_of(count), dim3(256), 0, ctx->stream, rows, first, count, subgroup, err_word(ctx));
  }
}

uint64_t validate_rows(msm_ctx* ctx, uint64_t first, uint64_t count, int subgroup) {
  err_reset(ctx);
  launch_validate(ctx, first, count, subgroup);
  return err_read(ctx);
}

// compressed points -> rows of the current point set of ONE device; validate: MSM_VALIDATE_* (a decoded point is on the curve
// by construction, so CURVE costs nothing more than NONE)
int set_compressed_one(msm_ctx* ctx, const void* points, uint64_t n, int on_device, int validate, uint64_t* bad_out) {
  const char* who = "msm_set_points_ex";
  HIPCHK(hipSetDevice(ctx->device));
  uint32_t* rows = ctx->reset_points(n);
  const uint32_t* d_wire = (const uint32_t*)points;
  const size_t cb = compressed_bytes(ctx);
  if (!on_device && n) {
    ctx->ensure(ctx->misc, n * cb);
    upload_staged(ctx, ctx->misc.p, points, n * cb);
    d_wire = (const uint32_t*)ctx->misc.p;
  }
  err_reset(ctx);
  if (n) {
    if (ctx->is_te())
      hipLaunchKernelGGL(ingest::k_te_points_decompress, grid_of(n), dim3(256), 0, ctx->stream, rows, d_wire, n, err_word(ctx));
    else
      W_LAUNCH(ctx, ingest::k_points_decompress, grid_of(n), dim3(256), 0, ctx->stream, rows, d_wire, n, err_word(ctx));
  }
  // the subgroup check runs whatever the decoder found, into the same word: the smallest bad index wins over both (a point
  // the decoder refused holds the identity row, which passes)
  if (validate == MSM_VALIDATE_SUBGROUP) launch_validate(ctx, 0, n, 1);
  const uint64_t code = err_read(ctx);
  if (!on_device) ctx->release(ctx->misc);
  if (code != NO_BAD) return fail_point(ctx, who, code, bad_out);
  ctx->pts().n = n;
  return MSM_OK;
}

// the first bad point of an uncompressed upload msm_set_points refused: the same tests again, with the index (devices[0])
uint64_t locate_uncompressed(msm_ctx* ctx, const void* points, uint64_t n, int on_device, int check_curve) {
  HIPCHK(hipSetDevice(ctx->device));
  const uint32_t* d_wire = (const uint32_t*)points;
  const size_t wb = 2 * ctx->coord_bytes();
  if (!on_device && n) {
    ctx->ensure(ctx->misc, n * wb);
    upload_staged(ctx, ctx->misc.p, points, n * wb);
    d_wire = (const uint32_t*)ctx->misc.p;
  }
  err_reset(ctx);
  if (n) {
    if (ctx->is_te())
      hipLaunchKernelGGL(ingest::k_te_wire_locate, grid_of(n), dim3(256), 0, ctx->stream, d_wire, n, check_curve, err_word(ctx));
    else
      W_LAUNCH(ctx, ingest::k_wire_locate, grid_of(n), dim3(256), 0, ctx->stream, d_wire, n, check_curve, err_word(ctx));
  }
  const uint64_t code = err_read(ctx);
  if (!on_device) ctx->release(ctx->misc);
  return code;
}

void forget_points(msm_ctx* ctx) {
  ctx->pts().n = 0;
  for (msm_ctx* c : ctx->children) c->pts().n = 0;
}

// host-side encoders of msm_get_points_ex
bool le_greater(const uint8_t* a, const uint32_t* w, int nw) {   // little-endian bytes a (4 nw of them) > words w ?
  for (int j = nw - 1; j >= 0; j--) {
    uint32_t v = (uint32_t)a[4 * j] | ((uint32_t)a[4 * j + 1] << 8) | ((uint32_t)a[4 * j + 2] << 16) | ((uint32_t)a[4 * j + 3] << 24);
    if (v != w[j]) return v > w[j];
  }
  return false;
}

void compress_one(int curve, const uint8_t* xy, uint8_t* out) {
  switch (curve) {
    case MSM_CURVE_BLS12_381_G1: {
      bool zero = true;
      for (int b = 0; b < 96; b++) zero &= xy[b] == 0;
      memset(out, 0, 48);
      if (zero) { out[0] = 0xC0; return; }
      for (int b = 0; b < 48; b++) out[b] = xy[47 - b];
      out[0] |= 0x80;
      if (le_greater(xy + 48, Fp381::HALFW, 12)) out[0] |= 0x20;
      return;
    }
    case MSM_CURVE_BLS12_377_G1: {
      bool zero = true;
      for (int b = 0; b < 96; b++) zero &= xy[b] == 0;
      memset(out, 0, 48);
      if (zero) { out[47] = 0x40; return; }
      memcpy(out, xy, 48);
      if (le_greater(xy + 48, Fp377::HALFW, 12)) out[47] |= 0x80;
      return;
    }
    case MSM_CURVE_BN254_G1:
    case MSM_CURVE_GRUMPKIN: {   // the BLS12-377 rules at 32 bytes
      bool zero = true;
      for (int b = 0; b < 64; b++) zero &= xy[b] == 0;
      memset(out, 0, 32);
      if (zero) { out[31] = 0x40; return; }
      memcpy(out, xy, 32);
      if (le_greater(xy + 32, curve == MSM_CURVE_BN254_G1 ? FpBn254::HALFW : FpGrumpkin::HALFW, 8)) out[31] |= 0x80;
      return;
    }
    case MSM_CURVE_PALLAS:   // the identity reads back as (0, 0): x = 0, y even
    case MSM_CURVE_VESTA:
      memcpy(out, xy, 32);
      if (xy[32] & 1) out[31] |= 0x80;
      return;
    default:   // Ed-on-BLS12-377: y and the sign of x
      memcpy(out, xy + 32, 32);
      if (le_greater(xy, Fp253::HALFW, 8)) out[31] |= 0x80;
      return;
  }
}

}  // namespace

extern "C" {

int msm_set_points_ex(msm_ctx* ctx, const void* points, uint64_t n, int on_device, int format, int validate, uint64_t* bad_index_out) {
  const char* who = "msm_set_points_ex";
  if (bad_index_out) *bad_index_out = NO_BAD;
  if (!ctx || (!points && n)) return fail(ctx, MSM_ERR_ARG, "%s: null argument", who);
  if (format != MSM_POINTS_UNCOMPRESSED && format != MSM_POINTS_COMPRESSED) return fail(ctx, MSM_ERR_ARG, "%s: unknown format %d", who, format);
  if (validate < MSM_VALIDATE_NONE || validate > MSM_VALIDATE_SUBGROUP) return fail(ctx, MSM_ERR_ARG, "%s: unknown validation %d", who, validate);
  if (n >= (1ull << 30)) return fail(ctx, MSM_ERR_ARG, "%s: n must be < 2^30", who);
  try {
    if (format == MSM_POINTS_UNCOMPRESSED) {
      const int check_curve = validate >= MSM_VALIDATE_CURVE;
      int rc = msm_set_points(ctx, points, n, on_device, check_curve);
      if (rc == MSM_ERR_POINT) {
        uint64_t code = locate_uncompressed(ctx, points, n, on_device, check_curve);
        if (code == NO_BAD) return rc;
        // the rows before the first refused point are those of valid wire points: a subgroup failure among them comes first
        if (validate == MSM_VALIDATE_SUBGROUP && (code >> 3)) code = std::min(code, validate_rows(ctx, 0, code >> 3, 1));
        return fail_point(ctx, who, code, bad_index_out);
      }
      if (rc != MSM_OK || validate != MSM_VALIDATE_SUBGROUP || !n) return rc;
      HIPCHK(hipSetDevice(ctx->device));
      const uint64_t code = validate_rows(ctx, 0, n, 1);   // one device validates: every device holds the same rows
      if (code == NO_BAD) return MSM_OK;
      forget_points(ctx);
      return fail_point(ctx, who, code, bad_index_out);
    }
    if (ctx->children.empty()) return set_compressed_one(ctx, points, n, on_device, validate, bad_index_out);
    // device list: every device decodes for itself; devices[0] alone runs the subgroup check
    std::vector<uint8_t> host;
    const void* src = points;
    if (on_device && n) {   // the buffer lives on devices[0]: the other devices take it through the host
      host.resize((size_t)n * compressed_bytes(ctx));
      HIPCHK(hipSetDevice(ctx->device));
      HIPCHK(hipMemcpy(host.data(), points, host.size(), hipMemcpyDeviceToHost));
      src = host.data();
    }
    uint64_t bad0 = NO_BAD;
    const int rc = on_all_devices(ctx, [&](msm_ctx* c) {
      if (c == ctx) return set_compressed_one(c, points, n, on_device, validate, &bad0);
      return set_compressed_one(c, src, n, 0, std::min(validate, (int)MSM_VALIDATE_CURVE), nullptr);
    });
    if (rc != MSM_OK) {
      forget_points(ctx);
      if (bad_index_out) *bad_index_out = bad0;
    }
    return rc;
  } MSM_CATCH_ALL(ctx)
}

int msm_validate_points(msm_ctx* ctx, uint64_t first, uint64_t count, int validate, uint64_t* bad_index_out) {
  const char* who = "msm_validate_points";
  if (bad_index_out) *bad_index_out = NO_BAD;
  if (!ctx) return MSM_ERR_ARG;
  if (validate < MSM_VALIDATE_NONE || validate > MSM_VALIDATE_SUBGROUP) return fail(ctx, MSM_ERR_ARG, "%s: unknown validation %d", who, validate);
  if (first > ctx->pts().n || count > ctx->pts().n - first)
    return fail(ctx, MSM_ERR_ARG, "%s: points [%llu, +%llu) but %llu resident points", who, (unsigned long long)first,
                (unsigned long long)count, (unsigned long long)ctx->pts().n);
  if (validate == MSM_VALIDATE_NONE || !count) return MSM_OK;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t code = validate_rows(ctx, first, count, validate == MSM_VALIDATE_SUBGROUP);
    if (code != NO_BAD) return fail_point(ctx, who, code, bad_index_out);
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_get_points_ex(msm_ctx* ctx, uint64_t first, uint64_t count, int format, uint8_t* out) {
  if (!ctx || !out) return fail(ctx, MSM_ERR_ARG, "msm_get_points_ex: null argument");
  if (format == MSM_POINTS_UNCOMPRESSED) return msm_get_points(ctx, first, count, out);
  if (format != MSM_POINTS_COMPRESSED) return fail(ctx, MSM_ERR_ARG, "msm_get_points_ex: unknown format %d", format);
  try {
    const size_t cb = ctx->coord_bytes();
    std::vector<uint8_t> xy((size_t)std::max<uint64_t>(count, 1) * 2 * cb);
    if (int rc = msm_get_points(ctx, first, count, xy.data())) return rc;
    for (uint64_t i = 0; i < count; i++) compress_one(ctx->curve, &xy[(size_t)i * 2 * cb], out + (size_t)i * cb);
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

}  // extern "C"
