// msm_run_narrow: an MSM whose scalars are declared narrow -- 1-, 2-, 4-, 8- or 16-byte integers, or 32-byte field elements
// holding small values -- of `bits` magnitude bits.  No endomorphism split (it would spread a 64-bit scalar over two halves of
// ~126 bits), one entry per point, K = ceil((bits + 1) / c) windows: the plan of msm_opts.no_glv with the scalar length taken
// from the call (make_plan), its digits from k_digits_narrow (narrow_kernels.h); the sort, the tree and the reduction run
// unchanged.  Always the plain path over table 0: window tables are neither built, used nor dropped.
// The reference has no counterpart (its fromPackedBytesSmall, src/scalar-glv.ts:44, is the codec of a GLV half).
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace msmi {

int narrow_format(msm_ctx* ctx, int32_t width_bytes, int32_t bits, int32_t is_signed, const msm_opts* opts, const char* who,
                  Plan::Narrow& out) {
  const int w = width_bytes;
  if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16 && w != 32)
    return fail(ctx, MSM_ERR_ARG, "%s: width_bytes must be 1, 2, 4, 8, 16 or 32 (got %d)", who, w);
  if (is_signed != 0 && is_signed != 1) return fail(ctx, MSM_ERR_ARG, "%s: is_signed must be 0 or 1", who);
  const int full = w == 32 ? 128 : 8 * w - (is_signed ? 1 : 0);   // magnitude bits the width can hold (128 at most)
  if (bits == 0 && w == 32) return fail(ctx, MSM_ERR_ARG, "%s: width 32 needs bits (1 .. 128)", who);
  if (bits < 0 || bits > 128 || bits > full)
    return fail(ctx, MSM_ERR_ARG, "%s: bits = %d is beyond what %d-byte %s scalars hold (%d; 128 at most)", who, bits, w,
                is_signed ? "signed" : "unsigned", full);
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "%s: narrow scalars run on single-device contexts only", who);
  if (int rc = refuse_shard_opts(ctx, opts, who, "a narrow")) return rc;
  out = Plan::Narrow();
  out.width = w;
  out.fmt.bits = bits ? bits : full;
  out.fmt.is_signed = is_signed;
  const uint32_t* q = curve_info(ctx->curve).q;
  for (int j = 0; j < 8; j++) out.fmt.q[j] = q[j];
  return MSM_OK;
}

int narrow_scalars_ok(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, int32_t width_bytes, const char* who) {
  if (n >> 32) return fail(ctx, MSM_ERR_ARG, "%s: more than 2^32 - 1 scalars", who);
  if (on_device && n && (uintptr_t)scalars % (uintptr_t)std::min(width_bytes, 16))
    return fail(ctx, MSM_ERR_ARG, "%s: device scalars must be aligned to %d bytes", who, std::min(width_bytes, 16));
  return MSM_OK;
}

const char* narrow_lane_base(const char* dev, int32_t width_bytes, Plan::Narrow& nar) {
  const uintptr_t align = (uintptr_t)std::max(4, std::min(width_bytes, 16));
  const uintptr_t off = (uintptr_t)dev % align;
  nar.first = off / width_bytes;
  return dev - off;
}

// Host scalars are uploaded whole before the run (2 - 32 x smaller than the wide form), timed as up_ms; device scalars stay where
// they are.  Returns the device array.
const char* stage_narrow(msm_ctx* ctx, const void* scalars, size_t bytes, int on_device, float* up_ms) {
  if (on_device) return (const char*)scalars;
  HIPCHK(hipEventRecord(ctx->ev[11], ctx->stream));
  ctx->ensure(ctx->scal, bytes + 16);
  upload_staged(ctx, ctx->scal.p, scalars, bytes);
  HIPCHK(hipEventRecord(ctx->ev[10], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipEventElapsedTime(up_ms, ctx->ev[11], ctx->ev[10]));
  return (const char*)ctx->scal.p;
}

}  // namespace msmi

extern "C" {

int msm_plan_narrow(const msm_ctx* ctx, uint64_t n, int32_t bits, const msm_opts* opts, int32_t* c_out, int32_t* K_out) {
  if (!ctx || bits < 1 || bits > 128) return fail(const_cast<msm_ctx*>(ctx), MSM_ERR_ARG, "msm_plan_narrow: bits must be 1 .. 128");
  Plan pl;   // plain arithmetic: nothing here can throw
  if (int rc = make_plan(ctx, n, opts, pl, false, bits)) return rc;
  if (c_out) *c_out = pl.c;
  if (K_out) *K_out = pl.K;
  return MSM_OK;
}

int msm_run_narrow(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, int32_t width_bytes, int32_t bits, int32_t is_signed,
                   const msm_opts* opts, msm_result* out) {
  if (!ctx || !out || (!scalars && n)) return fail(ctx, MSM_ERR_ARG, "msm_run_narrow: null argument");
  Plan pl;
  Plan::Narrow nar;
  if (int rc = narrow_format(ctx, width_bytes, bits, is_signed, opts, "msm_run_narrow", nar)) return rc;
  if (int rc = check_points(ctx, n, opts, MSM_ERR_NO_POINTS, "msm_run_narrow")) return rc;
  if (int rc = narrow_scalars_ok(ctx, scalars, n, on_device, width_bytes, "msm_run_narrow")) return rc;
  if (make_plan(ctx, n, opts, pl, false, nar.fmt.bits)) return fail(ctx, MSM_ERR_ARG, "msm_run_narrow: bad window size");
  if (!call_begin(ctx, pl, n, out)) return MSM_OK;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    float up_ms = 0;
    const char* dev = stage_narrow(ctx, scalars, (size_t)n * width_bytes, on_device, &up_ms);
    dev = narrow_lane_base(dev, width_bytes, nar);
    pl.nar = nar;
    std::vector<uint32_t> words;
    window_sums_impl(ctx, dev, n, 1, opts, 0, pl.K, pl, words, out, point_lo(opts));
    call_finish(ctx, words, pl, out, up_ms);
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_scalar_bits(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, int32_t* unsigned_bits_out, int32_t* signed_bits_out) {
  if (!ctx || (!scalars && n)) return fail(ctx, MSM_ERR_ARG, "msm_scalar_bits: null argument");
  if (int rc = narrow_scalars_ok(ctx, scalars, n, on_device, 32, "msm_scalar_bits")) return rc;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    uint32_t got[2] = {0, 0};
    if (n) {
      const uint32_t* d_scal = nullptr;
      stage_scalars(ctx, scalars, n, on_device, &d_scal);
      ctx->ensure(ctx->misc, 64);
      HIPCHK(hipMemsetAsync(ctx->misc.p, 0, 8, ctx->stream));
      NarrowFmt f{};
      const uint32_t* q = curve_info(ctx->curve).q;
      for (int j = 0; j < 8; j++) f.q[j] = q[j];
      const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16);
      hipLaunchKernelGGL(k_scalar_bits, dim3(grid), dim3(256), 0, ctx->stream, (uint32_t*)ctx->misc.p, d_scal, n, f);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(ctx->h_info, ctx->misc.p, 8, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      got[0] = ctx->h_info[0];
      got[1] = ctx->h_info[1];
    }
    if (unsigned_bits_out) *unsigned_bits_out = (int32_t)got[0];
    if (signed_bits_out) *signed_bits_out = (int32_t)got[1];
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

}  // extern "C"
