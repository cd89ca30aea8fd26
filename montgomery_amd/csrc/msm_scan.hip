// msm_scalars_scan, msm_scalars_inverse, msm_scalars_div_linear: prefix sums and products, the batch inverse and the division by
// X - z over vectors of 32-byte scalars in device memory, mod the group order q of the context's curve; and the two entries of the
// debug surface that move the tile and report the plan.  The plan, the lane bodies and the kernels are in scalar_scan.h, the
// argument checks in operator_checks.h, the reading of the call's scalars and the table of z's powers in scalar_host.h; here are
// the order of the checks, the aggregate buffer and the launches, one per step, on ctx->stream.  Every check runs before
// anything is written, and the aggregate buffer exists before the first launch.  Every call returns when its result is in place.
// No call touches point sets, window tables or the range-table candidate.
#include "operator_checks.h"
#include "scalar_host.h"
#include "scalar_scan.h"

using namespace msm;
using namespace msmi;

namespace {

// what every call checks before it looks at its scalars
int check_call(msm_ctx* ctx, const char* who, void* dst, const void* a, uint64_t n) {
  if (int rc = vectors_ok(ctx, who, n, {{dst, "dst"}, {a, "a"}}, "n", "dst and a")) return rc;
  return dst_ranges_ok(ctx, who, dst, n * 32, {{a, "a"}});
}

int tile_log_of(const msm_ctx* ctx) { return ctx->scan_tile_log ? ctx->scan_tile_log : scan::DEFAULT_TILE_LOG; }

// the scan of n >= 1 elements: `start` is the value before position 0 in the operator's form, canonical; level0: LV_REVERSE and
// LV_EXCLUSIVE of the call.  total_out (may be null): the inclusive value at the last position, 32 bytes little-endian.
template <class S, int OP>
void run_scan(msm_ctx* ctx, void* dst, const void* a, uint64_t n, uint32_t level0, const Fe<S>& start, const scan::PowTab<S>& pw,
              uint8_t* total_out) {
  const int tile_log = tile_log_of(ctx);
  const scan::Plan plan = scan::scan_plan(n, tile_log);
  // the total, then the aggregates of level 0, of level 1, ...: the top level has none
  size_t units = 1, at[scan::MAX_LEVELS] = {};
  for (int l = 0; l + 1 < plan.levels; l++) {
    at[l] = units;
    units += plan.tiles[l];
  }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ensure(ctx->scan_agg, units * 32);
  uint32_t* const buf = (uint32_t*)ctx->scan_agg.p;
  auto level = [&](int l) {
    scan::Level lv;
    lv.n = l ? plan.tiles[l - 1] : n;
    lv.e_log = (uint32_t)(tile_log - scan::MIN_TILE_LOG);
    lv.flags = l ? (uint32_t)scan::LV_EXCLUSIVE : (scan::LV_DATA | level0);
    lv.shift = l * tile_log;
    return lv;
  };
  auto elements = [&](int l) { return l ? buf + 8 * at[l - 1] : (uint32_t*)dst; };   // what level l scans (level 0: into dst)
  for (int l = 0; l + 1 < plan.levels; l++) {
    const uint32_t* src = l ? buf + 8 * at[l - 1] : (const uint32_t*)a;
    hipLaunchKernelGGL((scan::k_scan_reduce<S, OP>), dim3(plan.tiles[l]), dim3(scan::BLOCK), 0, ctx->stream, buf + 8 * at[l], src, level(l), pw);
    HIPCHK(hipGetLastError());
  }
  for (int l = plan.levels - 1; l >= 0; l--) {
    const uint32_t* src = l ? buf + 8 * at[l - 1] : (const uint32_t*)a;
    const uint32_t* carry = l + 1 < plan.levels ? buf + 8 * at[l] : nullptr;
    hipLaunchKernelGGL((scan::k_scan_apply<S, OP>), dim3(plan.tiles[l]), dim3(scan::BLOCK), 0, ctx->stream, elements(l), src, carry, start,
                       l ? nullptr : buf, level(l), pw);
    HIPCHK(hipGetLastError());
  }
  uint8_t res[32];
  if (total_out) HIPCHK(hipMemcpyAsync(res, buf, 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (total_out) memcpy(total_out, res, 32);
  ctx->last_scan_plan.assign(plan.tiles, plan.tiles + plan.levels);
}

}  // namespace

extern "C" {

int msm_scalars_scan(msm_ctx* ctx, void* dst, const void* a, uint64_t n, int op, uint32_t flags, const uint8_t* init, uint8_t* total_out) {
  const char* const who = "msm_scalars_scan";
  if (!ctx) return MSM_ERR_ARG;
  ctx->last_scan_plan.clear();
  if (int rc = check_call(ctx, who, dst, a, n)) return rc;
  if (op != MSM_SCAN_SUM && op != MSM_SCAN_PRODUCT) return fail(ctx, MSM_ERR_ARG, "%s: op must be MSM_SCAN_SUM or MSM_SCAN_PRODUCT", who);
  if (flags & ~(uint32_t)MSM_SCAN_EXCLUSIVE) return fail(ctx, MSM_ERR_ARG, "%s: unknown flag bits 0x%x", who, flags & ~(uint32_t)MSM_SCAN_EXCLUSIVE);
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      Fe<S> start;
      uint8_t neutral[32] = {(uint8_t)(op == MSM_SCAN_PRODUCT ? 1 : 0)};
      if (!host_scalar<S>(start, init ? init : neutral)) return scalar_too_big(ctx, who, "init");
      if (!n) {
        if (total_out) memcpy(total_out, init ? init : neutral, 32);
        return MSM_OK;
      }
      const uint32_t level0 = (flags & MSM_SCAN_EXCLUSIVE) ? (uint32_t)scan::LV_EXCLUSIVE : 0u;
      const scan::PowTab<S> pw = {};
      if (op == MSM_SCAN_PRODUCT) {
        sv::to_mont<S>(start, start);
        run_scan<S, scan::OP_PRODUCT>(ctx, dst, a, n, level0, start, pw, total_out);
      } else {
        run_scan<S, scan::OP_SUM>(ctx, dst, a, n, level0, start, pw, total_out);
      }
      return MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_div_linear(msm_ctx* ctx, void* dst, const void* a, uint64_t n, const uint8_t* z, uint8_t* rem_out) {
  const char* const who = "msm_scalars_div_linear";
  if (!ctx) return MSM_ERR_ARG;
  ctx->last_scan_plan.clear();
  if (int rc = check_call(ctx, who, dst, a, n)) return rc;
  if (!z) return fail(ctx, MSM_ERR_ARG, "%s: null scalar z", who);
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      Fe<S> zm, start;
      if (!host_scalar_mont<S>(zm, z)) return scalar_too_big(ctx, who, "z");
      if (!n) {
        if (rem_out) memset(rem_out, 0, 32);
        return MSM_OK;
      }
      // z^(2^k) in Montgomery form for every segment length of every level
      scan::PowTab<S> pw = {};
      fill_pow_table<S>(pw, zm, scan::POW_BITS);
      fe_set_zero<S>(start);
      run_scan<S, scan::OP_HORNER>(ctx, dst, a, n, scan::LV_REVERSE | scan::LV_EXCLUSIVE, start, pw, rem_out);
      return MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_inverse(msm_ctx* ctx, void* dst, const void* a, uint64_t n, uint64_t* n_zero_out) {
  const char* const who = "msm_scalars_inverse";
  if (!ctx) return MSM_ERR_ARG;
  if (int rc = check_call(ctx, who, dst, a, n)) return rc;
  if (!n) {
    if (n_zero_out) *n_zero_out = 0;
    return MSM_OK;
  }
  try {
    HIPCHK(hipSetDevice(ctx->device));
    constexpr uint64_t PER_BLOCK = (uint64_t)scan::INV_E * scan::BLOCK;
    const uint32_t blocks = (uint32_t)((n + PER_BLOCK - 1) / PER_BLOCK);
    ctx->ensure(ctx->scan_agg, (size_t)blocks * 4);
    uint32_t* const d_zeros = (uint32_t*)ctx->scan_agg.p;
    for_scalar_field(ctx->curve, [&](auto f) {
      using S = decltype(f);
      hipLaunchKernelGGL((scan::k_inverse<S, scan::INV_E>), dim3(blocks), dim3(scan::BLOCK), 0, ctx->stream, (uint32_t*)dst, (const uint32_t*)a, n,
                         d_zeros);
    });
    HIPCHK(hipGetLastError());
    // the blocks' counts are summed here: no atomics, and 4 bytes per block of elements is a small download
    std::vector<uint32_t> zeros(n_zero_out ? blocks : 0);
    if (n_zero_out) HIPCHK(hipMemcpyAsync(zeros.data(), d_zeros, (size_t)blocks * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (n_zero_out) {
      uint64_t sum = 0;
      for (uint32_t z : zeros) sum += z;
      *n_zero_out = sum;
    }
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_set_scan_tile_log(msm_ctx* ctx, int32_t tile_log) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_scan_tile_log: not on a device-list context");
  if (tile_log != 0 && (tile_log < scan::MIN_TILE_LOG || tile_log > scan::MAX_TILE_LOG))
    return fail(ctx, MSM_ERR_ARG, "msm_test_set_scan_tile_log: tile_log must be 0 (default) or %d .. %d", scan::MIN_TILE_LOG, scan::MAX_TILE_LOG);
  ctx->scan_tile_log = tile_log;
  return MSM_OK;
}

int msm_test_last_scan_plan(msm_ctx* ctx, int32_t* tiles_out, int cap) {
  if (!ctx || !ctx->children.empty() || cap < 0 || (cap && !tiles_out)) return -1;
  const int count = (int)ctx->last_scan_plan.size();
  for (int i = 0; i < count && i < cap; i++) tiles_out[i] = ctx->last_scan_plan[i];
  return count;
}

}  // extern "C"
