// msm_points_mul: D[i] = s[i] * A[a_lo + i], and msm_points_mul_base: D[i] = s[i] * P -- every row under its own scalar, the
// scalars a resident or a host vector (points_mul.h has the algorithm).  The variable-base kernel runs on a fixed grid whose
// per-lane tables live in ctx->pmul_tbl; the fixed-base call keeps one table of rows per context (ctx->pmul_base_tbl), built by
// the variable-base kernel over a broadcast base row and cached with the base's bytes.
// The checks of the context, the count, the sets and their rows are those of operator_checks.h.  Every check runs before anything
// is written.
#include "operator_checks.h"
#include "points_mul.h"

using namespace msm;
using namespace msmi;

namespace {

// rows from which an uncached base gets its table.  In profiles/points_mul_time.txt the table path with its
// build is ahead of the broadcast row at every measured count, 2^10 rows and up: both cost the latency of one row's chain, and the
// paths meet below that, where one launch is less than two
constexpr uint64_t BASE_TABLE_MIN_ROWS = 1ull << 10;

// what both entries check first; the context is not null
int scalars_ok(msm_ctx* ctx, const void* scalars, int on_device, uint64_t count, const char* who) {
  if (int rc = vectors_ok(ctx, who, count, {}, "count")) return rc;
  if (!scalars && count) return fail(ctx, MSM_ERR_ARG, "%s: null scalars", who);
  if (on_device && count && ((uintptr_t)scalars & 15)) return fail(ctx, MSM_ERR_ARG, "%s: device scalars must be aligned to 16 bytes", who);
  return MSM_OK;
}

// blocks per CU of the default grid: as many as the variable-base kernel of the curve keeps resident (its registers set that: 2 on
// the 12-word fields, 3 on the 8-word ones), so the grid is one round of blocks and the table no larger than the lanes in flight
uint32_t blocks_per_cu(msm_ctx* ctx) {
  if (!ctx->pmul_blocks_per_cu) {
    int nb = 0;
    if (ctx->is_te()) HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pmul::k_te_points_mul, pmul::BLOCK, 0));
    else
      for_weierstrass_curve(ctx->curve, [&](auto cv) {
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pmul::k_points_mul<decltype(cv)>, pmul::BLOCK, 0));
      });
    ctx->pmul_blocks_per_cu = std::max(nb, 1);
  }
  return (uint32_t)ctx->pmul_blocks_per_cu;
}

// blocks of the variable-base grid over `count` rows: one round of resident blocks, no more than the rows need and no more than
// the caller's workspace cap lets the table have
uint64_t var_blocks(msm_ctx* ctx, uint64_t count) {
  const uint64_t need = (count + pmul::BLOCK - 1) / pmul::BLOCK;
  uint64_t blocks = ctx->pmul_grid ? (uint64_t)ctx->pmul_grid : std::min<uint64_t>(need, (uint64_t)ctx->n_cu * blocks_per_cu(ctx));
  const uint64_t per_block = pmul::table_bytes(ctx->is_te(), ctx->nw(), 1);
  if (ctx->ws_limit) blocks = std::min<uint64_t>(blocks, ctx->ws_limit / per_block);   // the table counts against the caller's cap
  return std::max<uint64_t>(blocks, 1);
}

// the variable-base kernel over `count` rows: rows + i * row_stride under scalars + 8 i -> out + i * row_words
void launch_var(msm_ctx* ctx, uint32_t* out, const uint32_t* rows, uint32_t row_stride, const uint32_t* d_scal, uint64_t count) {
  ctx->last_pmul[0] = (int32_t)pmul_launch_var(ctx, out, rows, row_stride, d_scal, count);
}

int base_windows(const msm_ctx* ctx) {
  return pmul::windows(ctx->is_te() ? pmul::TE_BITS : curve_info(ctx->curve).glv_max_bits, pmul::W_BASE);
}

// the table of the base whose row is in ctx->pmul_row: one launch of the variable-base kernel over the scalars j 2^(w_b k)
void build_base_table(msm_ctx* ctx) {
  const int nwin = base_windows(ctx);
  const uint64_t t_rows = (uint64_t)nwin << (pmul::W_BASE - 1);
  std::vector<uint32_t> sc(t_rows * 8);
  pmul::table_scalars(sc.data(), pmul::W_BASE, nwin);
  ctx->ensure(ctx->scal, t_rows * 32);
  ctx->ensure(ctx->pmul_base_tbl, t_rows * ctx->row_words() * 4);
  HIPCHK(hipMemcpyAsync(ctx->scal.p, sc.data(), t_rows * 32, hipMemcpyHostToDevice, ctx->stream));
  launch_var(ctx, (uint32_t*)ctx->pmul_base_tbl.p, (const uint32_t*)ctx->pmul_row.p, 0, (const uint32_t*)ctx->scal.p, t_rows);
  HIPCHK(hipStreamSynchronize(ctx->stream));   // (sc and ctx->scal are free again)
}

}  // namespace

namespace msmi {

void pmul_reserve(msm_ctx* ctx, uint64_t count) {
  ctx->ensure(ctx->pmul_tbl, var_blocks(ctx, count) * pmul::table_bytes(ctx->is_te(), ctx->nw(), 1));
}

uint64_t pmul_launch_var(msm_ctx* ctx, uint32_t* out, const uint32_t* rows, uint32_t row_stride, const uint32_t* d_scal, uint64_t count) {
  const uint64_t blocks = var_blocks(ctx, count);
  pmul_reserve(ctx, count);
  const dim3 grid((uint32_t)blocks), block(pmul::BLOCK);
  uint4* tbl = (uint4*)ctx->pmul_tbl.p;
  if (ctx->is_te())
    hipLaunchKernelGGL(pmul::k_te_points_mul, grid, block, 0, ctx->stream, out, rows, row_stride, d_scal, count, tbl);
  else
    W_LAUNCH(ctx, pmul::k_points_mul, grid, block, 0, ctx->stream, out, rows, row_stride, d_scal, count, tbl);
  HIPCHK(hipGetLastError());
  return blocks;
}

}  // namespace msmi

extern "C" {

int msm_points_mul(msm_ctx* ctx, int32_t src, uint64_t a_lo, const void* scalars, int on_device, uint64_t count, int32_t dst) {
  const char* const who = "msm_points_mul";
  if (!ctx) return fail(ctx, MSM_ERR_ARG, "%s: null argument", who);
  if (int rc = scalars_ok(ctx, scalars, on_device, count, who)) return rc;
  for (int32_t id : {src, dst})
    if (int rc = live_set_ok(ctx, who, id)) return rc;
  if (int rc = rows_in_set_ok(ctx, who, src, a_lo, count)) return rc;
  if (int rc = src_in_dst_ok(ctx, who, src, dst, a_lo, count)) return rc;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t rw = ctx->row_words();
    const uint32_t* d_scal = nullptr;
    if (count) stage_scalars(ctx, scalars, count, on_device, &d_scal);
    msm_ctx::PointSet& D = ctx->sets[dst];
    uint32_t* out = ctx->reset_points(D, count);   // (a dst that is the source keeps its buffer: the checked range lies inside it)
    ctx->last_pmul[0] = 0;
    if (count) {
      launch_var(ctx, out, (const uint32_t*)ctx->sets[src].rows.p + a_lo * rw, (uint32_t)rw, d_scal, count);
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->last_pmul[1] = pmul::W_VAR;
    ctx->last_pmul[2] = 0;
    ctx->last_pmul[3] = 0;
    D.n = count;
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_points_mul_base(msm_ctx* ctx, const uint8_t* base_xy, const void* scalars, int on_device, uint64_t count, int32_t dst) {
  const char* const who = "msm_points_mul_base";
  if (!ctx) return fail(ctx, MSM_ERR_ARG, "%s: null argument", who);
  if (int rc = scalars_ok(ctx, scalars, on_device, count, who)) return rc;
  if (int rc = live_set_ok(ctx, who, dst)) return rc;
  // the base: checked and made a row on the host
  const size_t wire_bytes = 2 * ctx->coord_bytes();
  uint32_t xy[24] = {0}, row[ROW_WORDS] = {0};
  if (base_xy) memcpy(xy, base_xy, wire_bytes);
  int bad = 0;
  if (ctx->is_te()) bad = pmul::te_base_row(row, base_xy ? xy : nullptr);
  else for_weierstrass_curve(ctx->curve, [&](auto cv) { bad = pmul::base_row<decltype(cv)>(row, base_xy ? xy : nullptr); });
  if (bad) return fail(ctx, MSM_ERR_POINT, bad == 1 ? "%s: base coordinate >= p" : "%s: base not on the curve", who);
  // the cache key: the base's bytes behind a byte that tells the generator from a caller's point
  uint8_t key[97] = {0};
  key[0] = base_xy ? 1 : 2;
  if (base_xy) memcpy(key + 1, base_xy, wire_bytes);
  try {
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t rw = ctx->row_words();
    const bool cached = ctx->pmul_base_cached && memcmp(key, ctx->pmul_base_key, sizeof key) == 0;
    const bool table = ctx->pmul_base_path == 1 || (ctx->pmul_base_path == 0 && (cached || count >= BASE_TABLE_MIN_ROWS));
    ctx->last_pmul[0] = 0;
    if (count && !(table && cached)) {
      ctx->ensure(ctx->pmul_row, sizeof row);
      HIPCHK(hipMemcpyAsync(ctx->pmul_row.p, row, rw * 4, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (count && table && !cached) {
      ctx->pmul_base_cached = false;
      build_base_table(ctx);
      memcpy(ctx->pmul_base_key, key, sizeof key);
      ctx->pmul_base_cached = true;
    }
    const uint32_t* d_scal = nullptr;
    if (count) stage_scalars(ctx, scalars, count, on_device, &d_scal);
    msm_ctx::PointSet& D = ctx->sets[dst];
    uint32_t* out = ctx->reset_points(D, count);
    if (count) {
      if (table) {
        const dim3 grid((uint32_t)((count + pmul::BLOCK - 1) / pmul::BLOCK)), block(pmul::BLOCK);
        const uint32_t* tbl = (const uint32_t*)ctx->pmul_base_tbl.p;
        if (ctx->is_te()) hipLaunchKernelGGL(pmul::k_te_points_mul_base, grid, block, 0, ctx->stream, out, d_scal, count, tbl);
        else W_LAUNCH(ctx, pmul::k_points_mul_base, grid, block, 0, ctx->stream, out, d_scal, count, tbl);
        HIPCHK(hipGetLastError());
        ctx->last_pmul[0] = (int32_t)grid.x;
      } else {
        launch_var(ctx, out, (const uint32_t*)ctx->pmul_row.p, 0, d_scal, count);
      }
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->last_pmul[1] = table ? pmul::W_BASE : pmul::W_VAR;
    ctx->last_pmul[2] = table ? 1 : 2;
    ctx->last_pmul[3] = table ? (int32_t)((uint64_t)base_windows(ctx) << (pmul::W_BASE - 1)) : 0;
    D.n = count;
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

}  // extern "C"
