// Window tables: T resident tables of the point set, table j = 2^(c j) P, so that the windows of a window group of an MSM share
// one set of buckets (k_table_next, msm_kernels.h).  A call that runs as one group holds a table per window, T = K.  From the
// size at which it runs as two (window_groups_wanted, msm_internal.h) both groups read the SAME T = ceil(K / 2) tables, each
// relative to its own first window, and the host supplies the weight 2^(c T) between them (window_sums_once): half the memory
// and half the build.  The reference has no counterpart (4 GiB of wasm memory); it is what 288 GB of HBM are for: the three
// tables of 2^26 points under the six-window plan are 51.5 GB, the plain rows (table 0) included.  Built once per point set and
// plan -- by the first default-plan msm_run over the whole set, or ahead of it by msm_precompute / msm_reserve -- the way
// k_points_from_wire precomputes beta x once per set.
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace msmi {

// tables a set of n points holds under a plan of K windows: one per window of the widest group a run on them will use
static int tables_held(const msm_ctx* ctx, uint64_t n, int K) {
  const int groups = window_groups_wanted(ctx->is_te(), n, /*tables=*/true, K);
  return (K + groups - 1) / groups;
}
static uint64_t table_bytes(const msm_ctx* ctx, uint64_t n, int T) {
  return (uint64_t)T * std::max<uint64_t>(n, 1) * ctx->row_words() * 4;
}

// Tables of the WHOLE point set go into its row buffer (table 0 = the plain rows), those of a range [lo, lo + n) into a buffer
// of their own.  The old tables are forgotten first and the new ones described last: no way out of here, exceptions included,
// leaves the set describing tables it does not hold.  (An old buffer goes back before a new one is allocated.)
static void build_tables(msm_ctx* ctx, const Plan& pl, uint64_t lo, uint64_t n) {
  msm_ctx::PointSet& ps = ctx->pts();
  msm_ctx::WindowTables& t = ps.tab;
  const bool whole = lo == 0 && n == ps.n;
  const uint64_t row_words = ctx->row_words();
  const int T = tables_held(ctx, n, pl.K);
  const uint64_t bytes = table_bytes(ctx, n, T);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  auto ensure_or_retry = [&](DevBuf& b) {
    try {
      ctx->ensure(b, bytes);
    } catch (const HipFail& f) {
      // the workspaces of earlier calls only grow: give them back and try once more (the next MSM allocates what it needs)
      if (f.e != hipErrorOutOfMemory) throw;
      (void)hipGetLastError();
      release_workspaces(ctx);
      ctx->release(ctx->scal);
      ctx->ensure(b, bytes);
    }
  };
  uint32_t* rows = nullptr;
  if (whole) {
    t.drop();   // (range tables of this set, if any, are replaced)
    if (ps.rows.cap < bytes) {
      // a bigger buffer: table 0 (the plain rows) moves over, the old buffer goes back
      DevBuf big;
      ensure_or_retry(big);
      HIPCHK(hipMemcpyAsync(big.p, ps.rows.p, n * row_words * 4, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      ps.rows = std::move(big);
    }
    rows = (uint32_t*)ps.rows.p;
  } else {
    t.clear();   // (a buffer big enough is reused)
    ensure_or_retry(t.buf);
    rows = (uint32_t*)t.buf.p;
    HIPCHK(hipMemcpyAsync(rows, (const uint32_t*)ps.rows.p + lo * row_words, n * row_words * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }
  const uint32_t grid = (uint32_t)((n + 255) / 256);
  for (int k = 1; k < T; k++) {
    uint32_t* out = rows + (uint64_t)k * n * row_words;
    const uint32_t* in = rows + (uint64_t)(k - 1) * n * row_words;
    if (ctx->is_te()) hipLaunchKernelGGL(te::k_te_table_next, dim3(grid), dim3(256), 0, ctx->stream, out, in, n, pl.c);
    else W_LAUNCH(ctx, k_table_next, dim3(grid), dim3(256), 0, ctx->stream, out, in, n, pl.c);
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  t.c = pl.c;
  t.K = pl.K;
  t.lo = lo;
  t.n = n;
  t.in_rows = whole;
  t.T = T;
}

// can this call run on window tables at all?
static bool tables_eligible(const msm_ctx* ctx, uint64_t n, const msm_opts* opts, bool placed) {
  if (placed || (opts && (opts->no_tables || opts->bucket_shards > 1))) return false;
  if (!ctx->children.empty()) return false;           // a device list shards by points or windows over plain rows
  return point_lo(opts) + n <= ctx->pts().n && n >= 4096;
}
static bool whole_set(const msm_ctx* ctx, uint64_t n, const msm_opts* opts) { return n == ctx->pts().n && point_lo(opts) == 0; }
// tables of the whole set stay: a call over a range of the points neither replaces them nor builds its own (msm_precompute of
// the range, which asks for them explicitly, replaces them when it is sure to build)
static bool whole_set_tables_stay(const msm_ctx* ctx, uint64_t n, const msm_opts* opts) {
  return ctx->pts().tab.whole_set_pinned() && !whole_set(ctx, n, opts);
}
// the tables of n points under a plan of K windows fit the limit, and the entries of a group on them (one per table row and GLV
// half) the 31 bits of the sort's payloads
static bool tables_fit(const msm_ctx* ctx, uint64_t n, int K) {
  const int T = tables_held(ctx, n, K);
  return table_bytes(ctx, n, T) <= ctx->tables_limit && (uint64_t)T * (ctx->is_te() ? n : 2 * n) < (1ull << 31);
}
// tables of plan pl could be built for this call (where tables of the whole set do not stay)
static bool buildable(const msm_ctx* ctx, uint64_t n, const msm_opts* opts, const Plan& pl) {
  return tables_eligible(ctx, n, opts, false) && pl.K >= 2 && tables_fit(ctx, n, pl.K);
}

// A short top window would pile its entries on the lowest buckets of the merged window (a 2-bit top window: an eighth of all
// entries in four buckets): tables are built by default only for plans whose top window is about as wide as the others.
// (Since round 6 the sort cuts such bins into parts, so this is a matter of the tree's depth, no longer of one block's time.)
static bool plan_suits_tables(const Plan& pl) {
  if (pl.K < 2) return false;
  const int top_bits = pl.fold ? pl.c + 1 : pl.bits - (pl.K - 1) * pl.c;
  return top_bits >= pl.c - 3;
}

// Of the calls that may build tables by default, this one builds them now: a call over the whole set at once (the first
// default-plan call over it, as since round 5); a call over a RANGE of the points when it comes back for the same range -- the
// rank of a points-split run does, a caller that walks over the shards on one GPU does not, and a build (c doublings and an
// inversion per point and table: nine MSMs' worth at 2^23 points) per call would cost it far more than the tables return.
static bool builds_now(const msm_ctx* ctx, uint64_t n, const msm_opts* opts, int c) {
  return whole_set(ctx, n, opts) || (ctx->cand_n == n && ctx->cand_lo == point_lo(opts) && ctx->cand_c == c);
}

int make_run_plan(msm_ctx* ctx, uint64_t n, const msm_opts* opts, bool placed, Plan& pl, bool& tables_wanted, bool note_range) {
  tables_wanted = false;
  if (tables_eligible(ctx, n, opts, placed)) {
    const msm_ctx::WindowTables& t = ctx->pts().tab;
    msm_opts o;
    if (opts) o = *opts; else memset(&o, 0, sizeof o);
    const int asked = o.c;
    Plan pt, pd;
    // tables that exist decide: the call uses them if its plan is theirs -- an explicit c, or the default plan they were built
    // for (a default-plan call keeps using tables built by msm_precompute for another c only if that is also what it would pick)
    o.c = asked ? asked : t.c;
    if (t.covers(point_lo(opts), n) && make_plan(ctx, n, &o, pt) == MSM_OK && pt.c == t.c && pt.K == t.K &&
        (asked ? asked == t.c : make_plan(ctx, n, opts, pd, true) == MSM_OK && pd.c == t.c)) {
      pl = pt;
      tables_wanted = true;
      return MSM_OK;
    }
    // none yet (or others): a call with the default plan may build them if they fit the limit --
    // opts->c == 0, or the very window the library would pick (a facade that asks msm_plan first and hands its answer back)
    o.c = 0;
    if (!o.no_glv && make_plan(ctx, n, &o, pt, true) == MSM_OK && (asked == 0 || asked == pt.c) && plan_suits_tables(pt) &&
        buildable(ctx, n, opts, pt) && !whole_set_tables_stay(ctx, n, opts)) {
      const bool build_now = builds_now(ctx, n, opts, pt.c);
      if (note_range && !whole_set(ctx, n, opts)) {
        ctx->cand_lo = point_lo(opts);
        ctx->cand_n = n;
        ctx->cand_c = pt.c;
      }
      // The plan is the tables' plan from the first call on, which is what msm_plan (note_range = false) answers: a call that
      // does not build yet runs the plain path under it.  A caller sizes its slots and cuts its window shards from msm_plan's K,
      // and the sums of the ranks of a points split meet slot by slot: calls 1, 2, 3 ... over one range share one (c, K).
      pl = pt;
      tables_wanted = build_now || !note_range;
      return MSM_OK;
    }
  }
  return make_plan(ctx, n, opts, pl);
}

bool use_window_tables(msm_ctx* ctx, uint64_t n, const msm_opts* opts, Plan& pl) {
  const msm_ctx::PointSet& ps = ctx->pts();
  const uint64_t lo = point_lo(opts);
  if (!(tables_eligible(ctx, n, opts, false) && ps.tab.covers(lo, n) && ps.tab.c == pl.c && ps.tab.K == pl.K)) {
    if (!buildable(ctx, n, opts, pl) || whole_set_tables_stay(ctx, n, opts)) return false;
    build_tables(ctx, pl, lo, n);
  }
  pl.tab_rows = ps.table_rows();
  pl.tab_lo = ps.tab.lo;
  pl.tab_n = ps.tab.n;
  pl.tab_T = ps.tab.T;
  return true;
}

}  // namespace msmi

extern "C" {

int msm_precompute(msm_ctx* ctx, uint64_t n, const msm_opts* opts) {
  if (!ctx) return MSM_ERR_ARG;
  if (int rc = check_points(ctx, n, opts, MSM_ERR_ARG, "msm_precompute", /*empty_ok=*/false)) return rc;
  Plan pl;
  if (make_plan(ctx, n, opts, pl, /*for_tables=*/true)) return fail(ctx, MSM_ERR_ARG, "msm_precompute: bad window size");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    // asked for explicitly, tables of a range replace the whole set's -- if the build goes ahead; if not, those stay
    if (whole_set_tables_stay(ctx, n, opts) && buildable(ctx, n, opts, pl)) ctx->pts().tab.drop();
    (void)use_window_tables(ctx, n, opts, pl);   // not an error if they do not fit: the plain path stays
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_tables_info(const msm_ctx* ctx, int32_t* c_out, int32_t* K_out, uint64_t* bytes_out) {
  if (!ctx) return MSM_ERR_ARG;
  const msm_ctx::WindowTables& t = ctx->pts().tab;
  if (c_out) *c_out = t.c;
  if (K_out) *K_out = t.K;
  if (bytes_out) *bytes_out = t.K ? table_bytes(ctx, t.n, t.T) : 0;
  return MSM_OK;
}

int msm_tables_range(const msm_ctx* ctx, uint64_t* point_lo_out, uint64_t* n_out) {
  if (!ctx) return MSM_ERR_ARG;
  if (point_lo_out) *point_lo_out = ctx->pts().tab.lo;   // (0, 0) without tables
  if (n_out) *n_out = ctx->pts().tab.n;
  return MSM_OK;
}

int msm_set_tables_limit(msm_ctx* ctx, uint64_t bytes) {
  if (!ctx) return MSM_ERR_ARG;
  ctx->tables_limit = bytes;
  for (msm_ctx* c : ctx->children) c->tables_limit = bytes;
  return MSM_OK;
}

}  // extern "C"
