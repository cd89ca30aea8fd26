// msm_run_batch: B MSMs over the same resident points.  Where one MSM is mostly fixed latency (launches, read-backs, short
// dependent chains: below ~2^20 points), the batch runs FUSED: element b's window k becomes virtual window b K + k of one
// window group, so B elements share every launch of the digits, the sort, the tree and the bucket reduction -- the sort and
// the tree do not care which scalar a window came from.  Elsewhere the call runs element by element through msm_run.
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace msmi {

// Window of a fused batch.  msm_run's rule (pick_window) takes 16 bits from 2^12 points because a smaller window mostly buys
// more rounds of fixed latency; in a batch those rounds are shared and the bucket work grows with B.  Measured with
// tools/batch_time.py --csweep, c = 10 .. 16 (profiles/batch_msm_time.txt): BLS12-377 after GLV wants 13 bits (K = 10) from
// B = 16 at 2^12 .. 2^18 points (2^14 x 16: 3.44 ms against 7.35 at 16 bits; 2^18 x 64: 61.7 / 63.9) and at B = 4 up to 2^14
// points (2^14: 1.88 / 2.04), but keeps 16 at B = 4 from 2^16 (2.50 / 2.63).  Ed-on-BLS12-377 wants 12 bits (2^12 x 16: 1.35 ms
// against 1.78 at the cost model's 7; 2^14 x 64: 5.98 / 6.29 at its 9) and 14 from 2^17 points at B >= 16 (2^18 x 64: 40.9 / 43.1).  Other inputs (fewer than 2^12 points, no_glv) keep msm_run's window.
// BN254 G1, Grumpkin and Vesta run under the same rule, model only (not swept).
int pick_window_batch(bool te, uint64_t n, uint32_t B, int glv_max_bits) {
  if (te) return n < 4096 ? pick_window(te, n, glv_max_bits) : (n >= (1ull << 17) && B >= 16) ? 14 : 12;
  if (glv_max_bits && n >= 4096 && (B >= 16 || n <= (1ull << 14))) return 13;
  return pick_window(te, n, glv_max_bits);
}

std::vector<const uint32_t*> stage_batch_scalars(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, int on_device,
                                                 const Plan& pl) {
  std::vector<const uint32_t*> sc(B);
  if (on_device) {
    for (uint32_t b = 0; b < B; b++) sc[b] = (const uint32_t*)scalars[b];
  } else {
    // (narrow elements, msm_run_batch_narrow: n x width bytes each, every element on a 16-byte boundary)
    const size_t el_bytes = (size_t)n * (pl.nar.width ? pl.nar.width : 32), el_stride = (el_bytes + 15) & ~(size_t)15;
    ctx->ensure(ctx->scal, (size_t)B * el_stride);
    for (uint32_t b = 0; b < B; b++) {
      sc[b] = (const uint32_t*)((const char*)ctx->scal.p + (size_t)b * el_stride);
      upload_staged(ctx, (void*)sc[b], scalars[b], el_bytes);
    }
  }
  return sc;
}

void bind_batch_scalars(Plan& pl, NarrowBatchScalars& nbs, const std::vector<const uint32_t*>& sc, int b0, int cnt) {
  pl.batch = cnt;
  if (pl.nar.width) {
    for (int j = 0; j < cnt; j++) nbs.p[j] = sc[b0 + j];
    pl.nar.nb = &nbs;
  } else {
    for (int j = 0; j < cnt; j++) pl.batch_sc.p[j] = sc[b0 + j];
  }
}

}  // namespace msmi

namespace {

constexpr int GROUP_WINDOWS = 128;   // windows of one group under the one-level sort (group_schedule)

// where a batch may fuse at all: B >= 2, one device, fewer entries per window than the radix split takes
bool fuse_region(const msm_ctx* ctx, uint64_t n, uint32_t B) {
  const uint64_t entries = ctx->is_te() ? n : 2 * n;
  return B >= 2 && ctx->children.empty() && entries < one_level_entry_limit(ctx->is_te());
}

// the call fuses: inside the region, under a plan of the one-level sort (c <= 16)
bool fuse(const msm_ctx* ctx, uint64_t n, uint32_t B, const Plan& pl) {
  if (!fuse_region(ctx, n, B) || pl.c > 16 || pl.fold) return false;
  return pl.K <= GROUP_WINDOWS / 2;   // (at least two elements per group)
}

// one group of elements [b0, b0 + cnt): its kc = cnt K window sums -> part (kc slots)
void run_batch_group(msm_ctx* ctx, msm_ctx::Workspace& w, const Plan& pl_in, const std::vector<const uint32_t*>& sc, int b0, int cnt,
                     uint64_t n, uint64_t p_lo, bool lone, uint32_t* part, GroupStats& st) {
  Plan pl = pl_in;
  pl.lone = lone;
  NarrowBatchScalars nbs{};   // (narrow elements: up to NARROW_BATCH_MAX pointers, k_digits_narrow_batch)
  bind_batch_scalars(pl, nbs, sc, b0, cnt);
  const int kc = cnt * pl.K;
  SortOut so;
  HIPCHK(hipEventRecord(w.ev[0], w.stream));
  sort_window_group(ctx, w, nullptr, n, pl, 0, kc, st, so);
  st.max_bucket = std::max<uint64_t>(st.max_bucket, so.max_bucket);
  HIPCHK(hipEventRecord(w.ev[5], w.stream));
  TreeOut to;
  accumulate_window_group(ctx, w, pl, kc, p_lo, so, st, to);
  // unmerged: a merged reduction would fold the windows of different elements into one slot
  reduce_buckets(ctx, w, to.bucket_proj, pl.L, kc, part, false, pl.c);
  add_group_times(w, st);
}

int run_fused(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, int on_device, const msm_opts* opts, const Plan& pl,
              msm_result* out) {
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipEventRecord(ctx->ev[8], ctx->stream));
  const std::vector<const uint32_t*> sc = stage_batch_scalars(ctx, scalars, B, n, on_device, pl);
  HIPCHK(hipEventRecord(ctx->ev[9], ctx->stream));
  // groups of whole elements: at most 128 windows, BATCH_MAX elements, and what the workspace budget gives one group
  const uint64_t budget = ctx->ws_limit ? ctx->ws_limit : ctx->ws_budget;
  const long double room = (long double)budget / msm_ctx::N_WS / window_bytes(ctx, n, pl);
  const int wpg = (int)std::max<long double>(1, std::min<long double>(room, GROUP_WINDOWS));
  int per = std::max(1, std::min(wpg / pl.K, pl.nar.width ? NARROW_BATCH_MAX : BATCH_MAX));
  const int n_groups = (int)((B + per - 1) / per);
  per = (int)((B + n_groups - 1) / n_groups);   // even groups
  const int pw = ctx->sum_words();
  std::vector<uint32_t> words((size_t)B * pl.K * pw);
  HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // scalars and the error flag are in place before the group streams start
  const uint64_t p_lo = point_lo(opts);
  const bool serial = opts && opts->serial;
  ctx->last_sort_paths.clear();   // (a fused batch is not recorded: no report of an earlier call stays behind)
  GroupStats sts[msm_ctx::N_WS];
  run_on_workspaces(ctx, n_groups, serial, [&](int slot, int g) {
    const int b0 = g * per, cnt = std::min<int>(per, (int)B - b0);
    run_batch_group(ctx, ctx->ws[slot], pl, sc, b0, cnt, n, p_lo, serial, &words[(size_t)b0 * pl.K * pw], sts[slot]);
  });
  // (ev[10] goes in front of the read-back: the synchronisation below then covers it, and hipEventElapsedTime reads it once it
  // has completed -- an event recorded behind that synchronisation may still be pending when the host asks)
  HIPCHK(hipEventRecord(ctx->ev[10], ctx->stream));
  check_scalar_flags(ctx, pl, "msm_run_batch_narrow");
  // per element: the Horner step over its K window sums and the conversion to affine (one field inversion each), spread over
  // host threads -- ~0.03 ms per element on one thread
  const auto t0 = std::chrono::steady_clock::now();
  auto finish = [&](uint32_t b) { sums_finish(ctx, &words[(size_t)b * pl.K * pw], pl.K, pl.c, &out[b]); };
  const uint32_t n_fin = std::min<uint32_t>(8, B / 4);
  if (n_fin <= 1) {
    for (uint32_t b = 0; b < B; b++) finish(b);
  } else {
    std::atomic<uint32_t> nb{0};
    auto fin_worker = [&] {
      for (uint32_t b; (b = nb.fetch_add(1)) < B;) finish(b);
    };
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < n_fin; t++) {
      try { th.emplace_back(fin_worker); } catch (const std::system_error&) { break; }
    }
    fin_worker();
    for (auto& t : th) t.join();
  }
  const float fin_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  GroupStats st;
  for (const GroupStats& g : sts) st += g;
  float up_ms, tot_ms;
  HIPCHK(hipEventElapsedTime(&up_ms, ctx->ev[8], ctx->ev[9]));
  HIPCHK(hipEventElapsedTime(&tot_ms, ctx->ev[8], ctx->ev[10]));
  for (uint32_t b = 0; b < B; b++) {
    msm_result& r = out[b];
    r.c = pl.c;
    r.K = pl.K;
    r.tables = 0;
    stats_to_result(st, &r);
    r.phase_ms[MSM_T_UPLOAD] = up_ms;
    r.phase_ms[MSM_T_FINAL] = fin_ms;
    r.phase_ms[MSM_T_TOTAL] = tot_ms + fin_ms;
  }
  return MSM_OK;
}

// element by element through run_one(b), which fills out[b] -- msm_run (its window tables included) or msm_run_narrow; the
// statistics of the whole call go into every element
int run_each(uint32_t B, msm_result* out, const std::function<int(uint32_t)>& run_one) {
  msm_result tot;
  memset(&tot, 0, sizeof tot);
  for (uint32_t b = 0; b < B; b++) {
    if (int rc = run_one(b)) return rc;
    add_call_stats(tot, out[b]);
  }
  for (uint32_t b = 0; b < B; b++) {
    memcpy(out[b].phase_ms, tot.phase_ms, sizeof tot.phase_ms);
    out[b].rounds = tot.rounds;
    out[b].n_pairs = tot.n_pairs;
    out[b].n_pairs_algo = tot.n_pairs_algo;
    out[b].max_bucket = tot.max_bucket;
  }
  return MSM_OK;
}

}  // namespace

extern "C" int msm_run_batch(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, int on_device, const msm_opts* opts,
                             msm_result* out) {
  if (!ctx || !out || !scalars || B == 0) return fail(ctx, MSM_ERR_ARG, "msm_run_batch: null argument or empty batch");
  for (uint32_t b = 0; b < B && n; b++)
    if (!scalars[b]) return fail(ctx, MSM_ERR_ARG, "msm_run_batch: no scalars for element %u", b);
  if (int rc = refuse_shard_opts(ctx, opts, "msm_run_batch", "a batch")) return rc;
  if (int rc = check_points(ctx, n, opts, MSM_ERR_NO_POINTS, "msm_run_batch")) return rc;
  try {
    if (n) {
      Plan pl;
      msm_opts o;
      if (opts) o = *opts; else memset(&o, 0, sizeof o);
      const bool te = ctx->is_te();
      const int glv_bits = curve_info(ctx->curve).glv_max_bits;
      if (o.c <= 0) o.c = pick_window_batch(te, n, B, o.no_glv ? 0 : glv_bits);
      if (make_plan(ctx, n, &o, pl)) return fail(ctx, MSM_ERR_ARG, "msm_run_batch: bad window size");
      bool fused = fuse(ctx, n, B, pl);
      int fuse_knob = -1;
      MSM_KNOB(fuse_knob, "MSM_BATCH_FUSE", 0);   // (tuning builds: 0 = element by element, the sequential form for A/B runs)
      if (fuse_knob == 0) fused = false;
      if (fused) {
        for (uint32_t b = 0; b < B; b++) memset(&out[b], 0, sizeof(msm_result));
        return run_fused(ctx, scalars, B, n, on_device, opts, pl, out);
      }
    }
    return run_each(B, out, [&](uint32_t b) { return msm_run(ctx, scalars[b], n, on_device, opts, &out[b]); });
  } MSM_CATCH_ALL(ctx)
}

// msm_run_batch over narrow scalars (msm_narrow.hip has the format): the same fused groups, their digits from
// k_digits_narrow_batch; with K as small as 1 .. 5 a group of 128 windows holds up to NARROW_BATCH_MAX elements.  Outside the
// fused region -- or where a device pointer is not aligned to the load of a lane -- element by element through msm_run_narrow.
extern "C" int msm_run_batch_narrow(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, int on_device, int32_t width_bytes,
                                    int32_t bits, int32_t is_signed, const msm_opts* opts, msm_result* out) {
  if (!ctx || !out || !scalars || B == 0) return fail(ctx, MSM_ERR_ARG, "msm_run_batch_narrow: null argument or empty batch");
  for (uint32_t b = 0; b < B && n; b++)
    if (!scalars[b]) return fail(ctx, MSM_ERR_ARG, "msm_run_batch_narrow: no scalars for element %u", b);
  Plan::Narrow nar;
  if (int rc = narrow_format(ctx, width_bytes, bits, is_signed, opts, "msm_run_batch_narrow", nar)) return rc;
  if (int rc = check_points(ctx, n, opts, MSM_ERR_NO_POINTS, "msm_run_batch_narrow")) return rc;
  for (uint32_t b = 0; b < B; b++)
    if (int rc = narrow_scalars_ok(ctx, scalars[b], n, on_device, width_bytes, "msm_run_batch_narrow")) return rc;
  try {
    if (n) {
      // Where msm_run_batch fuses (B >= 2, one device, fewer than 2^21 entries per window) the elements share every launch only
      // under the one-level sort, c <= 16 -- so there the single-call rule, which takes 17 bits from 2^18 points for scalars of
      // up to 32 bits, gives way to its one-level form (the cost model capped at 13 bits).  That choice is NOT measured against
      // running the elements one by one at 17 bits: tools/narrow_time.py times single calls only.
      Plan pl;
      msm_opts o;
      if (opts) o = *opts; else memset(&o, 0, sizeof o);
      if (o.c <= 0 && fuse_region(ctx, n, B)) o.c = pick_window_narrow(ctx->is_te(), n, nar.fmt.bits, /*one_level=*/true);
      if (make_plan(ctx, n, &o, pl, false, nar.fmt.bits)) return fail(ctx, MSM_ERR_ARG, "msm_run_batch_narrow: bad window size");
      pl.nar = nar;
      bool fused = fuse(ctx, n, B, pl);
      // (1- and 2-byte device scalars may start inside a dword; the fused digit kernel wants every element on a dword)
      for (uint32_t b = 0; b < B && on_device; b++) fused &= ((uintptr_t)scalars[b] & 3) == 0;
      if (fused) {
        for (uint32_t b = 0; b < B; b++) memset(&out[b], 0, sizeof(msm_result));
        return run_fused(ctx, scalars, B, n, on_device, opts, pl, out);
      }
    }
    return run_each(B, out, [&](uint32_t b) {
      return msm_run_narrow(ctx, scalars[b], n, on_device, width_bytes, bits, is_signed, opts, &out[b]);
    });
  } MSM_CATCH_ALL(ctx)
}
