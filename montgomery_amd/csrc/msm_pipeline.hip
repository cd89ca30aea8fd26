// One MSM as window groups on the context's two streams, ranges of the points where a window does not fit or the scalars
// arrive over PCIe -- cut as group_schedule (msm_plan.hip) says --, the fan-out over the devices of a multi-device context, and
// the begin and finish the full-MSM entry points share.
// (reference: the SPMD threads of src/msm-batched-affine.ts:285-340; windows are independent until :312-333)
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace {

// Partition sums P_k for windows [k_lo, k_hi) over the points [p_lo, p_lo + n) -> slot k - k_lo of h_partials_out
// scalars: device pointer, n x 8 words.
// On window tables every group reads table j = 2^(c j) P for its window k_lo + j: its sum is relative to its OWN first window.
void run_window_group(msm_ctx* ctx, msm_ctx::Workspace& w, const uint32_t* d_scalars_all, uint64_t p_lo, uint64_t n, const Plan& pl_in,
                      int k_lo, int k_hi, uint32_t* h_partials_out, GroupStats& st, int32_t& path, uint64_t p_off = 0, const GroupDigits* share = nullptr) {
  hipStream_t s = w.stream;
  Plan pl = pl_in;
  const uint32_t* d_scalars = group_scalars(d_scalars_all, p_lo, pl);   // scalar i of the call <-> resident point p_off + i
  const uint32_t* idx = pl.idx ? pl.idx + p_lo : nullptr;               // (indexed call: <-> resident point idx[i])
  p_lo += p_off;
  const int kc = k_hi - k_lo;
  SortOut so;
  HIPCHK(hipEventRecord(w.ev[0], s));
  sort_window_group(ctx, w, d_scalars, n, pl, k_lo, k_hi, st, so, share);
  st.max_bucket = std::max<uint64_t>(st.max_bucket, so.max_bucket);
  path = so.path;
  if (idx) {
    // msm_run_indexed: the payloads name positions of the group; round 1 gathers rows of the whole resident table by them, so
    // they are rewritten to name the rows of idx[position] first (one coalesced pass whatever sort path wrote them)
    if (pl.tables || p_off) throw MsmFail{MSM_ERR_INTERNAL, "an indexed group on window tables or over a range of the points"};
    translate_payloads(s, ctx, const_cast<uint32_t*>(so.round1_slots), so.total_slots, idx);
    p_lo = 0;
  }
  HIPCHK(hipEventRecord(w.ev[5], s));   // the tree starts here
  TreeOut to;
  if (pl.tables) {
    // one merged window over the tables 0 .. kc - 1: its sum carries the windows' weights relative to the group's first window
    // already.  It goes into the group's first slot, identities into the others.
    if (kc > pl.tab_T) throw MsmFail{MSM_ERR_INTERNAL, "a window group on window tables with more windows than tables"};
    accumulate_window_group(ctx, w, pl, 1, 0, so, st, to);
    reduce_buckets(ctx, w, to.bucket_proj, pl.L, 1, h_partials_out, pl.merged, pl.c);
    for (int kk = 1; kk < kc; kk++) sum_set_identity(ctx, h_partials_out + (size_t)kk * ctx->sum_words());
  } else {
    accumulate_window_group(ctx, w, pl, kc, p_lo, so, st, to);
    reduce_buckets(ctx, w, to.bucket_proj, pl.L, kc, h_partials_out, pl.merged, pl.c);
  }
  add_group_times(w, st);
}

// ---- one call = prepare (scalars, budget, schedule), run (the schedule's groups on the two workspaces), combine (their sums) ----

// A call of window_sums_once between its steps: where its scalars are and how it is cut
struct CallSetup {
  const uint32_t* d_scal = nullptr;
  std::vector<uint64_t> piece_end;   // pipelined upload: point index where piece q ends (the last = n); empty: staged
  GroupSchedule sch;
};

// Host scalars of a big call cross PCIe BEHIND the computation, range by range of the points (PieceUpload); everything
// else is staged before the window groups start.  Records ev[8] .. ev[9] around the staging.
CallSetup prepare_call(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, bool serial, int k_lo, int k_hi, const Plan& pl,
                       uint64_t p_off) {
  CallSetup cs;
  HIPCHK(hipEventRecord(ctx->ev[8], ctx->stream));
  if (!on_device && pipelines_host_scalars(n)) {
    cs.piece_end = pipelined_piece_ends(n);
    ctx->ensure(ctx->scal, n * 32);   // before the workspace budget is taken from what the device has free
  } else {
    stage_scalars(ctx, scalars, n, on_device, &cs.d_scal);
  }
  HIPCHK(hipEventRecord(ctx->ev[9], ctx->stream));
  if (ctx->ws_limit) {
    ctx->ws_budget = ctx->ws_limit;
  } else if (n >= (1ull << 22)) {
    // big inputs: the budget is what the device has free NOW (point sets, scalar buffers and other contexts have come and
    // gone since the context was made) plus what the workspaces already hold
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    ctx->ws_budget = (uint64_t)((free_b + ctx->workspace_bytes()) * 0.85L);
  }
  cs.sch = group_schedule(ctx, n, p_off, k_lo, k_hi, pl, cs.piece_end, serial);
  if (cs.sch.piped) {
    cs.d_scal = (const uint32_t*)ctx->scal.p;
  } else if (!cs.piece_end.empty()) {
    // the workspace forces its own ranges: plain staged upload first
    cs.piece_end.clear();
    stage_scalars(ctx, scalars, n, on_device, &cs.d_scal);
  }
  return cs;
}

// Runs the groups of cs.sch under `pl` (the call's plan, its tables as the schedule left them): part[gi] = the sums of group gi,
// one slot per window of the group; st = the statistics of all groups.  Returns the wall time of a pipelined upload, or -1.
float run_groups(msm_ctx* ctx, const CallSetup& cs, const void* scalars, uint64_t n, const Plan& pl, bool serial, uint64_t p_off,
                 std::vector<std::vector<uint32_t>>& part, GroupStats& st) {
  const std::vector<GroupSchedule::Group>& groups = cs.sch.groups;
  const int pw = ctx->sum_words();
  ctx->last_sort_paths.clear();   // (a call that fails on its way reports nothing, not the call before it)
  HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // staged scalars are in place before the group streams start
  std::unique_ptr<PieceUpload> pipe;
  if (cs.sch.piped) {
    std::vector<size_t> ends;
    for (uint64_t e : cs.piece_end) ends.push_back((size_t)e * 32);
    pipe.reset(new PieceUpload(ctx, ctx->scal.p, scalars, n * 32, ends));
  }
  GroupDigits share;
  if (cs.sch.share_digits) {
    // one digit launch over both groups' windows, on the first workspace (only the bin split takes its histograms from there)
    HIPCHK(hipEventRecord(ctx->ev_dig[0], ctx->ws[0].stream));
    Plan pd = pl;
    const uint32_t* d_grp = group_scalars(cs.d_scal, groups[0].p_lo, pd);
    const SortGeometry g = sort_geometry(ctx, groups[0].p_n, pd, groups[0].ka, groups[1].kb);
    if (g.bin_split) share = launch_group_digits(ctx, ctx->ws[0], d_grp, groups[0].p_n, pd, groups[0].ka, g, ctx->ev_dig[1]);
  }
  Plan pg = pl;
  pg.lone = cs.sch.lone;
  GroupStats sts[msm_ctx::N_WS];
  part.assign(groups.size(), {});
  std::vector<int32_t> paths(groups.size(), -1);
  run_on_workspaces(ctx, (int)groups.size(), serial, [&](int slot, int gi) {
    const GroupSchedule::Group& g = groups[gi];
    part[gi].resize((size_t)(g.kb - g.ka) * pw);
    if (g.piece >= 0) pipe->wait_piece(g.piece, ctx->ws[slot].stream);
    run_window_group(ctx, ctx->ws[slot], cs.d_scal, g.p_lo, g.p_n, pg, g.ka, g.kb, part[gi].data(), sts[slot], paths[gi], p_off,
                     share.valid ? &share : nullptr);
  });
  ctx->last_sort_paths = std::move(paths);
  check_scalar_flags(ctx, pl, "msm_run_narrow");
  float upload_ms = -1;
  if (pipe) upload_ms = pipe->finish();   // joins the staging threads; their last copy is done
  if (share.valid) {
    float ms;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_dig[0], ctx->ev_dig[1]));
    st.ms_digits += ms;
  }
  for (const GroupStats& g : sts) st += g;
  return upload_ms;
}

// words[k - k_lo] = the sum of window k from the sums of the schedule's groups (part[gi]: one slot per window of group gi)
void combine_group_sums(const msm_ctx* ctx, const GroupSchedule& sch, int c, int k_lo, int k_hi,
                        const std::vector<std::vector<uint32_t>>& part, std::vector<uint32_t>& words) {
  const std::vector<GroupSchedule::Group>& groups = sch.groups;
  const int pw = ctx->sum_words();
  words.assign((size_t)(k_hi - k_lo) * pw, 0);
  if (sch.tables) {
    // every group's first slot holds the sum G_g of its windows with their weights relative to the group's first window, and
    // the groups start wpg windows apart: the call's sum is sum_g 2^(c wpg g) G_g, a Horner step over the first slots under
    // the window c wpg.  It is kept in slot 0 (identities elsewhere: the caller's Horner step over such slots would return
    // the same element).
    std::vector<uint32_t> firsts(groups.size() * (size_t)pw);
    for (size_t gi = 0; gi < groups.size(); gi++) memcpy(&firsts[gi * pw], part[gi].data(), (size_t)pw * 4);
    sums_horner(ctx, firsts.data(), (int)groups.size(), c * sch.wpg, words.data());
    for (int k = k_lo + 1; k < k_hi; k++) sum_set_identity(ctx, &words[(size_t)(k - k_lo) * pw]);
  } else if (sch.split_points) {
    // P_k = sum over the ranges of the points (groups of one or several windows each); an all-zero partial (Z = 0) is the
    // identity.  (Plan.merged: a group then carries sum_kk 2^(c kk) P_kk in its first slot and identities in the others --
    // slot-wise sums of such groups are still a valid set of slots for the Horner step.)
    for (int k = k_lo; k < k_hi; k++) {
      std::vector<const uint32_t*> ranges;
      for (size_t gi = 0; gi < groups.size(); gi++)
        if (groups[gi].ka <= k && k < groups[gi].kb && !part[gi].empty())
          ranges.push_back(part[gi].data() + (size_t)(k - groups[gi].ka) * pw);
      sum_slots(ctx, ranges, &words[(size_t)(k - k_lo) * pw]);
    }
  } else {
    for (size_t gi = 0; gi < groups.size(); gi++) memcpy(&words[(size_t)(groups[gi].ka - k_lo) * pw], part[gi].data(), part[gi].size() * 4);
  }
}

// windows [k_lo, k_hi) over the resident points [p_off, p_off + n); scalars[i] belongs to point p_off + i
int window_sums_once(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, int k_lo, int k_hi,
                     const Plan& pl_in, std::vector<uint32_t>& words, msm_result* stats, uint64_t p_off) {
  const bool serial = opts && opts->serial;
  const CallSetup cs = prepare_call(ctx, scalars, n, on_device, serial, k_lo, k_hi, pl_in, p_off);
  Plan pl = pl_in;   // (a call that turns out to run over ranges of the points leaves the window tables: group_schedule)
  pl.tables = cs.sch.tables;
  std::vector<std::vector<uint32_t>> part;
  GroupStats st;
  const float upload_ms = run_groups(ctx, cs, scalars, n, pl, serial, p_off, part, st);
  combine_group_sums(ctx, cs.sch, pl.c, k_lo, k_hi, part, words);
  HIPCHK(hipEventRecord(ctx->ev[10], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (stats) {
    float ms;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[9]));
    stats->phase_ms[MSM_T_UPLOAD] = upload_ms >= 0 ? upload_ms : ms;   // pipelined: host clock of the background transfer
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[10]));
    stats->phase_ms[MSM_T_TOTAL] = ms;
    stats_to_result(st, stats);
    stats->c = pl.c;
    stats->K = pl.K;
    stats->tables = pl.tables ? 1 : 0;
  }
  return MSM_OK;
}

}  // namespace

namespace msmi {

const uint32_t* group_scalars(const uint32_t* d_scalars_all, uint64_t p_lo, Plan& pl) {
  if (!pl.nar.width) return d_scalars_all + p_lo * 8;
  pl.nar.first += p_lo;
  return d_scalars_all;
}

void run_on_workspaces(msm_ctx* ctx, int n_jobs, bool serial, const std::function<void(int slot, int index)>& job) {
  std::atomic<int> next{0};
  auto worker = [&](int slot) {
    HIPCHK(hipSetDevice(ctx->device));
    for (int i; (i = next.fetch_add(1)) < n_jobs;) job(slot, i);
  };
  // Whatever either worker throws (HIP failure, bad_alloc, ...) is re-raised here only after BOTH have stopped and both
  // group streams are idle: no queued kernel of a failed call may still run when the context is used again.
  const int nthreads = serial ? 1 : std::min<int>(msm_ctx::N_WS, n_jobs);
  std::exception_ptr err;
  if (nthreads > 1) ctx->helper->run([&] { worker(1); });
  try { worker(0); } catch (...) { err = std::current_exception(); }
  if (nthreads > 1) {
    try { ctx->helper->wait(); } catch (...) { if (!err) err = std::current_exception(); }
  }
  if (err) {
    for (auto& w : ctx->ws) (void)hipStreamSynchronize(w.stream);
    std::rethrow_exception(err);
  }
}

void add_group_times(const msm_ctx::Workspace& w, GroupStats& st) {
  float ms;
  HIPCHK(hipEventElapsedTime(&ms, w.ev[0], w.ev[1])); st.ms_digits += ms;
  HIPCHK(hipEventElapsedTime(&ms, w.ev[1], w.ev[2])); st.ms_sort += ms;
  HIPCHK(hipEventElapsedTime(&ms, w.ev[5], w.ev[3])); st.ms_acc += ms;
  HIPCHK(hipEventElapsedTime(&ms, w.ev[5], w.ev[6])); st.ms_r1 += ms;
  HIPCHK(hipEventElapsedTime(&ms, w.ev[3], w.ev[4])); st.ms_red += ms;
}

void stats_to_result(const GroupStats& st, msm_result* r) {
  r->phase_ms[MSM_T_DIGITS] = st.ms_digits;
  r->phase_ms[MSM_T_SORT] = st.ms_sort;
  r->phase_ms[MSM_T_ACCUMULATE] = st.ms_acc;
  r->phase_ms[MSM_T_ACC_ROUND1] = st.ms_r1;
  r->phase_ms[MSM_T_REDUCE] = st.ms_red;
  r->n_pairs = st.n_pairs;
  r->n_pairs_algo = st.n_pairs_algo;
  r->max_bucket = st.max_bucket;
  r->rounds = st.rounds;
}

void add_call_stats(msm_result& tot, const msm_result& r, bool side_by_side) {
  for (int j = 0; j < MSM_N_PHASES; j++)
    tot.phase_ms[j] = side_by_side ? std::max(tot.phase_ms[j], r.phase_ms[j]) : tot.phase_ms[j] + r.phase_ms[j];
  tot.n_pairs += r.n_pairs;
  tot.n_pairs_algo += r.n_pairs_algo;
  tot.rounds += r.rounds;
  tot.max_bucket = std::max(tot.max_bucket, r.max_bucket);
}

void check_scalar_flags(msm_ctx* ctx, const Plan& pl, const char* who) {
  HIPCHK(hipMemcpyAsync(ctx->h_info, ctx->errflag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint32_t flags = ctx->h_info[0];
  // scalars >= q seen by k_digits: refused under msm_opts.strict (otherwise they were reduced mod q)
  if (pl.strict && (flags & ERR_SCALAR_GE_Q)) throw MsmFail{MSM_ERR_SCALAR, "a scalar is >= the group order q (msm_opts.strict)"};
  if (flags & NARROW_ERR_RANGE) throw MsmFail{MSM_ERR_SCALAR, std::string("a scalar lies outside the declared range (") + who + ")"};
  if (flags & ERR_FOLD_DIGIT) throw MsmFail{MSM_ERR_INTERNAL, "a digit of the folded top window exceeds its bucket range (GLV bound violated)"};
}

bool call_begin(const msm_ctx* ctx, Plan& pl, uint64_t n, msm_result* out) {
  pl.merged = true;
  memset(out, 0, sizeof(*out));
  out->c = pl.c;
  out->K = pl.K;
  if (n == 0) identity_to_result(ctx, out);
  return n != 0;
}

void call_finish(msm_ctx* ctx, const std::vector<uint32_t>& words, const Plan& pl, msm_result* out, float staging_ms) {
  HIPCHK(hipEventRecord(ctx->ev[10], ctx->stream));
  // (a run on tables leaves the whole sum, weights included, in slot 0 and identities in the others: the Horner step over all
  // K slots returns it unchanged, and is what a call that had to leave the tables -- ranges of the points -- needs)
  sums_finish(ctx, words.data(), pl.K, pl.c, out);
  HIPCHK(hipEventRecord(ctx->ev[11], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[10], ctx->ev[11]));
  out->phase_ms[MSM_T_FINAL] = ms;
  if (staging_ms >= 0) {
    out->phase_ms[MSM_T_UPLOAD] = staging_ms;
    ms += staging_ms;
  }
  out->phase_ms[MSM_T_TOTAL] += ms;
}

// Workspace buffers only grow, and a call with another shape (window size, curve of the point set, sort path) leaves buffers
// behind that the next shape does not use: if the device runs out of memory the workspaces are dropped and the call runs
// once more from a clean slate, where the budget model of group_schedule holds again.
int window_sums_impl(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, int k_lo, int k_hi,
                     const Plan& pl, std::vector<uint32_t>& words, msm_result* stats, uint64_t p_off) {
  // The budget model is an estimate and other contexts may take memory while the call runs, so one clean-slate retry is not a
  // guarantee: every further attempt also halves what the workspaces may take (more window groups, then ranges of the points),
  // which trades time for memory as include/msm_hip.h promises.  The caller's own limit is restored afterwards.
  const uint64_t limit0 = ctx->ws_limit;
  for (int attempt = 0;; attempt++) {
    try {
      const int rc = window_sums_once(ctx, scalars, n, on_device, opts, k_lo, k_hi, pl, words, stats, p_off);
      ctx->ws_limit = limit0;
      return rc;
    } catch (const HipFail& f) {
      if (f.e != hipErrorOutOfMemory || attempt >= 4) {
        ctx->ws_limit = limit0;
        throw;
      }
    } catch (...) {
      ctx->ws_limit = limit0;
      throw;
    }
    (void)hipGetLastError();
    release_workspaces(ctx);
    if (attempt >= 1) ctx->ws_limit = std::max<uint64_t>(ctx->ws_budget / 2, (uint64_t)64 << 20);
  }
}

}  // namespace msmi

namespace {
// Multi-device context: one MSM over the devices of the list, each from its own host thread on its own context.
//   by points (default): device d runs ALL windows [k_lo, k_hi) on its share [n d / G, n (d + 1) / G) of the points and needs
//     only that share of the scalars; the G sums of every window are added on the host (G - 1 projective additions each);
//   by window (msm_opts.by_window): the window range is cut into contiguous shards (windows are independent until the Horner
//     step, src/msm-batched-affine.ts:312-333), every device needs all n scalars.
// Scalars: `placed` != nullptr -- one device pointer per device, already on that device (by points: the device's share);
// else a host buffer, of which every device uploads what it needs, or a device buffer on devices[0], of which the other
// devices first copy their part peer-to-peer -- all devices at once, each from its own thread, under device 0's shard.
int multi_window_sums(msm_ctx* ctx, const void* scalars, const void* const* placed, uint64_t n, int on_device, const msm_opts* opts,
                      int k_lo, int k_hi, const Plan& pl, std::vector<uint32_t>& words, msm_result* stats, uint64_t p_off) {
  const int ndev = 1 + (int)ctx->children.size();
  const int nwin = k_hi - k_lo, pw = ctx->sum_words();
  const bool by_window = opts && opts->by_window;
  words.assign((size_t)nwin * pw, 0);
  std::vector<int> lo(ndev, k_lo), hi(ndev, k_hi);
  std::vector<uint64_t> p0(ndev, 0), pn(ndev, n);
  for (int d = 0, k = k_lo; d < ndev; d++) {
    if (by_window) {
      const int cnt = nwin / ndev + (d < nwin % ndev ? 1 : 0);
      lo[d] = k;
      hi[d] = k + cnt;
      k += cnt;
    } else {
      p0[d] = n * (uint64_t)d / ndev;
      pn[d] = n * (uint64_t)(d + 1) / ndev - p0[d];
    }
  }
  std::vector<std::vector<uint32_t>> part(ndev);
  std::vector<msm_result> st(ndev);
  for (auto& r : st) memset(&r, 0, sizeof r);
  auto shard = [&](int d) {
    if (hi[d] <= lo[d] || pn[d] == 0) return;
    msm_ctx* c = d == 0 ? ctx : ctx->children[d - 1];
    HIPCHK(hipSetDevice(c->device));
    const void* sc;
    int dev_side = on_device;
    if (placed) {
      sc = placed[d];
      dev_side = 1;
    } else {
      sc = (const uint8_t*)scalars + p0[d] * 32;
      if (on_device && d > 0) {
        c->ensure(c->scal, pn[d] * 32);
        HIPCHK(hipMemcpyPeerAsync(c->scal.p, c->device, sc, ctx->device, pn[d] * 32, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        sc = c->scal.p;
      }
    }
    window_sums_impl(c, sc, pn[d], dev_side, opts, lo[d], hi[d], pl, part[d], &st[d], p_off + p0[d]);
  };
  std::exception_ptr err;
  for (int d = 1; d < ndev; d++) ctx->fan[d - 1]->run([&, d] { shard(d); });
  try { shard(0); } catch (...) { err = std::current_exception(); }
  for (int d = 1; d < ndev; d++) {
    try { ctx->fan[d - 1]->wait(); } catch (...) { if (!err) err = std::current_exception(); }
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (err) std::rethrow_exception(err);
  if (by_window) {
    for (int d = 0; d < ndev; d++)
      if (hi[d] > lo[d]) memcpy(&words[(size_t)(lo[d] - k_lo) * pw], part[d].data(), part[d].size() * 4);
  } else {
    // P_k = sum over the devices; an all-zero partial (Z = 0) is the identity, a device without points has none at all
    for (int k = 0; k < nwin; k++) {
      std::vector<const uint32_t*> devs;
      for (int d = 0; d < ndev; d++)
        if (!part[d].empty()) devs.push_back(&part[d][(size_t)k * pw]);
      sum_slots(ctx, devs, &words[(size_t)k * pw]);
    }
  }
  if (stats) {
    for (int d = 0; d < ndev; d++) add_call_stats(*stats, st[d], /*side_by_side=*/true);   // the devices ran at the same time
    stats->c = pl.c;
    stats->K = pl.K;
  }
  return MSM_OK;
}

}  // namespace

namespace msmi {
// the one entry the ABI functions use: single- or multi-device
int any_window_sums(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, int k_lo, int k_hi,
                    const Plan& pl, std::vector<uint32_t>& words, msm_result* stats, const void* const* placed) {
  const uint64_t p_off = point_lo(opts);
  if (ctx->children.empty())
    return window_sums_impl(ctx, placed ? placed[0] : scalars, n, placed ? 1 : on_device, opts, k_lo, k_hi, pl, words, stats, p_off);
  return multi_window_sums(ctx, scalars, placed, n, on_device, opts, k_lo, k_hi, pl, words, stats, p_off);
}

}  // namespace msmi
