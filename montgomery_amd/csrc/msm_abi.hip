// The C ABI of include/msm_hip.h: contexts, resident point sets, msm_run / msm_window_sums / msm_combine, device buffers.
// (reference interface replaced: Curve.Parallel.* of src/parallel.ts:135-145,251-259)
#include "msm_internal.h"
#include <chrono>

using namespace msm;
using namespace msmi;

extern "C" {

uint32_t msm_abi_version(void) { return MSM_ABI_VERSION; }
uint32_t msm_abi_struct_bytes(int which) { return which == 0 ? (uint32_t)sizeof(msm_opts) : which == 1 ? (uint32_t)sizeof(msm_result) : 0u; }

int msm_ctx_create(msm_ctx** out, int curve, int device) {
  if (!out) return MSM_ERR_ARG;
  *out = nullptr;
  if (!curve_info_or_null(curve)) return MSM_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return MSM_ERR_NO_DEVICE;
  msm_ctx* ctx = new (std::nothrow) msm_ctx();
  if (!ctx) return MSM_ERR_INTERNAL;
  ctx->curve = curve;
  ctx->device = device;
  try {
    ctx->helper.reset(new HelperThread());
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->stream.create();
    for (auto& e : ctx->ev) e.create();
    for (auto& e : ctx->ev_dig) e.create();
    ctx->h_info.allocate(64 * 4);
    for (auto& w : ctx->ws) {
      w.stream.create();
      w.side.create();
      for (auto& e : w.ev) e.create();
      w.h_info.allocate(64 * 4);
      w.h_part.allocate(128 * 20 * W_SUM_WORDS * 4);
    }
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // leave room for the resident points (144 B/point at 2^26 = 9.7 GB) and fragmentation
    ctx->ws_budget = (uint64_t)(free_b * 0.55);
    // window tables of one point set (msm_set_tables_limit): 57.6 GB of 288 -- up to 2^26 BLS12-377 points, whose three shared
    // tables (two window groups over six windows) take 51.5 GB, the plain rows included
    ctx->tables_limit = (uint64_t)(total_b * 0.20);
    ctx->ensure(ctx->errflag, 16);
    sort_kernel_attributes();
  } catch (const HipFail& f) {
    fprintf(stderr, "msm_ctx_create: HIP error %s at line %d\n", hipGetErrorString(f.e), f.line);
    msm_ctx_destroy(ctx);
    return MSM_ERR_HIP;
  } catch (...) {
    msm_ctx_destroy(ctx);
    return MSM_ERR_INTERNAL;
  }
  ctx->hc.F.init(curve == MSM_CURVE_ED_ON_BLS12_377 ? Fp377::PW : curve_info(curve).pw);   // (the Edwards context uses hte)
  ctx->k_dev_to_host = ctx->hc.F.pow2(2 * ctx->hc.F.radix_bits() - 30 * ctx->nl());   // device radix 2^(30 NL); host radix 2^384 or 2^256
  {
    uint32_t pw[12] = {0};
    for (int i = 0; i < 8; i++) pw[i] = Fp253::PW[i];
    ctx->hte.init(pw, 3021);
    ctx->k_te_to_host = ctx->hte.F.pow2(2 * ctx->hte.F.radix_bits() - 270);
  }
  *out = ctx;
  return MSM_OK;
}

void msm_ctx_destroy(msm_ctx* ctx) {
  if (!ctx) return;
  for (msm_ctx* c : ctx->children) msm_ctx_destroy(c);
  delete ctx;
}

const char* msm_last_error(const msm_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

static int set_points_one(msm_ctx* ctx, const void* points, uint64_t n, int on_device, int check_curve) {
  if (!ctx || (!points && n)) return fail(ctx, MSM_ERR_ARG, "msm_set_points: null argument");
  if (n >= (1ull << 30)) return fail(ctx, MSM_ERR_ARG, "msm_set_points: n must be < 2^30");
  const bool te = ctx->is_te();
  const size_t wire_bytes = 2 * ctx->coord_bytes();   // x || y, little-endian
  try {
    HIPCHK(hipSetDevice(ctx->device));
    uint32_t* rows = ctx->reset_points(n);
    const uint32_t* d_wire = (const uint32_t*)points;
    if (!on_device && n) {
      ctx->ensure(ctx->misc, n * wire_bytes);
      upload_staged(ctx, ctx->misc.p, points, n * wire_bytes);
      d_wire = (const uint32_t*)ctx->misc.p;
    }
    HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, ctx->stream));
    if (n) {
      uint64_t grid = (n + 255) / 256;
      if (te)
        hipLaunchKernelGGL(te::k_te_points_from_wire, dim3((uint32_t)grid), dim3(256), 0, ctx->stream, rows, d_wire,
                           n, check_curve, (uint32_t*)ctx->errflag.p);
      else
        W_LAUNCH(ctx, k_points_from_wire, dim3((uint32_t)grid), dim3(256), 0, ctx->stream, rows, d_wire, n,
                           check_curve, (uint32_t*)ctx->errflag.p);
    }
    HIPCHK(hipMemcpyAsync(ctx->h_info, ctx->errflag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (!on_device) ctx->release(ctx->misc);
    if (ctx->h_info[0] & 1) return fail(ctx, MSM_ERR_POINT, "msm_set_points: coordinate >= p");
    if (ctx->h_info[0] & 2) return fail(ctx, MSM_ERR_POINT, "msm_set_points: point not on curve");
    ctx->pts().n = n;
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_set_points(msm_ctx* ctx, const void* points, uint64_t n, int on_device, int check_curve) {
  if (!ctx || ctx->children.empty()) return set_points_one(ctx, points, n, on_device, check_curve);
  // multi-device context: every device keeps the whole point set (an MSM then runs over a share of the points per device by
  // default, or over a share of the windows with msm_opts.by_window: either way without moving points)
  try {
    std::vector<uint8_t> host;
    const void* src = points;
    if (on_device && n) {   // the buffer lives on devices[0]: the other devices take it through the host
      host.resize((size_t)n * 2 * ctx->coord_bytes());
      HIPCHK(hipSetDevice(ctx->device));
      HIPCHK(hipMemcpy(host.data(), points, host.size(), hipMemcpyDeviceToHost));
      src = host.data();
    }
    return on_all_devices(ctx, [&](msm_ctx* c) {
      return (c == ctx) ? set_points_one(c, points, n, on_device, check_curve) : set_points_one(c, src, n, 0, check_curve);
    });
  } MSM_CATCH_ALL(ctx)
}

int msm_plan(const msm_ctx* ctx, uint64_t n, const msm_opts* opts, int32_t* c_out, int32_t* K_out) {
  Plan pl;   // plain arithmetic: nothing here can throw
  bool tables_wanted = false;
  // (a context with resident points answers for msm_run over them, window tables included; msm_window_sums and shards of
  // the points always run the plain plan, which is also what a context without points reports)
  // (msm_opts.merged_sums: the plan of msm_window_sums over a range of the points that may run on range tables)
  const bool run_like = ctx && n && ((n == ctx->pts().n && !point_lo(opts)) || (opts && opts->merged_sums));
  int rc = run_like ? make_run_plan(const_cast<msm_ctx*>(ctx), n, opts, false, pl, tables_wanted) : make_plan(ctx, n, opts, pl);
  if (rc) return rc;
  if (c_out) *c_out = pl.c;
  if (K_out) *K_out = pl.K;
  return MSM_OK;
}

int msm_window_sums(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, uint8_t* partials_out,
                    msm_result* stats) {
  if (!ctx || !partials_out || (!scalars && n)) return fail(ctx, MSM_ERR_ARG, "msm_window_sums: null argument");
  if (int rc = check_points(ctx, n, opts, MSM_ERR_NO_POINTS, "msm_window_sums")) return rc;
  Plan pl;
  // msm_opts.merged_sums: the caller only combines the sums (msm_combine / msm_combine_groups), so the call may hand them back
  // merged -- and with that run on window tables, those of the whole set or of the range of the points it covers
  const bool merged = opts && opts->merged_sums;
  bool tables_wanted = false;
  if (merged ? make_run_plan(ctx, n, opts, false, pl, tables_wanted, /*note_range=*/true) : make_plan(ctx, n, opts, pl))
    return fail(ctx, MSM_ERR_ARG, "msm_window_sums: bad window size");
  pl.merged = merged;
  int k_lo = opts ? opts->k_lo : 0, k_hi = opts ? opts->k_hi : 0;
  if (k_lo == 0 && k_hi == 0) k_hi = pl.K;
  if (k_lo < 0 || k_hi > pl.K || k_lo >= k_hi) return fail(ctx, MSM_ERR_ARG, "msm_window_sums: bad window shard [%d, %d) of %d", k_lo, k_hi, pl.K);
  if (stats) memset(stats, 0, sizeof(*stats));
  try {
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint32_t> words;
    pl.tables = n && tables_wanted && use_window_tables(ctx, n, opts, pl);
    if (n) any_window_sums(ctx, scalars, n, on_device, opts, k_lo, k_hi, pl, words, stats);
    for (int k = 0; k < k_hi - k_lo; k++)   // (no points: every sum is the identity)
      sum_to_wire(ctx, n ? &words[(size_t)k * ctx->sum_words()] : nullptr, partials_out + (size_t)k * SUM_WIRE_BYTES);
    if (stats) { stats->c = pl.c; stats->K = pl.K; }
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_combine(msm_ctx* ctx, const uint8_t* partials, int32_t K, int32_t c, msm_result* out) {
  // pure host arithmetic: ctx may be NULL (then BLS12-377 G1; msm_combine_curve names the curve without a context)
  if (!partials || !out || K <= 0 || c <= 0) return fail(ctx, MSM_ERR_ARG, "msm_combine: bad argument");
  try {
    if (ctx && ctx->is_te()) {
      int rc = te_combine_impl(partials, K, c, out);
      return rc ? fail(ctx, rc, "msm_combine: coordinate >= p") : MSM_OK;
    }
    return combine_impl(ctx, ctx ? ctx->hc : *static_host_curve(MSM_CURVE_BLS12_377_G1), partials, K, c, out, 1);
  } MSM_CATCH_ALL(ctx)
}

int msm_combine_groups(int curve, const uint8_t* partials, int32_t G, int32_t K, int32_t c, msm_result* out) {
  if (!partials || !out || K <= 0 || c <= 0 || G <= 0) return MSM_ERR_ARG;
  msm_ctx* const no_ctx = nullptr;
  try {
    if (curve == MSM_CURVE_ED_ON_BLS12_377) return te_combine_impl(partials, K, c, out, G);
    const msm_host::Curve6* C = static_host_curve(curve);
    if (!C) return MSM_ERR_ARG;
    return combine_impl(nullptr, *C, partials, K, c, out, G);
  } MSM_CATCH_ALL(no_ctx)
}

int msm_combine_curve(int curve, const uint8_t* partials, int32_t K, int32_t c, msm_result* out) {
  return msm_combine_groups(curve, partials, 1, K, c, out);
}

// msm_run over HOST scalars of a big input: the scalars cross PCIe behind the computation (PieceUpload, msm_upload.hip).  The
// sort of a window needs every digit of its range, so the unit of overlap is a range of the points: the call runs as whole
// MSMs over 1/16, 3/16 and the rest of the points (1/8, 3/8, rest below 2^25) as their scalars arrive -- each with the
// window the library picks for ITS size (round 4 ran all ranges under one window picked for an eighth of the input: the last,
// biggest range then missed the 21-bit plan) -- and adds the three results.  The link moves scalars ~4x as fast as the GPU
// consumes them, so every range may be ~4x its predecessor and still be there in time.
// (the reference's counterpart: scalarsFromBytes into shared wasm memory before the call, src/parallel.ts:119-133)
static int run_piped(msm_ctx* ctx, const void* scalars, uint64_t n, const msm_opts* opts, msm_result* out, const char* who) {
  memset(out, 0, sizeof(*out));
  try {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventRecord(ctx->ev[8], ctx->stream));
    const std::vector<uint64_t> piece_end = pipelined_piece_ends(n);
    ctx->ensure(ctx->scal, n * 32);   // before any workspace is sized from what the device has free
    std::vector<size_t> ends;
    for (uint64_t e : piece_end) ends.push_back((size_t)e * 32);
    PieceUpload pipe(ctx, ctx->scal.p, scalars, n * 32, ends);
    const uint32_t base_lo = (uint32_t)point_lo(opts);
    const size_t Q = piece_end.size();
    struct Range {
      uint64_t lo = 0, cnt = 0;
      Plan pq;
      msm_opts o;
      msm_result st;
      std::vector<uint32_t> words, sum;   // its window sums; their Horner sum, one slot
    };
    std::vector<Range> R(Q);
    for (size_t q = 0; q < Q; q++) {
      R[q].lo = q ? piece_end[q - 1] : 0;
      R[q].cnt = piece_end[q] - R[q].lo;
      if (opts) R[q].o = *opts; else memset(&R[q].o, 0, sizeof(msm_opts));
      R[q].o.point_lo = base_lo + (uint32_t)R[q].lo;
      memset(&R[q].st, 0, sizeof(msm_result));
      if (R[q].cnt && make_plan(ctx, R[q].cnt, &R[q].o, R[q].pq)) return fail(ctx, MSM_ERR_ARG, "%s: bad window size", who);
      R[q].pq.merged = true;
    }
    // the ranges in order, each as soon as its scalars are in HBM (a second pipeline on the device running the middle range beside
    // its neighbours was tried and bought nothing -- work is conserved: profiles/r05_experiments.txt item 11)
    for (size_t q = 0; q < Q; q++) {
      Range& r = R[q];
      if (r.cnt == 0) continue;
      pipe.wait_piece((int)q, ctx->stream);
      HIPCHK(hipStreamSynchronize(ctx->stream));       // the range's scalars are in HBM
      window_sums_impl(ctx, (const uint32_t*)ctx->scal.p + r.lo * 8, r.cnt, 1, &r.o, 0, r.pq.K, r.pq, r.words, &r.st, r.o.point_lo);
    }
    // the ranges' results are added as group elements: one field inversion for the call
    std::vector<const uint32_t*> sums;
    for (size_t q = 0; q < Q; q++) {
      Range& r = R[q];
      if (r.cnt == 0) continue;
      r.sum.resize(ctx->sum_words());
      sums_horner(ctx, r.words.data(), r.pq.K, r.pq.c, r.sum.data());
      sums.push_back(r.sum.data());
      add_call_stats(*out, r.st);
      out->c = r.pq.c;   // the plan of the last, biggest range
      out->K = r.pq.K;
    }
    out->phase_ms[MSM_T_UPLOAD] = pipe.finish();   // wall time of the background transfer
    std::vector<uint32_t> total(ctx->sum_words());
    sum_slots(ctx, sums, total.data());
    sums_finish(ctx, total.data(), 1, 0, out);
    HIPCHK(hipEventRecord(ctx->ev[11], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[11]));
    out->phase_ms[MSM_T_TOTAL] = ms;
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

static int run_impl(msm_ctx* ctx, const void* scalars, const void* const* placed, uint64_t n, int on_device, const msm_opts* opts,
                    msm_result* out, const char* who) {
  if (int rc = check_points(ctx, n, opts, MSM_ERR_NO_POINTS, who)) return rc;
  if (!placed && !on_device && pipelines_host_scalars(n) && ctx->children.empty() && !ctx->is_te() && !(opts && opts->c))
    return run_piped(ctx, scalars, n, opts, out, who);
  Plan pl;
  bool tables_wanted = false;   // window tables (msm_tables.hip): the plan is then the one tables want
  if (make_run_plan(ctx, n, opts, placed != nullptr, pl, tables_wanted, /*note_range=*/true)) return fail(ctx, MSM_ERR_ARG, "%s: bad window size", who);
  if (!call_begin(ctx, pl, n, out)) return MSM_OK;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint32_t> words;
    // window tables (msm_tables.hip): built here on the first default-plan call over the whole point set
    pl.tables = tables_wanted && use_window_tables(ctx, n, opts, pl);
    any_window_sums(ctx, scalars, n, on_device, opts, 0, pl.K, pl, words, out, placed);
    call_finish(ctx, words, pl, out);   // (the upload time the window sums measured stays)
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_run(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, msm_result* out) {
  if (!ctx || !out || (!scalars && n)) return fail(ctx, MSM_ERR_ARG, "msm_run: null argument");
  return run_impl(ctx, scalars, nullptr, n, on_device, opts, out, "msm_run");
}

int msm_run_placed(msm_ctx* ctx, const void* const* dev_scalars, uint64_t n, const msm_opts* opts, msm_result* out) {
  if (!ctx || !out || !dev_scalars) return fail(ctx, MSM_ERR_ARG, "msm_run_placed: null argument");
  if (opts && opts->by_window && !ctx->children.empty())
    return fail(ctx, MSM_ERR_ARG, "msm_run_placed: placed scalars are the shares of a points split (by_window must be 0)");
  const int ndev = 1 + (int)ctx->children.size();
  for (int d = 0; d < ndev; d++)
    if (!dev_scalars[d] && n * (uint64_t)(d + 1) / ndev > n * (uint64_t)d / ndev)
      return fail(ctx, MSM_ERR_ARG, "msm_run_placed: no scalars for device %d", d);
  return run_impl(ctx, nullptr, dev_scalars, n, 1, opts, out, "msm_run_placed");
}

int msm_reserve(msm_ctx* ctx, uint64_t n, const msm_opts* opts) {
  if (!ctx) return MSM_ERR_ARG;
  if (int rc = check_points(ctx, n, opts, MSM_ERR_NO_POINTS, "msm_reserve")) return rc;
  if (n == 0) return MSM_OK;
  try {
    // one MSM over generated scalars: every buffer the real call will need exists afterwards, and so do the window tables
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf dev;
    dev.allocate(n * 32);
    int rc = msm_generate_scalars(ctx, n, 0x5eed, dev.p, nullptr);
    msm_result r;
    if (rc == MSM_OK) rc = msm_run(ctx, dev.p, n, 1, opts, &r);
    return rc;
  } catch (...) {
    return fail(ctx, MSM_ERR_HIP, "msm_reserve: device allocation failed");
  }
}

int msm_get_points(msm_ctx* ctx, uint64_t first, uint64_t count, uint8_t* out_xy) {
  if (!ctx || !out_xy || first + count > ctx->pts().n) return fail(ctx, MSM_ERR_ARG, "msm_get_points: bad argument");
  if (ctx->is_te()) {
    try {
      HIPCHK(hipSetDevice(ctx->device));
      std::vector<uint32_t> rows((size_t)count * te::TE_ROW_WORDS);
      if (count)
        HIPCHK(hipMemcpy(rows.data(), (const uint32_t*)ctx->pts().rows.p + first * te::TE_ROW_WORDS, rows.size() * 4, hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < count; i++)
        for (int j = 0; j < 2; j++)
          device_coord_to_wire(ctx->hte.F, ctx->k_te_to_host, &rows[(size_t)i * te::TE_ROW_WORDS + 8 * j], 8, out_xy + i * 64 + 32 * j);
    } MSM_CATCH_ALL(ctx)
    return MSM_OK;
  }
  try {
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint32_t> rows((size_t)count * ROW_WORDS);
    if (count)
      HIPCHK(hipMemcpy(rows.data(), (const uint32_t*)ctx->pts().rows.p + first * ROW_WORDS, rows.size() * 4, hipMemcpyDeviceToHost));
    const int nw = ctx->nw();
    const size_t cb = ctx->coord_bytes();
    memset(out_xy, 0, (size_t)count * 2 * cb);
    for (uint64_t i = 0; i < count; i++) {
      const uint32_t* row = &rows[(size_t)i * ROW_WORDS];
      if (row[nw - 1] == INF_WORD) continue;
      for (int j = 0; j < 2; j++) device_coord_to_wire(ctx->hc.F, ctx->k_dev_to_host, row + nw * j, nw, out_xy + i * 2 * cb + cb * j);
    }
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

// ---- point-set handles: several resident point sets per context, one of them current ------------------------

static int pointset_select_one(msm_ctx* ctx, int32_t id) {
  if (id < 0 || id >= (int)ctx->sets.size() || (id != 0 && !ctx->sets[id].live))
    return fail(ctx, MSM_ERR_ARG, "msm_pointset_select: no point set %d", (int)id);
  if (id == ctx->cur_set) return MSM_OK;
  ctx->cur_set = id;
  ctx->cand_n = 0;
  return MSM_OK;
}

int msm_pointset_create(msm_ctx* ctx, int32_t* id_out) {
  if (!ctx || !id_out) return fail(ctx, MSM_ERR_ARG, "msm_pointset_create: null argument");
  try {
    return on_all_devices(ctx, [&](msm_ctx* c) {
      int id = -1;
      for (size_t i = 1; i < c->sets.size(); i++)
        if (!c->sets[i].live) { id = (int)i; break; }
      if (id < 0) { c->sets.emplace_back(); id = (int)c->sets.size() - 1; }   // children stay in lockstep: same ids
      c->sets[id] = msm_ctx::PointSet();
      c->sets[id].live = true;
      if (c == ctx) *id_out = id;
      return pointset_select_one(c, id);
    });
  } MSM_CATCH_ALL(ctx)
}

int msm_pointset_select(msm_ctx* ctx, int32_t id) {
  if (!ctx) return MSM_ERR_ARG;
  try {
    return on_all_devices(ctx, [&](msm_ctx* c) { return pointset_select_one(c, id); });
  } MSM_CATCH_ALL(ctx)
}

int msm_pointset_destroy(msm_ctx* ctx, int32_t id) {
  if (!ctx) return MSM_ERR_ARG;
  if (id <= 0 || id >= (int)ctx->sets.size() || !ctx->sets[id].live)
    return fail(ctx, MSM_ERR_ARG, "msm_pointset_destroy: no such point set %d (the default set 0 stays)", (int)id);
  try {
    return on_all_devices(ctx, [&](msm_ctx* c) {
      if (c->cur_set == id) pointset_select_one(c, 0);
      (void)hipSetDevice(c->device);
      c->sets[id].release();
      return (int)MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

// ---- device buffers for scalar handles ------------------------------------------------------------------------

int msm_device_alloc(msm_ctx* ctx, uint64_t bytes, void** dev_ptr_out) {
  if (!ctx || !dev_ptr_out) return fail(ctx, MSM_ERR_ARG, "msm_device_alloc: null argument");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf b;
    b.allocate(std::max<uint64_t>(bytes, 32));
    *dev_ptr_out = b.p;
    ctx->allocs.push_back(std::move(b));
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_device_free(msm_ctx* ctx, void* dev_ptr) {
  if (!ctx) return MSM_ERR_ARG;
  auto it = std::find_if(ctx->allocs.begin(), ctx->allocs.end(), [&](const DevBuf& b) { return b.p == dev_ptr; });
  if (it == ctx->allocs.end()) return fail(ctx, MSM_ERR_ARG, "msm_device_free: not a buffer of this context");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf b = std::move(*it);
    ctx->allocs.erase(it);
    b.release(/*checked=*/true);
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_device_upload(msm_ctx* ctx, void* dev_ptr, const void* host, uint64_t bytes) {
  if (!ctx || !dev_ptr || (!host && bytes)) return fail(ctx, MSM_ERR_ARG, "msm_device_upload: null argument");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes) {
      upload_staged(ctx, dev_ptr, host, bytes);
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_set_workspace_limit(msm_ctx* ctx, uint64_t bytes) {
  if (!ctx) return MSM_ERR_ARG;
  ctx->ws_limit = bytes;
  if (!bytes) {   // back to automatic: small calls use the creation-time rule again
    try {
      HIPCHK(hipSetDevice(ctx->device));
      size_t free_b = 0, total_b = 0;
      HIPCHK(hipMemGetInfo(&free_b, &total_b));
      ctx->ws_budget = (uint64_t)((free_b + ctx->workspace_bytes()) * 0.55L);
    } MSM_CATCH_ALL(ctx)
  }
  for (msm_ctx* c : ctx->children) {
    int rc = msm_set_workspace_limit(c, bytes);
    if (rc != MSM_OK) return rc;
  }
  return MSM_OK;
}

// ---- multi-device context ---------------------------------------------------------------------------------------

int msm_ctx_create_multi(msm_ctx** out, int curve, const int32_t* devices, int32_t n_devices) {
  if (!out || !devices || n_devices < 1) return MSM_ERR_ARG;
  *out = nullptr;
  msm_ctx* ctx = nullptr;
  int rc = msm_ctx_create(&ctx, curve, devices[0]);
  if (rc != MSM_OK) return rc;
  try {
    for (int i = 1; i < n_devices; i++) {
      msm_ctx* c = nullptr;
      rc = msm_ctx_create(&c, curve, devices[i]);
      if (rc != MSM_OK) {
        msm_ctx_destroy(ctx);
        return rc;
      }
      ctx->children.push_back(c);
      ctx->fan.emplace_back(new HelperThread());
    }
  } catch (...) {
    msm_ctx_destroy(ctx);
    return MSM_ERR_INTERNAL;
  }
  *out = ctx;
  return MSM_OK;
}

int msm_ctx_device_count(const msm_ctx* ctx) { return ctx ? 1 + (int)ctx->children.size() : 0; }

}  // extern "C"
