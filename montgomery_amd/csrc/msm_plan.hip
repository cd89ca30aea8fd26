// Plan of one MSM: window size, number of windows, launch geometry of the tree rounds, workspace budget model, the schedule of
// a call's window groups; and the error helpers every ABI entry ends in.  (reference: windowSize table src/msm-common.ts:25-41, K = ceil((b + 1) / c)
// src/msm-batched-affine.ts:90)
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace msmi {

int fail(msm_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) {
    ctx->err = buf;
    ctx->last_sort_paths.clear();   // (msm_test_last_sort_paths: a failed call reports no paths, not those of the call before it)
  }
  return code;
}

int check_points(msm_ctx* ctx, uint64_t n, const msm_opts* opts, int code, const char* who, bool empty_ok) {
  const uint64_t lo = point_lo(opts), resident = ctx->pts().n;
  if (lo + n <= resident && (n || empty_ok)) return MSM_OK;
  return fail(ctx, code, "%s: points [%llu, +%llu) but %llu resident points", who, (unsigned long long)lo, (unsigned long long)n,
              (unsigned long long)resident);
}

int refuse_shard_opts(msm_ctx* ctx, const msm_opts* opts, const char* who, const char* kind, bool no_point_lo) {
  if (!opts) return MSM_OK;
  const bool shard = opts->k_lo || opts->k_hi || opts->bucket_shards > 1 || opts->merged_sums || opts->by_window;
  if (!shard && !(no_point_lo && opts->point_lo)) return MSM_OK;
  return fail(ctx, MSM_ERR_ARG, "%s: %swindow shards, bucket shards, merged sums and by_window are not options of %s call", who,
              no_point_lo ? "point_lo, " : "", kind);
}

static const char* base_name(const char* p) {
  const char* s = strrchr(p ? p : "", '/');
  return s ? s + 1 : (p ? p : "?");
}

int fail_hip(msm_ctx* ctx, const HipFail& f) {
  return fail(ctx, MSM_ERR_HIP, "HIP error %d (%s) at %s:%d: %s", (int)f.e, hipGetErrorString(f.e), base_name(f.file), f.line, f.what);
}

// GPU-tuned window size (the reference's table, src/msm-common.ts:25-41, was tuned for 16 CPU threads and copies
// points).  Weierstrass + GLV (b + 1 = 127 or 128 bits): measured over N = 2^4 .. 2^28 (tools/small_sizes.py,
// tools/knob_matrix.py), c = 16 (K = 8, no degenerate top window, one window's counters fit the LDS) wins from N = 2^12 to
// 2^25 -- by 20 % over c = 13 at 2^14 .. 2^18, where a smaller window mostly buys more rounds of fixed latency -- and c = 8
// below.  From 2^26 points the big windows (K = 7 / 6: a quarter fewer pair additions) win with the three-pass sort, the
// chunk-ordered round 1 and, since round 4, the last descriptor rounds left to k_bucket_finish: 2^26 c = 22 149.2 against
// 155.6 ms (2^25: 83.0 against 80.4, so c = 16 stays there), 2^27 c = 21 296 against 300 (c = 22) and 314 (c = 16), 2^28
// c = 22 584 against 643 (profiles/r03_experiments.txt items 5 and 12, profiles/r04_experiments.txt item 8).
// Twisted Edwards (b + 1 = 252, no inversion per round): a cost model over the window sizes whose top window is not
// degenerate, ~9 multiplications per pair addition against ~64 per bucket; its picks are within 3 % of the best
// measured ones.
int pick_window(bool te, uint64_t n, int glv_max_bits) {
  // measured (profiles/r03_experiments.txt item 5): the mean bucket of the big windows wants ~128 entries
  // b = 126 (BLS12-377 after GLV): 127 = 6 * 21 + 1, so 21-bit windows fold the carry bit into the sixth window (make_plan) --
  // K = 6 with half the buckets of the 22-bit plan: 2^24 43.6 against 44.3 (c = 16), 2^25 79.7 against 80.7, 2^26 148.9 against
  // 151.5 (c = 22) and 158.3 (c = 16), 2^27 302.8 against 311.5 (c = 22) on one box (profiles/r04_experiments.txt item 13).
  // b = 127 (BLS12-381, Pallas): 128 = 5 * 22 + 18, the 22-bit plan has six whole windows (from 2^25 points, see below).
  // (127 = 7 * 18 + 1 folds too: seven 18-bit windows win from 2^22 points to 2^24 -- with the round-5 sort of the big windows
  // 2^22 11.4 against 12.1 ms, 2^23 20.6 / 21.8, level at 2^21 (6.8), behind the 21-bit plan at 2^24 (41.3 / 39.5): tools/plan_sweep.py)
  // BN254 G1 and Grumpkin (b = 126 on the 9-limb field: the same K for every c, the 6 x 21 fold included) take these thresholds.
  // Swept at 2^20, 2^23, 2^24 (profiles/cycle_curves_time.txt; BN254 / Grumpkin, ms): 2^20 c = 16 2.82 / 2.76 against 2.88 / 2.85
  // at 18; 2^23 c = 18 15.6 / 15.4 against 17.2 / 17.1 (16), 15.9 / 15.6 (19), 16.0 / 16.0 (21); 2^24 c = 21 30.0 / 29.6 against
  // 31.0 / 30.5 (18), 31.6 / 31.6 (19), 31.9 / 31.3 (22).  The crossovers themselves (2^22, 4096) and 2^25 .. 2^26: model only.
  if (!te && glv_max_bits == 126)
    return n >= (1ull << 24) ? 21 : n >= (1ull << 22) ? 18 : n >= 4096 ? 16 : 8;
  // b = 127 (BLS12-381, Pallas), with the round-5 sort of the big windows (tools/plan_sweep_curve.py, c = 16 / 19 / 22):
  // BLS12-381 2^23 22.6 / 22.1 / 24.7 ms, 2^24 44.0 / 43.3 / 44.0, 2^25 81.6 / 80.5 / 75.0; Pallas 2^23 15.6 / 14.5 / 16.3,
  // 2^24 32.0 / 30.6 / 29.7, 2^25 58.6 / 59.0 / 55.8; level at 2^22.  Vesta (Pallas' arithmetic, b = 127) takes
  // Pallas' thresholds: 2^23 c = 19 15.3 against 16.3 (16) and 19.0 (21); at 2^24 c = 22 is ahead, 29.3 against 30.5 (19), as on Pallas
  // in the same run (30.0 / 31.6): the shared threshold stays where the sweep above put it (profiles/cycle_curves_time.txt).
  if (!te) return n >= (1ull << 25) ? 22 : n >= (1ull << 23) ? 19 : n >= 4096 ? 16 : 8;
  // Edwards plain path with the bin split of round 5 (tools/plan_sweep_curve.py 1, ms at c = 16 / 18): 2^22 8.6 / 7.9, 2^23 15.0 / 14.2,
  // 2^24 28.0 / 26.3, 2^25 53.4 / 54.4, 2^26 101.8 / 105.7 (its gather round is not tile-ordered: beyond 2^25 the big windows lose)
  if (te && n >= (1ull << 22) && n < (1ull << 25)) return 18;
  static const int cand_te[] = {4, 6, 7, 9, 12, 14, 16};
  const int b1 = 252;
  int best = 4;
  double best_cost = 1e300;
  for (int i = 0; i < 7; i++) {
    int c = cand_te[i];
    int K = (b1 + c - 1) / c;
    double cost = (double)n * K * 8.0 + (double)K * (double)(1u << (c - 1)) * 64.0;
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}

// Window of a narrow call (msm_run_narrow): b = `bits` magnitude bits, one entry per point, K = ceil((b + 1) / c).  The
// candidates that matter are the c whose K c wastes few bits (b = 64: 13 x 5, 17 x 4, 22 x 3; b = 32: 11 x 3, 17 x 2; b = 16:
// 9 x 2, 17 x 1; b = 8: 9 x 1; b = 1: 2 x 1): for every K the smallest c that reaches it.
// Measured with tools/narrow_time.py --csweep at b = 1, 8, 16, 32, 64, 128 and n = 2^14 .. 2^24 on BLS12-377 and Ed-on-BLS12-377
// (profiles/narrow_scalar_time.txt section 1, the "c sweep" lines; ms, BLS12-377 first, then the Edwards curve):
//  * 5 .. 32 bits: one or two 17-bit windows (the bin split of the big windows, which cuts heavy bins into parts) beat the small
//    windows of the one-level sort as soon as the buckets get deep.  b = 16: 2^18 0.82 against 1.13 at c = 9 (Edwards 0.48 /
//    0.51), 2^20 1.00 / 2.30 (0.61 / 0.69).  b = 32: 2^18 0.93 against 1.08 at c = 11 (0.57 / 0.58), 2^20 1.24 / 1.70 (0.81 /
//    0.86).  b = 8: 2^18 c = 9 still wins, 1.03 against 1.19 (0.47 / 0.61); 2^20 1.48 against 1.70 at c = 9 but Edwards 0.70 /
//    0.57, so there from 2^22; 2^22 2.16 / 3.48 (1.07 / 2.43), 2^24 4.65 / 7.70 (2.55 / 8.56).  Below those sizes the
//    smallest window that covers the scalar in few windows wins (the model below).  5 .. 7 bits follow the 8-bit rule unmeasured.
//  * bit columns are the other way round: b = 1 under c = 2 (two buckets) against c = 17: 2^20 1.53 / 2.03, 2^22 2.13 / 3.27,
//    2^24 3.38 / 7.01 (Edwards 2^22 0.80 / 2.12, 2^24 1.47 / 6.27) -- up to 4 bits the model's window, b + 1, stays.
//  * above 32 bits, below 2^21 points: 13-bit windows (b = 64 at 2^20 1.92 against 2.35 at c = 11; b = 128 2.86 against 3.59
//    at c = 12 and 3.60 at c = 15), so the model is capped at 13 there.  From 2^21 points 17 bits for b = 64 (2^22 4.24 against
//    4.92 at c = 13 and 6.09 at c = 22; 2^24 12.9 / 14.9 / 14.1) and, which the model finds by itself, 19 bits for b = 128 at
//    2^24 (21.6 against 24.7 at c = 17; Edwards 14.6 / 16.2).  At 2^22 it takes 17 for b = 128, 7.85 where 19 would give 7.21
//    (not adopted: one point); on the Edwards curve 13 bits win there, 4.85 against 5.17, and stay below 2^23.
// Everything else is the COST MODEL alone: other bit lengths; BLS12-381, Pallas, Vesta, BN254 G1 and Grumpkin, and 2^26 points (c = 22 from 64 bits),
// which sections 2 and 3 of the file time under this rule but without a sweep.  The model: one pair addition per entry and
// window, about four per bucket to finish and reduce it, and a fixed 256 per window (launch geometry, host tail) so that tiny
// inputs do not run dozens of windows -- K (n + 4 buckets + 256).
// one_level: the window of a fused batch (msm_run_batch_narrow), which must stay inside the one-level sort: the model capped at
// 13 bits whatever the size -- not measured against running the elements one by one under the rule above.
int pick_window_narrow(bool te, uint64_t n, int bits, bool one_level) {
  if (bits > 4 && bits <= 32 && !one_level) {
    const uint64_t from = bits > 8 ? 1ull << 18 : te ? 1ull << 22 : 1ull << 20;
    if (n >= from) return 17;
  }
  const int c_max = (n >= (1ull << 21) && !one_level && !(te && bits > 64 && n < (1ull << 23))) ? 22 : 13;
  int best = 2;
  double best_cost = 1e300;
  for (int c = 2; c <= c_max; c++) {
    int K = (bits + c) / c;
    double buckets = (double)(1u << (c - 1));
    if (!te && c >= 18 && K > 1 && (bits + 1) - (K - 1) * c == 1) { K -= 1; buckets *= 2; }   // the fold rule of make_plan
    if (K > 64) continue;   // (make_plan's bound)
    const double cost = (double)K * ((double)n + 4.0 * buckets + 256.0);
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}

// On window tables all windows of a group share one set of buckets, so a wider window costs its 2^(c-1) buckets once instead
// of K times and the optimum moves up.  BLS12-377 after GLV (127 bits: 18- and 21-bit windows fold the carry bit, no short top
// window to skew the merged buckets), measured with tools/tables_csweep.py (profiles/r05_experiments.txt item 5): 16 bits below
// 2^16 points, 18 from there (2^18 1.58 against 1.76 ms plain, 2^20 3.65 / 3.90, 2^22 11.0 / 11.9, 2^23 20.3 / 21.7), 21 from
// 2^24 (36.7 / 40.1).  BN254 G1 and Grumpkin (127 bits too) take the same rule, model only.  BLS12-381, Pallas and Vesta keep the
// plain choice (their 18-bit plan would end in a two-bit top window).
// Ed-on-BLS12-377 (252 bits, no endomorphism: K = 13 .. 28 windows on the plain path, whose reduction and host tail grow with K):
// 14 bits below 2^17 points, 17 from there (K = 15; 2^18 0.98 against 1.09 ms plain, 2^20 2.11 / 2.63, 2^22 7.3 / 8.6; 16 bits
// 2.28, 18 bits 2.17 at 2^20) -- with the merged window's sums finished bit-sliced (reduce_buckets).
static int pick_window_tables(bool te, uint64_t n, int glv_max_bits) {
  if (te) return n >= (1ull << 17) ? 17 : 14;
  if (glv_max_bits == 126) return n >= (1ull << 24) ? 21 : n >= (1ull << 16) ? 18 : 16;   // (2^15: 0.86 ms at 16 bits, 0.90 at 18; 2^16: 1.03 / 1.00)
  return pick_window(te, n, glv_max_bits);
}

int make_plan(const msm_ctx* ctx, uint64_t n, const msm_opts* opts, Plan& pl, bool for_tables, int narrow_bits) {
  const bool te = ctx && ctx->is_te();
  const bool narrow = narrow_bits > 0;
  const int glv_bits = curve_info(ctx ? ctx->curve : MSM_CURVE_BLS12_377_G1).glv_max_bits;
  const int glv_arg = (opts && opts->no_glv) ? 0 : glv_bits;
  int c = (opts && opts->c > 0) ? opts->c : narrow ? pick_window_narrow(te, n, narrow_bits)
          : for_tables ? pick_window_tables(te, n, glv_arg) : pick_window(te, n, glv_arg);
  if (c < 2 || c > 24) return MSM_ERR_ARG;
  // b = Scalar.maxBits after GLV (src/wasm/glv.ts:216-226), or the bit length of q without it (src/msm-basic.ts:56); a narrow
  // call (msm_run_narrow) brings its own: the magnitude bits the caller declared, and no endomorphism split
  pl.no_glv = !te && (narrow || (opts && opts->no_glv));
  pl.strict = opts && opts->strict;
  const int b = narrow ? narrow_bits : te ? 251 : pl.no_glv ? curve_info(ctx ? ctx->curve : MSM_CURVE_BLS12_377_G1).q_bits : glv_bits;
  if (pl.no_glv && !narrow && c < 4) return MSM_ERR_ARG;   // keeps K <= 64
  if (narrow && (b + c) / c > 64) return MSM_ERR_ARG;      // (the same bound: 128 bits under c = 2 would be 65 windows)
  pl.c = c;
  pl.K = (b + 1 + c - 1) / c;  // K = ceil((b + 1) / c), src/msm-batched-affine.ts:90, src/msm-basic.ts:59
  pl.bits = b + 1;
  pl.L_log = c - 1;
  // K c >= b + 1 keeps the carry of the signed recoding inside the top window (src/msm-batched-affine.ts:183-193).  When
  // b + 1 = (K - 1) c + 1 -- BLS12-377 after GLV: 127 = 7 * 18 + 1 = 6 * 21 + 1 -- that top window holds the carry bit and
  // nothing else: every entry with a carry lands in its bucket 1, a full window's worth of tree work for one bit (c = 21 at
  // 2^26: seven windows in 155 ms, six of 22 bits in 149).  The big-window plans fold that bit into the window below instead:
  // K - 1 windows, the top one c + 1 bits wide and not recoded (its magnitude is at most 2^c, it cannot carry out), the
  // others as before.  Every window gets 2^c buckets (the lower ones fill the lower half); window k still weighs 2^(c k),
  // so sums, shards and msm_combine are unchanged.  Only for c >= 18: those windows sort with per-window effective bits
  // (WinSplit) already.
  pl.fold = !te && c >= 18 && pl.K > 1 && (b + 1) - (pl.K - 1) * c == 1;
  if (pl.fold) {
    pl.K -= 1;
    pl.L_log = c;
  }
  pl.L = 1u << pl.L_log;
  pl.b_lo = pl.bt_lo = 0;
  pl.b_n = pl.bt_n = 0xFFFFFFFFu;
  if (opts && opts->bucket_shards > 1) {
    // Rank g of G takes the g-th of G equal parts of the bucket range every window's digits really cover -- 2^(c-1) for a
    // recoded window, the whole 2^c of a folded top window, 2^(bits left) for a short one -- so that all ranks sort and add the
    // same number of entries.  The last part runs to the end of the window's buckets whatever the digits do.
    if (opts->bucket_shard < 0 || opts->bucket_shard >= opts->bucket_shards) return MSM_ERR_ARG;
    const uint32_t g = (uint32_t)opts->bucket_shard, G = (uint32_t)opts->bucket_shards;
    auto cut = [&](uint64_t span, uint32_t& lo, uint32_t& cnt) {
      lo = (uint32_t)(span * g / G);
      const uint64_t hi = g + 1 == G ? (uint64_t)pl.L : span * (g + 1) / G;
      cnt = (uint32_t)(hi - lo);
    };
    const int top_bits = pl.fold ? c : std::min(c - 1, pl.bits - (pl.K - 1) * c);
    cut(pl.K > 1 ? 1ull << (c - 1) : 1ull << std::max(0, top_bits), pl.b_lo, pl.b_n);
    cut(1ull << std::max(0, top_bits), pl.bt_lo, pl.bt_n);
  }
  return MSM_OK;
}

// gather: round 1 (random row reads: wants two waves per SIMD to cover the latency).  The other rounds read
// coalesced, prefetched planes; a lone wave already gets ~88 % of a SIMD's issue rate, and every lane pays one field
// inversion (~19 pair additions' worth) per round, so small rounds run better on half as many lanes with twice the
// steps (2^18: 2.62 -> 2.45 ms; neutral at 2^20, 1 % at 2^22; round 1 at 2^22 would lose 60 %).
// lone: the launch has the GPU to itself (a window group of one window with no second group beside it -- the
// 8-GPU shard).  All waves of one resident batch then move through the memory-heavy forward sweep and the ALU-heavy
// backward sweep in step; four batches of 128 steps instead of one of 512 stagger the phases (2^26, one window:
// 31.5 -> 29.2 ms).  With two groups on two streams the other stream already fills the gaps and 512 is better.
RoundGeom round_geom(const msm_ctx* ctx, uint64_t n_out, bool gather, bool lone) {
  uint64_t target = (uint64_t)ctx->n_cu * 4 * BA_WAVES * 64;  // as many lanes as the kernel's launch bounds keep resident
  // steps at full width below which a non-gather round runs on half as many lanes: every lane pays one inversion per
  // round (~13 pair additions' worth), and one wave per SIMD already gets 89 % of the multiplier's two-wave rate
  // (tools/ubench_mul2.hip).  Measured with the round-2 kernel: 2^20 4.05 -> 3.91 ms, 2^22 12.9 -> 12.4, neutral elsewhere.
  const uint64_t half_below = 128;
  if (!gather && n_out < target * half_below) target /= 2;
  uint32_t max_steps = (lone && n_out >= target * 512) ? 128 : 512;
  MSM_KNOB(max_steps, "MSM_MAX_STEPS", 1);
  uint64_t steps = (n_out + target - 1) / target;
  steps = std::max<uint64_t>(1, std::min<uint64_t>(steps, max_steps));
  uint64_t threads = (n_out + steps - 1) / steps;
  uint64_t grid = std::max<uint64_t>(1, (threads + 255) / 256);
  return RoundGeom{(uint32_t)steps, (uint32_t)grid, grid * 256};
}

// how many windows fit one group under the workspace budget
void release_workspaces(msm_ctx* ctx) {
  for (auto& w : ctx->ws) {
    (void)hipStreamSynchronize(w.stream);
    w.for_each_buffer([](DevBuf& b) { b.release(); });
  }
}

long double window_bytes(const msm_ctx* ctx, uint64_t n, const Plan& pl) {
  // bytes per window and point (Weierstrass: 2 entries per point): digits 8, records of the sort's passes 16, slots (or the pair
  // list of a big window) ~9, tree buffers 96 + 48, prefix scratch 56; the tile-ordered round 1 of a big window (c >= 18) adds
  // the element index of every pair (4) and the element records (128 bytes per pair), and its plane buffers start one round
  // later.  Per window and bucket: counters, cursors, up to 34 offset tables, and the block histograms of the sort.
  const bool te = ctx->is_te();
  const bool big = pl.c > 16;
  long double per_point = te ? (4 + 8 + 5 + 64 + 32) : (8 + 16 + 9 + 96 + 48 + 56);
  if (big && !te) per_point += 4 + 128 - 72;
  const long double hist_bins = big ? (long double)(pl.L >> 7) : (long double)pl.L;
  return (long double)n * per_point + (long double)pl.L * 4 * 40 + hist_bins * 4 * (2.0L * ctx->n_cu);
}
int windows_per_group(const msm_ctx* ctx, uint64_t n, const Plan& pl) {
  int w = (int)std::max<long double>(1, (long double)ctx->ws_budget / msm_ctx::N_WS / window_bytes(ctx, n, pl));
  return std::min(w, pl.K);
}
// how many ranges of the points ONE window has to be cut into for its workspace to fit (1: it fits as a whole)
uint64_t point_pieces(const msm_ctx* ctx, uint64_t n, const Plan& pl) {
  const long double room = (long double)ctx->ws_budget / msm_ctx::N_WS;
  uint64_t pieces = 1;
  while (pieces < 256 && n / pieces > 4096 && window_bytes(ctx, (n + pieces - 1) / pieces, pl) > room) pieces++;
  return pieces;
}

GroupSchedule group_schedule(const msm_ctx* ctx, uint64_t n, uint64_t p_off, int k_lo, int k_hi, const Plan& pl,
                             const std::vector<uint64_t>& piece_end, bool serial) {
  GroupSchedule sc;
  const bool te = ctx->is_te();
  // window groups: as large as the workspace budget allows; for big inputs two of them on two streams.  The streams
  // run in step (both sort, both gather, ...): what the second one buys is two tree kernels sharing the chip -- forward
  // (memory-heavy) and backward (issue-heavy) sweeps of different waves mix, the small last rounds fill each other's
  // idle CUs -- not a sort hidden under an accumulation (a sort started under the other group's tree finds no free
  // registers on any CU and takes four times as long: profiles/r04_experiments.txt item 1)
  int wpg = std::min(windows_per_group(ctx, n, pl), 128);
  // the radix-split and three-pass sorts describe their windows in a WinSplit of 16 entries (sort_kernels.h): a group that
  // may take one of them holds at most 16 windows (msmProjective with a small explicit window: K = 17 .. 29 at c = 15 .. 9)
  // (the one-level sort of small inputs -- a window's counters fit the LDS and fewer than 2^22 entries per window -- has no
  // such table: Ed-on-BLS12-377 at 2^20 keeps its 18 windows in one group)
  // (on window tables the merged window of a group may take the bin split whatever a single digit window would have taken,
  // and the digit kernel describes the fine bits of at most 16 windows: pack_fine_bits)
  if (leaves_one_level(te, pl, te ? n : 2 * n) || pl.tables) wpg = std::min(wpg, 16);
  const int nwin = k_hi - k_lo;
  int want_groups = window_groups_wanted(te, n, pl.tables, nwin);
  MSM_KNOB(want_groups, "MSM_GROUPS", 1);
  wpg = std::max(1, std::min(wpg, (nwin + want_groups - 1) / want_groups));
  // on window tables a group reads one table per window, from table 0: no group is wider than the tables the set holds
  // (whatever the knob, the workspace budget or the window range of msm_window_sums say)
  if (pl.tables) wpg = std::max(1, std::min(wpg, pl.tab_T));
  sc.wpg = wpg;
  // A single window (the 8-GPU shard) has no second window group to hide its sort and tails under: split it by
  // points instead -- two half-size sub-MSMs of the same window on the two streams, their sums added on the host.
  // The same split serves inputs whose single window no longer fits the workspace budget (2^29 points: 165 GB per window
  // at c = 22 next to a 137 GB row table): every window runs over as many ranges of the points as it takes, one after the
  // other on the two streams, and the sums of its ranges are added on the host.
  uint64_t pieces = 1;
  if (nwin == 1 && want_groups == 1 && !te && n >= (1ull << 24) && !MSM_KNOB_SET("MSM_GROUPS")) pieces = 2;
  pieces = std::max(pieces, point_pieces(ctx, n, pl));
  // the workspace forces its own ranges: plain staged upload first (rare: 2^29 points, or a tight msm_set_workspace_limit)
  sc.piped = !piece_end.empty() && point_pieces(ctx, n, pl) == 1;
  std::vector<GroupSchedule::Group>& groups = sc.groups;
  if (sc.piped) {
    // pipelined host scalars: per arriving range of the points the usual window groups (two above 2^22 points), in order
    uint64_t lo = 0;
    for (size_t q = 0; q < piece_end.size(); q++) {
      const uint64_t cnt = piece_end[q] - lo;
      const int g = (nwin >= 2 && cnt >= (1ull << 22)) ? 2 : 1;
      const int per = std::max(1, std::min(wpg, (nwin + g - 1) / g));
      for (int k = k_lo; k < k_hi; k += per) groups.push_back({k, std::min(k_hi, k + per), lo, cnt, (int)q});
      lo = piece_end[q];
    }
  } else if (pieces > 1) {
    for (int k = k_lo; k < k_hi; k++)
      for (uint64_t q = 0; q < pieces; q++) {
        const uint64_t lo = n * q / pieces, hi = n * (q + 1) / pieces;
        groups.push_back({k, k + 1, lo, hi - lo, -1});
      }
  } else {
    for (int k = k_lo; k < k_hi; k += wpg) groups.push_back({k, std::min(k_hi, k + wpg), 0, n, -1});
  }
  // does more than one group contribute to a window?  Then the sums of its ranges are added on the host (combine_group_sums).
  for (const GroupSchedule::Group& g : groups) sc.split_points |= g.p_n != n;
  // Window tables address row k * tab_n + i of the points they cover from the entry index alone, which counts from the GROUP's
  // first point and in units of the group's own n: a group over another range of the points (a tight workspace limit, the retry
  // after an out-of-memory error, host scalars arriving range by range) would read other points' rows.  Such a call runs the
  // plain path under the same window -- table 0 is the plain row table -- and hands back one sum per window slot, which the
  // caller's Horner step takes like the one weighted sum of a run on tables.
  sc.tables = pl.tables && !(sc.split_points || n != pl.tab_n || p_off != pl.tab_lo);
  // The two window groups of a call slice the same scalars: one launch of the digit kernel (on the first workspace's stream)
  // writes the digits and slice histograms of both -- one GLV decomposition per scalar instead of two (2^26: the two
  // concurrent launches took 2.3 ms, the one takes 1.5) -- and each group then takes its part (GroupDigits, msm_sort.hip).
  sc.share_digits = groups.size() == 2 && !te && groups[0].piece < 0 && groups[1].piece < 0 &&
                    groups[0].p_lo == groups[1].p_lo && groups[0].p_n == groups[1].p_n && groups[0].kb == groups[1].ka &&
                    groups[1].kb - groups[0].ka <= 16;   // (the digit kernel describes up to 16 windows: WinSplit)
  // a launch that has the chip to itself -- the one-window shard, or every launch of a serialised call (msm_opts.serial,
  // the exclusive timing of the roofline) -- walks its pairs in four short batches instead of one long one (round_geom)
  sc.lone = (groups.size() == 1 && (groups[0].kb - groups[0].ka == 1 || sc.tables)) || serial;
  return sc;
}

SortGeometry sort_geometry(const msm_ctx* ctx, uint64_t n, const Plan& pl, int k_lo, int k_hi) {
  SortGeometry g;
  const bool te = ctx->is_te();
  const uint32_t L = pl.L;
  const int cbits = pl.L_log;   // bits of a bucket index
  g.kc_d = k_hi - k_lo;
  g.two_n_d = te ? n : 2 * n;   // entries per digit window: both GLV halves, or the plain scalar
  g.n_entries = (uint64_t)g.kc_d * g.two_n_d;
  // On window tables the kc_d digit windows of the group are ONE window for everything behind the digit kernel: the digit
  // array [kc_d][two_n_d] read as one run of entries, entry j = (window, point, half) naming row j of the tables.
  g.kc = pl.tables ? 1 : g.kc_d;
  g.two_n = pl.tables ? g.n_entries : g.two_n_d;
  g.nb = (uint64_t)g.kc * L;

  // padding granule G = 2^g: about 1/8 of the mean bucket population (pads cost G/2 slots per bucket; what is
  // left after g regular rounds, ~8 elements per bucket, is finished without inversions by k_bucket_finish)
  // Bigger buckets leave more: pads are identity pairs that occupy a lane for nothing (mean / (2 * left) of all slots), and
  // k_bucket_finish is cheap next to them.  Measured (profiles/r04_experiments.txt items 6 and 14, best `left` per mean bucket):
  // 64 entries 8 with 16-bit windows (2^20: 3.89 against 3.93 ms) but 16 with the big ones (2^25: 81.5 -> 79.9);
  // 128 .. 256: 16 (2^21 6.92 -> 6.88, 2^22 12.45 -> 12.17, Ed-377 2^20 2.64 -> 2.59, 2^26 145.7 -> 142.5, 2^27 304.9 -> 301.8);
  // from 512: 32 (2^23 22.65 -> 22.18, 2^26 at c = 16 152.7 -> 152.1); 32 entries: 8 (2^24: 16 costs 8 %).
  g.mean = std::max<uint64_t>(1, g.two_n / (pl.fold ? L / 2 : L));   // (a folded plan's lower windows fill half their buckets)
  // (on window tables at 2^20 points, mean 112 at c = 18: 8 -- a third regular round -- 3.37 against 3.41 ms)
  uint64_t per_bucket_left = g.mean >= 512 ? 32 : (g.mean >= 128 || (g.mean >= 64 && pl.c >= 18 && !pl.tables)) ? 16 : 8;
  MSM_KNOB(per_bucket_left, "MSM_PBL", 1);
  while (g.logG < 10 && (1ull << (g.logG + 1)) * per_bucket_left <= g.mean) g.logG++;

  // Sort path: LDS-privatised histogram / ranking, every pass staged through the LDS so that a wave store is a full segment
  // (sort_kernels.h; a direct scatter sends each 4-byte payload to a line of its own: round 1 wrote 7.7x the algorithmic bytes).
  //   one level  : a window's counters fit the LDS (c <= 16) and the input is small
  //   radix split: c <= 16, big inputs -- 2^(c-8) coarse bins x 128 buckets, two passes over pairs of 4-byte arrays
  //   bin split  : c > 16 (up to c = 24, the largest window make_plan accepts) -- coarse bins x up to 2^12 buckets, two passes
  //                over 8-byte records, the histogram of the first fused into the digit kernel, the second emitting the pairs
  //                of round 1 in an order that keeps its row gathers local
  // (the merged window of a run on window tables has kc = 1: the radix split would give its last pass one block per coarse bin,
  // 2^(c-8) of them for the whole chip -- the bin split cuts it into 2^10 bins whatever the window is)
  g.bin_split = !window_fits_lds(pl) || (pl.tables && g.two_n >= (1ull << 22));
  g.radix = !g.bin_split && leaves_one_level(te, pl, g.two_n);   // (counters that fit the LDS: at most 2^8 coarse bins)
  if ((g.bin_split || g.radix) && g.kc > 16)
    throw MsmFail{MSM_ERR_INTERNAL, g.bin_split ? "more than 16 windows in a group of a window size above 16" : "more than 16 windows in a radix-split group"};
  for (int kk = 0; kk < g.kc && g.bin_split; kk++) {
    // bits the digits of this window really have: the top window of a scalar is usually short (msm_kernels.h, WinSplit)
    // (a window below the top one holds signed digits of magnitude <= 2^(c - 1); the top one what is left of the scalar)
    const bool top = (k_lo + kk) % pl.K == pl.K - 1;   // (window k of its element in a batch: msm_run_batch)
    const int eff = pl.tables ? cbits : std::max(1, top ? std::min(cbits, pl.bits - (k_lo + kk) * pl.c) : std::min(cbits, pl.c - 1));
    // up to 10 bits: pass A sorts the window outright; else 2^10 coarse bins (16-entry runs of a 16 k tile), 2^11 if the
    // fine part would otherwise exceed 2^12 buckets per bin
    const int ab_big = 10;
    const int abk = eff <= ab_big ? eff : std::max(ab_big, eff - (int)BS_MAX_FB);
    if (abk > (int)BS_MAX_AB) throw MsmFail{MSM_ERR_INTERNAL, "window too wide for the bin split"};
    g.ws.ab[kk] = (uint8_t)abk;
    g.ws.fb[kk] = (uint8_t)(eff - abk);
    g.hb = std::max(g.hb, 1u << abk);
    g.nbmax = std::max(g.nbmax, 1u << (eff - abk));
  }
  for (int kk = 0; kk < g.kc && g.radix; kk++) { g.ws.ab[kk] = (uint8_t)(cbits - (int)RX_FINE_BITS); g.ws.fb[kk] = (uint8_t)RX_FINE_BITS; }
  g.hb_stride = g.hb;
  if (g.radix) g.Hn = 1u << (cbits - (int)RX_FINE_BITS);
  g.V = (uint32_t)g.kc * (g.bin_split ? g.hb : g.Hn);
  g.chunk = g.two_n;
  g.pps = n;
  if (g.bin_split) {
    // the digit kernel histograms ALL windows of the group over its slice of the points: four slices per CU, one slice per
    // 4 096 points at least; the digit kernel wants a few blocks per CU whatever kc_d is, k_slice_scan walks the kc_d * sortB
    // rows of the merged window with 32 lanes per column
    g.sortB = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)4 * ctx->n_cu, n / 4096));
    // (pass A names an entry by its offset inside the slice in BS_SPAN_LOG bits: from 2^27 points the slices multiply instead of growing)
    const uint64_t max_pps = (1ull << BS_SPAN_LOG) / (te ? 1 : 2);
    g.sortB = (uint32_t)std::max<uint64_t>(g.sortB, (n + max_pps - 1) / max_pps);
    g.pps = (n + g.sortB - 1) / g.sortB;
    g.chunk = (te ? 1 : 2) * g.pps;
    // a block of pass A takes as many consecutive slices of the digit kernel as make two tiles
    g.per_block = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(g.sortB, std::max<uint64_t>(1, (1ull << BS_SPAN_LOG) / g.chunk)),
                                               std::max<uint64_t>(1, (2 * (uint64_t)BS_TILE + g.chunk - 1) / g.chunk));
    // heavy bins are cut into parts of part_len records, one block each (sort_kernels.h, "Parts of heavy bins"): twice the mean
    // bin, so that uniform digits never see one; a multiple of the tile of pass B.  The table comes out of k_vscan.
    g.part_len = (uint32_t)std::max<uint64_t>(1u << 16, ((2 * g.n_entries / g.V + BP_TILE - 1) / BP_TILE) * BP_TILE);
    g.part_grid = g.V + g.V / 2 + 1;
    // Big windows over a big table take the pair form: from more than 2^23 rows of 256 bytes = 2 GB (measured,
    // tools/chunk_plain.py on the round-5 tuning build: at 2^23 rows -- 2^23 points, or 2^20 on seven window tables -- the plain
    // slot form is 2.5 % ahead: 20.15 against 20.64 ms, 3.23 / 3.32; at 2^23.8 rows level; at 2^24 rows the tile order wins by
    // 10 %: 38.6 against 43.0).  chunk_rows_log: 23 unless a test has moved it.
    // (round 2 must be an index-free round to read the element records round 1 then writes: logG >= 2)
    const uint64_t table_rows = pl.tables ? (uint64_t)g.kc_d * n : n;
    g.pairs = !te && pl.c >= 18 && table_rows > (1ull << ctx->chunk_rows_log) && g.logG >= 2;
  } else {
    // big inputs: finer slices also keep the round-1 gathers of neighbouring lanes inside one Infinity-Cache-sized
    // range of point rows (measured: 193 -> 183 ms at 2^26); small inputs: fewer, larger blocks (less fixed cost)
    const uint64_t mult = g.two_n >= (1ull << 27) ? 8 : g.two_n >= (1ull << 24) ? 4 : 2;   // measured 2^21 .. 2^26
    const uint64_t want = std::max<uint64_t>(1, (mult * ctx->n_cu + g.kc - 1) / g.kc);
    g.sortB = (uint32_t)std::min<uint64_t>(want, std::max<uint64_t>(1, g.two_n / 8192));
    g.chunk = (g.two_n + g.sortB - 1) / g.sortB;
  }
  // The padded slots have a bound -- every non-empty bucket pads by less than G -- which lets the bin split's last pass start
  // before the totals are read back.  (the parts of a heavy bin pair their entries up on their own: a bucket gains at most one
  // slot per part that holds an odd number of its entries -- sort_kernels.h, "Parts of heavy bins")
  g.parts_extra = g.pairs ? std::min<uint64_t>(g.n_entries, (uint64_t)g.V * g.nbmax) : 0;
  g.slots_bound = g.n_entries + g.parts_extra + (((uint64_t)1 << g.logG) - 1) * std::min<uint64_t>(g.nb, g.n_entries);
  return g;
}

}  // namespace msmi
