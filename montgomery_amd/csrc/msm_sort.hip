// Digits and counting sort of one window group: scalars -> signed window digits -> bucket-sorted payload slots, every
// bucket padded to a multiple of 2^logG slots, plus the offset tables of the tail rounds.  What is cut where is decided by
// sort_geometry (msm_plan.hip); this file allocates, launches and reads back.
// (reference phases: decompose + slices src/msm-batched-affine.ts:175-203, integrateBucketCounts :423-447, sortPoints :456-502)
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace msmi {

void sort_kernel_attributes() {
  // dynamic LDS above the 64 KB a launch gets by default
  HIPCHK(hipFuncSetAttribute((const void*)k_hist, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)k_scatter_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)k_bin_split, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bin_split_lds(1u << BS_MAX_AB)));
  HIPCHK(hipFuncSetAttribute((const void*)k_bin_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bin_pairs_lds(1u << BS_MAX_FB)));
  HIPCHK(hipFuncSetAttribute((const void*)k_bin_slots, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bin_slots_lds(1u << BS_MAX_FB)));
  const int dig_lds = 16 * (1 << BS_MAX_AB) * 4;   // the fused histogram of up to 16 windows
#define MSM_DIGITS_ATTR(ID, CV) HIPCHK(hipFuncSetAttribute((const void*)k_digits<CV>, hipFuncAttributeMaxDynamicSharedMemorySize, dig_lds));
  MSM_W_CURVES(MSM_DIGITS_ATTR)
#undef MSM_DIGITS_ATTR
  HIPCHK(hipFuncSetAttribute((const void*)te::k_te_digits, hipFuncAttributeMaxDynamicSharedMemorySize, dig_lds));
#define MSM_NARROW_ATTR(W)                                                                                                    \
  HIPCHK(hipFuncSetAttribute((const void*)k_digits_narrow<W>, hipFuncAttributeMaxDynamicSharedMemorySize, dig_lds));          \
  HIPCHK(hipFuncSetAttribute((const void*)k_te_digits_narrow<W>, hipFuncAttributeMaxDynamicSharedMemorySize, dig_lds));
  MSM_NARROW_WIDTHS(MSM_NARROW_ATTR)
#undef MSM_NARROW_ATTR
}

// k_digits / k_te_digits write the digits and, for the bin split, the histogram of its first pass (one slice of the points per
// block); k_digits_narrow / k_te_digits_narrow of the call's width write the same for a narrow call (msm_run_narrow); the _batch
// forms write the digits of a fused batch (msm_run_batch: the kc_d windows are the K windows of pl.batch elements, virtual
// windows), which is sized to take the one-level sort (msm_batch.hip) and needs no slice histograms.
GroupDigits launch_group_digits(msm_ctx* ctx, msm_ctx::Workspace& w, const uint32_t* d_scalars, uint64_t n, const Plan& pl, int k_lo,
                                const SortGeometry& g, hipEvent_t ready) {
  hipStream_t s = w.stream;
  const bool te = ctx->is_te();
  ctx->ensure(w.dig, g.n_entries * 4);
  if (g.bin_split) ctx->ensure(w.block_hist, (size_t)g.kc_d * g.sortB * g.hb * 4 + 64);
  uint32_t* dig = (uint32_t*)w.dig.p;
  uint32_t* err = (uint32_t*)ctx->errflag.p;
  const int W = pl.nar.width, per_lane = W == 1 ? 4 : W == 2 ? 2 : 1;   // (a lane of the 1- and 2-byte formats takes 4 / 2 scalars)
  const int fold = pl.fold ? 1 : 0, glv_flags = (pl.no_glv ? 0 : 1) | (pl.fold ? 2 : 0), strict = pl.strict ? 1 : 0;
  if (pl.batch) {
    if (g.bin_split || g.radix || k_lo != 0 || g.kc_d != pl.batch * pl.K || (W && !pl.nar.nb))
      throw MsmFail{MSM_ERR_INTERNAL, "a batch group outside the one-level sort"};
    const uint32_t grid = (uint32_t)(((n + per_lane - 1) / per_lane + 255) / 256);   // one thread per lane's points
#define MSM_NARROW_LAUNCH_B(WW)                                                                                               \
  if (W == WW) {                                                                                                              \
    if (te) hipLaunchKernelGGL(k_te_digits_narrow_batch<WW>, dim3(grid), dim3(256), 0, s, dig, *pl.nar.nb, (uint32_t)pl.batch, \
                               (uint32_t)n, pl.c, pl.K, fold, pl.nar.fmt, err);                                               \
    else hipLaunchKernelGGL(k_digits_narrow_batch<WW>, dim3(grid), dim3(256), 0, s, dig, *pl.nar.nb, (uint32_t)pl.batch,      \
                            (uint32_t)n, pl.c, pl.K, fold, pl.nar.fmt, err);                                                  \
  }
    MSM_NARROW_WIDTHS(MSM_NARROW_LAUNCH_B)
#undef MSM_NARROW_LAUNCH_B
    if (!W && te)
      hipLaunchKernelGGL(te::k_te_digits_batch, dim3(grid), dim3(256), 0, s, dig, pl.batch_sc, (uint32_t)pl.batch, (uint32_t)n, pl.c, pl.K,
                         strict, err);
    else if (!W)
      W_LAUNCH(ctx, k_digits_batch, dim3(grid), dim3(256), 0, s, dig, pl.batch_sc, (uint32_t)pl.batch, (uint32_t)n, pl.c, pl.K, glv_flags,
               strict, err);
  } else {
    // (a slice per block leaves four blocks per CU: 1024 threads each keep the SIMDs full, 256 left them at four waves)
    const uint32_t per = g.bin_split ? (uint32_t)g.pps : 256u * per_lane;
    const uint32_t grid = g.bin_split ? g.sortB : (uint32_t)((n + per - 1) / per);
    const uint32_t threads = g.bin_split ? 1024u : 256u;
    uint32_t* hist = g.bin_split ? (uint32_t*)w.block_hist.p : nullptr;
    const size_t lds = g.bin_split ? (size_t)g.kc_d * g.hb * 4 : 0;
    WinSplit ws_d = g.ws;   // the digit kernel counts per DIGIT window: on tables all of them with the merged window's cut
    if (pl.tables) for (int kk = 0; kk < 16; kk++) ws_d.fb[kk] = g.ws.fb[0];
    const uint64_t fbp = pack_fine_bits(ws_d);
#define MSM_NARROW_LAUNCH(WW)                                                                                                 \
  if (W == WW) {                                                                                                              \
    if (te) hipLaunchKernelGGL(k_te_digits_narrow<WW>, dim3(grid), dim3(threads), lds, s, dig, (const void*)d_scalars,        \
                               pl.nar.first, (uint32_t)n, pl.c, pl.K, k_lo, g.kc_d, fold, pl.nar.fmt, err, per, hist, g.hb, fbp); \
    else hipLaunchKernelGGL(k_digits_narrow<WW>, dim3(grid), dim3(threads), lds, s, dig, (const void*)d_scalars, pl.nar.first, \
                            (uint32_t)n, pl.c, pl.K, k_lo, g.kc_d, fold, pl.nar.fmt, err, per, hist, g.hb, fbp);              \
  }
    MSM_NARROW_WIDTHS(MSM_NARROW_LAUNCH)
#undef MSM_NARROW_LAUNCH
    if (!W && te)
      hipLaunchKernelGGL(te::k_te_digits, dim3(grid), dim3(threads), lds, s, dig, d_scalars, (uint32_t)n, pl.c, pl.K, k_lo, g.kc_d, strict,
                         err, per, hist, g.hb, fbp, pl.b_lo, pl.b_n, pl.bt_lo, pl.bt_n);
    else if (!W)
      W_LAUNCH(ctx, k_digits, dim3(grid), dim3(threads), lds, s, dig, d_scalars, (uint32_t)n, pl.c, pl.K, k_lo, g.kc_d, glv_flags, strict,
               err, per, hist, g.hb, fbp, pl.b_lo, pl.b_n, pl.bt_lo, pl.bt_n);
  }
  if (ready) HIPCHK(hipEventRecord(ready, s));
  return GroupDigits{k_lo, dig, g.bin_split ? (uint32_t*)w.block_hist.p : nullptr, g.hb, g.sortB, g.pps, g.chunk, ready, true};
}

// largest bucket -> number of tail rounds RT, then the multi-block scan of RT + 2 quantities.  The scan kernels take RT
// from the device (pscan_nq), so ONE read-back behind them brings the largest bucket and the totals together.
void scan_bucket_sizes(msm_ctx* ctx, msm_ctx::Workspace& w, uint64_t nb, uint32_t logG, bool find_max) {
  hipStream_t s = w.stream;
  if (find_max) {
    HIPCHK(hipMemsetAsync(w.info.p, 0, 64 * 4, s));
    hipLaunchKernelGGL(k_bucket_max, dim3((uint32_t)std::min<uint64_t>(1024, (nb + 255) / 256)), dim3(256), 0, s,
                       (const uint32_t*)w.counts.p, (uint32_t)nb, (uint32_t*)w.info.p);
  }
  const uint32_t nblocks = (uint32_t)((nb + PS_SPAN - 1) / PS_SPAN);
  ctx->ensure(w.scan_partial, (size_t)PS_MAX_NQ * nblocks * 4);
  hipLaunchKernelGGL(k_pscan_partial, dim3(nblocks), dim3(PS_BLOCK), 0, s, (const uint32_t*)w.counts.p, (uint32_t)nb, logG,
                     (const uint32_t*)w.info.p, (uint32_t*)w.scan_partial.p, nblocks);
  hipLaunchKernelGGL(k_pscan_top, dim3(1), dim3(SCAN_THREADS), 0, s, (uint32_t*)w.scan_partial.p, nblocks, logG,
                     (uint32_t*)w.info.p);
  hipLaunchKernelGGL(k_pscan_final, dim3(nblocks), dim3(PS_BLOCK), 0, s, (const uint32_t*)w.counts.p, (uint32_t)nb, logG,
                     (const uint32_t*)w.scan_partial.p, nblocks, (uint32_t*)w.cursor.p, (uint32_t*)w.tail_off.p,
                     (const uint32_t*)w.info.p);
  HIPCHK(hipEventRecord(w.ev[7], s));
}

ScanTotals read_scan_totals(msm_ctx::Workspace& w, uint32_t logG) {
  ScanTotals t;
  HIPCHK(hipStreamWaitEvent(w.side, w.ev[7], 0));
  HIPCHK(hipMemcpyAsync(w.h_info, w.info.p, 64 * 4, hipMemcpyDeviceToHost, w.side));
  HIPCHK(hipStreamSynchronize(w.side));
  t.total_slots = w.h_info[0];
  t.max_bucket = w.h_info[1];
  t.algo_pairs = (uint64_t)w.h_info[INFO_ALGO_PAIRS] | ((uint64_t)w.h_info[INFO_ALGO_PAIRS + 1] << 32);
  const uint32_t capmax = (t.max_bucket + (1u << logG) - 1) >> logG;
  while (t.RT < 32 && (1u << t.RT) < capmax) t.RT++;
  return t;
}

namespace {

// the scans and the one read-back every path shares; the totals go into the group's statistics
ScanTotals scan_and_read(msm_ctx::Workspace& w, const SortGeometry& g, GroupStats& st) {
  const ScanTotals tot = read_scan_totals(w, g.logG);
  st.n_pairs_algo += tot.algo_pairs;
  st.max_bucket = std::max<uint64_t>(st.max_bucket, tot.max_bucket);
  if (tot.total_slots > g.slots_bound) throw MsmFail{MSM_ERR_INTERNAL, "the padded slots exceed their bound"};
  return tot;
}

// The front half of the two sorts whose counters fit the LDS (c <= 16): per-slice histograms of the digits in w.dig, the bucket
// sizes, the scans, the read-back, and the slots, still empty
ScanTotals count_in_lds(msm_ctx* ctx, msm_ctx::Workspace& w, const Plan& pl, const SortGeometry& g, GroupStats& st, SortOut& so) {
  hipStream_t s = w.stream;
  hipLaunchKernelGGL(k_hist, dim3(g.sortB, g.kc), dim3(SORT_THREADS), (size_t)pl.L * 4, s, (uint32_t*)w.block_hist.p,
                     (const uint32_t*)w.dig.p, g.two_n, g.chunk, pl.L);
  hipLaunchKernelGGL(k_colscan, dim3((uint32_t)((g.nb + 255) / 256)), dim3(256), 0, s, (uint32_t*)w.block_hist.p,
                     (uint32_t*)w.counts.p, g.sortB, pl.L, (uint32_t)g.kc);
  scan_bucket_sizes(ctx, w, g.nb, g.logG, true);
  const ScanTotals tot = scan_and_read(w, g, st);
  ctx->ensure(w.slots, std::max<uint64_t>(tot.total_slots, 2) * 4);
  HIPCHK(hipMemsetAsync(w.slots.p, 0xFF, std::max<uint64_t>(tot.total_slots, 2) * 4, s));
  so.round1_slots = (const uint32_t*)w.slots.p;
  return tot;
}
void scatter_one_level(msm_ctx::Workspace& w, const Plan& pl, const SortGeometry& g) {
  hipLaunchKernelGGL(k_scatter_lds, dim3(g.sortB, g.kc), dim3(SORT_THREADS), (size_t)pl.L * 4, w.stream, (uint32_t*)w.slots.p,
                     (const uint32_t*)w.cursor.p, (const uint32_t*)w.block_hist.p, (const uint32_t*)w.dig.p, g.two_n, g.chunk, pl.L);
}

ScanTotals sort_one_level(msm_ctx* ctx, msm_ctx::Workspace& w, const Plan& pl, const SortGeometry& g, GroupStats& st, SortOut& so) {
  const ScanTotals tot = count_in_lds(ctx, w, pl, g, st, so);
  scatter_one_level(w, pl, g);
  so.path = MSM_SORT_ONE_LEVEL;
  return tot;
}

// Radix split: the one-level sort's histogram, then two passes -- unless one bucket is too heavy for their last one
ScanTotals sort_radix(msm_ctx* ctx, msm_ctx::Workspace& w, const Plan& pl, const SortGeometry& g, GroupStats& st, SortOut& so) {
  hipStream_t s = w.stream;
  const uint32_t L = pl.L, kc = (uint32_t)g.kc, sortB = g.sortB, Hn = g.Hn, V = g.V;
  const ScanTotals tot = count_in_lds(ctx, w, pl, g, st, so);
  if (radix_bucket_too_heavy(g, tot.max_bucket)) {
    scatter_one_level(w, pl, g);
  } else {
    // pass A: coarse split into dig2 / idx2; pass B: one block per coarse bin, payloads to their padded slots
    ctx->ensure(w.part, ((size_t)kc * sortB * Hn + 2 * (size_t)V + 2) * 4);
    uint32_t* d_blk_off = (uint32_t*)w.part.p;
    uint32_t* d_vtot = d_blk_off + (size_t)kc * sortB * Hn;
    uint32_t* d_vstart = d_vtot + V;
    ctx->ensure(w.dig2, g.n_entries * 4);
    ctx->ensure(w.idx2, g.n_entries * 4);
    const uint64_t co = (uint64_t)kc * (sortB + 1) * Hn;
    hipLaunchKernelGGL(k_coarse_offsets, dim3((uint32_t)((co + 255) / 256)), dim3(256), 0, s, d_blk_off, d_vtot,
                       (const uint32_t*)w.block_hist.p, (const uint32_t*)w.counts.p, sortB, L, Hn, kc);
    hipLaunchKernelGGL(k_vscan, dim3(1), dim3(SCAN_THREADS), 0, s, d_vstart, (const uint32_t*)d_vtot, V, (uint32_t*)nullptr, PartTables{});
    hipLaunchKernelGGL(k_radix_coarse, dim3(sortB, kc), dim3(RX_THREADS), 0, s, (uint32_t*)w.dig2.p, (uint32_t*)w.idx2.p,
                       (const uint32_t*)d_vstart, (const uint32_t*)d_blk_off, (const uint32_t*)w.dig.p, g.two_n, g.chunk, Hn, g.ws);
    hipLaunchKernelGGL(k_radix_fine, dim3(V), dim3(RXB_THREADS), 0, s, (uint32_t*)w.slots.p, (const uint32_t*)w.cursor.p,
                       (const uint32_t*)d_vstart, (const uint32_t*)w.dig2.p, (const uint32_t*)w.idx2.p, Hn, L, g.ws);
  }
  so.path = MSM_SORT_RADIX;
  return tot;
}

// Bin split (c > 16, and the merged window of a big run on window tables): the slices' prefixes and the bin starts, pass A, the
// bucket sizes, the scans, and the last pass in its slot or pair form.  dig, hist: the group's digits and slice histograms.
ScanTotals sort_bin_split(msm_ctx* ctx, msm_ctx::Workspace& w, const Plan& pl, const SortGeometry& g, const uint32_t* dig,
                          uint32_t* hist, GroupStats& st, SortOut& so) {
  hipStream_t s = w.stream;
  const uint32_t L = pl.L, kc = (uint32_t)g.kc, sortB = g.sortB, hb = g.hb_stride, V = g.V, nbmax = g.nbmax;
  // per (window, bin): the slices' prefixes and the total -> the bin starts (V + 1 of them in the record array)
  ctx->ensure(w.part, ((size_t)2 * V + 2) * 4);
  uint32_t* d_bin_tot = (uint32_t*)w.part.p;
  uint32_t* d_bin_start = d_bin_tot + V;
  ctx->ensure(w.rec, g.n_entries * 8);
  // (on tables the slices of all kc_d digit windows are the slices of the one merged window, in the same row order)
  hipLaunchKernelGGL(k_slice_scan, dim3((hb + 31) / 32, kc), dim3(1024), 0, s, hist, d_bin_tot,
                     pl.tables ? sortB * (uint32_t)g.kc_d : sortB, hb, kc);
  // the parts of heavy bins: their table comes out of k_vscan
  ctx->ensure(w.parts, ((size_t)2 * (V + 1) + (V + 2)) * 4);
  uint32_t* d_extra_first = (uint32_t*)w.parts.p;
  uint32_t* d_mp_first = d_extra_first + (V + 1);
  uint32_t* d_part_pair_off = d_mp_first + (V + 1);
  PartTables ptab{d_extra_first, d_mp_first, d_part_pair_off, hb, g.part_len, {}};
  for (int kk = 0; kk < 16; kk++) ptab.fb[kk] = g.ws.fb[kk];
  hipLaunchKernelGGL(k_vscan, dim3(1), dim3(SCAN_THREADS), 0, s, d_bin_start, (const uint32_t*)d_bin_tot, V, (uint32_t*)w.info.p, ptab);
  hipLaunchKernelGGL(k_bin_split, dim3((sortB + g.per_block - 1) / g.per_block, g.kc_d), dim3(BS_THREADS), bin_split_lds(hb), s,
                     (uint2*)w.rec.p, (const uint32_t*)d_bin_start, (const uint32_t*)hist, dig, g.two_n_d, g.chunk, hb, g.ws,
                     pl.tables ? 1u : 0u, sortB, g.per_block);
  // k_bin_count leaves the largest bucket and the pair count in `info` as k_bucket_max does for the other paths, and writes
  // every bucket of the bins it is launched for: `counts` needs a fill only where a window's digits do not span all L buckets
  if (!g.spans_all(pl.L_log)) HIPCHK(hipMemsetAsync(w.counts.p, 0, g.nb * 4, s));   // (`info` was cleared by k_vscan)
  ctx->ensure(w.sub, (size_t)(V + 2) * nbmax * 4);   // rows: the parts of multi-part bins, at most V of them
  hipLaunchKernelGGL(k_bin_count, dim3(g.part_grid), dim3(BC_THREADS), (size_t)nbmax * 4, s, (uint32_t*)w.counts.p, (const uint32_t*)d_bin_start,
                     (const uint2*)w.rec.p, hb, L, g.ws, (uint32_t*)w.info.p, V, (const uint32_t*)d_extra_first, (const uint32_t*)d_mp_first,
                     g.part_len, (uint32_t*)w.sub.p, nbmax);
  hipLaunchKernelGGL(k_part_scan, dim3(V), dim3(PSC_THREADS), 0, s, (uint32_t*)w.counts.p, (uint32_t*)w.sub.p, d_part_pair_off,
                     (const uint32_t*)d_extra_first, (const uint32_t*)d_mp_first, hb, L, nbmax, g.ws, (uint32_t*)w.info.p,
                     g.pairs ? 1u : 0u);
  // (the count pass has left the largest bucket in `info`)
  scan_bucket_sizes(ctx, w, g.nb, g.logG, false);
  // Pair form: round 1 walks the pairs in the order the last pass emits them -- tile by tile of a bin's records, which are in
  // point order -- and writes every sum to the element index that comes with the pair, as 64-byte records that round 2 reads
  // back (batch_add.h).  Needed once the 128 slots of a wave span more than ~1 GB of rows (sort_geometry).  Smaller tables take
  // the bucket-ordered slots of k_bin_slots.
  auto launch_last_pass = [&](bool pairs, uint64_t slots_cap) {
    so.chunked = pairs;
    so.round1_dest = nullptr;
    so.rec_y_off = 0;
    if (pairs) {
      const uint64_t pairs_cap = slots_cap / 2 + 1;
      ctx->ensure(w.slots2, pairs_cap * 8);
      ctx->ensure(w.dest, pairs_cap * 4);
      so.rec_y_off = (pairs_cap * 64 + 255) & ~(uint64_t)255;
      ctx->ensure(w.rows1, 2 * so.rec_y_off + 256);
      hipLaunchKernelGGL(k_bin_pairs, dim3(g.part_grid), dim3(BP_THREADS), bin_pairs_lds(nbmax), s, (uint2*)w.slots2.p, (uint32_t*)w.dest.p,
                         (const uint2*)w.rec.p, (const uint32_t*)d_bin_start, (const uint32_t*)w.cursor.p, hb, L, nbmax, g.ws, V,
                         (const uint32_t*)d_extra_first, (const uint32_t*)d_mp_first, g.part_len, (const uint32_t*)w.sub.p,
                         (const uint32_t*)d_part_pair_off);
      so.round1_slots = (const uint32_t*)w.slots2.p;
      so.round1_dest = (const uint32_t*)w.dest.p;
    } else {
      ctx->ensure(w.slots, std::max<uint64_t>(slots_cap, 2) * 4);
      HIPCHK(hipMemsetAsync(w.slots.p, 0xFF, std::max<uint64_t>(slots_cap, 2) * 4, s));
      so.round1_slots = (const uint32_t*)w.slots.p;
      hipLaunchKernelGGL(k_bin_slots, dim3(g.part_grid), dim3(BP_THREADS), bin_slots_lds(nbmax), s, (uint32_t*)w.slots.p,
                         (const uint2*)w.rec.p, (const uint32_t*)d_bin_start, (const uint32_t*)w.cursor.p, hb, L, nbmax, g.ws, V,
                         (const uint32_t*)d_extra_first, (const uint32_t*)d_mp_first, g.part_len, (const uint32_t*)w.sub.p);
    }
  };
  // The last pass needs nothing from the host but room for what it writes, and the padded slots have a bound, so it is launched
  // BEHIND the scans at once and the read-back of the totals (which the tree's launches wait for) crosses on a side stream while
  // it runs: no idle gap of a host round trip in front of it (25 us of the 3.4 ms of an MSM over 2^20 points).
  launch_last_pass(g.pairs, g.slots_bound);
  const ScanTotals tot = scan_and_read(w, g, st);
  if (g.pairs && pair_form_tree_empty(tot.total_slots)) launch_last_pass(false, 2);
  so.path = so.chunked ? MSM_SORT_PAIRS : MSM_SORT_SLOTS;
  return tot;
}

}  // namespace

// windows [k_lo, k_hi) over n points whose scalars start at d_scalars (n x 8 words); queues everything on w.stream, records
// w.ev[0] (start), w.ev[1] (digits done), w.ev[2] (sort done) and returns after ONE read-back (largest bucket, scan totals ->
// w.h_info: the launch geometry of the tree)
void sort_window_group(msm_ctx* ctx, msm_ctx::Workspace& w, const uint32_t* d_scalars, uint64_t n, const Plan& pl, int k_lo, int k_hi,
                       GroupStats& st, SortOut& so, const GroupDigits* share) {
  hipStream_t s = w.stream;
  so = SortOut{};
  SortGeometry g = sort_geometry(ctx, n, pl, k_lo, k_hi);
  const bool consume = share && share->valid;
  if (consume) {
    if (!g.bin_split) throw MsmFail{MSM_ERR_INTERNAL, "shared digits for a group that does not take the bin split"};
    // (the producer sliced all groups' windows at once: same slices, and the stride of the widest window's bins)
    if (share->sortB != g.sortB || share->pps != g.pps || share->chunk != g.chunk || share->hb < g.hb)
      throw MsmFail{MSM_ERR_INTERNAL, "shared digits do not match the group's sort geometry"};
    g.hb_stride = share->hb;
  }
  ctx->ensure(w.counts, g.nb * 4);
  ctx->ensure(w.cursor, (g.nb + 1) * 4);   // [nb] = the total (k_pscan_final)
  ctx->ensure(w.tail_off, (size_t)34 * (g.nb + 1) * 4);
  ctx->ensure(w.info, 64 * 4);
  if (!g.bin_split) ctx->ensure(w.block_hist, (size_t)g.kc * g.sortB * pl.L * 4 + 64);

  if (consume) HIPCHK(hipStreamWaitEvent(s, share->ready, 0));   // (the producer's launch is timed by the caller, not as this group's wait)
  HIPCHK(hipEventRecord(w.ev[0], s));
  // where this group's digits and slice histograms are: its own buffers, or its part of the producer's
  const GroupDigits d = consume ? *share : launch_group_digits(ctx, w, d_scalars, n, pl, k_lo, g);
  const uint32_t* dig = d.dig + (uint64_t)(k_lo - d.k_lo) * g.two_n_d;
  uint32_t* hist = d.hist + (uint64_t)(k_lo - d.k_lo) * g.sortB * g.hb_stride;   // (bin split only)
  HIPCHK(hipEventRecord(w.ev[1], s));
  const ScanTotals tot = g.bin_split ? sort_bin_split(ctx, w, pl, g, dig, hist, st, so)
                         : g.radix   ? sort_radix(ctx, w, pl, g, st, so)
                                     : sort_one_level(ctx, w, pl, g, st, so);
  HIPCHK(hipEventRecord(w.ev[2], s));
  so.logG = g.logG;
  so.RT = tot.RT;
  so.total_slots = tot.total_slots;
  so.max_bucket = tot.max_bucket;
}

}  // namespace msmi
