// Host-side unit-test shim of the window-group schedule and the sort geometry: msmi::group_schedule and msmi::sort_geometry of
// montgomery_amd/csrc/msm_plan.hip, which this file is compiled together with, over a default-constructed context that has no
// stream and no helper thread -- only the curve, the CU count, the workspace budget and the pair-form threshold they read
// (tests/test_group_schedule.py, tests/test_sort_geometry.py).  No GPU is touched.
#include "msm_internal.h"
using namespace msmi;

namespace {

struct Call {
  msm_ctx ctx;
  Plan pl;
  bool ok = false;
  Call(int curve, int n_cu, uint64_t ws_budget, uint64_t n, int c, int no_glv) {
    ctx.curve = curve;
    ctx.n_cu = n_cu;
    ctx.ws_budget = ws_budget;
    msm_opts o;
    memset(&o, 0, sizeof o);
    o.c = c;
    o.no_glv = no_glv;
    ok = make_plan(&ctx, n, &o, pl) == MSM_OK;
  }
};

}  // namespace

extern "C" {

// the plan make_plan gives an explicit window: out = {K, L_log}; 0 if it refuses c
int gs_plan(int curve, uint64_t n, int c, int no_glv, int32_t* out) {
  Call cl(curve, 256, 0, n, c, no_glv);
  if (!cl.ok) return 0;
  out[0] = cl.pl.K;
  out[1] = cl.pl.L_log;
  return 1;
}

// window_bytes of the budget model, rounded down to whole bytes
uint64_t gs_window_bytes(int curve, int n_cu, uint64_t n, int c, int no_glv) {
  Call cl(curve, n_cu, 0, n, c, no_glv);
  return cl.ok ? (uint64_t)window_bytes(&cl.ctx, n, cl.pl) : 0;
}

// The schedule of windows [k_lo, k_hi) over n points from p_off under the plan of window c.  tab_T > 0: the plan carries window
// tables, tab_T of them over the points [tab_lo, tab_lo + tab_n).  host_scalars: they are piped where the library pipes them.
// Groups -> ka, kb, p_lo, p_n, piece (room for `cap` each); flags = {wpg, tables, split_points, piped, share_digits, lone}.
// Returns the number of groups, -1 if make_plan refuses the window, -2 if there are more than cap.
int gs_schedule(int curve, int n_cu, uint64_t ws_budget, uint64_t n, uint64_t p_off, int c, int no_glv, int k_lo, int k_hi, int tab_T,
                uint64_t tab_lo, uint64_t tab_n, int host_scalars, int serial, int cap, int32_t* ka, int32_t* kb, uint64_t* p_lo,
                uint64_t* p_n, int32_t* piece, int32_t* flags) {
  Call cl(curve, n_cu, ws_budget, n, c, no_glv);
  if (!cl.ok) return -1;
  cl.pl.tables = tab_T > 0;
  cl.pl.tab_T = tab_T;
  cl.pl.tab_lo = tab_lo;
  cl.pl.tab_n = tab_n;
  std::vector<uint64_t> piece_end;
  if (host_scalars && pipelines_host_scalars(n)) piece_end = pipelined_piece_ends(n);
  const GroupSchedule sc = group_schedule(&cl.ctx, n, p_off, k_lo, k_hi, cl.pl, piece_end, serial != 0);
  if (sc.groups.size() > (size_t)cap) return -2;
  for (size_t i = 0; i < sc.groups.size(); i++) {
    ka[i] = sc.groups[i].ka;
    kb[i] = sc.groups[i].kb;
    p_lo[i] = sc.groups[i].p_lo;
    p_n[i] = sc.groups[i].p_n;
    piece[i] = sc.groups[i].piece;
  }
  const int32_t f[6] = {sc.wpg, sc.tables, sc.split_points, sc.piped, sc.share_digits, sc.lone};
  memcpy(flags, f, sizeof f);
  return (int)sc.groups.size();
}

// leaves_one_level for a window of the call's plan over all n points; -1 if make_plan refuses the window
int gs_leaves_one_level(int curve, uint64_t n, int c, int no_glv) {
  Call cl(curve, 256, 0, n, c, no_glv);
  if (!cl.ok) return -1;
  return leaves_one_level(cl.ctx.is_te(), cl.pl, cl.ctx.is_te() ? n : 2 * n) ? 1 : 0;
}

// sort_geometry of windows [k_lo, k_hi) over n points under the plan of window c (tables: on window tables).  f = {kc_d, kc,
// two_n_d, two_n, n_entries, nb, mean, logG, bin_split, radix, pairs, hb, hb_stride, nbmax, Hn, V, sortB, pps, chunk, per_block,
// part_len, part_grid, parts_extra, slots_bound, L_log, fold, K, bits}; ab, fb: 16 entries each.  Returns 1, 0 if make_plan refuses the
// window, -1 if sort_geometry refuses the group: f[0] = its error code, msg = its text.
int gs_sort_geometry(int curve, int n_cu, uint64_t n, int c, int no_glv, int k_lo, int k_hi, int tables, int chunk_rows_log,
                     uint64_t* f, uint8_t* ab, uint8_t* fb, char* msg, int msg_cap) {
  Call cl(curve, n_cu, 0, n, c, no_glv);
  if (!cl.ok) return 0;
  cl.pl.tables = tables != 0;
  cl.ctx.chunk_rows_log = chunk_rows_log;
  try {
    const SortGeometry g = sort_geometry(&cl.ctx, n, cl.pl, k_lo, k_hi);
    const uint64_t v[28] = {(uint64_t)g.kc_d, (uint64_t)g.kc, g.two_n_d, g.two_n, g.n_entries, g.nb, g.mean, g.logG, g.bin_split, g.radix,
                            g.pairs, g.hb, g.hb_stride, g.nbmax, g.Hn, g.V, g.sortB, g.pps, g.chunk, g.per_block, g.part_len,
                            g.part_grid, g.parts_extra, g.slots_bound, (uint64_t)cl.pl.L_log, cl.pl.fold, (uint64_t)cl.pl.K, (uint64_t)cl.pl.bits};
    memcpy(f, v, sizeof v);
    memcpy(ab, g.ws.ab, 16);
    memcpy(fb, g.ws.fb, 16);
    return 1;
  } catch (const MsmFail& e) {
    f[0] = (uint64_t)e.code;
    snprintf(msg, (size_t)msg_cap, "%s", e.msg.c_str());
    return -1;
  }
}

}  // extern "C"
