// Host-side unit-test shim of the window-group schedule: msmi::group_schedule of montgomery_amd/csrc/msm_plan.hip, which this file
// is compiled together with, over a default-constructed context that has no stream and no helper thread -- only the curve, the CU
// count and the workspace budget the schedule reads (tests/test_group_schedule.py).  No GPU is touched.
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

}  // extern "C"
