// msm_points_ntt: the number-theoretic transform over the rows of a resident point set, D[k] = sum_j (shift omega^k)^j A[a_lo + j]
// and its inverse (points_ntt.h has the plan, the lane mapping and the butterfly lane).  The host reads omega and shift by the rules
// of msm_scalars_ntt (scalar_host.h), keeps the vector omega^j of one (log2n, omega, direction) in the context, and launches on
// ctx->stream: the bit reversal, one kernel per stage on the fixed grid of msm_points_mul -- whose per-lane table workspace it
// shares -- and, for a coset or an inverse, one pass of the msm_points_mul kernel over a powers vector.
// The Edwards curve has transforms of one and two points only (its q - 1 has two-adicity 1) and no butterfly kernel: its one
// stage is two launches of the msm_points_lincomb kernel.
// The checks of the context, the sets and their rows are those of operator_checks.h.  Every check runs before anything is written.
#include "operator_checks.h"
#define MSM_PMUL_DECLARE_TE 1   // (the two plain kernels of points_mul.h are defined in msm_points_mul.hip)
#include "points_ntt.h"
#include "scalar_host.h"

using namespace msm;
using namespace msmi;

namespace {

const char* const WHO = "msm_points_ntt";

// what a call computes once from its omega and shift
template <class S>
struct CallScalars {
  Fe<S> w;            // omega, or omega^-1 for the inverse: Montgomery form
  uint8_t key[32];    // omega as the caller would pass it
  bool scale;         // rows are multiplied by scale_s scale_x^j: before the stages (forward) or after them (inverse)
  Fe<S> scale_s;      // plain
  Fe<S> scale_x;      // Montgomery form
};

template <class S>
int read_scalars(msm_ctx* ctx, CallScalars<S>& cs, uint32_t L, const uint8_t* omega, const uint8_t* shift, bool inverse) {
  Fe<S> om, sh, one;
  fe_set_one<S>(one);
  om = sh = one;
  memset(cs.key, 0, sizeof cs.key);
  if (L >= 1) {
    uint32_t w[8];
    if (omega) {
      if (!scalar_words<S>(w, omega)) return scalar_too_big(ctx, WHO, "omega");
      m_from_words<S>(om, w);
      Fe<S> t;
      m_pow2k<S>(t, om, (int)L - 1);
      if (!m_is_minus_one<S>(t))
        return fail(ctx, MSM_ERR_ARG, "%s: omega has the wrong order: omega^(n/2) must be q - 1 (a primitive 2^%u-th root of unity)", WHO, L);
    } else {
      library_root<S>(om, L);
      m_to_words<S>(w, om);
    }
    words_to_bytes(cs.key, w);
  }
  bool shifted = false;
  if (shift) {
    uint32_t w[8];
    if (!scalar_words<S>(w, shift)) return scalar_too_big(ctx, WHO, "shift");
    uint32_t any = 0;
    for (int j = 0; j < 8; j++) any |= w[j];
    if (!any) return fail(ctx, MSM_ERR_ARG, "%s: shift must not be 0 (the inverse transform divides by it)", WHO);
    const bool is_one = w[0] == 1 && !(w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]);
    if (!is_one && L >= 1) {
      m_from_words<S>(sh, w);
      shifted = true;
    }
  }
  cs.w = om;
  cs.scale = L >= 1 && (inverse || shifted);
  cs.scale_x = sh;
  Fe<S> s = one;
  if (inverse) {
    if (L >= 1) m_inverse<S>(cs.w, om);
    if (shifted) m_inverse<S>(cs.scale_x, sh);
    m_inverse_n<S>(s, L);
  }
  uint32_t sw[8];
  m_to_words<S>(sw, s);
  fe_unpack<S>(cs.scale_s, sw);
  return MSM_OK;
}

// dst[i] = s x^i, i < count: k_sv_powers (scalar_vec.h)
template <class S>
void launch_powers(msm_ctx* ctx, uint32_t* dst, uint64_t count, const Fe<S>& s_plain, const Fe<S>& x_mont) {
  const int nbits = (int)ceil_log2_u64(count);
  sv::PowTable<S> pw = {};
  fill_pow_table<S>(pw, x_mont, nbits);
  hipLaunchKernelGGL((sv::k_sv_powers<S>), dim3((uint32_t)((count + sv::BLOCK - 1) / sv::BLOCK)), dim3(sv::BLOCK), 0, ctx->stream, dst, count, s_plain,
                     pw, nbits);
  HIPCHK(hipGetLastError());
}

// the vector w^j, j < n / 2, of (L, omega, direction): nothing is built when the context holds it already
template <class S>
void ensure_twiddles(msm_ctx* ctx, uint32_t L, const CallScalars<S>& cs, bool inverse) {
  if (ctx->pntt_tw_log2n == (int)L && ctx->pntt_tw_inverse == inverse && memcmp(ctx->pntt_tw_omega, cs.key, 32) == 0) return;
  ctx->pntt_tw_log2n = -1;
  const uint64_t half = 1ull << (L - 1);
  ctx->ensure(ctx->pntt_tw, half * 32);
  Fe<S> one_plain;
  fe_set_zero<S>(one_plain);
  one_plain.l[0] = 1;
  launch_powers<S>(ctx, (uint32_t*)ctx->pntt_tw.p, half, one_plain, cs.w);
  ctx->pntt_tw_log2n = (int)L;
  ctx->pntt_tw_inverse = inverse;
  memcpy(ctx->pntt_tw_omega, cs.key, 32);
}

// stage s >= 2 of the curves that have one (Grumpkin's q - 1 has two-adicity 1: no multiplying stage, and no kernel for it)
template <class Fn>
void for_multiplying_curve(msm_ctx* ctx, Fn&& fn) {
  for_weierstrass_curve(ctx->curve, [&](auto cv) {
    if constexpr (!std::is_same_v<decltype(cv), CvGrumpkin>) fn(cv);
    else throw MsmFail{MSM_ERR_INTERNAL, "msm_points_ntt: a multiplying stage on Grumpkin"};
  });
}

// blocks per CU of the default grid: what the multiplying stage kernel of the curve keeps resident
uint32_t blocks_per_cu(msm_ctx* ctx) {
  if (!ctx->pntt_blocks_per_cu) {
    int nb = 0;
    for_multiplying_curve(ctx, [&](auto cv) {
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pntt::k_points_ntt_stage<decltype(cv), true>, pntt::BLOCK, 0));
    });
    ctx->pntt_blocks_per_cu = std::max(nb, 1);
  }
  return (uint32_t)ctx->pntt_blocks_per_cu;
}

// blocks of the stage launches over n / 2 butterflies: one round of resident blocks, no more than the butterflies need, and no more
// than the table of the lanes may take under msm_set_workspace_limit
uint64_t stage_blocks(msm_ctx* ctx, uint64_t half) {
  const uint64_t need = (half + pntt::BLOCK - 1) / pntt::BLOCK;
  uint64_t blocks = ctx->pntt_grid ? (uint64_t)ctx->pntt_grid : std::min<uint64_t>(need, (uint64_t)ctx->n_cu * blocks_per_cu(ctx));
  const uint64_t per_block = pmul::table_bytes(false, ctx->nw(), 1);
  if (ctx->ws_limit) blocks = std::min<uint64_t>(blocks, ctx->ws_limit / per_block);
  return std::max<uint64_t>(blocks, 1);
}

// the one stage of a two-point transform on the Edwards curve: (A, B) -> (A + B, A - B) through the msm_points_lincomb kernel into
// two rows of ctx->misc, then back
void te_stage(msm_ctx* ctx, uint32_t* rows) {
  const uint64_t rw = ctx->row_words();
  uint32_t one[8] = {1}, minus_one[8];
  q_minus<FrEd377>(minus_one, 1);
  uint32_t* tmp = lincomb_scratch_rows(ctx, 2);
  lincomb_launch(ctx, tmp, rows, rows + rw, 1, one, one, 0);
  lincomb_launch(ctx, tmp + rw, rows, rows + rw, 1, one, minus_one, 1);   // (both read the rows before either result goes back)
  HIPCHK(hipMemcpyAsync(rows, tmp, 2 * rw * 4, hipMemcpyDeviceToDevice, ctx->stream));
}

template <class S>
int run(msm_ctx* ctx, int32_t src, uint64_t a_lo, uint32_t L, const uint8_t* omega, const uint8_t* shift, bool inverse, int32_t dst) {
  CallScalars<S> cs;
  if (int rc = read_scalars<S>(ctx, cs, L, omega, shift, inverse)) return rc;
  const uint64_t n = 1ull << L, half = n >> 1, rw = ctx->row_words();
  if (int rc = rows_in_set_ok(ctx, WHO, src, a_lo, n)) return rc;
  if (int rc = src_in_dst_ok(ctx, WHO, src, dst, a_lo, n)) return rc;

  // device memory, all of it before the first row is written
  HIPCHK(hipSetDevice(ctx->device));
  const bool te = ctx->is_te();
  uint64_t blocks = 0;
  if (L >= 2) {
    ensure_twiddles<S>(ctx, L, cs, inverse);
    blocks = stage_blocks(ctx, half);
    ctx->ensure(ctx->pmul_tbl, blocks * pmul::table_bytes(false, ctx->nw(), 1));
  } else if (L == 1 && !te) {
    blocks = 1;
  }
  if (cs.scale) {
    ctx->ensure(ctx->scal, n * 32);
    pmul_reserve(ctx, n);
    launch_powers<S>(ctx, (uint32_t*)ctx->scal.p, n, cs.scale_s, cs.scale_x);
  }
  if (L == 1 && te) lincomb_scratch_rows(ctx, 2);

  msm_ctx::PointSet& D = ctx->sets[dst];
  const uint32_t* a_rows = (const uint32_t*)ctx->sets[src].rows.p + a_lo * rw;   // (a dst that is the source keeps its buffer)
  uint32_t* rows = ctx->reset_points(D, n);
  const bool pre = cs.scale && !inverse, post = cs.scale && inverse;
  const dim3 row_grid((uint32_t)((n + pntt::BLOCK - 1) / pntt::BLOCK)), block(pntt::BLOCK);
  // the rows in bit-reversed order, a coset's factors shift^j on them first
  if (pre) {
    pmul_launch_var(ctx, rows, a_rows, (uint32_t)rw, (const uint32_t*)ctx->scal.p, n);
    a_rows = rows;
  }
  if (a_rows == rows) {
    if (L >= 2) hipLaunchKernelGGL(pntt::k_points_bitrev_swap, row_grid, block, 0, ctx->stream, (uint4*)rows, L, (uint32_t)rw);
  } else if (L >= 2) {
    hipLaunchKernelGGL(pntt::k_points_bitrev_gather, row_grid, block, 0, ctx->stream, (uint4*)rows, (const uint4*)a_rows, L, (uint32_t)rw);
  } else {
    HIPCHK(hipMemcpyAsync(rows, a_rows, n * rw * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }
  HIPCHK(hipGetLastError());
  // the stages
  const dim3 grid((uint32_t)blocks);
  const uint32_t* tw = (const uint32_t*)ctx->pntt_tw.p;
  uint4* tbl = (uint4*)ctx->pmul_tbl.p;
  for (uint32_t s = 1; s <= L; s++) {
    if (te) te_stage(ctx, rows);
    else if (s == 1) W_LAUNCH_MODE(ctx, pntt::k_points_ntt_stage, false, grid, block, 0, ctx->stream, rows, (const uint32_t*)nullptr, L, s, (uint4*)nullptr);
    else
      for_multiplying_curve(ctx, [&](auto cv) {
        hipLaunchKernelGGL((pntt::k_points_ntt_stage<decltype(cv), true>), grid, block, 0, ctx->stream, rows, tw, L, s, tbl);
      });
    HIPCHK(hipGetLastError());
  }
  // the inverse's factors n^-1 shift^-j
  if (post) pmul_launch_var(ctx, rows, rows, (uint32_t)rw, (const uint32_t*)ctx->scal.p, n);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  D.n = n;

  const uint64_t muls = pntt::multiplications((int)L);
  const int32_t plan[7] = {(int32_t)L, (int32_t)L, (int32_t)blocks, L >= 1 ? 1 : 0, pre, post, (int32_t)std::min<uint64_t>(muls, INT32_MAX)};
  memcpy(ctx->last_pntt, plan, sizeof plan);
  return MSM_OK;
}

}  // namespace

extern "C" {

int msm_points_ntt(msm_ctx* ctx, int32_t src, uint64_t a_lo, uint32_t log2n, const uint8_t* omega, const uint8_t* shift, int inverse,
                   int32_t dst) {
  if (!ctx) return fail(ctx, MSM_ERR_ARG, "%s: null argument", WHO);
  memset(ctx->last_pntt, 0, sizeof ctx->last_pntt);
  if (int rc = single_device_ok(ctx, WHO)) return rc;
  for (int32_t id : {src, dst})
    if (int rc = live_set_ok(ctx, WHO, id)) return rc;
  try {
    uint32_t cap = 0;
    if (int rc = msm_scalars_ntt_max_log2n(ctx, &cap)) return rc;
    if (log2n > cap) return fail(ctx, MSM_ERR_ARG, "%s: log2n = %u, but this scalar field has transforms up to 2^%u only", WHO, log2n, cap);
    return with_scalar_field(ctx, [&](auto f) -> int { return run<decltype(f)>(ctx, src, a_lo, log2n, omega, shift, inverse != 0, dst); });
  } MSM_CATCH_ALL(ctx)
}

}  // extern "C"
