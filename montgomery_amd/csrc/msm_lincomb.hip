// msm_points_lincomb: D[i] = a * A[a_lo + i] + b * B[b_lo + i] over resident rows, written as the rows [0, count) of a point set --
// the one entry point that PRODUCES resident points from resident points (the generator fold of an inner-product argument,
// scaling, element-wise sums, negation).  The host recodes (a, b) into a program once (points_lincomb.h), copies it to the
// device and launches one lane per output point; a copy (a = 1, no second term) moves rows without a kernel.
// The checks of the sets and their rows are those of operator_checks.h, the scalars are read by scalar_host.h.
// Every check runs before anything is written; msm_pointset_size reports what a set holds.
// lincomb_launch runs the same kernel over rows of another translation unit's (the two-point transform of msm_points_ntt.hip on
// the Edwards curve).
#include "operator_checks.h"
#include "points_lincomb.h"
#include "scalar_host.h"

using namespace msm;
using namespace msmi;

namespace {

const char* const WHO = "msm_points_lincomb";

void make_program(const msm_ctx* ctx, lincomb::Program& P, const uint32_t* a, const uint32_t* b) {
  if (ctx->is_te()) {
    lincomb::make_program_te(P, a, b);
    return;
  }
  for_weierstrass_curve(ctx->curve, [&](auto cv) { lincomb::make_program<typename decltype(cv)::G>(P, a, b); });
}

// where program `slot` (0, 1) lives: behind 256 bytes of ctx->misc (the index check's word lives there)
constexpr size_t PROG_BYTES = lincomb::MAX_OPS;   // four ops to a word
constexpr size_t ROWS_AT = 256 + 2 * PROG_BYTES;

// the program of P on the device and one lane per output row
void launch_program(msm_ctx* ctx, const lincomb::Program& P, uint32_t* out, const uint32_t* rows_a, const uint32_t* rows_b, uint64_t count, int slot) {
  uint32_t words[lincomb::MAX_OPS / 4] = {0};
  for (int k = 0; k < P.n; k++) words[k >> 2] |= (uint32_t)P.ops[k] << (8 * (k & 3));
  ctx->ensure(ctx->misc, 256 + (slot + 1) * PROG_BYTES);
  uint32_t* d_prog = (uint32_t*)((char*)ctx->misc.p + 256 + slot * PROG_BYTES);
  HIPCHK(hipMemcpyAsync(d_prog, words, sizeof words, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // (`words` ends with this frame)
  const dim3 grid((uint32_t)((count + 255) / 256)), block(256);
  if (ctx->is_te())
    hipLaunchKernelGGL(lincomb::k_te_points_lincomb, grid, block, 0, ctx->stream, out, rows_a, rows_b, count, d_prog, (uint32_t)P.n);
  else
    W_LAUNCH(ctx, lincomb::k_points_lincomb, grid, block, 0, ctx->stream, out, rows_a, rows_b, count, d_prog, (uint32_t)P.n);
  HIPCHK(hipGetLastError());
}

}  // namespace

namespace msmi {

uint32_t* lincomb_scratch_rows(msm_ctx* ctx, uint64_t n_rows) {
  ctx->ensure(ctx->misc, ROWS_AT + n_rows * ctx->row_words() * 4);
  return (uint32_t*)((char*)ctx->misc.p + ROWS_AT);
}

void lincomb_launch(msm_ctx* ctx, uint32_t* out, const uint32_t* rows_a, const uint32_t* rows_b, uint64_t count, const uint32_t* a,
                    const uint32_t* b, int slot) {
  lincomb::Program P;
  make_program(ctx, P, a, b);
  launch_program(ctx, P, out, rows_a, rows_b, count, slot);
}

}  // namespace msmi

extern "C" {

int msm_pointset_size(const msm_ctx* ctx, int32_t id, uint64_t* n_out) {
  msm_ctx* c = const_cast<msm_ctx*>(ctx);
  if (!ctx || !n_out) return fail(c, MSM_ERR_ARG, "msm_pointset_size: null argument");
  if (int rc = live_set_ok(c, "msm_pointset_size", id)) return rc;
  *n_out = ctx->sets[id].n;
  return MSM_OK;
}

int msm_points_lincomb(msm_ctx* ctx, int32_t src_a, uint64_t a_lo, const uint8_t* a, int32_t src_b, uint64_t b_lo, const uint8_t* b,
                       uint64_t count, int32_t dst) {
  if (!ctx || !a || (src_b >= 0 && !b)) return fail(ctx, MSM_ERR_ARG, "%s: null argument", WHO);
  if (int rc = vectors_ok(ctx, WHO, count, {}, "count")) return rc;
  for (int32_t id : {src_a, dst})
    if (int rc = live_set_ok(ctx, WHO, id)) return rc;
  if (src_b >= 0)
    if (int rc = live_set_ok(ctx, WHO, src_b)) return rc;
  uint32_t aw[8], bw[8] = {0};
  try {
    const auto scalars_below_q = [&](auto f) -> int {
      using S = decltype(f);
      return scalar_words<S>(aw, a) && (src_b < 0 || scalar_words<S>(bw, b)) ? MSM_OK : scalar_too_big(ctx, WHO, "scalar");
    };
    if (int rc = with_scalar_field(ctx, scalars_below_q)) return rc;
    if (int rc = rows_in_set_ok(ctx, WHO, src_a, a_lo, count)) return rc;
    if (src_b >= 0)
      if (int rc = rows_in_set_ok(ctx, WHO, src_b, b_lo, count)) return rc;
    if (int rc = src_in_dst_ok(ctx, WHO, src_a, dst, a_lo, count)) return rc;
    if (int rc = src_in_dst_ok(ctx, WHO, src_b, dst, b_lo, count)) return rc;
    // a term under the scalar 0 is no term; the call is then about the other one (0 * A + b * B = b * B)
    bool has_b = src_b >= 0 && !lincomb::words8_zero(bw);
    if (has_b && lincomb::words8_zero(aw)) {
      src_a = src_b;
      a_lo = b_lo;
      memcpy(aw, bw, sizeof aw);
      has_b = false;
    }
    HIPCHK(hipSetDevice(ctx->device));
    lincomb::Program P;
    make_program(ctx, P, aw, has_b ? bw : nullptr);
    const uint64_t rw = ctx->row_words();
    msm_ctx::PointSet& D = ctx->sets[dst];
    // dst is replaced as by msm_set_points: tables dropped, room for `count` rows.  A dst that is a source keeps its buffer --
    // the checked ranges lie inside what it holds -- so the fold of a 2^26-point set allocates nothing.
    uint32_t* out = ctx->reset_points(D, count);
    if (count) {
      const uint32_t* rows_a = (const uint32_t*)ctx->sets[src_a].rows.p + a_lo * rw;
      const uint32_t* rows_b = has_b ? (const uint32_t*)ctx->sets[src_b].rows.p + b_lo * rw : rows_a;
      if (P.copy) {
        if (rows_a != out) HIPCHK(hipMemcpyAsync(out, rows_a, count * rw * 4, hipMemcpyDeviceToDevice, ctx->stream));
      } else {
        launch_program(ctx, P, out, rows_a, rows_b, count, 0);
      }
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    D.n = count;
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

}  // extern "C"
