// msm_scalars_sumcheck_round, msm_scalars_bind, msm_scalars_eq: the round polynomial of a sumcheck over multilinear tables, the
// binding of one variable and the table eq(r, .) over vectors of 32-byte scalars in device memory, mod the group order q of the
// context's curve; and the two entries of the debug surface that set the round's grid and report the last shapes.  The index
// maps, the value bounds, the lane bodies and the kernels are in scalar_mle.h, the argument checks in operator_checks.h, the
// reading of the call's scalars in scalar_host.h; here are the order of the checks, the context's two buffers and the launches
// on ctx->stream.  Every check runs before anything is written, and the buffers exist before the first launch.  Every call
// returns when its result is in place.  No call touches point sets, window tables or the range-table candidate.
#include "operator_checks.h"
#include "scalar_host.h"
#include "scalar_mle.h"

using namespace msm;
using namespace msmi;

namespace {

// what all three check first: the context, one device, the table's size
int table_ok(msm_ctx* ctx, const char* who, uint32_t log2n, uint32_t lowest, const char* name) {
  if (int rc = single_device_ok(ctx, who)) return rc;
  if (log2n < lowest || log2n > (uint32_t)mle::MAX_VARS)
    return fail(ctx, MSM_ERR_ARG, "%s: %s must be %u .. %d", who, name, lowest, mle::MAX_VARS);
  return MSM_OK;
}

// the m entries of a pointer array: none null, all aligned
int entries_ok(msm_ctx* ctx, const char* who, const void* const* vecs, uint32_t m, const char* name) {
  if (!vecs) return fail(ctx, MSM_ERR_ARG, "%s: null pointer %s", who, name);
  for (uint32_t j = 0; j < m; j++) {
    if (!vecs[j]) return fail(ctx, MSM_ERR_ARG, "%s: null pointer %s[%u]", who, name, j);
    if ((uintptr_t)vecs[j] & 15) return fail(ctx, MSM_ERR_ARG, "%s: %s[%u] must be aligned to 16 bytes", who, name, j);
  }
  return MSM_OK;
}

bool disjoint(const void* p, uint64_t p_bytes, const void* s, uint64_t s_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)s;
  return a + p_bytes <= b || b + s_bytes <= a;
}

template <class S, int SHAPE, int M>
void launch_round(msm_ctx* ctx, uint32_t blocks, uint32_t* d_out, uint32_t* d_part, const void* const* vecs, uint64_t h, uint32_t var) {
  mle::RoundVecs<M> rv;
  for (int j = 0; j < M; j++) rv.a[j] = (const uint32_t*)vecs[j];
  hipLaunchKernelGGL((mle::k_mle_round<S, SHAPE, M>), dim3(blocks), dim3(mle::BLOCK), 0, ctx->stream, d_part, rv, h, var);
  hipLaunchKernelGGL((mle::k_mle_round_finish<S, SHAPE, M>), dim3(1), dim3(mle::BLOCK), 0, ctx->stream, d_out, (const uint32_t*)d_part, blocks);
}

}  // namespace

extern "C" {

int msm_scalars_sumcheck_round(msm_ctx* ctx, const void* const* vecs, uint32_t m, uint32_t log2n, uint32_t var, int shape,
                               uint8_t* evals_out) {
  const char* const who = "msm_scalars_sumcheck_round";
  if (!ctx) return MSM_ERR_ARG;
  ctx->last_mle[0] = ctx->last_mle[1] = ctx->last_mle[2] = 0;
  if (int rc = table_ok(ctx, who, log2n, 1, "log2n")) return rc;
  if (var >= log2n) return fail(ctx, MSM_ERR_ARG, "%s: var must be below log2n", who);
  if (shape != MSM_SUMCHECK_PROD && shape != MSM_SUMCHECK_R1CS)
    return fail(ctx, MSM_ERR_ARG, "%s: shape must be MSM_SUMCHECK_PROD or MSM_SUMCHECK_R1CS", who);
  if (shape == MSM_SUMCHECK_R1CS ? m != 4 : (m < 1 || m > (uint32_t)mle::MAX_VECS))
    return fail(ctx, MSM_ERR_ARG, "%s: m must be 1 .. %d for MSM_SUMCHECK_PROD and 4 for MSM_SUMCHECK_R1CS", who, mle::MAX_VECS);
  if (int rc = entries_ok(ctx, who, vecs, m, "vecs")) return rc;
  if (!evals_out) return fail(ctx, MSM_ERR_ARG, "%s: null pointer evals_out", who);
  try {
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t h = 1ull << (log2n - 1);
    const uint32_t values = (uint32_t)mle::round_values(shape, (int)m);
    const uint32_t blocks = ctx->mle_grid ? (uint32_t)ctx->mle_grid
                                          : (uint32_t)std::min<uint64_t>(mle::ROUND_MAX_BLOCKS, (h + mle::BLOCK - 1) / mle::BLOCK);
    // the results, then one partial per value and block
    ctx->ensure(ctx->mle_part, (size_t)32 * (mle::MAX_VECS + 1) * (1 + mle::ROUND_MAX_BLOCKS));
    uint32_t* const d_out = (uint32_t*)ctx->mle_part.p;
    uint32_t* const d_part = d_out + 8 * (mle::MAX_VECS + 1);
    for_scalar_field(ctx->curve, [&](auto f) {
      using S = decltype(f);
      if (shape == MSM_SUMCHECK_R1CS) launch_round<S, MSM_SUMCHECK_R1CS, 4>(ctx, blocks, d_out, d_part, vecs, h, var);
      else if (m == 1) launch_round<S, MSM_SUMCHECK_PROD, 1>(ctx, blocks, d_out, d_part, vecs, h, var);
      else if (m == 2) launch_round<S, MSM_SUMCHECK_PROD, 2>(ctx, blocks, d_out, d_part, vecs, h, var);
      else if (m == 3) launch_round<S, MSM_SUMCHECK_PROD, 3>(ctx, blocks, d_out, d_part, vecs, h, var);
      else launch_round<S, MSM_SUMCHECK_PROD, 4>(ctx, blocks, d_out, d_part, vecs, h, var);
    });
    HIPCHK(hipGetLastError());
    uint8_t res[32 * (mle::MAX_VECS + 1)];
    HIPCHK(hipMemcpyAsync(res, d_out, (size_t)32 * values, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    memcpy(evals_out, res, (size_t)32 * values);
    ctx->last_mle[0] = (int32_t)blocks;
    ctx->last_mle[1] = (int32_t)h;
    ctx->last_mle[2] = (int32_t)values;
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_bind(msm_ctx* ctx, void* const* dst, const void* const* a, uint32_t m, uint32_t log2n, uint32_t var, const uint8_t* r) {
  const char* const who = "msm_scalars_bind";
  if (!ctx) return MSM_ERR_ARG;
  if (int rc = table_ok(ctx, who, log2n, 1, "log2n")) return rc;
  if (var >= log2n) return fail(ctx, MSM_ERR_ARG, "%s: var must be below log2n", who);
  if (m < 1 || m > (uint32_t)mle::MAX_BIND) return fail(ctx, MSM_ERR_ARG, "%s: m must be 1 .. %d", who, mle::MAX_BIND);
  if (int rc = entries_ok(ctx, who, (const void* const*)dst, m, "dst")) return rc;
  if (int rc = entries_ok(ctx, who, a, m, "a")) return rc;
  if (!r) return fail(ctx, MSM_ERR_ARG, "%s: null scalar r", who);
  const uint64_t h = 1ull << (log2n - 1), dst_bytes = h * 32, src_bytes = h * 64;
  for (uint32_t j = 0; j < m; j++) {
    for (uint32_t k = 0; k < j; k++)
      if (!disjoint(dst[j], dst_bytes, dst[k], dst_bytes)) return fail(ctx, MSM_ERR_ARG, "%s: dst[%u] overlaps dst[%u]", who, j, k);
    for (uint32_t k = 0; k < m; k++) {
      if (k == j && dst[j] == a[j] && var == log2n - 1) continue;   // in place: lane i reads rows i and i + h and writes row i
      if (!disjoint(dst[j], dst_bytes, a[k], src_bytes))
        return fail(ctx, MSM_ERR_ARG, "%s: dst[%u] overlaps a[%u] (dst[j] may be a[j] itself when var is the top variable, else disjoint)",
                    who, j, k);
    }
  }
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      Fe<S> rm;
      if (!host_scalar_mont<S>(rm, r)) return scalar_too_big(ctx, who, "r");
      HIPCHK(hipSetDevice(ctx->device));
      mle::BindVecs bv = {};
      for (uint32_t j = 0; j < m; j++) {
        bv.dst[j] = (uint32_t*)dst[j];
        bv.a[j] = (const uint32_t*)a[j];
      }
      hipLaunchKernelGGL((mle::k_mle_bind<S>), dim3((uint32_t)((h + mle::BLOCK - 1) / mle::BLOCK), m), dim3(mle::BLOCK), 0, ctx->stream, bv, h,
                         var, rm);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
      return MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_eq(msm_ctx* ctx, void* dst, const uint8_t* r, uint32_t v, const uint8_t* s) {
  const char* const who = "msm_scalars_eq";
  if (!ctx) return MSM_ERR_ARG;
  ctx->last_mle[3] = -1;
  if (int rc = table_ok(ctx, who, v, 0, "v")) return rc;
  if (!dst) return fail(ctx, MSM_ERR_ARG, "%s: null pointer dst", who);
  if ((uintptr_t)dst & 15) return fail(ctx, MSM_ERR_ARG, "%s: dst must be aligned to 16 bytes", who);
  if (v && !r) return fail(ctx, MSM_ERR_ARG, "%s: null pointer r", who);
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      const uint8_t one[32] = {1};
      Fe<S> sm, unit;
      if (!host_scalar_mont<S>(sm, s ? s : one)) return scalar_too_big(ctx, who, "s");
      // the Montgomery forms of (1 - r_j, r_j)
      mle::EqFactors<S> fac = {};
      fe_set_one<S>(unit);
      for (uint32_t j = 0; j < v; j++) {
        Fe<S> rm, om;
        if (!host_scalar_mont<S>(rm, r + 32 * j)) return scalar_too_big(ctx, who, "an entry of r");
        fe_sub_p<S>(om, unit, rm);
        fe_reduce_2p<S>(om);
        for (int i = 0; i < S::NL; i++) {
          fac.l[j][0][i] = om.l[i];
          fac.l[j][1][i] = rm.l[i];
        }
      }
      HIPCHK(hipSetDevice(ctx->device));
      const uint32_t k = mle::eq_split(v);
      const uint64_t n = 1ull << v, entries = (1ull << k) + (1ull << (v - k));
      ctx->ensure(ctx->mle_tab, entries * 32);
      uint32_t* const tab = (uint32_t*)ctx->mle_tab.p;
      hipLaunchKernelGGL((mle::k_mle_eq_tables<S>), dim3((uint32_t)((entries + mle::BLOCK - 1) / mle::BLOCK)), dim3(mle::BLOCK), 0, ctx->stream,
                         tab, fac, v, k, sm);
      hipLaunchKernelGGL((mle::k_mle_eq<S>), dim3((uint32_t)((n + mle::BLOCK - 1) / mle::BLOCK)), dim3(mle::BLOCK), 0, ctx->stream,
                         (uint32_t*)dst, (const uint32_t*)tab, n, k);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
      ctx->last_mle[3] = (int32_t)k;
      return MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

int msm_test_set_sumcheck_grid(msm_ctx* ctx, int32_t blocks) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_sumcheck_grid: not on a device-list context");
  if (blocks < 0 || blocks > (int32_t)mle::ROUND_MAX_BLOCKS)
    return fail(ctx, MSM_ERR_ARG, "msm_test_set_sumcheck_grid: blocks must be 0 (default) or 1 .. %u", mle::ROUND_MAX_BLOCKS);
  ctx->mle_grid = blocks;
  return MSM_OK;
}

int msm_test_last_sumcheck(msm_ctx* ctx, int32_t* out, int cap) {
  if (!ctx || !ctx->children.empty() || cap < 0 || (cap && !out)) return -1;
  for (int i = 0; i < 4 && i < cap; i++) out[i] = ctx->last_mle[i];
  return 4;
}

}  // extern "C"
