// msm_scalars_ntt, msm_scalars_root_of_unity, msm_scalars_ntt_max_log2n: the resident number-theoretic transform over vectors of
// 32-byte scalars mod the group order q.  The plan, the tile geometry, the lane bodies and the kernel are in scalar_ntt.h, the
// host's field arithmetic (roots, orders, inverses, power tables) in scalar_host.h, the argument checks in operator_checks.h; here
// are what a call computes with them once (omega and its order, shift^-1, n^-1), the twiddle cache and the launches, one per pass,
// on ctx->stream.  Every check runs before anything is written, and every device buffer a call needs exists before its first
// launch.  No call touches point sets, window tables or the range-table candidate.
#include "operator_checks.h"
#include "scalar_host.h"
#include "scalar_ntt.h"

using namespace msm;
using namespace msmi;

namespace {

template <class S>
uint32_t max_log2n() { return (uint32_t)std::min(two_adicity<S>(), ntt::MAX_LOG2N); }

// ---------------------------------------------------------------- tables

// dst[i] = the Montgomery form of s x^i, i < count (a power of two): k_sv_powers from s R
template <class S>
void launch_powers(msm_ctx* ctx, uint32_t* dst, uint32_t count, const Fe<S>& s_mont, const Fe<S>& x_mont) {
  const int nbits = (int)ceil_log2_u64(count);
  sv::PowTable<S> pw = {};
  fill_pow_table<S>(pw, x_mont, nbits);
  hipLaunchKernelGGL((sv::k_sv_powers<S>), dim3((count + sv::BLOCK - 1) / sv::BLOCK), dim3(sv::BLOCK), 0, ctx->stream, dst, (uint64_t)count,
                     s_mont, pw, nbits);
  HIPCHK(hipGetLastError());
}

// entries of one direction's twiddle tables, and of a scale table
struct TableSizes {
  uint32_t lo, hi, g;
  explicit TableSizes(int L) {
    const int h = ntt::table_low_bits(L), gl = L < ntt::LDS_LOG ? L : ntt::LDS_LOG;
    lo = 1u << h;
    hi = 1u << (L - h);
    g = gl ? 1u << (gl - 1) : 1u;
  }
  size_t twiddle_words() const { return 8 * ((size_t)lo + hi + g); }
  size_t scale_words() const { return 8 * ((size_t)lo + hi); }
};

// [lo | hi] of x at dst: s x^e, e < 2^h; x^(e 2^h), e < 2^(L-h)
template <class S>
void build_two_level(msm_ctx* ctx, uint32_t* dst, int L, const Fe<S>& s_mont, const Fe<S>& x_mont) {
  const TableSizes sz(L);
  Fe<S> one, xh;
  fe_set_one<S>(one);
  launch_powers<S>(ctx, dst, sz.lo, s_mont, x_mont);
  m_pow2k<S>(xh, x_mont, ntt::table_low_bits(L));
  launch_powers<S>(ctx, dst + 8 * (size_t)sz.lo, sz.hi, one, xh);
}

// the twiddle cache: the tables of (L, omega), both directions; nothing is built when the context holds them already
template <class S>
void ensure_twiddles(msm_ctx* ctx, int L, const Fe<S>& om, const uint8_t (&key)[32]) {
  const TableSizes sz(L);
  if (ctx->ntt_tw_log2n == L && memcmp(ctx->ntt_tw_omega, key, 32) == 0) return;
  ctx->ntt_tw_log2n = -1;
  ctx->ensure(ctx->ntt_tw, 2 * sz.twiddle_words() * 4);
  Fe<S> one, omi, x;
  fe_set_one<S>(one);
  m_inverse<S>(omi, om);
  for (int dir = 0; dir < 2; dir++) {
    uint32_t* base = (uint32_t*)ctx->ntt_tw.p + dir * sz.twiddle_words();
    const Fe<S>& w = dir ? omi : om;
    build_two_level<S>(ctx, base, L, one, w);
    m_pow2k<S>(x, w, L - (L < ntt::LDS_LOG ? L : ntt::LDS_LOG));
    launch_powers<S>(ctx, base + 8 * ((size_t)sz.lo + sz.hi), sz.g, one, x);
  }
  ctx->ntt_tw_log2n = L;
  memcpy(ctx->ntt_tw_omega, key, 32);
}

// ---------------------------------------------------------------- the call

template <class S>
int run_ntt(msm_ctx* ctx, const char* who, void* dst, const void* a, uint32_t L, uint32_t B, const uint8_t* omega, const uint8_t* shift,
            bool inverse) {
  // the call's scalars
  Fe<S> om, sh, scale_c;
  fe_set_one<S>(om);
  fe_set_zero<S>(scale_c);
  uint8_t key[32] = {0};
  // (the library's root of the size the cache holds: no root is computed, the tables stand)
  const bool cached = !omega && ctx->ntt_tw_log2n == (int)L && ctx->ntt_tw_library;
  if (L >= 1 && !cached) {
    uint32_t w[8];
    if (omega) {
      if (!scalar_words<S>(w, omega)) return scalar_too_big(ctx, who, "omega");
      m_from_words<S>(om, w);
      Fe<S> t;
      m_pow2k<S>(t, om, (int)L - 1);
      if (!m_is_minus_one<S>(t))
        return fail(ctx, MSM_ERR_ARG, "%s: omega has the wrong order: omega^(n/2) must be q - 1 (a primitive 2^%u-th root of unity)", who, L);
    } else {
      library_root<S>(om, L);
      m_to_words<S>(w, om);
    }
    words_to_bytes(key, w);
  }
  int scale = ntt::SCALE_NONE;
  if (shift) {
    uint32_t w[8];
    if (!scalar_words<S>(w, shift)) return scalar_too_big(ctx, who, "shift");
    uint32_t any = 0;
    for (int j = 0; j < 8; j++) any |= w[j];
    if (!any) return fail(ctx, MSM_ERR_ARG, "%s: shift must not be 0 (the inverse transform divides by it)", who);
    const bool is_one = w[0] == 1 && (any == 1) && !(w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]);
    if (!is_one && L >= 1) {
      m_from_words<S>(sh, w);
      scale = ntt::SCALE_TABLE;
    }
  }
  Fe<S> ninv;
  m_inverse_n<S>(ninv, L);
  if (inverse && L >= 1 && scale == ntt::SCALE_NONE) {
    scale = ntt::SCALE_CONST;
    scale_c = ninv;
  }

  // device memory, all of it before the first launch
  HIPCHK(hipSetDevice(ctx->device));
  const int tile_log = ctx->ntt_tile_log ? ctx->ntt_tile_log : ntt::DEFAULT_TILE_LOG;
  const ntt::Plan plan = ntt::ntt_plan((int)L, tile_log);
  const TableSizes sz((int)L);
  const uint64_t total = (uint64_t)B << L;
  if (plan.passes >= 2) ctx->ensure(ctx->ntt_scratch, total * 32);
  if (scale == ntt::SCALE_TABLE) ctx->ensure(ctx->ntt_shift, sz.scale_words() * 4);
  if (!cached) {
    ensure_twiddles<S>(ctx, (int)L, om, key);
    ctx->ntt_tw_library = !omega;
  }

  ntt::Tables tb = {};
  const uint32_t* tw = (const uint32_t*)ctx->ntt_tw.p + (inverse ? sz.twiddle_words() : 0);
  tb.wa = tw;
  tb.wb = tw + 8 * (size_t)sz.lo;
  tb.g = tw + 8 * ((size_t)sz.lo + sz.hi);
  if (scale == ntt::SCALE_TABLE) {
    // forward: shift^j; inverse: n^-1 shift^-k.  Built per call: a shift is one scalar of the call, not a property of the domain
    Fe<S> x = sh, s;
    fe_set_one<S>(s);
    if (inverse) {
      m_inverse<S>(x, sh);
      s = ninv;
    }
    build_two_level<S>(ctx, (uint32_t*)ctx->ntt_shift.p, (int)L, s, x);
    tb.sa = (const uint32_t*)ctx->ntt_shift.p;
    tb.sb = tb.sa + 8 * (size_t)sz.lo;
  }

  const int launches = plan.passes ? plan.passes : 1;
  for (int i = 0; i < launches; i++) {
    const ntt::Pass ps = ntt::pass_geometry(plan, i, B, scale, inverse);
    const uint32_t* src = ps.first ? (const uint32_t*)a : (const uint32_t*)ctx->ntt_scratch.p;
    uint32_t* out = ps.last ? (uint32_t*)dst : (uint32_t*)ctx->ntt_scratch.p;
    hipLaunchKernelGGL((ntt::k_ntt_pass<S>), dim3((uint32_t)ntt::pass_blocks(ps)), dim3(ntt::BLOCK), 0, ctx->stream, out, src, ps, tb, scale_c);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->last_ntt_plan.assign(plan.stages, plan.stages + plan.passes);
  return MSM_OK;
}

}  // namespace

extern "C" {

int msm_scalars_ntt_max_log2n(const msm_ctx* ctx, uint32_t* out) {
  if (!ctx || !out) return MSM_ERR_ARG;
  try {
    for_scalar_field(ctx->curve, [&](auto f) { *out = max_log2n<decltype(f)>(); });
    return MSM_OK;
  } catch (...) {
    return MSM_ERR_INTERNAL;
  }
}

int msm_scalars_root_of_unity(const msm_ctx* ctx, uint32_t log2n, uint8_t* out) {
  if (!ctx || !out) return MSM_ERR_ARG;
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      if (log2n > (uint32_t)two_adicity<S>()) return MSM_ERR_ARG;
      Fe<S> r;
      uint32_t w[8];
      library_root<S>(r, log2n);
      m_to_words<S>(w, r);
      words_to_bytes(out, w);
      return MSM_OK;
    });
  } catch (...) {
    return MSM_ERR_INTERNAL;
  }
}

int msm_scalars_ntt(msm_ctx* ctx, void* dst, const void* a, uint32_t log2n, uint32_t B, const uint8_t* omega, const uint8_t* shift,
                    int inverse) {
  const char* const who = "msm_scalars_ntt";
  if (!ctx) return MSM_ERR_ARG;
  ctx->last_ntt_plan.clear();
  if (int rc = single_device_ok(ctx, who)) return rc;
  try {
    uint32_t cap = 0;
    for_scalar_field(ctx->curve, [&](auto f) { cap = max_log2n<decltype(f)>(); });
    if (log2n > cap) return fail(ctx, MSM_ERR_ARG, "%s: log2n = %u, but this scalar field has transforms up to 2^%u only", who, log2n, cap);
    if (B == 0) return fail(ctx, MSM_ERR_ARG, "%s: B must be at least 1", who);
    const uint64_t total = (uint64_t)B << log2n;
    if (int rc = vectors_ok(ctx, who, total, {{dst, "dst"}, {a, "a"}}, "B n", "dst and a")) return rc;
    if (int rc = dst_ranges_ok(ctx, who, dst, total * 32, {{a, "a"}})) return rc;
    return with_scalar_field(ctx, [&](auto f) -> int { return run_ntt<decltype(f)>(ctx, who, dst, a, log2n, B, omega, shift, inverse != 0); });
  } MSM_CATCH_ALL(ctx)
}

}  // extern "C"
