// msm_scalars_ntt, msm_scalars_root_of_unity, msm_scalars_ntt_max_log2n: the resident number-theoretic transform over vectors of
// 32-byte scalars mod the group order q.  The plan, the tile geometry, the lane bodies and the kernel are in scalar_ntt.h; here
// are the host's field work (roots, orders, shift^-1 and n^-1, once per call), the twiddle cache and the launches, one per pass,
// on ctx->stream.  Every check runs before anything is written, and every device buffer a call needs exists before its first
// launch.  No call touches point sets, window tables or the range-table candidate.
#include "msm_internal.h"
#include "scalar_ntt.h"

using namespace msm;
using namespace msmi;

namespace {

// ---------------------------------------------------------------- host field work: Fe<S> in canonical Montgomery form

template <class S>
void m_mul(Fe<S>& r, const Fe<S>& a, const Fe<S>& b) {
  fe_mul<S>(r, a, b);
  fe_reduce_2p<S>(r);
}

template <class S>
void m_from_words(Fe<S>& r, const uint32_t (&w)[8]) {   // w < q
  fe_unpack<S>(r, w);
  sv::to_mont<S>(r, r);
}

template <class S>
void m_to_words(uint32_t (&w)[8], const Fe<S>& a) {
  Fe<S> one, r;
  fe_set_zero<S>(one);
  one.l[0] = 1;
  m_mul<S>(r, a, one);
  fe_pack<S>(w, r);
}

// base^e, e as 8 words
template <class S>
void m_pow(Fe<S>& r, const Fe<S>& base, const uint32_t (&e)[8]) {
  Fe<S> acc;
  fe_set_one<S>(acc);
  for (int bit = 255; bit >= 0; bit--) {
    m_mul<S>(acc, acc, acc);
    if ((e[bit / 32] >> (bit % 32)) & 1u) m_mul<S>(acc, acc, base);
  }
  r = acc;
}

// out = q - v for a small v, as words
template <class S>
void q_minus(uint32_t (&out)[8], uint32_t v) {
  uint64_t borrow = v;
  for (int j = 0; j < 8; j++) {
    const uint64_t d = (uint64_t)S::PW[j] - borrow;
    out[j] = (uint32_t)d;
    borrow = (d >> 32) & 1u;
  }
}

inline void shift_right(uint32_t (&w)[8], int k) {   // k < 32
  if (!k) return;
  for (int j = 0; j < 8; j++) w[j] = (w[j] >> k) | (j + 1 < 8 ? w[j + 1] << (32 - k) : 0u);
}

template <class S>
int two_adicity() {
  uint32_t w[8];
  q_minus<S>(w, 1);
  int s = 0;
  while (!((w[s / 32] >> (s % 32)) & 1u)) s++;
  return s;
}

template <class S>
bool m_is_minus_one(const Fe<S>& a) {
  uint32_t w[8], m1[8];
  m_to_words<S>(w, a);
  q_minus<S>(m1, 1);
  return memcmp(w, m1, sizeof w) == 0;
}

// the smallest positive quadratic non-residue: g^((q-1)/2) = -1
template <class S>
uint32_t non_residue() {
  uint32_t half[8];
  q_minus<S>(half, 1);
  shift_right(half, 1);
  for (uint32_t g = 2;; g++) {
    uint32_t w[8] = {g};
    Fe<S> gm, r;
    m_from_words<S>(gm, w);
    m_pow<S>(r, gm, half);
    if (m_is_minus_one<S>(r)) return g;
  }
}

// g^((q-1) / 2^log2n), log2n <= the two-adicity
template <class S>
void library_root(Fe<S>& r, uint32_t log2n) {
  uint32_t e[8];
  q_minus<S>(e, 1);
  for (uint32_t k = log2n; k;) {
    const int step = k > 31 ? 31 : (int)k;
    shift_right(e, step);
    k -= step;
  }
  uint32_t w[8] = {non_residue<S>()};
  Fe<S> gm;
  m_from_words<S>(gm, w);
  m_pow<S>(r, gm, e);
}

template <class S>
void m_inverse(Fe<S>& r, const Fe<S>& a) {   // a != 0
  uint32_t e[8];
  q_minus<S>(e, 2);
  m_pow<S>(r, a, e);
}

// 2^-log2n
template <class S>
void m_inverse_n(Fe<S>& r, uint32_t log2n) {
  uint32_t w[8];
  uint64_t c = 1;   // (q + 1) / 2
  for (int j = 0; j < 8; j++) {
    c += S::PW[j];
    w[j] = (uint32_t)c;
    c >>= 32;
  }
  shift_right(w, 1);
  Fe<S> half;
  m_from_words<S>(half, w);
  fe_set_one<S>(r);
  for (uint32_t k = 0; k < log2n; k++) m_mul<S>(r, r, half);
}

// 32 bytes little-endian below q -> words; false: >= q
template <class S>
bool scalar_words(uint32_t (&w)[8], const uint8_t* bytes) {
  for (int j = 0; j < 8; j++)
    w[j] = (uint32_t)bytes[4 * j] | ((uint32_t)bytes[4 * j + 1] << 8) | ((uint32_t)bytes[4 * j + 2] << 16) | ((uint32_t)bytes[4 * j + 3] << 24);
  for (int j = 7; j >= 0; j--) {
    if (w[j] < S::PW[j]) return true;
    if (w[j] > S::PW[j]) return false;
  }
  return false;
}

void words_to_bytes(uint8_t* out, const uint32_t (&w)[8]) {
  for (int j = 0; j < 8; j++)
    for (int b = 0; b < 4; b++) out[4 * j + b] = (uint8_t)(w[j] >> (8 * b));
}

template <class S>
uint32_t max_log2n() { return (uint32_t)std::min(two_adicity<S>(), ntt::MAX_LOG2N); }

// ---------------------------------------------------------------- tables

// dst[i] = the Montgomery form of s x^i, i < count (a power of two): k_sv_powers from s R
template <class S>
void launch_powers(msm_ctx* ctx, uint32_t* dst, uint32_t count, const Fe<S>& s_mont, Fe<S> x_mont) {
  const int nbits = (int)ceil_log2_u64(count);
  sv::PowTable<S> pw = {};
  for (int k = 0; k < nbits; k++) {
    for (int j = 0; j < S::NL; j++) pw.l[k][j] = x_mont.l[j];
    m_mul<S>(x_mont, x_mont, x_mont);
  }
  hipLaunchKernelGGL((sv::k_sv_powers<S>), dim3((count + sv::BLOCK - 1) / sv::BLOCK), dim3(sv::BLOCK), 0, ctx->stream, dst, (uint64_t)count,
                     s_mont, pw, nbits);
  HIPCHK(hipGetLastError());
}

template <class S>
void m_pow2k(Fe<S>& r, const Fe<S>& a, int k) {   // a^(2^k)
  r = a;
  for (int i = 0; i < k; i++) m_mul<S>(r, r, r);
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

bool ranges_ok(const void* dst, const void* src, uint64_t bytes) {
  const uintptr_t d = (uintptr_t)dst, s = (uintptr_t)src;
  return d == s || d + bytes <= s || s + bytes <= d;
}

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
      if (!scalar_words<S>(w, omega)) return fail(ctx, MSM_ERR_SCALAR, "%s: omega >= q (scalars of this call are never reduced)", who);
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
    if (!scalar_words<S>(w, shift)) return fail(ctx, MSM_ERR_SCALAR, "%s: shift >= q (scalars of this call are never reduced)", who);
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
    int rc = MSM_OK;
    for_scalar_field(ctx->curve, [&](auto f) {
      using S = decltype(f);
      if (log2n > (uint32_t)two_adicity<S>()) { rc = MSM_ERR_ARG; return; }
      Fe<S> r;
      uint32_t w[8];
      library_root<S>(r, log2n);
      m_to_words<S>(w, r);
      words_to_bytes(out, w);
    });
    return rc;
  } catch (...) {
    return MSM_ERR_INTERNAL;
  }
}

int msm_scalars_ntt(msm_ctx* ctx, void* dst, const void* a, uint32_t log2n, uint32_t B, const uint8_t* omega, const uint8_t* shift,
                    int inverse) {
  const char* const who = "msm_scalars_ntt";
  if (!ctx) return MSM_ERR_ARG;
  ctx->last_ntt_plan.clear();
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "%s: runs on single-device contexts only", who);
  try {
    int rc = MSM_OK;
    for_scalar_field(ctx->curve, [&](auto f) {
      using S = decltype(f);
      const uint32_t cap = max_log2n<S>();
      if (log2n > cap) {
        rc = fail(ctx, MSM_ERR_ARG, "%s: log2n = %u, but this scalar field has transforms up to 2^%u only", who, log2n, cap);
        return;
      }
      if (B == 0) { rc = fail(ctx, MSM_ERR_ARG, "%s: B must be at least 1", who); return; }
      const uint64_t total = (uint64_t)B << log2n;
      if (total >= (1ull << 30)) { rc = fail(ctx, MSM_ERR_ARG, "%s: B n must be < 2^30", who); return; }
      if (!dst || !a) { rc = fail(ctx, MSM_ERR_ARG, "%s: null pointer %s", who, dst ? "a" : "dst"); return; }
      if (((uintptr_t)dst | (uintptr_t)a) & 15) { rc = fail(ctx, MSM_ERR_ARG, "%s: dst and a must be aligned to 16 bytes", who); return; }
      if (!ranges_ok(dst, a, total * 32)) {
        rc = fail(ctx, MSM_ERR_ARG, "%s: dst overlaps a in part (it may be a itself or disjoint from it)", who);
        return;
      }
      rc = run_ntt<S>(ctx, who, dst, a, log2n, B, omega, shift, inverse != 0);
    });
    return rc;
  } MSM_CATCH_ALL(ctx)
}

}  // extern "C"
