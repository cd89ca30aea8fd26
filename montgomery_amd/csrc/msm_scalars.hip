// Resident scalar-vector operations: msm_scalars_lincomb, msm_scalars_mul, msm_scalars_inner, msm_scalars_powers over vectors of
// 32-byte scalars in device memory, mod the group order q of the context's curve, and msm_device_download.  The kernels and their
// lane bodies are in scalar_vec.h; the host puts the call's scalars into Montgomery form once (scalar_host.h: the fe_* templates run
// on the host too) and launches on ctx->stream.  The argument checks are those of operator_checks.h.  Every check runs before
// anything is written; every call returns when its result is in place.  No call touches point sets, window tables or the
// range-table candidate.
#include "operator_checks.h"
#include "scalar_host.h"

using namespace msm;
using namespace msmi;

namespace {

// the dispatch of MSM_SCALAR_FIELDS names, for every curve, the field whose modulus is the curve's group order
template <class S>
constexpr bool modulus_is(const uint32_t (&q)[8]) {
  for (int j = 0; j < 8; j++)
    if (S::PW[j] != q[j]) return false;
  return S::NL == 9 && S::NW == 8;
}
static_assert(modulus_is<Fp253>(CvBls377::G::Q), "scalar field of BLS12-377");
static_assert(modulus_is<FrEd377>(FRED_Q), "scalar field of Ed-on-BLS12-377");
static_assert(modulus_is<Fr381>(CvBls381::G::Q), "scalar field of BLS12-381");
static_assert(modulus_is<FpVesta>(CvPallas::G::Q), "scalar field of Pallas");
static_assert(modulus_is<FpGrumpkin>(CvBn254::G::Q), "scalar field of BN254");
static_assert(modulus_is<FpBn254>(CvGrumpkin::G::Q), "scalar field of Grumpkin");
static_assert(modulus_is<FpPallas>(CvVesta::G::Q), "scalar field of Vesta");

dim3 lane_grid(uint64_t n) { return dim3((uint32_t)((n + sv::BLOCK - 1) / sv::BLOCK)); }

}  // namespace

extern "C" {

int msm_device_download(msm_ctx* ctx, void* host, const void* dev_ptr, uint64_t bytes) {
  if (!ctx || !dev_ptr || (!host && bytes)) return fail(ctx, MSM_ERR_ARG, "msm_device_download: null argument");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes) {
      HIPCHK(hipMemcpyAsync(host, dev_ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_lincomb(msm_ctx* ctx, void* dst, const uint8_t* x, const void* a, const uint8_t* y, const void* b, uint64_t n) {
  const char* const who = "msm_scalars_lincomb";
  if (int rc = vectors_ok(ctx, who, n, {{dst, "dst"}, {a, "a"}, {b, "b", true}})) return rc;
  if (!x || (b && !y)) return fail(ctx, MSM_ERR_ARG, "%s: null scalar", who);
  if (int rc = dst_ranges_ok(ctx, who, dst, n * 32, {{a, "a"}, {b, "b"}})) return rc;
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      Fe<S> xm, ym;
      fe_set_zero<S>(ym);
      if (!host_scalar_mont<S>(xm, x)) return scalar_too_big(ctx, who, "x");
      if (b && !host_scalar_mont<S>(ym, y)) return scalar_too_big(ctx, who, "y");
      if (!n) return MSM_OK;
      HIPCHK(hipSetDevice(ctx->device));
      const uint32_t *pa = (const uint32_t*)a, *pb = (const uint32_t*)(b ? b : a);
      if (b)
        hipLaunchKernelGGL((sv::k_sv_lincomb<S, true>), lane_grid(n), dim3(sv::BLOCK), 0, ctx->stream, (uint32_t*)dst, pa, pb, n, xm, ym);
      else
        hipLaunchKernelGGL((sv::k_sv_lincomb<S, false>), lane_grid(n), dim3(sv::BLOCK), 0, ctx->stream, (uint32_t*)dst, pa, pb, n, xm, ym);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
      return MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_mul(msm_ctx* ctx, void* dst, const void* a, const void* b, uint64_t n) {
  const char* const who = "msm_scalars_mul";
  if (int rc = vectors_ok(ctx, who, n, {{dst, "dst"}, {a, "a"}, {b, "b"}})) return rc;
  if (int rc = dst_ranges_ok(ctx, who, dst, n * 32, {{a, "a"}, {b, "b"}})) return rc;
  if (!n) return MSM_OK;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    for_scalar_field(ctx->curve, [&](auto f) {
      using S = decltype(f);
      hipLaunchKernelGGL((sv::k_sv_mul<S>), lane_grid(n), dim3(sv::BLOCK), 0, ctx->stream, (uint32_t*)dst, (const uint32_t*)a,
                         (const uint32_t*)b, n);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_inner(msm_ctx* ctx, const void* a, const void* b, uint64_t n, uint8_t* out) {
  const char* const who = "msm_scalars_inner";
  if (int rc = vectors_ok(ctx, who, n, {{a, "a"}, {b, "b"}})) return rc;
  if (!out) return fail(ctx, MSM_ERR_ARG, "%s: null pointer out", who);
  if (!n) {
    memset(out, 0, 32);
    return MSM_OK;
  }
  try {
    HIPCHK(hipSetDevice(ctx->device));
    // behind 256 bytes of ctx->misc (the index check's word lives there): the result, then one partial per block
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(sv::INNER_MAX_BLOCKS, (n + sv::BLOCK - 1) / sv::BLOCK);
    ctx->ensure(ctx->misc, 256 + 32 + (size_t)sv::INNER_MAX_BLOCKS * 32);
    uint32_t* d_out = (uint32_t*)((char*)ctx->misc.p + 256);
    uint32_t* d_part = d_out + 8;
    for_scalar_field(ctx->curve, [&](auto f) {
      using S = decltype(f);
      hipLaunchKernelGGL((sv::k_sv_inner<S>), dim3(blocks), dim3(sv::BLOCK), 0, ctx->stream, d_part, (const uint32_t*)a, (const uint32_t*)b, n);
      hipLaunchKernelGGL((sv::k_sv_inner_finish<S>), dim3(1), dim3(sv::BLOCK), 0, ctx->stream, d_out, (const uint32_t*)d_part, blocks);
    });
    HIPCHK(hipGetLastError());
    uint8_t res[32];
    HIPCHK(hipMemcpyAsync(res, d_out, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    memcpy(out, res, 32);
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_scalars_powers(msm_ctx* ctx, void* dst, const uint8_t* s, const uint8_t* x, uint64_t n) {
  const char* const who = "msm_scalars_powers";
  if (int rc = vectors_ok(ctx, who, n, {{dst, "dst"}})) return rc;
  if (!s || !x) return fail(ctx, MSM_ERR_ARG, "%s: null scalar", who);
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      Fe<S> sp, xm;
      if (!host_scalar<S>(sp, s)) return scalar_too_big(ctx, who, "s");
      if (!host_scalar_mont<S>(xm, x)) return scalar_too_big(ctx, who, "x");
      if (!n) return MSM_OK;
      // x^(2^k) in Montgomery form for every bit an index below n can have
      const int nbits = (int)ceil_log2_u64(n);
      sv::PowTable<S> pw = {};
      fill_pow_table<S>(pw, xm, nbits);
      HIPCHK(hipSetDevice(ctx->device));
      hipLaunchKernelGGL((sv::k_sv_powers<S>), lane_grid(n), dim3(sv::BLOCK), 0, ctx->stream, (uint32_t*)dst, n, sp, pw, nbits);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
      return MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

}  // extern "C"
