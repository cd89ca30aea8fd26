// The argument checks that the operators over resident vectors and point sets share (msm_scalars.hip, msm_scan.hip, msm_ntt.hip, msm_mle.hip,
// msm_spmv.hip, msm_lincomb.hip, msm_points_mul.hip): each returns MSM_OK, or refuses the call through fail() with the entry point's name in
// front.  Plain functions that read the context and write nothing but its error text; an entry point calls them in the order in
// which its refusals are documented to win.  tests/test_scalar_host.py checks the range and row rules on the CPU.
#pragma once
#include "msm_internal.h"
#include <initializer_list>

namespace msmi {

// a vector of 32-byte scalars in device memory, by the name the refusals give it
struct Range {
  const void* p;
  const char* name;
  bool optional = false;   // may be null with n > 0 (the b of a one-term lincomb)
};

// these operators work in the memory of one device
inline int single_device_ok(msm_ctx* ctx, const char* who) {
  return ctx->children.empty() ? MSM_OK : fail(ctx, MSM_ERR_ARG, "%s: runs on single-device contexts only", who);
}

// What a call over resident vectors checks before it looks at its scalars: a single-device context, the count n (`n_name` in the
// refusal) below 2^30, then per vector a null pointer and its alignment.  joint: every null pointer is refused before any
// alignment, and a misaligned vector under that one name ("dst and a").
inline int vectors_ok(msm_ctx* ctx, const char* who, uint64_t n, std::initializer_list<Range> vecs, const char* n_name = "n",
                      const char* joint = nullptr) {
  if (!ctx) return MSM_ERR_ARG;
  if (int rc = single_device_ok(ctx, who)) return rc;
  if (n >= (1ull << 30)) return fail(ctx, MSM_ERR_ARG, "%s: %s must be < 2^30", who, n_name);
  for (const Range& v : vecs) {
    if (n && !v.p && !v.optional) return fail(ctx, MSM_ERR_ARG, "%s: null pointer %s", who, v.name);
    if (!joint && ((uintptr_t)v.p & 15)) return fail(ctx, MSM_ERR_ARG, "%s: %s must be aligned to 16 bytes", who, v.name);
  }
  for (const Range& v : vecs)
    if (joint && ((uintptr_t)v.p & 15)) return fail(ctx, MSM_ERR_ARG, "%s: %s must be aligned to 16 bytes", who, joint);
  return MSM_OK;
}

// dst against every source that is there, `bytes` each: the same range (a lane reads its inputs before its stores) or disjoint ones
inline int dst_ranges_ok(msm_ctx* ctx, const char* who, const void* dst, uint64_t bytes, std::initializer_list<Range> srcs) {
  const uintptr_t d = (uintptr_t)dst, len = (uintptr_t)bytes;
  for (const Range& v : srcs) {
    const uintptr_t s = (uintptr_t)v.p;
    if (v.p && !(d == s || d + len <= s || s + len <= d))
      return fail(ctx, MSM_ERR_ARG, "%s: dst overlaps %s in part (it may be %s itself or disjoint from it)", who, v.name, v.name);
  }
  return MSM_OK;
}

// dst (dst_bytes) against a source of another length that its lanes read at arbitrary places: disjoint, nothing else
inline int dst_disjoint_ok(msm_ctx* ctx, const char* who, const void* dst, uint64_t dst_bytes, const void* src, uint64_t src_bytes,
                           const char* name) {
  const uintptr_t d = (uintptr_t)dst, s = (uintptr_t)src;
  if (dst_bytes && src_bytes && !(d + dst_bytes <= s || s + src_bytes <= d))
    return fail(ctx, MSM_ERR_ARG, "%s: dst overlaps %s (a row reads arbitrary entries of %s: the two must be disjoint)", who, name, name);
  return MSM_OK;
}

// ---------------------------------------------------------------- point sets and their rows

inline bool live_set(const msm_ctx* ctx, int32_t id) {
  return id >= 0 && id < (int)ctx->sets.size() && (id == 0 || ctx->sets[id].live);
}

inline int live_set_ok(msm_ctx* ctx, const char* who, int32_t id) {
  return live_set(ctx, id) ? MSM_OK : fail(ctx, MSM_ERR_ARG, "%s: no point set %d", who, (int)id);
}

// the rows [lo, lo + count) of a live set are there
inline int rows_in_set_ok(msm_ctx* ctx, const char* who, int32_t set, uint64_t lo, uint64_t count) {
  if (lo + count > ctx->sets[set].n)
    return fail(ctx, MSM_ERR_NO_POINTS, "%s: rows [%llu, %llu) of set %d, which holds %llu", who, (unsigned long long)lo,
                (unsigned long long)(lo + count), (int)set, (unsigned long long)ctx->sets[set].n);
  return MSM_OK;
}

// a source range inside dst: the rows [0, count) themselves (lane i reads and writes row i only) or rows at and above `count`
inline bool rows_overlap_ok(uint64_t lo, uint64_t count) { return count == 0 || lo == 0 || lo >= count; }

inline int src_in_dst_ok(msm_ctx* ctx, const char* who, int32_t src, int32_t dst, uint64_t lo, uint64_t count) {
  if (src == dst && !rows_overlap_ok(lo, count))
    return fail(ctx, MSM_ERR_ARG, "%s: a source range inside the destination must be its rows [0, count) or start at or above row count", who);
  return MSM_OK;
}

}  // namespace msmi
