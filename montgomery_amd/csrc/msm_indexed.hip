// msm_run_indexed, msm_run_indexed_narrow: out = sum_j scalars[j] * P[indices[j]] over a chosen multiset of the resident points
// -- a sparse witness column, lookup multiplicities -- without the dense vector of mostly zeros the other entry points need.
// The sort moves 4-byte payloads, not points, and round 1 of the tree gathers its operands from the resident rows BY payload
// (batch_add.h ba_locate<MODE_GATHER>, te_kernels.h load_row), so digits, sort and pairing run unchanged over the m positions
// of the call -- the window is picked for m -- and one pass rewrites the payloads from positions to resident entries before
// round 1 reads them (k_index_payloads, launched by run_window_group).  Everything after round 1 is index-free already.
// The indices are checked on the GPU before any of this (k_index_check): no row outside the table is ever read.
// Always the plain path over table 0: window tables are neither built, used nor dropped.  The reference has no counterpart.
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace {

constexpr unsigned long long IDX_ALL_GOOD = ~0ull;

// *bad = min over the positions j with idx[j] >= n_resident of (j << 32 | idx[j]) -- the smallest bad position and its value;
// untouched (IDX_ALL_GOOD from the host) when every index is in range.  One streaming pass, 16 bytes per lane; a wave-level
// minimum and one atomic per wave that saw a bad index (the 64-bit minimum of `report`, points_ingest.h).
__global__ void __launch_bounds__(256) k_index_check(const uint32_t* idx, uint64_t m, uint32_t n_resident, unsigned long long* bad) {
  const uint64_t T = (uint64_t)gridDim.x * blockDim.x, t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long worst = IDX_ALL_GOOD;
  auto look = [&](uint64_t j, uint32_t v) {
    if (v >= n_resident) worst = min(worst, ((unsigned long long)j << 32) | v);
  };
  // the array may start on any 4-byte boundary: positions up to the first 16-byte boundary and behind the last one go one by one
  const uint64_t head = min(m, (uint64_t)((16u - (uint32_t)((uintptr_t)idx & 15u)) & 15u) / 4);
  const uint64_t quads = (m - head) / 4;
  const uint4* q4 = reinterpret_cast<const uint4*>(idx + head);
  for (uint64_t g = t0; g < quads; g += T) {
    const uint4 v = q4[g];
    const uint64_t j = head + 4 * g;
    look(j, v.x); look(j + 1, v.y); look(j + 2, v.z); look(j + 3, v.w);
  }
  if (t0 < head) look(t0, idx[t0]);
  const uint64_t tail = head + 4 * quads;
  if (tail + t0 < m) look(tail + t0, idx[tail + t0]);   // (fewer than 4 positions: the first lanes of the grid)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)worst, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(worst >> 32), d, 64);
    worst = min(worst, ((unsigned long long)hi << 32) | lo);
  }
  if ((threadIdx.x & 63u) == 0 && worst != IDX_ALL_GOOD) atomicMin(bad, worst);
}

// payload (entry << 1) | sign with entry = (position << SH) | half  ->  the same with idx[position] for the position
// (SH = 1: Weierstrass rows, two entries per point; SH = 0: Edwards rows, one).  The absent marker stays.
template <int SH>
__device__ __forceinline__ uint32_t index_payload(uint32_t p, const uint32_t* idx) {
  constexpr uint32_t LOW = (2u << SH) - 1u;
  // an absent slot reads idx[0] (valid memory: m >= 1) and ignores it: no divergent load
  const uint32_t pos = p == 0xFFFFFFFFu ? 0u : p >> (SH + 1);
  const uint32_t r = (idx[pos] << (SH + 1)) | (p & LOW);
  return p == 0xFFFFFFFFu ? p : r;
}

// slots[0 .. n_slots): 16 bytes per lane read and written in place (the array is a device allocation of its own: aligned), one
// scattered 4-byte read of idx per payload -- next to the 128-byte row gather per payload of the round that follows.
template <int SH>
__global__ void __launch_bounds__(256) k_index_payloads(uint32_t* slots, uint64_t n_slots, const uint32_t* idx) {
  const uint64_t T = (uint64_t)gridDim.x * blockDim.x, t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t quads = n_slots / 4;
  uint4* s4 = reinterpret_cast<uint4*>(slots);
  for (uint64_t g = t0; g < quads; g += T) {
    uint4 v = s4[g];
    v.x = index_payload<SH>(v.x, idx);
    v.y = index_payload<SH>(v.y, idx);
    v.z = index_payload<SH>(v.z, idx);
    v.w = index_payload<SH>(v.w, idx);
    s4[g] = v;
  }
  const uint64_t tail = 4 * quads + t0;   // (fewer than 4 slots)
  if (tail < n_slots) slots[tail] = index_payload<SH>(slots[tail], idx);
}

uint32_t stream_grid(const msm_ctx* ctx, uint64_t items_per_lane_total) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items_per_lane_total + 255) / 256, (uint64_t)ctx->n_cu * 8));
}

// what both entry points refuse (the narrow form adds narrow_format's checks)
int indexed_args_ok(msm_ctx* ctx, const void* scalars, const uint32_t* indices, uint64_t m, int on_device, const msm_opts* opts,
                    msm_result* out, const char* who) {
  if (!ctx || !out || ((!scalars || !indices) && m)) return fail(ctx, MSM_ERR_ARG, "%s: null argument", who);
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "%s: indexed calls run on single-device contexts only", who);
  if (int rc = refuse_shard_opts(ctx, opts, who, "an indexed", /*no_point_lo=*/true)) return rc;
  if (m >= (1ull << 30)) return fail(ctx, MSM_ERR_ARG, "%s: m must be < 2^30", who);
  if (on_device && m && (uintptr_t)indices % 4) return fail(ctx, MSM_ERR_ARG, "%s: device indices must be aligned to 4 bytes", who);
  return MSM_OK;
}

// (m may exceed the resident count, so check_points does not apply: any resident point will do)
int has_points(msm_ctx* ctx, const char* who) {
  return ctx->pts().n ? MSM_OK : fail(ctx, MSM_ERR_NO_POINTS, "%s: no resident points", who);
}

// Indices (and host scalars) into HBM, the index check, and its read-back -- the one synchronisation in front of the run, which
// host input needs anyway.  Returns the device arrays; throws MSM_ERR_ARG naming the smallest bad position.
void stage_indexed(msm_ctx* ctx, const void* scalars, const uint32_t* indices, uint64_t m, int on_device, size_t scalar_bytes,
                   const char* who, const char** d_scal, const uint32_t** d_idx, float* up_ms) {
  constexpr size_t IDX_OFF = 256;   // ctx->misc: the word of the check, then the indices of a host call
  HIPCHK(hipEventRecord(ctx->ev[11], ctx->stream));
  ctx->ensure(ctx->misc, IDX_OFF + (on_device ? 0 : (size_t)m * 4));
  *d_scal = (const char*)scalars;
  *d_idx = indices;
  if (!on_device) {
    ctx->ensure(ctx->scal, scalar_bytes + 16);
    upload_staged(ctx, ctx->scal.p, scalars, scalar_bytes);
    upload_staged(ctx, (char*)ctx->misc.p + IDX_OFF, indices, (size_t)m * 4);
    *d_scal = (const char*)ctx->scal.p;
    *d_idx = (const uint32_t*)((const char*)ctx->misc.p + IDX_OFF);
  }
  unsigned long long* d_bad = (unsigned long long*)ctx->misc.p;
  HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
  hipLaunchKernelGGL(k_index_check, dim3(stream_grid(ctx, (m + 3) / 4)), dim3(256), 0, ctx->stream, *d_idx, m,
                     (uint32_t)ctx->pts().n, d_bad);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ctx->h_info, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[10], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipEventElapsedTime(up_ms, ctx->ev[11], ctx->ev[10]));
  const unsigned long long bad = (unsigned long long)ctx->h_info[0] | ((unsigned long long)ctx->h_info[1] << 32);
  if (bad != IDX_ALL_GOOD) {
    char msg[192];
    snprintf(msg, sizeof msg, "%s: indices[%llu] = %llu but %llu resident points", who, bad >> 32, bad & 0xFFFFFFFFull,
             (unsigned long long)ctx->pts().n);
    throw MsmFail{MSM_ERR_ARG, msg};
  }
}

// the run itself over staged input, from the plan to the affine result
void run_indexed(msm_ctx* ctx, const void* d_scal, uint64_t m, const msm_opts* opts, const Plan& pl, float up_ms, msm_result* out) {
  std::vector<uint32_t> words;
  window_sums_impl(ctx, d_scal, m, 1, opts, 0, pl.K, pl, words, out, 0);
  call_finish(ctx, words, pl, out, up_ms);   // (up_ms: indices and host scalars into HBM, and the index check)
}

}  // namespace

namespace msmi {

void translate_payloads(hipStream_t s, const msm_ctx* ctx, uint32_t* slots, uint64_t n_slots, const uint32_t* idx) {
  if (!n_slots) return;
  const uint32_t grid = stream_grid(ctx, (n_slots + 3) / 4);
  if (ctx->is_te()) hipLaunchKernelGGL(k_index_payloads<0>, dim3(grid), dim3(256), 0, s, slots, n_slots, idx);
  else hipLaunchKernelGGL(k_index_payloads<1>, dim3(grid), dim3(256), 0, s, slots, n_slots, idx);
  HIPCHK(hipGetLastError());
}

}  // namespace msmi

extern "C" {

int msm_run_indexed(msm_ctx* ctx, const void* scalars, const uint32_t* indices, uint64_t m, int on_device, const msm_opts* opts,
                    msm_result* out) {
  const char* who = "msm_run_indexed";
  if (int rc = indexed_args_ok(ctx, scalars, indices, m, on_device, opts, out, who)) return rc;
  if (int rc = has_points(ctx, who)) return rc;
  Plan pl;
  if (make_plan(ctx, m, opts, pl)) return fail(ctx, MSM_ERR_ARG, "%s: bad window size", who);
  if (!call_begin(ctx, pl, m, out)) return MSM_OK;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    const char* d_scal = nullptr;
    float up_ms = 0;
    stage_indexed(ctx, scalars, indices, m, on_device, (size_t)m * 32, who, &d_scal, &pl.idx, &up_ms);
    run_indexed(ctx, d_scal, m, opts, pl, up_ms, out);
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_run_indexed_narrow(msm_ctx* ctx, const void* scalars, const uint32_t* indices, uint64_t m, int on_device, int32_t width_bytes,
                           int32_t bits, int32_t is_signed, const msm_opts* opts, msm_result* out) {
  const char* who = "msm_run_indexed_narrow";
  if (int rc = indexed_args_ok(ctx, scalars, indices, m, on_device, opts, out, who)) return rc;
  Plan pl;
  Plan::Narrow nar;
  if (int rc = narrow_format(ctx, width_bytes, bits, is_signed, opts, who, nar)) return rc;
  if (int rc = narrow_scalars_ok(ctx, scalars, m, on_device, width_bytes, who)) return rc;
  if (int rc = has_points(ctx, who)) return rc;
  if (make_plan(ctx, m, opts, pl, false, nar.fmt.bits)) return fail(ctx, MSM_ERR_ARG, "%s: bad window size", who);
  if (!call_begin(ctx, pl, m, out)) return MSM_OK;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    const char* dev = nullptr;
    float up_ms = 0;
    stage_indexed(ctx, scalars, indices, m, on_device, (size_t)m * width_bytes, who, &dev, &pl.idx, &up_ms);
    dev = narrow_lane_base(dev, width_bytes, nar);   // as msm_run_narrow
    pl.nar = nar;
    run_indexed(ctx, dev, m, opts, pl, up_ms, out);
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

}  // extern "C"
