// msm_matrix_create, msm_matrix_destroy, msm_matrix_info, msm_scalars_matvec: sparse matrices in CSR that live in device memory as
// point sets do, and dst = alpha M x (+ dst) over vectors of 32-byte scalars in device memory, mod the group order q of the
// context's curve.  The CSR rule, the plan of the long rows, the host transposition, the value bounds, the lane bodies and the
// kernels are in scalar_spmv.h, the argument checks in operator_checks.h, the reading of alpha in scalar_host.h; here are the
// order of the checks, the ownership of a matrix's arrays and the launches on ctx->stream.  Validation, the conversion of the
// coefficients and the plan are paid once, at creation, as window tables are paid once per point set: a product is two or three
// launches over arrays that are known to be sound.  No index is used as an address before the whole matrix has passed the check.
// Every call returns when its result is in place.  No call touches point sets, window tables or the range-table candidate.
#include "operator_checks.h"
#include "scalar_host.h"
#include "scalar_spmv.h"

using namespace msm;
using namespace msmi;

namespace {

constexpr uint32_t CREATE_FLAGS = MSM_MATRIX_TRANSPOSE, MATVEC_FLAGS = MSM_MATVEC_ACCUMULATE;

uint32_t check_grid(const msm_ctx* ctx, uint64_t items) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + spmv::BLOCK - 1) / spmv::BLOCK, (uint64_t)ctx->n_cu * 8));
}

bool live_matrix(const msm_ctx* ctx, int32_t id) { return id > 0 && id < (int)ctx->mats.size() && ctx->mats[id].live; }

int live_matrix_ok(msm_ctx* ctx, const char* who, int32_t id) {
  return live_matrix(ctx, id) ? MSM_OK : fail(ctx, MSM_ERR_ARG, "%s: no matrix %d", who, (int)id);
}

[[noreturn]] void refuse(const spmv::CsrDefect& d, uint32_t prev, uint64_t rows, uint64_t cols, uint64_t nnz) {
  char what[160], msg[224];
  spmv::describe_defect(what, sizeof what, d, prev, rows, cols, nnz);
  snprintf(msg, sizeof msg, "msm_matrix_create: %s", what);
  throw MsmFail{MSM_ERR_ARG, msg};
}

// the word a validation kernel leaves behind -> the defect, kind 0 if there is none
spmv::CsrDefect read_defect(msm_ctx* ctx, const unsigned long long* d_bad, int kind) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ctx->h_info, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const unsigned long long bad = (unsigned long long)ctx->h_info[0] | ((unsigned long long)ctx->h_info[1] << 32);
  if (bad == spmv::ALL_GOOD) return spmv::CsrDefect{};
  return spmv::CsrDefect{kind, bad >> 32, (uint32_t)bad};
}

// Device input: row_ptr, then -- only if it passed -- col, each by a kernel that stays inside the array's stated length.  Throws the
// refusal.  The word of the check lives at the start of ctx->misc.
void check_on_device(msm_ctx* ctx, const uint32_t* row_ptr, const uint32_t* col, uint64_t rows, uint64_t cols, uint64_t nnz) {
  ctx->ensure(ctx->misc, 16);
  unsigned long long* d_bad = (unsigned long long*)ctx->misc.p;
  HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
  hipLaunchKernelGGL(spmv::k_spmv_check_row_ptr, dim3(check_grid(ctx, rows + 1)), dim3(spmv::BLOCK), 0, ctx->stream, row_ptr, rows, nnz, d_bad);
  spmv::CsrDefect d = read_defect(ctx, d_bad, 1);
  if (d.kind) {
    uint32_t prev = 0;
    if (d.pos) HIPCHK(hipMemcpy(&prev, row_ptr + d.pos - 1, 4, hipMemcpyDeviceToHost));
    refuse(d, prev, rows, cols, nnz);
  }
  if (!nnz) return;
  HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
  hipLaunchKernelGGL(spmv::k_spmv_check_col, dim3(check_grid(ctx, nnz)), dim3(spmv::BLOCK), 0, ctx->stream, col, nnz, cols, d_bad);
  d = read_defect(ctx, d_bad, 2);
  if (d.kind) refuse(d, 0, rows, cols, nnz);
}

void copy_in(msm_ctx* ctx, DevBuf& b, const void* src, size_t bytes, int on_device) {
  ctx->ensure(b, bytes);
  if (!bytes) return;
  if (on_device) {
    HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    upload_staged(ctx, b.p, src, bytes);
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the source may be a local of the creation that a refusal further down unwinds
  }
}

spmv::MatrixView view_of(const msm_ctx::Matrix& m) {
  spmv::MatrixView v;
  v.row_ptr = (const uint32_t*)m.row_ptr.p;
  v.col = (const uint32_t*)m.col.p;
  v.valm = (const uint32_t*)m.val.p;
  v.parts = (const spmv::Part*)m.parts.p;
  v.long_rows = (const uint32_t*)m.long_rows.p;
  v.long_first = (const uint32_t*)m.long_first.p;
  v.partials = (uint32_t*)m.partials.p;
  v.rows = (uint32_t)m.rows;
  v.n_parts = m.n_parts;
  v.n_long = m.n_long;
  v.short_max = m.short_max;
  return v;
}

template <class S, bool ONES>
int launch_product(msm_ctx* ctx, const spmv::MatrixView& v, uint32_t* dst, const uint32_t* x, uint32_t mode, const Fe<S>& alpham) {
  int launches = 0;
  if (v.n_parts) {
    hipLaunchKernelGGL((spmv::k_spmv_parts<S, ONES>), dim3((v.n_parts + spmv::WAVES - 1) / spmv::WAVES), dim3(spmv::BLOCK), 0, ctx->stream, v, x);
    launches++;
  }
  hipLaunchKernelGGL((spmv::k_spmv_rows<S, ONES>), dim3((v.rows + spmv::BLOCK - 1) / spmv::BLOCK), dim3(spmv::BLOCK), 0, ctx->stream, v, dst, x,
                     mode, alpham);
  launches++;
  if (v.n_long) {
    hipLaunchKernelGGL((spmv::k_spmv_long_finish<S>), dim3((v.n_long + spmv::BLOCK - 1) / spmv::BLOCK), dim3(spmv::BLOCK), 0, ctx->stream, v, dst,
                       mode, alpham);
    launches++;
  }
  return launches;
}

}  // namespace

extern "C" {

int msm_matrix_create(msm_ctx* ctx, uint64_t rows, uint64_t cols, uint64_t nnz, const uint32_t* row_ptr, const uint32_t* col,
                      const void* val, int on_device, uint32_t flags, int32_t* id_out) {
  const char* const who = "msm_matrix_create";
  if (!ctx) return MSM_ERR_ARG;
  if (int rc = single_device_ok(ctx, who)) return rc;
  if (!id_out) return fail(ctx, MSM_ERR_ARG, "%s: null pointer id_out", who);
  if (flags & ~CREATE_FLAGS) return fail(ctx, MSM_ERR_ARG, "%s: unknown flag bits 0x%x", who, flags & ~CREATE_FLAGS);
  const bool transpose = flags & MSM_MATRIX_TRANSPOSE;
  if (transpose && on_device)
    return fail(ctx, MSM_ERR_ARG, "%s: MSM_MATRIX_TRANSPOSE takes host input only (the transposition runs on the host)", who);
  if (rows >= spmv::MAX_DIM || cols >= spmv::MAX_DIM) return fail(ctx, MSM_ERR_ARG, "%s: rows and cols must be < 2^30", who);
  if (nnz >= spmv::MAX_NNZ) return fail(ctx, MSM_ERR_ARG, "%s: nnz must be < 2^31", who);
  if (!row_ptr) return fail(ctx, MSM_ERR_ARG, "%s: null pointer row_ptr", who);
  if (nnz && !col) return fail(ctx, MSM_ERR_ARG, "%s: null pointer col", who);
  if (on_device && (((uintptr_t)row_ptr | (uintptr_t)col) & 3)) return fail(ctx, MSM_ERR_ARG, "%s: device row_ptr and col must be aligned to 4 bytes", who);
  if (on_device && ((uintptr_t)val & 15)) return fail(ctx, MSM_ERR_ARG, "%s: device val must be aligned to 16 bytes", who);
  try {
    HIPCHK(hipSetDevice(ctx->device));
    msm_ctx::Matrix m;   // under construction: what it holds is freed unless the creation reaches its end
    m.ones = val == nullptr;
    const uint32_t short_max = ctx->spmv_short_max ? ctx->spmv_short_max : spmv::DEFAULT_SHORT_MAX;
    const uint32_t part_len = ctx->spmv_part_len ? ctx->spmv_part_len : spmv::DEFAULT_PART_LEN;
    // the arrays as the matrix will hold them; host_rp: row_ptr on the host, which the plan reads
    std::vector<uint32_t> t_rp, t_col, t_val, dl_rp;
    const uint32_t* host_rp = row_ptr;
    const void* src_val = val;
    if (on_device) {
      check_on_device(ctx, row_ptr, col, rows, cols, nnz);
      dl_rp.resize(rows + 1);
      HIPCHK(hipMemcpy(dl_rp.data(), row_ptr, (rows + 1) * 4, hipMemcpyDeviceToHost));
      host_rp = dl_rp.data();
    } else {
      const spmv::CsrDefect d = spmv::check_csr(row_ptr, col, rows, cols, nnz);
      if (d.kind) refuse(d, d.kind == 1 && d.pos ? row_ptr[d.pos - 1] : 0u, rows, cols, nnz);
      if (transpose) {
        t_rp.resize(cols + 1);
        t_col.resize(nnz);
        if (val) t_val.resize(nnz * 8);
        spmv::transpose_csr(rows, cols, nnz, row_ptr, col, (const uint32_t*)val, t_rp.data(), t_col.data(), val ? t_val.data() : nullptr);
        std::swap(rows, cols);
        host_rp = row_ptr = t_rp.data();
        col = t_col.data();
        if (val) src_val = t_val.data();
      }
    }
    const spmv::Plan pl = spmv::make_plan(host_rp, rows, short_max, part_len);
    m.rows = rows;
    m.cols = cols;
    m.nnz = nnz;
    m.short_max = short_max;
    m.part_len = part_len;
    m.n_long = (uint32_t)pl.long_rows.size();
    m.n_parts = (uint32_t)pl.parts.size();
    copy_in(ctx, m.row_ptr, row_ptr, (rows + 1) * 4, on_device);
    copy_in(ctx, m.col, col, nnz * 4, on_device);
    if (m.n_long) {
      copy_in(ctx, m.parts, pl.parts.data(), pl.parts.size() * sizeof(spmv::Part), 0);
      copy_in(ctx, m.long_rows, pl.long_rows.data(), pl.long_rows.size() * 4, 0);
      copy_in(ctx, m.long_first, pl.long_first.data(), pl.long_first.size() * 4, 0);
      ctx->ensure(m.partials, (size_t)m.n_parts * 32);
    }
    if (!m.ones && nnz) {
      // host coefficients are uploaded into the matrix's own array and converted in place; device ones are converted on the way in
      const uint32_t* from = (const uint32_t*)src_val;
      if (!on_device) {
        copy_in(ctx, m.val, src_val, nnz * 32, 0);
        from = (const uint32_t*)m.val.p;
      } else {
        ctx->ensure(m.val, nnz * 32);
      }
      for_scalar_field(ctx->curve, [&](auto f) {
        using S = decltype(f);
        hipLaunchKernelGGL((spmv::k_spmv_values<S>), dim3((uint32_t)((nnz + spmv::BLOCK - 1) / spmv::BLOCK)), dim3(spmv::BLOCK), 0, ctx->stream,
                           (uint32_t*)m.val.p, from, nnz);
      });
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the caller's buffers, and the host copies above, are free from here on
    int id = -1;
    for (size_t i = 1; i < ctx->mats.size(); i++)
      if (!ctx->mats[i].live) { id = (int)i; break; }
    if (id < 0) { ctx->mats.emplace_back(); id = (int)ctx->mats.size() - 1; }
    m.live = true;
    ctx->mats[id] = std::move(m);
    *id_out = id;
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_matrix_destroy(msm_ctx* ctx, int32_t id) {
  const char* const who = "msm_matrix_destroy";
  if (!ctx) return MSM_ERR_ARG;
  if (int rc = single_device_ok(ctx, who)) return rc;
  if (int rc = live_matrix_ok(ctx, who, id)) return rc;
  (void)hipSetDevice(ctx->device);
  ctx->mats[id].release();
  return MSM_OK;
}

int msm_matrix_info(const msm_ctx* ctx, int32_t id, uint64_t* rows_out, uint64_t* cols_out, uint64_t* nnz_out, uint64_t* bytes_out) {
  const char* const who = "msm_matrix_info";
  if (!ctx) return MSM_ERR_ARG;
  msm_ctx* c = const_cast<msm_ctx*>(ctx);   // (the error text)
  if (int rc = single_device_ok(c, who)) return rc;
  if (int rc = live_matrix_ok(c, who, id)) return rc;
  const msm_ctx::Matrix& m = ctx->mats[id];
  if (rows_out) *rows_out = m.rows;
  if (cols_out) *cols_out = m.cols;
  if (nnz_out) *nnz_out = m.nnz;
  if (bytes_out) *bytes_out = m.bytes();
  return MSM_OK;
}

int msm_scalars_matvec(msm_ctx* ctx, int32_t id, void* dst, const void* x, const uint8_t* alpha, uint32_t flags) {
  const char* const who = "msm_scalars_matvec";
  if (!ctx) return MSM_ERR_ARG;
  for (int32_t& v : ctx->last_spmv) v = 0;
  if (int rc = single_device_ok(ctx, who)) return rc;
  if (int rc = live_matrix_ok(ctx, who, id)) return rc;
  if (flags & ~MATVEC_FLAGS) return fail(ctx, MSM_ERR_ARG, "%s: unknown flag bits 0x%x", who, flags & ~MATVEC_FLAGS);
  const msm_ctx::Matrix& m = ctx->mats[id];
  if (int rc = vectors_ok(ctx, who, m.rows, {{dst, "dst"}}, "rows")) return rc;
  // x is read only where a column index points: an empty matrix needs none
  if (int rc = vectors_ok(ctx, who, m.nnz ? m.cols : 0, {{x, "x"}}, "cols")) return rc;
  if (int rc = dst_disjoint_ok(ctx, who, dst, m.rows * 32, x, m.nnz ? m.cols * 32 : 0, "x")) return rc;
  try {
    return with_scalar_field(ctx, [&](auto f) -> int {
      using S = decltype(f);
      Fe<S> alpham;
      fe_set_zero<S>(alpham);
      if (alpha && !host_scalar_mont<S>(alpham, alpha)) return scalar_too_big(ctx, who, "alpha");
      const uint32_t mode = (alpha ? spmv::FIN_ALPHA : 0u) | (flags & MSM_MATVEC_ACCUMULATE ? spmv::FIN_ACCUMULATE : 0u);
      int launches = 0;
      if (m.rows) {
        HIPCHK(hipSetDevice(ctx->device));
        const spmv::MatrixView v = view_of(m);
        launches = m.ones ? launch_product<S, true>(ctx, v, (uint32_t*)dst, (const uint32_t*)x, mode, alpham)
                          : launch_product<S, false>(ctx, v, (uint32_t*)dst, (const uint32_t*)x, mode, alpham);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
      }
      ctx->last_spmv[0] = (int32_t)m.short_max;
      ctx->last_spmv[1] = (int32_t)m.part_len;
      ctx->last_spmv[2] = (int32_t)m.n_long;
      ctx->last_spmv[3] = (int32_t)m.n_parts;
      ctx->last_spmv[4] = launches;
      return MSM_OK;
    });
  } MSM_CATCH_ALL(ctx)
}

}  // extern "C"
