// Host-side unit-test shim of the resident sparse matrix-vector product: the CSR rule, the plan of the long rows, the host
// transposition and the lane bodies of montgomery_amd/csrc/scalar_spmv.h compiled for the CPU, over the scalar field
// MSM_SCALAR_FIELDS gives every curve (tests/test_spmv_host.py).  Elements cross as 8 words, plain little-endian integers below
// 2^256, as the kernels read them from device memory; alpha crosses as 8 canonical words and goes to Montgomery form as the entry
// point does it.
#include "scalar_vec.h"
#include "scalar_host.h"
#include "scalar_spmv.h"
#include <cstring>
using namespace msm;
using namespace msmi;

namespace {

using Words8 = const uint32_t[8];

// One row of n entries as the kernels sum it: the coefficients go through value_lane as at creation, the entries [0, cut) are one
// accumulator, the entries [cut, n) a second one that becomes a canonical partial (what k_spmv_parts stores), the two are combined
// and the row is finished over a dst that holds `old`.  mode: spmv::FIN_*.  ones: the all-ones form (coef is not read).
template <class S>
void run_row(int ones, int n, const uint32_t* coef, const uint32_t* x, int cut, uint32_t mode, const uint32_t* alpha, const uint32_t* old,
             uint32_t* out) {
  Fe<S> acc[2], alpham;
  fe_set_zero<S>(acc[0]);
  fe_set_zero<S>(acc[1]);
  fe_set_zero<S>(alpham);
  if (mode & spmv::FIN_ALPHA) m_from_words<S>(alpham, *(Words8*)alpha);
  for (int j = 0; j < n; j++) {
    alignas(16) uint32_t vx[8], vc[8], vm[8];
    memcpy(vx, x + 8 * j, sizeof vx);
    Fe<S> t;
    if (ones) {
      spmv::term<S, true>(t, vx, vx);
    } else {
      memcpy(vc, coef + 8 * j, sizeof vc);
      spmv::value_lane<S>(vm, vc);
      spmv::term<S, false>(t, vx, vm);
    }
    sv::inner_combine<S>(acc[j >= cut], t);
  }
  fe_reduce_2p<S>(acc[1]);
  sv::inner_combine<S>(acc[0], acc[1]);
  alignas(16) uint32_t vo[8];
  memcpy(vo, old, sizeof vo);
  spmv::finish_row<S>(vo, acc[0], mode, alpham);
  memcpy(out, vo, sizeof vo);
}

template <class S>
void run_value(const uint32_t* val, uint32_t* out) {
  alignas(16) uint32_t vi[8], vo[8];
  memcpy(vi, val, sizeof vi);
  spmv::value_lane<S>(vo, vi);
  memcpy(out, vo, sizeof vo);
}

}  // namespace

#define SPMV_DISPATCH()                                     \
  switch (curve) {                                          \
    MSM_SCALAR_FIELDS(SPMV_CASE)                            \
    default: return -1;                                     \
  }

extern "C" {

int spmv_default_short_max(void) { return (int)spmv::DEFAULT_SHORT_MAX; }
int spmv_default_part_len(void) { return (int)spmv::DEFAULT_PART_LEN; }

int spmv_row(int curve, int ones, int n, const uint32_t* coef, const uint32_t* x, int cut, uint32_t mode, const uint32_t* alpha,
             const uint32_t* old, uint32_t* out) {
#define SPMV_CASE(ID, S) case ID: run_row<S>(ones, n, coef, x, cut, mode, alpha, old, out); return 0;
  SPMV_DISPATCH()
#undef SPMV_CASE
}

// the Montgomery form of a raw coefficient, canonical, 8 words
int spmv_value(int curve, const uint32_t* val, uint32_t* out) {
#define SPMV_CASE(ID, S) case ID: run_value<S>(val, out); return 0;
  SPMV_DISPATCH()
#undef SPMV_CASE
}

// the plan of a valid row_ptr: parts_out takes min(parts, cap) triples (row, first, len), long_rows_out the long rows (at most
// rows), long_first_out one word more.  Returns the parts; *n_long_out the long rows.
int spmv_plan(const uint32_t* row_ptr, uint64_t rows, uint32_t short_max, uint32_t part_len, uint32_t* parts_out, int cap,
              uint32_t* long_rows_out, uint32_t* long_first_out, int* n_long_out) {
  const spmv::Plan pl = spmv::make_plan(row_ptr, rows, short_max, part_len);
  for (size_t p = 0; p < pl.parts.size() && (int)p < cap; p++) {
    parts_out[3 * p] = pl.parts[p].row;
    parts_out[3 * p + 1] = pl.parts[p].first;
    parts_out[3 * p + 2] = pl.parts[p].len;
  }
  for (size_t k = 0; k < pl.long_rows.size(); k++) long_rows_out[k] = pl.long_rows[k];
  for (size_t k = 0; k < pl.long_first.size(); k++) long_first_out[k] = pl.long_first[k];
  *n_long_out = (int)pl.long_rows.size();
  return (int)pl.parts.size();
}

// the CSR rule as msm_matrix_create applies it to host input: returns the kind (0 none, 1 row_ptr, 2 col), the position and the
// value, and the refusal's text
int spmv_check(const uint32_t* row_ptr, const uint32_t* col, uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t* pos_out,
               uint32_t* value_out, char* msg_out, int msg_cap) {
  const spmv::CsrDefect d = spmv::check_csr(row_ptr, col, rows, cols, nnz);
  *pos_out = d.pos;
  *value_out = d.value;
  if (msg_cap > 0) msg_out[0] = 0;
  if (d.kind) spmv::describe_defect(msg_out, (size_t)msg_cap, d, d.kind == 1 && d.pos ? row_ptr[d.pos - 1] : 0u, rows, cols, nnz);
  return d.kind;
}

// the rule entry by entry, as a lane of the validation kernels applies it
int spmv_row_ptr_entry_ok(uint64_t i, uint32_t prev, uint32_t v, uint64_t rows, uint64_t nnz) {
  return spmv::row_ptr_entry_ok(i, prev, v, rows, nnz);
}
int spmv_col_entry_ok(uint32_t v, uint64_t cols) { return spmv::col_entry_ok(v, cols); }

void spmv_transpose(uint64_t rows, uint64_t cols, uint64_t nnz, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* val,
                    uint32_t* t_row_ptr, uint32_t* t_col, uint32_t* t_val) {
  spmv::transpose_csr(rows, cols, nnz, row_ptr, col, val, t_row_ptr, t_col, t_val);
}
}
