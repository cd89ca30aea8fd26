// Resident sparse matrices and y = alpha M x (+ y) mod q (msm_matrix_create / _destroy / _info, msm_scalars_matvec; msm_spmv.hip): a
// matrix in CSR that lives in device memory as a point set does, times a vector of scalar_vec.h -- plain 32-byte little-endian
// integers in device memory, any value below 2^256, every element written canonical.  A.z, B.z, C.z of an R1CS, M^T.eq of Spartan's
// second phase, and with all coefficients 1 the gather y[i] = T[idx[i]] and the row sum.  The reference has no counterpart.
// Templates over the scalar FIELD S (MSM_SCALAR_FIELDS), 9 limbs of 30 bits, R = 2^270.
//
// The work is one fe_mul per nonzero, as in msm_scalars_inner; what is new is the gather of x and the balance of the rows.  R1CS rows
// are short (1 to 4 entries, a few of thousands); a transposed R1CS has rows of millions (the column of the constant 1).  So, as
// the sort does with heavy bins, the rows are split once, on the host, when the matrix is created (make_plan: a pure function of
// row_ptr and two thresholds): a row of at most short_max entries is SHORT and one lane sums it (k_spmv_rows); every longer row is
// cut into PARTS of at most part_len consecutive entries, one wave sums a part with coalesced reads of col and val and writes one
// partial (k_spmv_parts), and one lane per long row adds that row's partials in order and finishes it (k_spmv_long_finish).
// No atomics on field elements, and no dependence of the bits on the geometry: FIELD ADDITION IS EXACT, every partial and every
// result is canonical, so however the terms of a row are grouped the row's bits are the same (tests/test_gpu_matvec.py proves it).
//
// Values.  The coefficients are brought to canonical Montgomery form once, at creation (k_spmv_values: val R^2 / R); Montgomery form
// stays inside the matrix and never reaches a vector.  With q > 2^250, q < 2^255, R = 2^270 and fe_mul returning a value below
// q + a b / R for operands with normalised limbs (header of scalar_vec.h):
//   valM                  canonical, < q                (raw < 2^256 times R^2 < q: < q + 2^256 q / 2^270 < 2 q, one subtraction)
//   term = x valM / R     x raw < 2^256: < q + 2^256 q / 2^270 = q (1 + 2^-14) < 2 q; congruent to x val: the plain product
//   term, all-ones form   reduce_wide(x) of scalar_mle.h: x < 2^256 < 2^262 -> < 2 q, no multiplication
//   acc                   sums of terms through sv::inner_combine: (< 2 q) + (< 2 q) < 4 q, one subtraction of 2 q -> < 2 q
//   partial               fe_reduce_2p(acc): canonical, so a sum of partials goes through inner_combine like a sum of terms
// The finish of a row, acc < 2 q:
//   without alpha         t = acc < 2 q
//   with alpha            t = acc alphaM / R < q + 2 q q / 2^270 < q (1 + 2^-14) < 2 q, alphaM the canonical Montgomery form of alpha
//   store                 fe_reduce_2p(t)
//   MSM_MATVEC_ACCUMULATE t + reduce_wide(dst[r]) < 4 q < 2^257 (fits the limbs), fe_reduce_4p
// An empty row has acc = 0 and takes the same finish.
#pragma once
#include "scalar_vec.h"
#include "scalar_mle.h"
#include <vector>

namespace msm {
namespace spmv {

constexpr int BLOCK = 256;                    // lanes per block
constexpr int WAVES = BLOCK / 64;             // parts per block of k_spmv_parts
// The two thresholds of the plan, from the sweep of tools/bench_matvec.py (profiles/matvec_time.txt).  short_max:
// anything from 8 to 64 times the same on both workloads; one lane summing a row of 2^10 entries is 35 times slower than its waves.
// part_len: a row of n entries costs about 17 ns per entry of a part (one wave walks it) plus 0.33 us per partial (one lane adds
// them), least near sqrt(19 n): 4096 wins at 2^20 entries, 16384 at 2^24; 8192 is within a fifth of the better one at both.
constexpr uint32_t DEFAULT_SHORT_MAX = 32;    // rows of at most this many entries are summed by one lane
constexpr uint32_t DEFAULT_PART_LEN = 8192;   // entries one wave sums
constexpr uint64_t MAX_DIM = 1ull << 30, MAX_NNZ = 1ull << 31;   // rows, cols < MAX_DIM; nnz < MAX_NNZ
constexpr unsigned long long ALL_GOOD = ~0ull;   // the word of the validation kernels when nothing is wrong

// the finish of a row: bits of `mode`
enum { FIN_ALPHA = 1, FIN_ACCUMULATE = 2 };

// ---------------------------------------------------------------- the CSR rule: one statement for the host and the kernels

// entry i <= rows of row_ptr: v = row_ptr[i], prev = row_ptr[i - 1] (ignored at i == 0)
MSM_DEV bool row_ptr_entry_ok(uint64_t i, uint32_t prev, uint32_t v, uint64_t rows, uint64_t nnz) {
  if (i == 0 && v != 0) return false;
  if (i > 0 && v < prev) return false;
  if (i == rows && v != nnz) return false;
  return true;
}
MSM_DEV bool col_entry_ok(uint32_t v, uint64_t cols) { return v < cols; }
// what the validation kernels take the minimum of: the smallest bad position wins, its value rides along
MSM_DEV unsigned long long defect_word(uint64_t pos, uint32_t v) { return ((unsigned long long)pos << 32) | v; }

// kind: 0 none, 1 row_ptr (pos <= rows), 2 col (pos < nnz)
struct CsrDefect {
  int kind = 0;
  uint64_t pos = 0;
  uint32_t value = 0;
};

// the smallest bad position of row_ptr; col is not looked at
inline CsrDefect check_row_ptr(const uint32_t* row_ptr, uint64_t rows, uint64_t nnz) {
  for (uint64_t i = 0; i <= rows; i++)
    if (!row_ptr_entry_ok(i, i ? row_ptr[i - 1] : 0u, row_ptr[i], rows, nnz)) return CsrDefect{1, i, row_ptr[i]};
  return CsrDefect{};
}
inline CsrDefect check_col(const uint32_t* col, uint64_t nnz, uint64_t cols) {
  for (uint64_t j = 0; j < nnz; j++)
    if (!col_entry_ok(col[j], cols)) return CsrDefect{2, j, col[j]};
  return CsrDefect{};
}
// row_ptr defects come before col defects, and col is indexed only after row_ptr has passed
inline CsrDefect check_csr(const uint32_t* row_ptr, const uint32_t* col, uint64_t rows, uint64_t cols, uint64_t nnz) {
  const CsrDefect d = check_row_ptr(row_ptr, rows, nnz);
  return d.kind ? d : check_col(col, nnz, cols);
}
// the refusal's text after "msm_matrix_create: "; prev: row_ptr[pos - 1] of a row_ptr defect at pos > 0
inline void describe_defect(char* out, size_t cap, const CsrDefect& d, uint32_t prev, uint64_t rows, uint64_t cols, uint64_t nnz) {
  if (d.kind == 2)
    snprintf(out, cap, "col[%llu] = %u but cols = %llu", (unsigned long long)d.pos, d.value, (unsigned long long)cols);
  else if (d.pos == 0)
    snprintf(out, cap, "row_ptr[0] = %u but must be 0", d.value);
  else if (d.value < prev)
    snprintf(out, cap, "row_ptr[%llu] = %u but row_ptr[%llu] = %u (row_ptr must not decrease)", (unsigned long long)d.pos, d.value,
             (unsigned long long)(d.pos - 1), prev);
  else
    snprintf(out, cap, "row_ptr[%llu] = %u but nnz = %llu (the last entry of row_ptr)", (unsigned long long)d.pos, d.value,
             (unsigned long long)nnz);
}

// ---------------------------------------------------------------- the plan: a pure function of row_ptr and two thresholds

// `len` consecutive entries of row `row` from entry `first` of col / val
struct Part {
  uint32_t row, first, len;
};

struct Plan {
  uint32_t short_max = 0, part_len = 0;
  std::vector<Part> parts;           // the parts of a row are contiguous, in the order of its entries; rows in rising order
  std::vector<uint32_t> long_rows;   // the long rows, rising
  std::vector<uint32_t> long_first;  // long_rows.size() + 1 entries: the parts of long row k are [long_first[k], long_first[k + 1])
};

// row_ptr is valid CSR (check_row_ptr); short_max, part_len >= 1.  No HIP call.
inline Plan make_plan(const uint32_t* row_ptr, uint64_t rows, uint32_t short_max, uint32_t part_len) {
  Plan pl;
  pl.short_max = short_max;
  pl.part_len = part_len;
  pl.long_first.push_back(0);
  for (uint64_t r = 0; r < rows; r++) {
    const uint32_t first = row_ptr[r], len = row_ptr[r + 1] - first;
    if (len <= short_max) continue;
    for (uint32_t o = 0; o < len; o += part_len) pl.parts.push_back(Part{(uint32_t)r, first + o, len - o < part_len ? len - o : part_len});
    pl.long_rows.push_back((uint32_t)r);
    pl.long_first.push_back((uint32_t)pl.parts.size());
  }
  return pl;
}

// ---------------------------------------------------------------- the transposition: a stable counting sort over the columns

// (rows x cols, valid CSR) -> (cols x rows): within a transposed row the entries keep the order of the original rows, and of the
// entries inside a row.  val / t_val: nnz x 8 words, or both null (the all-ones form).  t_row_ptr: cols + 1 words; t_col: nnz.
inline void transpose_csr(uint64_t rows, uint64_t cols, uint64_t nnz, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* val,
                          uint32_t* t_row_ptr, uint32_t* t_col, uint32_t* t_val) {
  for (uint64_t c = 0; c <= cols; c++) t_row_ptr[c] = 0;
  for (uint64_t j = 0; j < nnz; j++) t_row_ptr[col[j] + 1]++;
  for (uint64_t c = 0; c < cols; c++) t_row_ptr[c + 1] += t_row_ptr[c];
  std::vector<uint32_t> cursor(t_row_ptr, t_row_ptr + cols);
  for (uint64_t r = 0; r < rows; r++)
    for (uint32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
      const uint32_t d = cursor[col[j]]++;
      t_col[d] = (uint32_t)r;
      if (val)
        for (int w = 0; w < 8; w++) t_val[8 * (uint64_t)d + w] = val[8 * (uint64_t)j + w];
    }
}

// ---------------------------------------------------------------- lane bodies (host and device)

// raw coefficient -> canonical Montgomery form, 8 words
template <class S>
MSM_DEV void value_lane(uint32_t* dst, const uint32_t* val) {
  Fe<S> v, r2;
  fe_load<S>(v, val);
  sv::set_const<S>(r2, S::R2);
  fe_mul<S>(v, v, r2);    // < 2 q
  fe_reduce_2p<S>(v);
  fe_store<S>(dst, v);
}

// one term, < 2 q: x val (valm: the coefficient's Montgomery form), or x itself in the all-ones form
template <class S, bool ONES>
MSM_DEV void term(Fe<S>& t, const uint32_t* x, const uint32_t* valm) {
  fe_load<S>(t, x);
  if constexpr (ONES) {
    mle::reduce_wide<S>(t);
  } else {
    Fe<S> v;
    fe_load<S>(v, valm);
    fe_mul<S>(t, t, v);
  }
}

// acc += the terms of the entries first, first + step, .. below end
template <class S, bool ONES>
MSM_DEV void sum_entries(Fe<S>& acc, const uint32_t* x, const uint32_t* col, const uint32_t* valm, uint32_t first, uint32_t end,
                         uint32_t step) {
#pragma unroll 1
  for (uint32_t j = first; j < end; j += step) {
    Fe<S> t;
    term<S, ONES>(t, x + 8 * (uint64_t)col[j], valm + 8 * (uint64_t)j);
    sv::inner_combine<S>(acc, t);
  }
}

// the sum of a row's terms (< 2 q) -> dst, canonical.  The old dst is loaded before the store.
template <class S>
MSM_DEV void finish_row(uint32_t* dst, Fe<S> acc, uint32_t mode, const Fe<S>& alpham) {
  if (mode & FIN_ALPHA) fe_mul<S>(acc, acc, alpham);   // < 2 q
  if (mode & FIN_ACCUMULATE) {
    Fe<S> old;
    fe_load<S>(old, dst);
    mle::reduce_wide<S>(old);                          // < 2 q
    fe_add<S>(acc, acc, old);                          // < 4 q
    fe_reduce_4p<S>(acc);
  } else {
    fe_reduce_2p<S>(acc);
  }
  fe_store<S>(dst, acc);
}

// ---------------------------------------------------------------- kernels

// the device form of the matrix and its plan, as the three kernels of a product read it
struct MatrixView {
  const uint32_t* row_ptr;   // rows + 1
  const uint32_t* col;       // nnz
  const uint32_t* valm;      // nnz x 8 words in Montgomery form; unused in the all-ones form
  const Part* parts;         // n_parts
  const uint32_t* long_rows; // n_long
  const uint32_t* long_first;// n_long + 1
  uint32_t* partials;        // n_parts x 8 words
  uint32_t rows, n_parts, n_long, short_max;
};

// the minimum of `worst` over the wave, and one atomic per wave that saw a defect
__device__ __forceinline__ void report_defect(unsigned long long worst, unsigned long long* bad) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)worst, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(worst >> 32), d, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    worst = o < worst ? o : worst;
  }
  if ((threadIdx.x & 63u) == 0 && worst != ALL_GOOD) atomicMin(bad, worst);
}

// *bad = the smallest defect_word over the bad positions of row_ptr[0 .. rows]; reads nothing else
__global__ void __launch_bounds__(BLOCK) k_spmv_check_row_ptr(const uint32_t* row_ptr, uint64_t rows, uint64_t nnz, unsigned long long* bad) {
  unsigned long long worst = ALL_GOOD;
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i <= rows; i += stride) {
    const uint32_t v = row_ptr[i], prev = i ? row_ptr[i - 1] : 0u;
    if (!row_ptr_entry_ok(i, prev, v, rows, nnz)) {
      const unsigned long long w = defect_word(i, v);
      worst = w < worst ? w : worst;
    }
  }
  report_defect(worst, bad);
}

// the same over col[0 .. nnz): launched only after row_ptr has passed
__global__ void __launch_bounds__(BLOCK) k_spmv_check_col(const uint32_t* col, uint64_t nnz, uint64_t cols, unsigned long long* bad) {
  unsigned long long worst = ALL_GOOD;
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < nnz; j += stride) {
    const uint32_t v = col[j];
    if (!col_entry_ok(v, cols)) {
      const unsigned long long w = defect_word(j, v);
      worst = w < worst ? w : worst;
    }
  }
  report_defect(worst, bad);
}

// dst[j] = the Montgomery form of val[j]; dst may be val itself (a lane loads before it stores)
template <class S>
__global__ void __launch_bounds__(BLOCK) k_spmv_values(uint32_t* dst, const uint32_t* val, uint64_t nnz) {
  const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= nnz) return;
  value_lane<S>(dst + 8 * j, val + 8 * j);
}

// one lane per row: a short row (empty ones included) is summed and finished; long rows are left to the two kernels below
template <class S, bool ONES>
__global__ void __launch_bounds__(BLOCK) k_spmv_rows(MatrixView m, uint32_t* dst, const uint32_t* x, uint32_t mode, Fe<S> alpham) {
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= m.rows) return;
  const uint32_t first = m.row_ptr[r], end = m.row_ptr[r + 1];
  if (end - first > m.short_max) return;
  Fe<S> acc;
  fe_set_zero<S>(acc);
  sum_entries<S, ONES>(acc, x, m.col, m.valm, first, end, 1);
  finish_row<S>(dst + 8 * (uint64_t)r, acc, mode, alpham);
}

// one wave per part: the lanes stride over its entries, the sum goes down the wave by shuffles, lane 0 writes the partial, canonical
template <class S, bool ONES>
__global__ void __launch_bounds__(BLOCK) k_spmv_parts(MatrixView m, const uint32_t* x) {
  const uint32_t lane = threadIdx.x & 63u, p = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (p >= m.n_parts) return;   // (the whole wave)
  const Part part = m.parts[p];
  Fe<S> acc;
  fe_set_zero<S>(acc);
  sum_entries<S, ONES>(acc, x, m.col, m.valm, part.first + lane, part.first + part.len, 64);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Fe<S> o;
#pragma unroll
    for (int j = 0; j < S::NL; j++) o.l[j] = (uint32_t)__shfl_down((int)acc.l[j], off, 64);
    sv::inner_combine<S>(acc, o);   // (lanes whose partner lies outside the wave add their own value: never read)
  }
  if (lane == 0) {
    fe_reduce_2p<S>(acc);
    fe_store<S>(m.partials + 8 * (uint64_t)p, acc);
  }
}

// one lane per long row: its partials in order, then the finish
template <class S>
__global__ void __launch_bounds__(BLOCK) k_spmv_long_finish(MatrixView m, uint32_t* dst, uint32_t mode, Fe<S> alpham) {
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= m.n_long) return;
  Fe<S> acc;
  fe_set_zero<S>(acc);
#pragma unroll 1
  for (uint32_t p = m.long_first[k]; p < m.long_first[k + 1]; p++) {
    Fe<S> t;
    fe_load<S>(t, m.partials + 8 * (uint64_t)p);
    sv::inner_combine<S>(acc, t);
  }
  finish_row<S>(dst + 8 * (uint64_t)m.long_rows[k], acc, mode, alpham);
}

}  // namespace spmv
}  // namespace msm
