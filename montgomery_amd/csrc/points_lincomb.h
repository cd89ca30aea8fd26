// Point-set linear combinations D[i] = a * A[i] + b * B[i] over resident rows (msm_points_lincomb, msm_lincomb.hip): the fold
// of the generators between two rounds of an inner-product argument, the scaling of a set by one scalar, the element-wise sum
// of two sets, the negation of a set.  The reference has no counterpart (its points live in wasm memory and are folded there).
//
// Both scalars are the same for every lane, so the HOST turns (a, b) into a PROGRAM once per call and every lane interprets it:
// one byte per op,
//     OP_DBL                              acc <- 2 acc
//     OP_ADD + 2 * operand + negative     acc <- acc +- operand,   operand 0 = A, 1 = phi(A), 2 = B, 3 = phi(B)
// walked from the first byte to the last over an accumulator that starts as the identity.  Every branch on an op is
// wave-uniform; lanes diverge only inside the additions, on the identity and equal-x cases proj_add_mixed handles (curve.h).
// The operands are the affine rows themselves: phi(P) = (beta x, y) is the second line of a row, -P is (x, p - y) -- on the
// Edwards curve (-x, y) with t -> -t -- so no operand costs a multiplication.  A lane re-reads its operand from its row at
// every addition (256 bytes per lane, cache-resident) instead of holding both operands beside the accumulator.
//
// The recoder (make_program) is plain host code, so it is tested on the CPU together with the lane bodies
// (tests/csrc/lincomb_host.hip).  Weierstrass curves: glv_decompose splits every non-trivial scalar into two signed halves of
// at most MAX_BITS bits, the (up to four) halves go to non-adjacent form and are walked jointly from the top digit down:
// at most MAX_BITS doublings (a NAF is one digit longer than its value; the top digit needs no doubling) and about MAX_BITS / 3
// additions per half.  The Edwards curve has no endomorphism: the NAFs of a and b themselves, up to 251 doublings.
// The scalars 0, 1 and q - 1 never reach the recoding: 0 gives no term, 1 the row, q - 1 its negative -- one digit at position
// 0, so they add no doubling and at most one addition.  A program that is "+A" alone is a copy: it is left EMPTY and flagged
// (Program::copy), and the host moves the rows without a kernel.
#pragma once
#include "te_kernels.h"

namespace msm {
namespace lincomb {

constexpr uint8_t OP_DBL = 0, OP_ADD = 1;
constexpr int OPERAND_A = 0, OPERAND_B = 2;   // (+ 1: the endomorphism image)
constexpr int MAX_OPS = 1024;                 // 251 doublings + 2 x 126 additions (Edwards) is the longest program
constexpr int MAX_DIGITS = 258;

struct Program {
  uint8_t ops[MAX_OPS];
  int n = 0, n_dbl = 0, n_add = 0;
  bool copy = false;   // D = A as it is: no op
};

// one signed multiple of one operand: value = (neg ? -1 : 1) * mag
struct Term {
  uint32_t mag[9] = {0};   // (one word of headroom for the carries of the NAF)
  bool neg = false;
  int operand = 0;
};

inline bool words8_zero(const uint32_t* s) {
  uint32_t o = 0;
  for (int j = 0; j < 8; j++) o |= s[j];
  return o == 0;
}
inline bool words8_is(const uint32_t* s, uint32_t v) {
  uint32_t o = s[0] ^ v;
  for (int j = 1; j < 8; j++) o |= s[j];
  return o == 0;
}
// s == q - 1 (q odd)
inline bool words8_is_q_minus_1(const uint32_t* s, const uint32_t* q) {
  uint32_t o = s[0] ^ (q[0] - 1u);
  for (int j = 1; j < 8; j++) o |= s[j] ^ q[j];
  return o == 0;
}

// non-adjacent form of t.mag, least significant digit first: digits in {-1, 0, 1}, no two neighbours non-zero; returns their number
inline int naf_digits(int8_t* d, const Term& t) {
  uint32_t k[9];
  for (int j = 0; j < 9; j++) k[j] = t.mag[j];
  int n = 0;
  for (;;) {
    uint32_t any = 0;
    for (int j = 0; j < 9; j++) any |= k[j];
    if (!any) break;
    int8_t digit = 0;
    if (k[0] & 1u) {
      digit = (int8_t)(2 - (int)(k[0] & 3u));   // 1 or -1: k - digit is divisible by 4
      if (digit < 0) {
        for (int j = 0; j < 9 && ++k[j] == 0; j++) {}
      } else {
        k[0] &= ~1u;
      }
    }
    d[n++] = digit;
    for (int j = 0; j < 8; j++) k[j] = (k[j] >> 1) | (k[j + 1] << 31);
    k[8] >>= 1;
  }
  return n;
}

// the joint walk over the terms' digits, top digit first
inline void build_program(Program& P, const Term* terms, int n_terms) {
  static_assert(MAX_DIGITS >= 257, "a NAF is one digit longer than its value");
  int8_t dig[4][MAX_DIGITS];
  int len[4] = {0, 0, 0, 0}, top = 0;
  for (int t = 0; t < n_terms; t++) {
    len[t] = naf_digits(dig[t], terms[t]);
    top = len[t] > top ? len[t] : top;
  }
  P.n = P.n_dbl = P.n_add = 0;
  P.copy = false;
  for (int i = top - 1; i >= 0; i--) {
    if (i < top - 1) { P.ops[P.n++] = OP_DBL; P.n_dbl++; }
    for (int t = 0; t < n_terms; t++) {
      if (i >= len[t] || dig[t][i] == 0) continue;
      const bool neg = (dig[t][i] < 0) != terms[t].neg;
      P.ops[P.n++] = (uint8_t)(OP_ADD + 2 * terms[t].operand + (neg ? 1 : 0));
      P.n_add++;
    }
  }
  if (P.n == 1 && P.ops[0] == OP_ADD + 2 * OPERAND_A) {
    P.n = P.n_add = 0;
    P.copy = true;
  }
}

// the terms of s * (operand): none for 0, the row or its negative for 1 and q - 1, otherwise `split` decides
template <class Split>
inline void scalar_terms(Term* terms, int& n_terms, const uint32_t* s, const uint32_t* q, int operand, Split&& split) {
  if (words8_zero(s)) return;
  if (words8_is(s, 1u) || words8_is_q_minus_1(s, q)) {
    Term& t = terms[n_terms++];
    t = Term();
    t.mag[0] = 1;
    t.neg = !words8_is(s, 1u);
    t.operand = operand;
    return;
  }
  split(terms, n_terms, s, operand);
}

// Weierstrass curves: s = s0 + s1 lambda, s0 on the row, s1 on its endomorphism image.  a, b: 8 words each, < q; b may be null.
template <class G>
inline void make_program(Program& P, const uint32_t* a, const uint32_t* b) {
  Term terms[4];
  int n_terms = 0;
  auto split = [](Term* ts, int& n, const uint32_t* s, int operand) {
    uint32_t w[8];
    for (int j = 0; j < 8; j++) w[j] = s[j];
    GlvHalf h[2];
    glv_decompose<G>(h[0], h[1], w);
    for (int e = 0; e < 2; e++) {
      Term& t = ts[n++];
      t = Term();
      for (int j = 0; j < 4; j++) t.mag[j] = h[e].mag[j];
      t.neg = h[e].neg;
      t.operand = operand + e;
    }
  };
  scalar_terms(terms, n_terms, a, G::Q, OPERAND_A, split);
  if (b) scalar_terms(terms, n_terms, b, G::Q, OPERAND_B, split);
  build_program(P, terms, n_terms);
}

// the Edwards curve: the scalars as they are
inline void make_program_te(Program& P, const uint32_t* a, const uint32_t* b) {
  Term terms[4];
  int n_terms = 0;
  auto whole = [](Term* ts, int& n, const uint32_t* s, int operand) {
    Term& t = ts[n++];
    t = Term();
    for (int j = 0; j < 8; j++) t.mag[j] = s[j];
    t.operand = operand;
  };
  scalar_terms(terms, n_terms, a, FRED_Q, OPERAND_A, whole);
  if (b) scalar_terms(terms, n_terms, b, FRED_Q, OPERAND_B, whole);
  build_program(P, terms, n_terms);
}

// op k of a program packed four to a word (a uniform address: a scalar load on the device)
MSM_DEV uint32_t program_op(const uint32_t* prog, uint32_t k) { return (prog[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// ---------------------------------------------------------------------------------------------
// lane bodies: one output row from the lane's two source rows.  `out` may be row_a or row_b (the in-place fold): everything is
// read before the one store at the end.  row_b is never read by a program without B terms (the host passes row_a again).
// ---------------------------------------------------------------------------------------------

template <class CV>
MSM_DEV void lincomb_lane(uint32_t* out, const uint32_t* row_a, const uint32_t* row_b, const uint32_t* prog, uint32_t n_ops) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  const bool inf_a = row_a[NW - 1] == INF_WORD, inf_b = row_b[NW - 1] == INF_WORD;
  Proj<F> acc;
  proj_set_zero<F>(acc);
#pragma unroll 1
  for (uint32_t k = 0; k < n_ops; k++) {
    const uint32_t op = program_op(prog, k);
    if (op == OP_DBL) {
      proj_double<F>(acc, acc);
      continue;
    }
    const uint32_t sel = op - OP_ADD;   // operand << 1 | negative
    const uint32_t* line = ((sel & 4u) ? row_b : row_a) + ((sel & 2u) ? ROW_HALF : 0);
    uint32_t w[NW];
    Proj<F> Q;
    load_words12(w, line);
    fe_unpack<F>(Q.X, w);
    load_words12(w, line + NW);
    fe_unpack<F>(Q.Y, w);
    if (sel & 1u) {
      Fe<F> z;
      fe_set_zero<F>(z);
      fe_sub_p<F>(Q.Y, z, Q.Y);   // p - y (y canonical; p itself for y = 0 is a valid operand < 2p)
    }
    Q.Z = Q.X;   // (ignored by the mixed addition)
    proj_add_mixed<F>(acc, acc, Q, (sel & 4u) ? inf_b : inf_a);
  }
  if (proj_is_zero<F>(acc)) {
    store_row_identity<NW / 4>(out);
    return;
  }
  Fe<F> zi, x, y, bx, beta;   // to affine as k_table_next does it: one inversion per point
  fe_reduce_4p<F>(acc.Z);
  fe_inv<F>(zi, acc.Z);
  fe_mul<F>(x, acc.X, zi);
  fe_reduce_2p<F>(x);
  fe_mul<F>(y, acc.Y, zi);
  fe_reduce_2p<F>(y);
#pragma unroll
  for (int l = 0; l < NL; l++) beta.l[l] = F::BETAL[l];
  fe_mul<F>(bx, x, beta);
  fe_reduce_2p<F>(bx);
  store_row(out, x, y, bx);
}

// Ed-on-BLS12-377: unified additions (complete: no edge cases), the identity is the ordinary row of (0, 1)
MSM_DEV void te_lincomb_lane(uint32_t* out, const uint32_t* row_a, const uint32_t* row_b, const uint32_t* prog, uint32_t n_ops) {
  using te::FT;
  using te::TL;
  te::Ext acc;
  te::te_set_identity(acc);
#pragma unroll 1
  for (uint32_t k = 0; k < n_ops; k++) {
    const uint32_t op = program_op(prog, k);
    if (op == OP_DBL) {
      te::te_add(acc, acc, acc);
      continue;
    }
    const uint32_t sel = op - OP_ADD;
    const uint32_t* row = (sel & 4u) ? row_b : row_a;
    uint32_t w[te::TW];
    te::Ext Q;
    te::load_words8(w, row);      fe_unpack<FT>(Q.X, w);
    te::load_words8(w, row + 8);  fe_unpack<FT>(Q.Y, w);
    te::load_words8(w, row + 16); fe_unpack<FT>(Q.T, w);
    fe_set_one<FT>(Q.Z);
    if (sel & 1u) {   // -(x, y) = (-x, y), t -> -t
      Fe<FT> z;
      fe_set_zero<FT>(z);
      fe_sub_2p<FT>(Q.X, z, Q.X);
      fe_sub_2p<FT>(Q.T, z, Q.T);
    }
    te::te_add(acc, acc, Q);
  }
  Fe<FT> zi, x, y, t, kt, kk;   // as k_te_table_next
  fe_reduce_4p<FT>(acc.Z);
  fe_inv<FT>(zi, acc.Z);   // Z != 0 for every point of a complete Edwards curve
  fe_mul<FT>(x, acc.X, zi);
  fe_mul<FT>(y, acc.Y, zi);
  fe_mul<FT>(t, x, y);
  TE_CONST(kk, K2DL);
  fe_mul<FT>(kt, t, kk);
  fe_reduce_2p<FT>(x);
  fe_reduce_2p<FT>(y);
  fe_reduce_2p<FT>(t);
  fe_reduce_2p<FT>(kt);
  fe_store<FT>(out, x);
  fe_store<FT>(out + 8, y);
  fe_store<FT>(out + 16, t);
  fe_store<FT>(out + 24, kt);
}

// ---------------------------------------------------------------------------------------------
// kernels: one lane per output point.  rows_a / rows_b already point at the first source row of the call.
// ---------------------------------------------------------------------------------------------

template <class CV>
__global__ void __launch_bounds__(256) k_points_lincomb(uint32_t* dst, const uint32_t* rows_a, const uint32_t* rows_b, uint64_t count,
                                                        const uint32_t* prog, uint32_t n_ops) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  lincomb_lane<CV>(dst + i * ROW_WORDS, rows_a + i * ROW_WORDS, rows_b + i * ROW_WORDS, prog, n_ops);
}

__global__ void __launch_bounds__(256) k_te_points_lincomb(uint32_t* dst, const uint32_t* rows_a, const uint32_t* rows_b, uint64_t count,
                                                           const uint32_t* prog, uint32_t n_ops) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  te_lincomb_lane(dst + i * te::TE_ROW_WORDS, rows_a + i * te::TE_ROW_WORDS, rows_b + i * te::TE_ROW_WORDS, prog, n_ops);
}

}  // namespace lincomb
}  // namespace msm
