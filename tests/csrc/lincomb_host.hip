// Host-side unit-test shim of msm_points_lincomb: the recoder (make_program) and the lane bodies (lincomb_lane, te_lincomb_lane)
// of montgomery_amd/csrc/points_lincomb.h compiled for the CPU, on all seven curves (tests/test_points_lincomb_host.py).  Rows
// are made here the way k_points_from_wire / k_te_points_from_wire make them, so that a lane's output can be compared bit for
// bit with the row of the expected affine point.
#include "points_lincomb.h"
#include <cstring>
using namespace msm;

namespace {

template <class CV>
void make_row(const uint32_t* xw_in, const uint32_t* yw_in, int identity, uint32_t* row_out) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  alignas(16) uint32_t row[ROW_WORDS] = {0};
  if (identity) {
    store_row_identity<NW / 4>(row);
  } else {
    uint32_t xw[NW], yw[NW];
    for (int j = 0; j < NW; j++) { xw[j] = xw_in[j]; yw[j] = yw_in[j]; }
    Fe<F> x, y, r2, beta, bx;
    fe_unpack<F>(x, xw);
    fe_unpack<F>(y, yw);
    for (int l = 0; l < NL; l++) { r2.l[l] = F::R2[l]; beta.l[l] = F::BETAL[l]; }
    fe_mul<F>(x, x, r2);
    fe_reduce_2p<F>(x);
    fe_mul<F>(y, y, r2);
    fe_reduce_2p<F>(y);
    fe_mul<F>(bx, x, beta);
    fe_reduce_2p<F>(bx);
    store_row(row, x, y, bx);
  }
  memcpy(row_out, row, sizeof row);
}

void make_row_te(const uint32_t* xw_in, const uint32_t* yw_in, uint32_t* row_out) {
  using te::FT;
  using te::TL;
  alignas(16) uint32_t row[te::TE_ROW_WORDS];
  uint32_t xw[te::TW], yw[te::TW];
  for (int j = 0; j < te::TW; j++) { xw[j] = xw_in[j]; yw[j] = yw_in[j]; }
  Fe<FT> x, y, t, kt, r2, k;
  fe_unpack<FT>(x, xw);
  fe_unpack<FT>(y, yw);
  TE_CONST(r2, R2);
  TE_CONST(k, K2DL);
  fe_mul<FT>(x, x, r2);
  fe_mul<FT>(y, y, r2);
  fe_mul<FT>(t, x, y);
  fe_mul<FT>(kt, t, k);
  fe_reduce_2p<FT>(x);
  fe_reduce_2p<FT>(y);
  fe_reduce_2p<FT>(t);
  fe_reduce_2p<FT>(kt);
  fe_store<FT>(row, x);
  fe_store<FT>(row + 8, y);
  fe_store<FT>(row + 16, t);
  fe_store<FT>(row + 24, kt);
  memcpy(row_out, row, sizeof row);
}

void pack_ops(uint32_t* words, const uint8_t* ops, int n) {
  for (int k = 0; k < lincomb::MAX_OPS / 4; k++) words[k] = 0;
  for (int k = 0; k < n; k++) words[k >> 2] |= (uint32_t)ops[k] << (8 * (k & 3));
}

template <class CV>
void lane(const uint32_t* row_a, const uint32_t* row_b, const uint8_t* ops, int n_ops, uint32_t* row_out) {
  alignas(16) uint32_t a[ROW_WORDS], b[ROW_WORDS], out[ROW_WORDS] = {0};
  uint32_t words[lincomb::MAX_OPS / 4];
  memcpy(a, row_a, sizeof a);
  memcpy(b, row_b, sizeof b);
  pack_ops(words, ops, n_ops);
  lincomb::lincomb_lane<CV>(out, a, b, words, (uint32_t)n_ops);
  memcpy(row_out, out, sizeof out);
}

}  // namespace

// X(curve id of include/msm_hip.h, configuration)
#define LC_W_CURVES(X) X(0, CvBls377) X(2, CvBls381) X(3, CvPallas) X(4, CvBn254) X(5, CvGrumpkin) X(6, CvVesta)

extern "C" {

int lc_row_words(int curve) { return curve == 1 ? te::TE_ROW_WORDS : ROW_WORDS; }
int lc_coord_words(int curve) {
  switch (curve) {
#define LC_CASE(ID, CV) case ID: return CV::F::NW;
    LC_W_CURVES(LC_CASE)
#undef LC_CASE
    case 1: return te::TW;
  }
  return -1;
}
// MAX_BITS of the curve's GLV halves (Edwards: the bits of q)
int lc_max_bits(int curve) {
  switch (curve) {
#define LC_CASE(ID, CV) case ID: return CV::G::MAX_BITS;
    LC_W_CURVES(LC_CASE)
#undef LC_CASE
    case 1: return 251;
  }
  return -1;
}
int lc_max_ops(void) { return lincomb::MAX_OPS; }

// the program of (a, b): ops_out holds lc_max_ops() bytes; info = {n, doublings, additions, copy}.  b may be null (no second term)
int lc_program(int curve, const uint32_t* a, const uint32_t* b, uint8_t* ops_out, int32_t* info) {
  lincomb::Program P;
  switch (curve) {
#define LC_CASE(ID, CV) case ID: lincomb::make_program<CV::G>(P, a, b); break;
    LC_W_CURVES(LC_CASE)
#undef LC_CASE
    case 1: lincomb::make_program_te(P, a, b); break;
    default: return -1;
  }
  memcpy(ops_out, P.ops, (size_t)P.n);
  info[0] = P.n; info[1] = P.n_dbl; info[2] = P.n_add; info[3] = P.copy;
  return 0;
}

// affine (x, y) as plain little-endian words -> the resident row msm_set_points writes (identity != 0: the identity row of a
// Weierstrass curve; the Edwards identity is the ordinary point (0, 1))
int lc_make_row(int curve, const uint32_t* x, const uint32_t* y, int identity, uint32_t* row_out) {
  switch (curve) {
#define LC_CASE(ID, CV) case ID: make_row<CV>(x, y, identity, row_out); break;
    LC_W_CURVES(LC_CASE)
#undef LC_CASE
    case 1: make_row_te(x, y, row_out); break;
    default: return -1;
  }
  return 0;
}

// one lane: row_out = the program over (row_a, row_b)
int lc_lane(int curve, const uint32_t* row_a, const uint32_t* row_b, const uint8_t* ops, int n_ops, uint32_t* row_out) {
  if (n_ops < 0 || n_ops > lincomb::MAX_OPS) return -1;
  switch (curve) {
#define LC_CASE(ID, CV) case ID: lane<CV>(row_a, row_b, ops, n_ops, row_out); break;
    LC_W_CURVES(LC_CASE)
#undef LC_CASE
    case 1: {
      alignas(16) uint32_t a[te::TE_ROW_WORDS], b[te::TE_ROW_WORDS], out[te::TE_ROW_WORDS];
      uint32_t words[lincomb::MAX_OPS / 4];
      memcpy(a, row_a, sizeof a);
      memcpy(b, row_b, sizeof b);
      pack_ops(words, ops, n_ops);
      lincomb::te_lincomb_lane(out, a, b, words, (uint32_t)n_ops);
      memcpy(row_out, out, sizeof out);
      break;
    }
    default: return -1;
  }
  return 0;
}
}
