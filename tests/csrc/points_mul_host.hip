// Host-side unit-test shim of msm_points_mul / msm_points_mul_base: the recoding and the four lane bodies of
// montgomery_amd/csrc/points_mul.h compiled for the CPU, on all seven curves and at every candidate window
// (tests/test_points_mul_host.py).  The per-lane table is a plain array of the caller's, laid out as on the device (cap lanes,
// this lane = g), so a test can run a lane twice over the same slots.
#include "points_mul.h"
#include <cstring>
#include <vector>
using namespace msm;

namespace {

constexpr int MAX_WIN = 96;   // windows of the longest chain: 84 on the Edwards curve at w = 3

// digits (least significant first), sign and the part of the recoded value above the last window, of one magnitude
template <int NX, int W>
void digits_of(const uint32_t (&r)[NX], int nwin, int32_t* dig, int32_t* top) {
  for (int k = 0; k < nwin; k++) {
    uint32_t mag;
    bool neg;
    pmul::digit<NX, W>(r, k, mag, neg);
    dig[k] = neg ? -(int32_t)mag : (int32_t)mag;
  }
  uint32_t above = 0;
  for (int b = W * nwin; b < 32 * NX; b++) above |= (r[b / 32] >> (b % 32)) & 1u;
  *top = (int32_t)above;
}

// Weierstrass: mags = the two half magnitudes (4 words each), dig = 2 x MAX_WIN, info = {nwin, neg0, neg1, top0, top1}
template <class CV, int W>
void recode_w(const uint32_t* scalar, uint32_t* mags, int32_t* dig, int32_t* info) {
  alignas(16) uint32_t src[8];
  memcpy(src, scalar, sizeof src);
  uint32_t r0[5], r1[5];
  bool sign[2];
  pmul::split_recode<CV, W>(r0, r1, sign, src);
  uint32_t s[8], q[8];
  for (int j = 0; j < 8; j++) q[j] = CV::G::Q[j];
  pmul::scalar_mod_q<16>(s, src, q);
  GlvHalf h0, h1;
  glv_decompose<typename CV::G>(h0, h1, s);
  for (int j = 0; j < 4; j++) { mags[j] = h0.mag[j]; mags[4 + j] = h1.mag[j]; }
  const int nwin = pmul::windows(CV::G::MAX_BITS, W);
  info[0] = nwin;
  info[1] = sign[0];
  info[2] = sign[1];
  digits_of<5, W>(r0, nwin, dig, &info[3]);
  digits_of<5, W>(r1, nwin, dig + MAX_WIN, &info[4]);
}

// Edwards: mags = the scalar mod q (8 words), one chain
template <int W>
void recode_te(const uint32_t* scalar, uint32_t* mags, int32_t* dig, int32_t* info) {
  alignas(16) uint32_t src[8];
  memcpy(src, scalar, sizeof src);
  uint32_t r[pmul::TE_NX], s[8], q[8];
  pmul::te_recode<W>(r, src);
  for (int j = 0; j < 8; j++) q[j] = FRED_Q[j];
  pmul::scalar_mod_q<56>(s, src, q);
  for (int j = 0; j < 8; j++) mags[j] = s[j];
  const int nwin = pmul::windows(pmul::TE_BITS, W);
  info[0] = nwin;
  info[1] = info[2] = info[4] = 0;
  digits_of<pmul::TE_NX, W>(r, nwin, dig, &info[3]);
  for (int k = 0; k < MAX_WIN; k++) dig[MAX_WIN + k] = 0;
}

template <class CV, int W>
void lane_w(const uint32_t* row_in, const uint32_t* scalar, uint4* tbl, uint64_t cap, uint64_t g, uint32_t* row_out) {
  alignas(16) uint32_t row[ROW_WORDS], out[ROW_WORDS] = {0}, s[8];
  memcpy(row, row_in, sizeof row);
  memcpy(s, scalar, sizeof s);
  pmul::mul_lane<CV, W>(out, row, s, tbl, cap, g);
  memcpy(row_out, out, sizeof out);
}
template <int W>
void lane_te(const uint32_t* row_in, const uint32_t* scalar, uint4* tbl, uint64_t cap, uint64_t g, uint32_t* row_out) {
  alignas(16) uint32_t row[te::TE_ROW_WORDS], out[te::TE_ROW_WORDS] = {0}, s[8];
  memcpy(row, row_in, sizeof row);
  memcpy(s, scalar, sizeof s);
  pmul::te_mul_lane<W>(out, row, s, tbl, cap, g);
  memcpy(row_out, out, sizeof out);
}

template <class CV, int W>
void base_lane_w(const uint32_t* scalar, const uint32_t* table, uint32_t* row_out) {
  alignas(16) uint32_t out[ROW_WORDS] = {0}, s[8];
  memcpy(s, scalar, sizeof s);
  pmul::base_lane<CV, W>(out, s, table);
  memcpy(row_out, out, sizeof out);
}
template <int W>
void base_lane_te(const uint32_t* scalar, const uint32_t* table, uint32_t* row_out) {
  alignas(16) uint32_t out[te::TE_ROW_WORDS] = {0}, s[8];
  memcpy(s, scalar, sizeof s);
  pmul::te_base_lane<W>(out, s, table);
  memcpy(row_out, out, sizeof out);
}

}  // namespace

// X(curve id of include/msm_hip.h, configuration)
#define PM_W_CURVES(X) X(0, CvBls377) X(2, CvBls381) X(3, CvPallas) X(4, CvBn254) X(5, CvGrumpkin) X(6, CvVesta)
// every candidate window, variable base and fixed base
#define PM_WIDTHS(X, ...) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__) X(10, __VA_ARGS__)

extern "C" {

int pm_max_win(void) { return MAX_WIN; }
int pm_built_w(void) { return pmul::W_VAR; }
int pm_built_wb(void) { return pmul::W_BASE; }
int pm_row_words(int curve) { return curve == 1 ? te::TE_ROW_WORDS : ROW_WORDS; }
int pm_coord_words(int curve) {
  switch (curve) {
#define PM_CASE(ID, CV) case ID: return CV::F::NW;
    PM_W_CURVES(PM_CASE)
#undef PM_CASE
    case 1: return te::TW;
  }
  return -1;
}
// bits a chain covers: MAX_BITS of the curve's GLV halves (Edwards: the bits of q)
int pm_chain_bits(int curve) {
  switch (curve) {
#define PM_CASE(ID, CV) case ID: return CV::G::MAX_BITS;
    PM_W_CURVES(PM_CASE)
#undef PM_CASE
    case 1: return pmul::TE_BITS;
  }
  return -1;
}
// uint4 elements of the table of `cap` lanes at window w
uint64_t pm_table_elems(int curve, int w, uint64_t cap) {
  const int nw = pm_coord_words(curve);
  return nw < 0 ? 0 : ((uint64_t)1 << (w - 1)) * pmul::TBL_COORDS * (uint64_t)(nw / 4) * cap;
}

// the recoding of one scalar (8 words): see recode_w / recode_te
int pm_recode(int curve, int w, const uint32_t* scalar, uint32_t* mags, int32_t* dig, int32_t* info) {
#define PM_WCASE(W, ID, CV) if (curve == ID && w == W) { recode_w<CV, W>(scalar, mags, dig, info); return 0; }
#define PM_CASE(ID, CV) PM_WIDTHS(PM_WCASE, ID, CV)
  PM_W_CURVES(PM_CASE)
#undef PM_CASE
#undef PM_WCASE
#define PM_WCASE(W, ...) if (curve == 1 && w == W) { recode_te<W>(scalar, mags, dig, info); return 0; }
  PM_WIDTHS(PM_WCASE)
#undef PM_WCASE
  return -1;
}

// affine (x, y) as plain little-endian words (NULL: the generator; all zero: the identity) -> the resident row; returns what
// base_row returns (1: a coordinate >= p, 2: off the curve)
int pm_make_row(int curve, const uint32_t* xy, uint32_t* row_out) {
  switch (curve) {
#define PM_CASE(ID, CV) case ID: return pmul::base_row<CV>(row_out, xy);
    PM_W_CURVES(PM_CASE)
#undef PM_CASE
    case 1: return pmul::te_base_row(row_out, xy);
  }
  return -1;
}

// one variable-base lane: row_out = scalar * row, over the slots of lane g of the caller's table.  Every curve at the built
// window; BLS12-377 and the Edwards curve at all three candidates (each instantiation is a large function)
int pm_lane(int curve, int w, const uint32_t* row, const uint32_t* scalar, void* tbl, uint64_t cap, uint64_t g, uint32_t* row_out) {
  if (g >= cap) return -1;
#define PM_WCASE(W, ID, CV) if (curve == ID && w == W) { lane_w<CV, W>(row, scalar, (uint4*)tbl, cap, g, row_out); return 0; }
#define PM_CASE(ID, CV) PM_WCASE(pmul::W_VAR, ID, CV)
  PM_W_CURVES(PM_CASE)
#undef PM_CASE
  PM_WCASE(3, 0, CvBls377) PM_WCASE(4, 0, CvBls377) PM_WCASE(5, 0, CvBls377)
#undef PM_WCASE
#define PM_WCASE(W) if (curve == 1 && w == W) { lane_te<W>(row, scalar, (uint4*)tbl, cap, g, row_out); return 0; }
  PM_WCASE(3) PM_WCASE(4) PM_WCASE(5)
#undef PM_WCASE
  return -1;
}

// rows of the fixed-base table at window w
int pm_base_table_rows(int curve, int w) {
  const int bits = pm_chain_bits(curve);
  return bits < 0 ? -1 : pmul::windows(bits, w) << (w - 1);
}
// the table of one base row, the way the library builds it: the variable-base body (at the built window) over the scalars
// j 2^(w k)
int pm_base_table(int curve, int w, const uint32_t* base_row, uint32_t* table_out) {
  const int rows = pm_base_table_rows(curve, w), rw = pm_row_words(curve);
  if (rows < 0) return -1;
  std::vector<uint32_t> sc((size_t)rows * 8);
  pmul::table_scalars(sc.data(), w, rows >> (w - 1));
  std::vector<uint4> tbl(pm_table_elems(curve, pmul::W_VAR, 1));
  for (int i = 0; i < rows; i++)
    if (pm_lane(curve, pmul::W_VAR, base_row, &sc[(size_t)i * 8], tbl.data(), 1, 0, table_out + (size_t)i * rw)) return -1;
  return 0;
}
// one fixed-base lane: every curve at the built window; BLS12-377 and the Edwards curve at all three candidates
int pm_base_lane(int curve, int w, const uint32_t* scalar, const uint32_t* table, uint32_t* row_out) {
#define PM_WCASE(W, ID, CV) if (curve == ID && w == W) { base_lane_w<CV, W>(scalar, table, row_out); return 0; }
#define PM_CASE(ID, CV) PM_WCASE(pmul::W_BASE, ID, CV)
  PM_W_CURVES(PM_CASE)
#undef PM_CASE
  PM_WCASE(6, 0, CvBls377) PM_WCASE(8, 0, CvBls377) PM_WCASE(10, 0, CvBls377)
#undef PM_WCASE
#define PM_WCASE(W) if (curve == 1 && w == W) { base_lane_te<W>(scalar, table, row_out); return 0; }
  PM_WCASE(6) PM_WCASE(8) PM_WCASE(10)
#undef PM_WCASE
  return -1;
}
}
