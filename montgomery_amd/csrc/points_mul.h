// Per-row scalar multiplication of resident points (msm_points_mul, msm_points_mul_base; msm_points_mul.hip): D[i] = s[i] * A[i]
// and D[i] = s[i] * P, every row under its OWN scalar.  msm_points_lincomb (points_lincomb.h) is wave-uniform because all lanes
// walk one program; here the scalars differ per lane, so control flow is made uniform another way: a FIXED number of signed
// windows and a table indexed by the lane's digit.  The reference has no counterpart.
//
// Recoding.  A magnitude m below 2^bits is cut into NWIN = ceil((bits + 1) / w) windows of w bits with the carry rule of
// window_step (msm_kernels.h): a window value above L = 2^(w-1) becomes its complement to 2 L with a carry into the next window,
// digits in [-(L - 1), L].  Adding the constant BIAS = (L - 1) * sum_k 2^(w k) to m ONCE does all carries at once: window k of
// m + BIAS holds (l_k + L - 1) mod 2 L, and it wraps exactly when l_k = raw_k + carry_k exceeds L, so
//     digit_k = bits [w k, w k + w) of (m + BIAS) - (L - 1)
// with no state between windows: the walk extracts digit k at a wave-uniform bit position, top window first.  m + BIAS stays
// below 2^(w NWIN), the top carry is always 0 (m < 2^bits <= 2^(w NWIN - 1), BIAS < 2^(w NWIN - 1)).
//
// Variable base (mul_lane, te_mul_lane).  Per lane: the scalar mod q, glv_decompose on the Weierstrass curves, both halves
// recoded; a table T[j] = j P, j = 1 .. L, in device memory (entry e, coordinate c, 16-byte piece p of lane g at
// tbl[((e * 4 + c) * NP + p) * cap + g]: the lanes of a wave reading one entry touch neighbouring addresses); then from the top
// window w doublings, acc +- T[|d0|], acc +- phi(T[|d1|]) (phi = one multiplication of x by beta).  Weierstrass entries are
// made affine with one inversion per lane (Montgomery's trick over Z_2 .. Z_L, the prefix products kept in coordinate 3 of the
// entries), so the walk uses mixed additions; Edwards entries stay extended (the unified addition is complete and 9 M either way).
// A zero digit goes through the addition's identity flag.  The kernel runs on a fixed grid with a grid-stride loop, so the
// table is sized by the grid; a lane rebuilds its slots for every row it takes.
//
// Fixed base (base_lane, te_base_lane).  One shared table of resident ROWS, T[k][j] = j 2^(w_b k) P, built by the variable-base
// kernel itself over a broadcast base row.  A lane adds +-T[k][|d0|] (first line of the row) and +-phi(T[k][|d1|]) (its beta x
// line) for every window k: no doubling, one inversion at the end.
//
// Everything here is __host__ __device__, so the recoding and all four lane bodies run on the CPU in tests/csrc/points_mul_host.hip.
#pragma once
#include "te_kernels.h"

#ifndef MSM_PMUL_W
#define MSM_PMUL_W 4    // window of the variable-base walk
#endif
#ifndef MSM_PMUL_WB
#define MSM_PMUL_WB 10  // window of the fixed-base table
#endif
#ifndef MSM_PMUL_PROJ
#define MSM_PMUL_PROJ 0   // 1: the per-lane table entries of the Weierstrass curves stay projective (no inversion, full additions)
#endif

namespace msm {
namespace pmul {

constexpr int W_VAR = MSM_PMUL_W, W_BASE = MSM_PMUL_WB;
constexpr bool PROJ_ENTRIES = MSM_PMUL_PROJ != 0;
constexpr int TE_BITS = 251;    // bit length of the Edwards curve's group order
constexpr int TBL_COORDS = 4;   // coordinates an entry of the per-lane table has room for
constexpr int BLOCK = 256;

constexpr int windows(int bits, int w) { return (bits + w) / w; }   // ceil((bits + 1) / w)
constexpr int words_for(int bits) { return (bits + 31) / 32; }

// word j of BIAS = (2^(w-1) - 1) * sum_{k < nwin} 2^(w k)   (windows do not overlap: an OR of shifted copies)
constexpr uint32_t bias_word(int w, int nwin, int j) {
  const uint64_t v = (1ull << (w - 1)) - 1ull;
  uint32_t out = 0;
  for (int k = 0; k < nwin; k++) {
    const int lo = w * k - 32 * j;
    if (lo >= 32 || lo + w <= 0) continue;
    out |= lo >= 0 ? (uint32_t)(v << lo) : (uint32_t)(v >> -lo);
  }
  return out;
}

// r = mag (NM words) + BIAS over NX words, 32 NX >= w NWIN
template <int NX, int NM, int W, int NWIN>
MSM_DEV void recode(uint32_t (&r)[NX], const uint32_t* mag) {
  static_assert(32 * NX >= W * NWIN, "the recoded value must fit");
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < NX; j++) {
    c += (uint64_t)(j < NM ? mag[j] : 0u) + bias_word(W, NWIN, j);
    r[j] = (uint32_t)c;
    c >>= 32;
  }
}

// signed digit k of a recoded value: |d| <= 2^(W-1)
template <int NX, int W>
MSM_DEV void digit(const uint32_t (&r)[NX], int k, uint32_t& mag, bool& neg) {
  const int d = (int)bn_bits<NX>(r, W * k, W) - ((1 << (W - 1)) - 1);
  neg = d < 0;
  mag = (uint32_t)(neg ? -d : d);
}

// the scalar at src mod q (msm_run's rule without `strict`: load_scalar_mod_q, msm_kernels.h)
template <int MAX_SUB>
MSM_DEV void scalar_mod_q(uint32_t (&s)[8], const uint32_t* src, const uint32_t (&q)[8]) {
  load_words12<8>(s, src);
  for (int it = 0; it < MAX_SUB && words8_ge(s, q); it++) bn_addsub<8, 8>(s, q, true);
}

// y <- -y where neg (a select, no branch); y < 2p in and out
template <class F>
MSM_DEV void fe_neg_if(Fe<F>& y, bool neg) {
  Fe<F> z, n;
  fe_set_zero<F>(z);
  fe_sub_2p<F>(n, z, y);    // (0, 2p]
  fe_reduce_2p<F>(n);       // [0, p]
  const uint32_t m = neg ? 0xFFFFFFFFu : 0u;   // (a mask, not a conditional expression: the limbs stay values in registers)
#pragma unroll
  for (int l = 0; l < F::NL; l++) y.l[l] = (n.l[l] & m) | (y.l[l] & ~m);
}

template <class F>
MSM_DEV void load_fe(Fe<F>& r, const uint32_t* p) {
  uint32_t w[F::NW];
  load_words12(w, p);
  fe_unpack<F>(r, w);
}

// ---------------------------------------------------------------------------------------------
// Weierstrass curves
// ---------------------------------------------------------------------------------------------

template <class F>
MSM_DEV void tbl_load(Fe<F>& r, const uint4* tbl, uint64_t cap, uint64_t g, uint32_t e, int coord) {
  uint32_t w[F::NW];
  load_planes3(w, tbl, cap, (int)(e * TBL_COORDS + coord) * (F::NW / 4), g);
  fe_unpack<F>(r, w);
}
template <class F>
MSM_DEV void tbl_store(uint4* tbl, uint64_t cap, uint64_t g, uint32_t e, int coord, const Fe<F>& v) {
  uint32_t w[F::NW];
  fe_pack<F>(w, v);
  store_planes3(tbl, cap, (int)(e * TBL_COORDS + coord) * (F::NW / 4), g, w);
}

// entries 0 .. L - 1 = 1 P .. L P, affine (x, y) in coordinates 0 and 1; P = (px, py) is not the identity.  Entry j >= 1 is kept
// projective first (X, Y, Z and the prefix product c_j = Z_1 .. Z_j), then one inversion of c_(L-1) makes them all affine.
// A point outside the prime-order subgroup whose multiple is the identity (Z = 0) gets garbage, never a fault: c = 0 inverts to 0.
template <class F, int W>
MSM_DEV void table_build(uint4* tbl, uint64_t cap, uint64_t g, const Fe<F>& px, const Fe<F>& py) {
  constexpr uint32_t L = 1u << (W - 1);
  tbl_store<F>(tbl, cap, g, 0, 0, px);
  tbl_store<F>(tbl, cap, g, 0, 1, py);
  Proj<F> P, acc;
  P.X = px;
  P.Y = py;
  fe_set_one<F>(P.Z);
  if (PROJ_ENTRIES) tbl_store<F>(tbl, cap, g, 0, 2, P.Z);
  proj_double<F>(acc, P);
  Fe<F> c = acc.Z;
#pragma unroll 1
  for (uint32_t e = 1; e < L; e++) {
    if (e > 1) {
      proj_add_mixed<F>(acc, acc, P, false);
      fe_mul<F>(c, c, acc.Z);
    }
    tbl_store<F>(tbl, cap, g, e, 0, acc.X);
    tbl_store<F>(tbl, cap, g, e, 1, acc.Y);
    tbl_store<F>(tbl, cap, g, e, 2, acc.Z);
    tbl_store<F>(tbl, cap, g, e, 3, c);
  }
  if (PROJ_ENTRIES) return;
  Fe<F> inv, zi, z, v;
  fe_reduce_4p<F>(c);
  fe_inv<F>(inv, c);   // 1 / (Z_1 .. Z_(L-1))
#pragma unroll 1
  for (uint32_t e = L - 1; e >= 1; e--) {
    if (e > 1) {
      tbl_load<F>(v, tbl, cap, g, e - 1, 3);
      fe_mul<F>(zi, inv, v);   // 1 / Z_e
      tbl_load<F>(z, tbl, cap, g, e, 2);
      fe_mul<F>(inv, inv, z);  // 1 / (Z_1 .. Z_(e-1))
    } else {
      zi = inv;
    }
    tbl_load<F>(v, tbl, cap, g, e, 0);
    fe_mul<F>(v, v, zi);
    tbl_store<F>(tbl, cap, g, e, 0, v);
    tbl_load<F>(v, tbl, cap, g, e, 1);
    fe_mul<F>(v, v, zi);
    tbl_store<F>(tbl, cap, g, e, 1, v);
  }
}

// to affine and the row of msm_set_points, as lincomb_lane (points_lincomb.h) ends
template <class F>
MSM_DEV void finish_row(uint32_t* out, Proj<F>& acc) {
  if (proj_is_zero<F>(acc)) {
    store_row_identity<F::NW / 4>(out);
    return;
  }
  Fe<F> zi, x, y, bx, beta;
  fe_reduce_4p<F>(acc.Z);
  fe_inv<F>(zi, acc.Z);
  fe_mul<F>(x, acc.X, zi);
  fe_reduce_2p<F>(x);
  fe_mul<F>(y, acc.Y, zi);
  fe_reduce_2p<F>(y);
#pragma unroll
  for (int l = 0; l < F::NL; l++) beta.l[l] = F::BETAL[l];
  fe_mul<F>(bx, x, beta);
  fe_reduce_2p<F>(bx);
  store_row(out, x, y, bx);
}

// the two recoded GLV halves of the scalar at src; sign[e] = the half is negative
template <class CV, int W>
MSM_DEV void split_recode(uint32_t (&r0)[5], uint32_t (&r1)[5], bool (&sign)[2], const uint32_t* src) {
  using G = typename CV::G;
  constexpr int NWIN = windows(G::MAX_BITS, W);
  uint32_t s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; j++) q[j] = G::Q[j];   // (value use only: the constant tables have no device address)
  scalar_mod_q<16>(s, src, q);
  GlvHalf h0, h1;
  glv_decompose<G>(h0, h1, s);
  recode<5, 4, W, NWIN>(r0, h0.mag);
  recode<5, 4, W, NWIN>(r1, h1.mag);
  sign[0] = h0.neg;
  sign[1] = h1.neg;
}

// out = s * (row), s = the 32-byte scalar at `scalar`.  `out` may be `row`: the row and the scalar are read before the one store.
// tbl, cap, g: the lane's table slots (see the head of this file).
template <class CV, int W>
MSM_DEV void mul_lane(uint32_t* out, const uint32_t* row, const uint32_t* scalar, uint4* tbl, uint64_t cap, uint64_t g) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  constexpr int NWIN = windows(CV::G::MAX_BITS, W);
  uint32_t r0[5], r1[5];
  bool sign[2];
  split_recode<CV, W>(r0, r1, sign, scalar);
  const bool inf = row[NW - 1] == INF_WORD;
  if (!inf) {
    Fe<F> px, py;
    load_fe<F>(px, row);
    load_fe<F>(py, row + NW);
    table_build<F, W>(tbl, cap, g, px, py);
  }
  Fe<F> beta;
#pragma unroll
  for (int l = 0; l < NL; l++) beta.l[l] = F::BETAL[l];
  Proj<F> acc;
  proj_set_zero<F>(acc);
#pragma unroll 1
  for (int k = NWIN - 1; k >= 0; k--) {
    if (k != NWIN - 1) {
#pragma unroll 1
      for (int j = 0; j < W; j++) proj_double<F>(acc, acc);
    }
#pragma unroll 1
    for (int e = 0; e < 2; e++) {
      uint32_t mag;
      bool neg;
      if (e == 0) digit<5, W>(r0, k, mag, neg);
      else digit<5, W>(r1, k, mag, neg);
      const uint32_t slot = mag ? mag - 1 : 0;
      Proj<F> Q;
      tbl_load<F>(Q.X, tbl, cap, g, slot, 0);
      tbl_load<F>(Q.Y, tbl, cap, g, slot, 1);
      if (e == 1) fe_mul<F>(Q.X, Q.X, beta);   // phi(x, y) = (beta x, y)
      fe_neg_if<F>(Q.Y, neg != sign[e]);
      if (PROJ_ENTRIES) {
        tbl_load<F>(Q.Z, tbl, cap, g, slot, 2);
        proj_add_impl<F, false>(acc, acc, Q, inf || mag == 0);
      } else {
        Q.Z = Q.X;   // (ignored by the mixed addition)
        proj_add_mixed<F>(acc, acc, Q, inf || mag == 0);
      }
    }
  }
  finish_row<F>(out, acc);
}

// out = s * P over the shared table of rows T[k][j - 1] = j 2^(W k) P
template <class CV, int W>
MSM_DEV void base_lane(uint32_t* out, const uint32_t* scalar, const uint32_t* table) {
  using F = typename CV::F;
  constexpr int NW = F::NW;
  constexpr int NWIN = windows(CV::G::MAX_BITS, W);
  constexpr uint32_t L = 1u << (W - 1);
  uint32_t r0[5], r1[5];
  bool sign[2];
  split_recode<CV, W>(r0, r1, sign, scalar);
  Proj<F> acc;
  proj_set_zero<F>(acc);
#pragma unroll 1
  for (int k = 0; k < NWIN; k++) {
#pragma unroll 1
    for (int e = 0; e < 2; e++) {
      uint32_t mag;
      bool neg;
      if (e == 0) digit<5, W>(r0, k, mag, neg);
      else digit<5, W>(r1, k, mag, neg);
      const uint32_t* line = table + ((uint64_t)k * L + (mag ? mag - 1 : 0)) * ROW_WORDS + (e ? ROW_HALF : 0);
      Proj<F> Q;
      load_fe<F>(Q.X, line);
      load_fe<F>(Q.Y, line + NW);
      const bool inf = line[NW - 1] == INF_WORD;
      fe_neg_if<F>(Q.Y, neg != sign[e]);
      Q.Z = Q.X;
      proj_add_mixed<F>(acc, acc, Q, inf || mag == 0);
    }
  }
  finish_row<F>(out, acc);
}

// ---------------------------------------------------------------------------------------------
// Ed-on-BLS12-377: no endomorphism, one chain over the whole scalar; unified additions, the identity is the point (0, 1)
// ---------------------------------------------------------------------------------------------

constexpr int TE_NX = 9;   // words of a recoded scalar: w NWIN <= 260 bits at w = 10

template <int W>
MSM_DEV void te_recode(uint32_t (&r)[TE_NX], const uint32_t* src) {
  uint32_t s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; j++) q[j] = FRED_Q[j];
  scalar_mod_q<56>(s, src, q);
  recode<TE_NX, 8, W, windows(TE_BITS, W)>(r, s);
}

MSM_DEV void te_neg_select(te::Ext& Q, bool neg, bool zero) {
  using te::FT;
  Fe<FT> z, nx, nt, one;
  fe_set_zero<FT>(z);
  fe_set_one<FT>(one);
  fe_sub_2p<FT>(nx, z, Q.X);
  fe_sub_2p<FT>(nt, z, Q.T);
  // masks, not conditional expressions over the limbs: every limb stays a value in a register
  const uint32_t mz = zero ? 0xFFFFFFFFu : 0u, mn = neg ? 0xFFFFFFFFu : 0u;
#pragma unroll
  for (int l = 0; l < te::TL; l++) {
    Q.X.l[l] = ((nx.l[l] & mn) | (Q.X.l[l] & ~mn)) & ~mz;
    Q.T.l[l] = ((nt.l[l] & mn) | (Q.T.l[l] & ~mn)) & ~mz;
    Q.Y.l[l] = (one.l[l] & mz) | (Q.Y.l[l] & ~mz);
    Q.Z.l[l] = (one.l[l] & mz) | (Q.Z.l[l] & ~mz);
  }
}

// as te_lincomb_lane (points_lincomb.h) ends
MSM_DEV void te_finish_row(uint32_t* out, te::Ext& acc) {
  using te::FT;
  using te::TL;
  Fe<FT> zi, x, y, t, kt, kk;
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

// table entry e of lane g: an extended point, TBL_COORDS coordinates of two pieces each
template <int W>
MSM_DEV void te_mul_lane(uint32_t* out, const uint32_t* row, const uint32_t* scalar, uint4* tbl, uint64_t cap, uint64_t g) {
  using te::FT;
  constexpr int NWIN = windows(TE_BITS, W);
  constexpr uint32_t L = 1u << (W - 1);
  constexpr uint64_t PLANES = TBL_COORDS * 2;
  uint32_t r[TE_NX];
  te_recode<W>(r, scalar);
  te::Ext P, acc;
  load_fe<FT>(P.X, row);
  load_fe<FT>(P.Y, row + 8);
  load_fe<FT>(P.T, row + 16);
  fe_set_one<FT>(P.Z);
  acc = P;
  te::store_ext(tbl, cap, g, acc);
#pragma unroll 1
  for (uint32_t e = 1; e < L; e++) {
    te::te_add(acc, acc, P);
    te::store_ext(tbl + e * PLANES * cap, cap, g, acc);
  }
  te::te_set_identity(acc);
#pragma unroll 1
  for (int k = NWIN - 1; k >= 0; k--) {
    if (k != NWIN - 1) {
#pragma unroll 1
      for (int j = 0; j < W; j++) te::te_add(acc, acc, acc);
    }
    uint32_t mag;
    bool neg;
    digit<TE_NX, W>(r, k, mag, neg);
    te::Ext Q;
    te::load_ext(Q, tbl + (mag ? mag - 1 : 0) * PLANES * cap, cap, g);
    te_neg_select(Q, neg, mag == 0);
    te::te_add(acc, acc, Q);
  }
  te_finish_row(out, acc);
}

template <int W>
MSM_DEV void te_base_lane(uint32_t* out, const uint32_t* scalar, const uint32_t* table) {
  using te::FT;
  constexpr int NWIN = windows(TE_BITS, W);
  constexpr uint32_t L = 1u << (W - 1);
  uint32_t r[TE_NX];
  te_recode<W>(r, scalar);
  te::Ext acc;
  te::te_set_identity(acc);
#pragma unroll 1
  for (int k = 0; k < NWIN; k++) {
    uint32_t mag;
    bool neg;
    digit<TE_NX, W>(r, k, mag, neg);
    const uint32_t* row = table + ((uint64_t)k * L + (mag ? mag - 1 : 0)) * te::TE_ROW_WORDS;
    te::Ext Q;
    load_fe<FT>(Q.X, row);
    load_fe<FT>(Q.Y, row + 8);
    load_fe<FT>(Q.T, row + 16);
    fe_set_one<FT>(Q.Z);
    te_neg_select(Q, neg, mag == 0);
    te::te_add(acc, acc, Q);
  }
  te_finish_row(out, acc);
}

// ---------------------------------------------------------------------------------------------
// The base of msm_points_mul_base as a resident row, made on the host the way k_points_from_wire / k_te_points_from_wire make
// rows.  xy = x || y as plain little-endian words (NULL: the curve's generator).  Returns 0, 1 (a coordinate >= p) or 2 (not
// on the curve); the all-zero encoding is the identity.
// ---------------------------------------------------------------------------------------------

template <class CV>
inline int base_row(uint32_t* row_out, const uint32_t* xy) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  alignas(16) uint32_t row[ROW_WORDS] = {0};
  uint32_t xw[NW], yw[NW], any = 0;
  for (int j = 0; j < NW; j++) {
    xw[j] = xy ? xy[j] : F::GXW[j];
    yw[j] = xy ? xy[NW + j] : F::GYW[j];
    any |= xw[j] | yw[j];
  }
  if (!any) {
    store_row_identity<NW / 4>(row);
  } else {
    Fe<F> x, y, r2, beta, bx, lhs, rhs, bb;
    fe_unpack<F>(x, xw);
    fe_unpack<F>(y, yw);
    if (xy) {   // (the generator constants are in Montgomery form already)
      if (words_ge_p<F>(xw) || words_ge_p<F>(yw)) return 1;
      for (int l = 0; l < NL; l++) r2.l[l] = F::R2[l];
      fe_mul<F>(x, x, r2);
      fe_reduce_2p<F>(x);
      fe_mul<F>(y, y, r2);
      fe_reduce_2p<F>(y);
    }
    for (int l = 0; l < NL; l++) { beta.l[l] = F::BETAL[l]; bb.l[l] = F::BL[l]; }
    fe_mul<F>(bx, x, beta);
    fe_reduce_2p<F>(bx);
    fe_sqr<F>(lhs, y);
    fe_sqr<F>(rhs, x);
    fe_mul<F>(rhs, rhs, x);
    fe_add<F>(rhs, rhs, bb);
    fe_sub_4p<F>(lhs, lhs, rhs);
    fe_cond_sub<F, 4>(lhs);
    if (!fe_is_zero_mod_p<F>(lhs)) return 2;
    store_row(row, x, y, bx);
  }
  for (int j = 0; j < ROW_WORDS; j++) row_out[j] = row[j];
  return 0;
}

inline int te_base_row(uint32_t* row_out, const uint32_t* xy) {
  using te::FT;
  using te::TL;
  using te::TW;
  alignas(16) uint32_t row[te::TE_ROW_WORDS];
  uint32_t xw[TW], yw[TW], any = 0;
  for (int j = 0; j < TW; j++) {
    xw[j] = xy ? xy[j] : FT::GXW[j];
    yw[j] = xy ? xy[TW + j] : FT::GYW[j];
    any |= xw[j] | yw[j];
  }
  Fe<FT> x, y, t, kt, r2, k;
  if (!any) {
    fe_set_zero<FT>(x);
    fe_set_one<FT>(y);
  } else {
    fe_unpack<FT>(x, xw);
    fe_unpack<FT>(y, yw);
    if (xy) {
      if (te::words8_ge_p(xw) || te::words8_ge_p(yw)) return 1;
      TE_CONST(r2, R2);
      fe_mul<FT>(x, x, r2);
      fe_mul<FT>(y, y, r2);
    }
  }
  TE_CONST(k, K2DL);
  fe_mul<FT>(t, x, y);
  fe_mul<FT>(kt, t, k);
  {
    Fe<FT> xx, yy, lhs, rhs, dd, one;
    fe_sqr<FT>(xx, x);
    fe_sqr<FT>(yy, y);
    fe_sub_2p<FT>(lhs, yy, xx);
    TE_CONST(dd, DL);
    fe_sqr<FT>(rhs, t);
    fe_mul<FT>(rhs, rhs, dd);
    fe_set_one<FT>(one);
    fe_add<FT>(rhs, rhs, one);
    fe_sub_4p<FT>(lhs, lhs, rhs);
    fe_cond_sub<FT, 4>(lhs);
    fe_reduce_4p<FT>(lhs);
    if (!fe_is_zero_canonical<FT>(lhs)) return 2;
  }
  fe_reduce_2p<FT>(x);
  fe_reduce_2p<FT>(y);
  fe_reduce_2p<FT>(t);
  fe_reduce_2p<FT>(kt);
  fe_store<FT>(row, x);
  fe_store<FT>(row + 8, y);
  fe_store<FT>(row + 16, t);
  fe_store<FT>(row + 24, kt);
  for (int j = 0; j < te::TE_ROW_WORDS; j++) row_out[j] = row[j];
  return 0;
}

// the scalars the table of the fixed base is built from: entry (k, j - 1) = j 2^(w k), 8 words each.  Where w nwin exceeds 256
// (the Edwards curve at w = 10: 26 windows) the large j of the top window do not fit and are cut at 2^256; no digit reaches
// them, the top window of a scalar below 2^251 holds bit 250 and a carry
inline void table_scalars(uint32_t* out, int w, int nwin) {
  const uint32_t L = 1u << (w - 1);
  for (int k = 0; k < nwin; k++)
    for (uint32_t j = 1; j <= L; j++) {
      uint32_t* s = out + ((size_t)k * L + (j - 1)) * 8;
      for (int i = 0; i < 8; i++) s[i] = 0;
      const int bit = w * k;
      const uint64_t v = (uint64_t)j << (bit % 32);
      if (bit / 32 < 8) s[bit / 32] = (uint32_t)v;
      if (bit / 32 + 1 < 8) s[bit / 32 + 1] = (uint32_t)(v >> 32);
    }
}

// ---------------------------------------------------------------------------------------------
// kernels: a fixed grid, lane g takes the rows g, g + cap, ... (cap = all lanes of the grid); row_stride = 0 broadcasts one row
// ---------------------------------------------------------------------------------------------

// The plane stride of the table as a PER-LANE value: as a uniform one the compiler keeps the scalar address of every plane of
// the table across the row loop and runs out of scalar registers (16 to 37 of them went to vector lanes and back)
__device__ __forceinline__ uint64_t lane_value(uint64_t cap) {
  uint32_t v = (uint32_t)cap;   // (a grid has at most 2^16 blocks of 256 lanes)
  asm volatile("" : "+v"(v));
  return v;
}

template <class CV>
__global__ void __launch_bounds__(BLOCK) k_points_mul(uint32_t* dst, const uint32_t* rows, uint32_t row_stride, const uint32_t* scalars,
                                                      uint64_t count, uint4* tbl) {
  const uint64_t cap = (uint64_t)gridDim.x * BLOCK, g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
#pragma unroll 1
  for (uint64_t i = g; i < count; i += cap)
    mul_lane<CV, W_VAR>(dst + i * ROW_WORDS, rows + i * row_stride, scalars + i * 8, tbl, lane_value(cap), g);
}

// (the two kernels that are no templates have their one definition in msm_points_mul.hip: a second translation unit of the
// library that wants the lane bodies defines MSM_PMUL_DECLARE_TE and gets declarations)
__global__ void __launch_bounds__(BLOCK) k_te_points_mul(uint32_t* dst, const uint32_t* rows, uint32_t row_stride, const uint32_t* scalars,
                                                         uint64_t count, uint4* tbl)
#ifdef MSM_PMUL_DECLARE_TE
    ;
#else
{
  const uint64_t cap = (uint64_t)gridDim.x * BLOCK, g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
#pragma unroll 1
  for (uint64_t i = g; i < count; i += cap)
    te_mul_lane<W_VAR>(dst + i * te::TE_ROW_WORDS, rows + i * row_stride, scalars + i * 8, tbl, lane_value(cap), g);
}
#endif

template <class CV>
__global__ void __launch_bounds__(BLOCK) k_points_mul_base(uint32_t* dst, const uint32_t* scalars, uint64_t count, const uint32_t* table) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= count) return;
  base_lane<CV, W_BASE>(dst + i * ROW_WORDS, scalars + i * 8, table);
}

__global__ void __launch_bounds__(BLOCK) k_te_points_mul_base(uint32_t* dst, const uint32_t* scalars, uint64_t count, const uint32_t* table)
#ifdef MSM_PMUL_DECLARE_TE
    ;
#else
{
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= count) return;
  te_base_lane<W_BASE>(dst + i * te::TE_ROW_WORDS, scalars + i * 8, table);
}
#endif

// bytes of the per-lane tables of a grid of `blocks` blocks
inline uint64_t table_bytes(bool te, int nw, uint64_t blocks) {
  const uint64_t per_entry = te ? (uint64_t)TBL_COORDS * 32 : (uint64_t)TBL_COORDS * nw * 4;
  return blocks * BLOCK * (1ull << (W_VAR - 1)) * per_entry;
}

}  // namespace pmul
}  // namespace msm
