// The number-theoretic transform over resident POINTS (msm_points_ntt; msm_points_ntt.hip): D[k] = sum_j (shift omega^k)^j A[j]
// over the rows of a point set, and its inverse -- the monomial commitment key [tau^j] G becomes the Lagrange key [L_k(tau)] G
// without tau and without the points leaving the device.  The reference has no counterpart.
//
// Plan.  Radix 2, decimation in time, in place in the destination rows: the rows are put into bit-reversed order (an out-of-place
// gather, or pairwise swaps when the source rows are the destination rows), then stage s = 1 .. log2n, one launch each, runs the
// n / 2 butterflies (A, B) -> (A + w B, A - w B) of its blocks of m = 2^s rows; w = omega^(j n / m) for the butterfly at position
// j < m / 2 of its block, read from the vector omega^0 .. omega^(n/2 - 1) at stride n / m.
//
// Lane mapping.  Lane t < n / 2 of stage s takes position j = t / (n / m) of block t mod (n / m): consecutive lanes are the SAME
// position of consecutive blocks, so the lanes of a wave share their twiddle wherever n / m >= 64, and the butterflies of position
// 0 -- w = 1, n / m of them per stage -- leave out the scalar multiplication as whole waves.  Stage 1 has no other butterflies and
// is launched without the multiplication in its code.  A forward transform without a shift therefore multiplies
// sum_{s >= 2} (n / 2 - n / 2^s) = (n / 2)(log2n - 2) + 1 times (log2n >= 2).
//
// Butterfly lane.  w B is the walk of msm_points_mul (mul_walk: GLV split, biased signed windows, the lane's affine table in
// the workspace of that kernel, mixed additions) without its finish; A + w B and A - w B are two mixed additions of the affine row
// A onto +-(w B), and both go to affine with ONE inversion (Montgomery's trick over the two Z).  The lane reads its twiddle and both
// rows before its first store, and no other lane of the stage touches these two rows.  Identity rows, equal rows, A = +-w B are
// what the addition formulas' own cases cover (curve.h); a result that is the identity takes the identity row.
//
// Everything but the kernels is __host__ __device__: the index maps and the lane body run on the CPU in tests/csrc/points_ntt_host.hip.
#pragma once
#include "points_mul.h"

namespace msm {
namespace pntt {

constexpr int BLOCK = pmul::BLOCK;

// ---------------------------------------------------------------------------------------------
// index maps (n = 2^log2n < 2^30)
// ---------------------------------------------------------------------------------------------

// the log2n low bits of i, reversed
MSM_DEV uint32_t bit_reverse(uint32_t i, int log2n) {
  uint32_t r = i;
  r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
  r = ((r >> 2) & 0x33333333u) | ((r & 0x33333333u) << 2);
  r = ((r >> 4) & 0x0F0F0F0Fu) | ((r & 0x0F0F0F0Fu) << 4);
  r = ((r >> 8) & 0x00FF00FFu) | ((r & 0x00FF00FFu) << 8);
  r = (r >> 16) | (r << 16);
  return log2n ? r >> (32 - log2n) : 0u;
}

// butterfly t < n / 2 of stage s (1 .. log2n): its two rows, its position in the block and the index of its twiddle
struct Fly {
  uint32_t a, b;   // rows: b = a + m / 2
  uint32_t j;      // position in the block, j < m / 2; 0: w = 1
  uint32_t tw;     // j n / m < n / 2
};
MSM_DEV Fly butterfly(uint32_t t, int log2n, int s) {
  const int sh = log2n - s;   // log2 of the number of blocks, which is the stride of the twiddles
  Fly f;
  f.j = t >> sh;
  f.a = ((t & ((1u << sh) - 1u)) << s) + f.j;
  f.b = f.a + (1u << (s - 1));
  f.tw = f.j << sh;
  return f;
}

// butterflies of a transform whose twiddle is not 1 (the scalar multiplications of an unshifted forward transform)
constexpr uint64_t multiplications(int log2n) { return log2n < 2 ? 0 : (((uint64_t)1 << (log2n - 1)) * (uint64_t)(log2n - 2) + 1); }

// ---------------------------------------------------------------------------------------------
// the butterfly lane (Weierstrass curves)
// ---------------------------------------------------------------------------------------------

// Selects are masks over the limbs, not conditional expressions over structs: every limb stays a value in a register (a choice
// between two structs is a choice between two addresses to the compiler, and both structs then live in scratch memory).
template <class F>
MSM_DEV void fe_pick(Fe<F>& r, bool c, const Fe<F>& a, const Fe<F>& b) {   // r = c ? a : b
  const uint32_t m = c ? 0xFFFFFFFFu : 0u;
#pragma unroll
  for (int l = 0; l < F::NL; l++) r.l[l] = (a.l[l] & m) | (b.l[l] & ~m);
}

// the row as a projective point; the identity row: Z = 0, and X, Y are words that no formula reads
template <class F>
MSM_DEV void load_row_proj(Proj<F>& P, const uint32_t* row) {
  Fe<F> one, zero;
  fe_set_one<F>(one);
  fe_set_zero<F>(zero);
  pmul::load_fe<F>(P.X, row);
  pmul::load_fe<F>(P.Y, row + F::NW);
  fe_pick<F>(P.Z, row[F::NW - 1] == INF_WORD, zero, one);
}

// acc = s * (row), projective, s = the 32-byte scalar at `scalar`: the walk of pmul::mul_lane, which ends in that lane's own
// finish.  (The two are not one function: with the walk cut out of mul_lane the register allocation of k_points_mul moves, 8
// bytes of scratch on the 12-word fields, and that kernel compiles from unchanged text.)  Nothing is stored but the lane's table
// slots: tbl, cap, g (points_mul.h).
template <class CV, int W>
MSM_DEV void mul_walk(Proj<typename CV::F>& acc, const uint32_t* row, const uint32_t* scalar, uint4* tbl, uint64_t cap, uint64_t g) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  constexpr int NWIN = pmul::windows(CV::G::MAX_BITS, W);
  static_assert(!pmul::PROJ_ENTRIES, "the butterfly walks affine table entries");
  uint32_t r0[5], r1[5];
  bool sign[2];
  pmul::split_recode<CV, W>(r0, r1, sign, scalar);
  const bool inf = row[NW - 1] == INF_WORD;
  if (!inf) {
    Fe<F> px, py;
    pmul::load_fe<F>(px, row);
    pmul::load_fe<F>(py, row + NW);
    pmul::table_build<F, W>(tbl, cap, g, px, py);
  }
  Fe<F> beta;
#pragma unroll
  for (int l = 0; l < NL; l++) beta.l[l] = F::BETAL[l];
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
      if (e == 0) pmul::digit<5, W>(r0, k, mag, neg);
      else pmul::digit<5, W>(r1, k, mag, neg);
      const uint32_t slot = mag ? mag - 1 : 0;
      Proj<F> Q;
      pmul::tbl_load<F>(Q.X, tbl, cap, g, slot, 0);
      pmul::tbl_load<F>(Q.Y, tbl, cap, g, slot, 1);
      if (e == 1) fe_mul<F>(Q.X, Q.X, beta);   // phi(x, y) = (beta x, y)
      pmul::fe_neg_if<F>(Q.Y, neg != (e ? sign[1] : sign[0]));   // (sign[e] is an array in scratch memory here)
      Q.Z = Q.X;   // (ignored by the mixed addition)
      proj_add_mixed<F>(acc, acc, Q, inf || mag == 0);
    }
  }
}

// the row of (X / Z, Y / Z) given zi = 1 / Z, as pmul::finish_row writes it; the identity: the identity row
template <class F>
MSM_DEV void affine_row(uint32_t* out, const Proj<F>& R, const Fe<F>& zi, bool inf) {
  if (inf) {
    store_row_identity<F::NW / 4>(out);
    return;
  }
  Fe<F> x, y, bx, beta;
  fe_mul<F>(x, R.X, zi);
  fe_reduce_2p<F>(x);
  fe_mul<F>(y, R.Y, zi);
  fe_reduce_2p<F>(y);
#pragma unroll
  for (int l = 0; l < F::NL; l++) beta.l[l] = F::BETAL[l];
  fe_mul<F>(bx, x, beta);
  fe_reduce_2p<F>(bx);
  store_row(out, x, y, bx);
}

// both points to affine with one inversion, and their rows as msm_set_points writes them (pmul::finish_row for two)
template <class F>
MSM_DEV void finish_rows(uint32_t* out0, uint32_t* out1, const Proj<F>& R0, const Proj<F>& R1) {
  const bool inf0 = proj_is_zero<F>(R0), inf1 = proj_is_zero<F>(R1);
  Fe<F> one, z0, z1, inv, zi;
  fe_set_one<F>(one);
  fe_pick<F>(z0, inf0, one, R0.Z);   // (the identity stays out of the product: its row is written apart)
  fe_pick<F>(z1, inf1, one, R1.Z);
  fe_mul<F>(inv, z0, z1);
  fe_reduce_4p<F>(inv);
  fe_inv<F>(inv, inv);               // 1 / (Z0 Z1)
  fe_mul<F>(zi, inv, z1);            // 1 / Z0
  affine_row<F>(out0, R0, zi, inf0);
  fe_mul<F>(zi, inv, z0);
  affine_row<F>(out1, R1, zi, inf1);
}

// (row_a, row_b) <- (A + w B, A - w B), w = the 32-byte scalar at `twiddle`; mul = false: w = 1 and neither the twiddle nor the
// table is read.  tbl, cap, g: the lane's table slots (points_mul.h).  Both rows and the twiddle are read before the first store.
template <class CV, int W>
MSM_DEV void butterfly_lane(uint32_t* row_a, uint32_t* row_b, const uint32_t* twiddle, bool mul, uint4* tbl, uint64_t cap, uint64_t g) {
  using F = typename CV::F;
  Proj<F> wb, A, R0, R1;
  if (mul) mul_walk<CV, W>(wb, row_b, twiddle, tbl, cap, g);
  else load_row_proj<F>(wb, row_b);
  const bool inf_a = row_a[F::NW - 1] == INF_WORD;
  pmul::load_fe<F>(A.X, row_a);   // (the identity row: words that the addition does not read)
  pmul::load_fe<F>(A.Y, row_a + F::NW);
  A.Z = A.X;                      // (ignored by the mixed addition)
  proj_add_mixed<F>(R0, wb, A, inf_a);
  pmul::fe_neg_if<F>(wb.Y, true);
  proj_add_mixed<F>(R1, wb, A, inf_a);
  finish_rows<F>(row_a, row_b, R0, R1);
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------

// one stage on the fixed grid of k_points_mul: lane g takes the butterflies g, g + cap, ... and rebuilds its table slots for
// each.  MUL = false: stage 1, every twiddle is 1 (tw and tbl may be null).
template <class CV, bool MUL>
__global__ void __launch_bounds__(BLOCK) k_points_ntt_stage(uint32_t* rows, const uint32_t* tw, uint32_t log2n, uint32_t stage, uint4* tbl) {
  const uint64_t cap = (uint64_t)gridDim.x * BLOCK, g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const uint64_t half = 1ull << (log2n - 1);
#pragma unroll 1
  for (uint64_t t = g; t < half; t += cap) {
    const Fly f = butterfly((uint32_t)t, (int)log2n, (int)stage);
    butterfly_lane<CV, pmul::W_VAR>(rows + (uint64_t)f.a * ROW_WORDS, rows + (uint64_t)f.b * ROW_WORDS, tw + (uint64_t)f.tw * 8, MUL && f.j != 0, tbl,
                                    pmul::lane_value(cap), g);
  }
}

// dst[i] = src[bit_reverse(i)], whole rows of row_words words; dst and src do not overlap
__global__ void __launch_bounds__(BLOCK) k_points_bitrev_gather(uint4* dst, const uint4* src, uint32_t log2n, uint32_t row_words) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >> log2n) return;
  const uint32_t q = row_words / 4;
  const uint4* s = src + (uint64_t)bit_reverse((uint32_t)i, (int)log2n) * q;
  uint4* d = dst + i * q;
  for (uint32_t k = 0; k < q; k++) d[k] = s[k];
}

// the same in place: lane i swaps rows i and bit_reverse(i) where i is the smaller of the two
__global__ void __launch_bounds__(BLOCK) k_points_bitrev_swap(uint4* rows, uint32_t log2n, uint32_t row_words) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >> log2n) return;
  const uint64_t r = bit_reverse((uint32_t)i, (int)log2n);
  if (r <= i) return;
  const uint32_t q = row_words / 4;
  uint4 *a = rows + i * q, *b = rows + r * q;
  for (uint32_t k = 0; k < q; k++) {
    const uint4 va = a[k], vb = b[k];
    a[k] = vb;
    b[k] = va;
  }
}

}  // namespace pntt
}  // namespace msm
