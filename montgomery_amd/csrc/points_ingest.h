// Point ingest beyond the plain x || y upload of k_points_from_wire / k_te_points_from_wire: compressed points decoded on the
// device (one square root per point), the prime-order subgroup check [q] P = O over resident rows, and the kernels that find
// the first bad point of a failed uncompressed upload.  Wire formats: include/msm_hip.h (msm_set_points_ex) and INTEGRATION.md.
//
// Every kernel here reports a failure as ONE 64-bit atomicMin of (index << 3) | reason into a word the host set to all-ones:
// whatever order the lanes run in, what is left is the smallest failing index and its reason.
//
// Lock-step: the square roots run fixed exponent chains (constants of gen_constants.py) and a Tonelli-Shanks with a fixed
// iteration count; the subgroup check walks the fixed bits of q.  The only data-dependent control flow is the early exit of a
// lane whose point is the identity or already failed, and the edge cases of proj_add_mixed (P = +-acc), which a point of the
// subgroup meets at the last step only.
#pragma once
#include <type_traits>
#include "msm_kernels.h"
#include "te_kernels.h"

namespace msm {
namespace ingest {

enum : uint32_t { R_COORD = 1, R_FLAGS = 2, R_NO_POINT = 3, R_NOT_ON_CURVE = 4, R_SUBGROUP = 5 };

__device__ __forceinline__ void report(unsigned long long* err, uint64_t i, uint32_t reason) {
  atomicMin(err, ((unsigned long long)i << 3) | reason);
}

template <int W>
MSM_DEV bool words_gt(const uint32_t (&a)[W], const uint32_t* b) {   // a > b ?
  bool gt = false, lt = false;
#pragma unroll
  for (int j = W - 1; j >= 0; j--) {
    if (!gt && !lt) {
      if (a[j] > b[j]) gt = true;
      else if (a[j] < b[j]) lt = true;
    }
  }
  return gt;
}

// canonical plain integer of a Montgomery-form value < 4.5 p, as packed words
template <class C>
MSM_DEV void fe_plain_words(uint32_t (&w)[C::NW], const Fe<C>& a) {
  Fe<C> one, t;
  fe_set_zero<C>(one);
  one.l[0] = 1;
  fe_mul<C>(t, a, one);   // a R^-1 < p + 1
  fe_reduce_2p<C>(t);
  fe_pack<C>(w, t);
}

// r = p - a for a canonical a (0 stays 0)
template <class C>
MSM_DEV void fe_neg_canonical(Fe<C>& r, const Fe<C>& a) {
  Fe<C> z;
  fe_set_zero<C>(z);
  fe_sub_p<C>(r, z, a);
  fe_reduce_2p<C>(r);
}

// a^SQRT_E, MSB first over the constant exponent (uniform across the wave, as fe_inv_fermat)
template <class C>
MSM_DEV void fe_pow_sqrt_e(Fe<C>& r, const Fe<C>& a) {
  Fe<C> acc;
  fe_set_one<C>(acc);
#pragma unroll 1
  for (int bit = C::SQRT_EBITS - 1; bit >= 0; bit--) {
    fe_sqr<C>(acc, acc);
    if ((C::SQRT_EW[bit / 32] >> (bit % 32)) & 1u) fe_mul<C>(acc, acc, a);
  }
  r = acc;
}

// r = a square root of a (Montgomery form, any value < 4p), canonical; returns whether r^2 = a, i.e. whether a is a square.
//   p = 3 mod 4 (BLS12-381): r = a^((p + 1) / 4).
//   p - 1 = 2^S t otherwise: Tonelli-Shanks in the fixed-iteration form.  x = a^((t + 1) / 2), b = a^t, z = g^t; at step
//   k = S-1 .. 1 b^(2^k) = 1, z has order 2^(k+1) and x^2 = a b.  If b^(2^(k-1)) != 1 it is -1, and x z, b z^2 restore the
//   invariant one level down.  Every lane does all S - 1 steps (the multiplications of both outcomes, then a select):
//   S^2 / 2 squarings in all, 1 035 for BLS12-377 (S = 46) -- against a data-dependent loop whose trip count would differ
//   from lane to lane and leave the wave at its worst lane's count anyway.
template <class C>
MSM_DEV bool fe_sqrt(Fe<C>& r, const Fe<C>& a_in) {
  Fe<C> a = a_in, x;
  fe_reduce_4p<C>(a);
  if constexpr (C::TWO_ADICITY == 1) {
    fe_pow_sqrt_e<C>(x, a);
  } else {
    Fe<C> w, b, z, e, one, xz, bz;
    fe_pow_sqrt_e<C>(w, a);   // a^((t - 1) / 2)
    fe_mul<C>(x, a, w);
    fe_mul<C>(b, x, w);
#pragma unroll
    for (int l = 0; l < C::NL; l++) z.l[l] = C::SQRT_ZL[l];
    fe_set_one<C>(one);
#pragma unroll 1
    for (int k = C::TWO_ADICITY - 1; k >= 1; k--) {
      e = b;
#pragma unroll 1
      for (int j = 1; j < k; j++) fe_sqr<C>(e, e);
      fe_reduce_2p<C>(e);
      const bool flip = !fe_equal<C>(e, one);
      fe_mul<C>(xz, x, z);
      fe_sqr<C>(z, z);
      fe_mul<C>(bz, b, z);
      fe_select<C>(x, flip, xz, x);
      fe_select<C>(b, flip, bz, b);
    }
  }
  fe_reduce_2p<C>(x);
  Fe<C> xx;
  fe_sqr<C>(xx, x);
  fe_reduce_2p<C>(xx);
  r = x;
  return fe_equal<C>(xx, a);
}

// the pasta encoding (sign = y odd, no infinity flag: x = 0 is no point of y^2 = x^3 + 5 and stands for the identity)
template <class CV>
constexpr bool pasta_format() { return std::is_same<CV, CvPallas>::value || std::is_same<CV, CvVesta>::value; }
// the curve group has prime order: every point of the curve is in the subgroup
template <class CV>
constexpr bool cofactor_one() {
  return pasta_format<CV>() || std::is_same<CV, CvBn254>::value || std::is_same<CV, CvGrumpkin>::value;
}

// bit length of the group order q (8 words)
constexpr int order_bits(const uint32_t* q) {
  for (int j = 7; j >= 0; j--)
    for (int b = 31; b >= 0; b--)
      if ((q[j] >> b) & 1u) return 32 * j + b + 1;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// k_points_decompress: N compressed Weierstrass points -> point rows (the rows k_points_from_wire makes from x || y)
//   BLS12-381 (ZCash): 48 bytes, x big-endian; first byte 0x80 compressed (required), 0x40 infinity, 0x20 sign (y > (p-1)/2)
//   BLS12-377 (arkworks): 48 bytes, x little-endian; last byte 0x80 sign (y > (p-1)/2), 0x40 infinity; bits 377-381 unused
//   BN254 G1, Grumpkin (arkworks): the BLS12-377 rules at 32 bytes (bit 255 sign, bit 254 infinity; a 254-bit x leaves both free)
//   Pallas, Vesta (pasta): 32 bytes, x little-endian; bit 255 sign (y odd); all-zero bytes = the identity
// ---------------------------------------------------------------------------------------------

template <class CV>
__global__ void __launch_bounds__(256) k_points_decompress(uint32_t* rows, const uint32_t* wire, uint64_t n,
                                                           unsigned long long* err) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[NW], xw[NW];
  load_words12(w, wire + i * NW);
  uint32_t* row = rows + i * ROW_WORDS;
  bool inf = false, sign = false, bad_flags = false;
  uint32_t rest = 0;   // every bit of x but the flags
  if constexpr (std::is_same<CV, CvBls381>::value) {
#pragma unroll
    for (int j = 0; j < NW; j++) xw[j] = __builtin_bswap32(w[NW - 1 - j]);
    const uint32_t fl = xw[NW - 1] >> 29;
    xw[NW - 1] &= 0x1FFFFFFFu;
    inf = (fl & 2u) != 0;
    sign = (fl & 1u) != 0;
    bad_flags = !(fl & 4u) || (inf && sign);
  } else if constexpr (!pasta_format<CV>()) {   // arkworks: the two top bits of the last word are flags
#pragma unroll
    for (int j = 0; j < NW; j++) xw[j] = w[j];
    constexpr uint32_t XMASK = (1u << (F::BITS - 32 * (NW - 1))) - 1u;   // the bits of x in the last word
    static_assert(F::BITS > 32 * (NW - 1) && F::BITS <= 32 * NW - 2, "x must leave the two flag bits free");
    const uint32_t top = xw[NW - 1];
    sign = (top >> 31) != 0;
    inf = ((top >> 30) & 1u) != 0;
    bad_flags = (inf && sign) || (top & (0x3FFFFFFFu & ~XMASK));   // BLS12-377: bits 377-381 are not used
    xw[NW - 1] &= XMASK;
  } else {
#pragma unroll
    for (int j = 0; j < NW; j++) xw[j] = w[j];
    sign = (xw[NW - 1] >> 31) != 0;
    xw[NW - 1] &= 0x7FFFFFFFu;
  }
#pragma unroll
  for (int j = 0; j < NW; j++) rest |= xw[j];
  if constexpr (pasta_format<CV>()) inf = !sign && rest == 0;   // x = 0 is no point of y^2 = x^3 + 5
  if (inf && rest) bad_flags = true;
  if (bad_flags || inf) {
    store_row_identity<NW / 4>(row);
    if (bad_flags) report(err, i, R_FLAGS);
    return;
  }
  if (words_ge_p<F>(xw)) {
    store_row_identity<NW / 4>(row);
    report(err, i, R_COORD);
    return;
  }
  Fe<F> x, y, r2, beta, bb, rhs, bx;
  fe_unpack<F>(x, xw);
#pragma unroll
  for (int l = 0; l < NL; l++) { r2.l[l] = F::R2[l]; beta.l[l] = F::BETAL[l]; bb.l[l] = F::BL[l]; }
  fe_mul<F>(x, x, r2);
  fe_reduce_2p<F>(x);
  fe_sqr<F>(rhs, x);
  fe_mul<F>(rhs, rhs, x);
  fe_add<F>(rhs, rhs, bb);   // x^3 + b < 3p
  if (!fe_sqrt<F>(y, rhs)) {
    store_row_identity<NW / 4>(row);
    report(err, i, R_NO_POINT);
    return;
  }
  uint32_t yp[NW];
  fe_plain_words<F>(yp, y);
  const bool odd = pasta_format<CV>() ? (yp[0] & 1u) != 0 : words_gt<NW>(yp, F::HALFW);
  if (odd != sign) {
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) any |= yp[j];
    if (!any) {   // y = 0 is its own negation: the sign bit cannot be honoured
      store_row_identity<NW / 4>(row);
      report(err, i, R_FLAGS);
      return;
    }
    fe_neg_canonical<F>(y, y);
  }
  fe_mul<F>(bx, x, beta);
  fe_reduce_2p<F>(bx);
  store_row(row, x, y, bx);
}

// ---------------------------------------------------------------------------------------------
// k_points_validate: resident rows [first, first + count): the curve equation, and with `subgroup` [q] P = O by double-and-add
// over the fixed bits of q (proj_double / proj_add_mixed).  Pallas, Vesta, BN254 G1 and Grumpkin have cofactor 1: every curve point is in the group.
// (No endomorphism shortcut: [q] P is right without a torsion argument per curve, see DESIGN.md "Point ingest".)
// ---------------------------------------------------------------------------------------------

template <class CV>
__global__ void __launch_bounds__(256) k_points_validate(const uint32_t* rows, uint64_t first, uint64_t count, int subgroup,
                                                         unsigned long long* err) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint64_t i = first + t;
  uint32_t xw[NW], yw[NW];
  load_words12(xw, rows + i * ROW_WORDS);
  load_words12(yw, rows + i * ROW_WORDS + NW);
  if (xw[NW - 1] == INF_WORD) return;
  Proj<F> P;
  fe_unpack<F>(P.X, xw);
  fe_unpack<F>(P.Y, yw);
  {
    Fe<F> lhs, rhs, bb;
#pragma unroll
    for (int l = 0; l < NL; l++) bb.l[l] = F::BL[l];
    fe_sqr<F>(lhs, P.Y);
    fe_sqr<F>(rhs, P.X);
    fe_mul<F>(rhs, rhs, P.X);
    fe_add<F>(rhs, rhs, bb);
    fe_sub_4p<F>(lhs, lhs, rhs);
    fe_cond_sub<F, 4>(lhs);
    if (!fe_is_zero_mod_p<F>(lhs)) {
      report(err, i, R_NOT_ON_CURVE);
      return;
    }
  }
  if (cofactor_one<CV>() || !subgroup) return;
  constexpr int QB = order_bits(CV::G::Q);
  fe_set_one<F>(P.Z);
  Proj<F> acc;
  proj_set_zero<F>(acc);
#pragma unroll 1
  for (int bit = QB - 1; bit >= 0; bit--) {
    proj_double<F>(acc, acc);
    if ((CV::G::Q[bit / 32] >> (bit % 32)) & 1u) proj_add_mixed<F>(acc, acc, P, false);
  }
  if (!proj_is_zero<F>(acc)) report(err, i, R_SUBGROUP);
}

// ---------------------------------------------------------------------------------------------
// k_wire_locate: the first bad point of an uncompressed upload that k_points_from_wire refused (its error flags carry no index):
// the same tests on the same wire words
// ---------------------------------------------------------------------------------------------

template <class CV>
__global__ void __launch_bounds__(256) k_wire_locate(const uint32_t* wire, uint64_t n, int check_curve, unsigned long long* err) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t xw[NW], yw[NW];
  load_words12(xw, wire + i * (2 * NW));
  load_words12(yw, wire + i * (2 * NW) + NW);
  uint32_t any = 0;
#pragma unroll
  for (int j = 0; j < NW; j++) any |= xw[j] | yw[j];
  if (any == 0) return;
  if (words_ge_p<F>(xw) || words_ge_p<F>(yw)) {
    report(err, i, R_COORD);
    return;
  }
  if (!check_curve) return;
  Fe<F> x, y, r2, lhs, rhs, bb;
  fe_unpack<F>(x, xw);
  fe_unpack<F>(y, yw);
#pragma unroll
  for (int l = 0; l < NL; l++) { r2.l[l] = F::R2[l]; bb.l[l] = F::BL[l]; }
  fe_mul<F>(x, x, r2);
  fe_mul<F>(y, y, r2);
  fe_sqr<F>(lhs, y);
  fe_sqr<F>(rhs, x);
  fe_mul<F>(rhs, rhs, x);
  fe_add<F>(rhs, rhs, bb);
  fe_sub_4p<F>(lhs, lhs, rhs);
  fe_cond_sub<F, 4>(lhs);
  if (!fe_is_zero_mod_p<F>(lhs)) report(err, i, R_NOT_ON_CURVE);
}

// ---------------------------------------------------------------------------------------------
// Ed-on-BLS12-377 (a = -1, d = 3021): 32 bytes, y little-endian, bit 255 = sign of x (x > (r-1)/2), bits 253-254 unused.
// x^2 = (y^2 - 1) / (d y^2 + 1): one inversion (fe_inv) and one square root per point.  The identity (0, 1) is an ordinary
// point here (y = 1, sign 0).
// ---------------------------------------------------------------------------------------------

using te::FT;
using te::TW;
using te::TL;   // (TE_CONST)

__global__ void __launch_bounds__(256) k_te_points_decompress(uint32_t* rows, const uint32_t* wire, uint64_t n,
                                                              unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t yw[TW];
  te::load_words8(yw, wire + i * TW);
  uint32_t* row = rows + i * te::TE_ROW_WORDS;
  const bool sign = (yw[TW - 1] >> 31) != 0;
  uint32_t reason = 0;
  if (yw[TW - 1] & 0x60000000u) reason = R_FLAGS;
  yw[TW - 1] &= 0x7FFFFFFFu;
  if (!reason && te::words8_ge_p(yw)) reason = R_COORD;
  Fe<FT> x, y, t, kt, k;
  fe_set_zero<FT>(x);
  fe_set_one<FT>(y);
  if (!reason) {
    Fe<FT> yy, num, den, one, dd, r2;
    fe_unpack<FT>(y, yw);
    TE_CONST(r2, R2);
    TE_CONST(dd, DL);
    fe_set_one<FT>(one);
    fe_mul<FT>(y, y, r2);
    fe_reduce_2p<FT>(y);
    fe_sqr<FT>(yy, y);
    fe_sub_2p<FT>(num, yy, one);
    fe_mul<FT>(den, yy, dd);
    fe_add<FT>(den, den, one);
    fe_reduce_4p<FT>(den);
    if (fe_is_zero_canonical<FT>(den)) {
      reason = R_NO_POINT;   // d y^2 = -1 (cannot happen on this curve: -1 / d is no square)
    } else {
      Fe<FT> di, xx;
      fe_inv<FT>(di, den);
      fe_mul<FT>(xx, num, di);
      if (!fe_sqrt<FT>(x, xx)) reason = R_NO_POINT;
    }
  }
  if (!reason) {
    uint32_t xp[TW];
    fe_plain_words<FT>(xp, x);
    if (words_gt<TW>(xp, FT::HALFW) != sign) {
      uint32_t any = 0;
#pragma unroll
      for (int j = 0; j < TW; j++) any |= xp[j];
      if (!any) reason = R_FLAGS;   // x = 0 with the sign bit set
      else fe_neg_canonical<FT>(x, x);
    }
  }
  if (reason) {   // a defined row: the identity (0, 1)
    fe_set_zero<FT>(x);
    fe_set_one<FT>(y);
    report(err, i, reason);
  }
  fe_mul<FT>(t, x, y);
  TE_CONST(k, K2DL);
  fe_mul<FT>(kt, t, k);
  fe_reduce_2p<FT>(t);
  fe_reduce_2p<FT>(kt);
  fe_store<FT>(row, x);
  fe_store<FT>(row + 8, y);
  fe_store<FT>(row + 16, t);
  fe_store<FT>(row + 24, kt);
}

// curve equation -x^2 + y^2 = 1 + d x^2 y^2 of the row, then with `subgroup` [q] P = (0, 1) by unified additions (te_add)
__global__ void __launch_bounds__(256) k_te_points_validate(const uint32_t* rows, uint64_t first, uint64_t count, int subgroup,
                                                            unsigned long long* err) {
  const uint64_t tt = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tt >= count) return;
  const uint64_t i = first + tt;
  const uint32_t* row = rows + i * te::TE_ROW_WORDS;
  uint32_t w[TW];
  te::Ext P;
  te::load_words8(w, row);      fe_unpack<FT>(P.X, w);
  te::load_words8(w, row + 8);  fe_unpack<FT>(P.Y, w);
  te::load_words8(w, row + 16); fe_unpack<FT>(P.T, w);
  fe_set_one<FT>(P.Z);
  {
    Fe<FT> xx, yy, lhs, rhs, dd, one;
    fe_sqr<FT>(xx, P.X);
    fe_sqr<FT>(yy, P.Y);
    fe_sub_2p<FT>(lhs, yy, xx);
    TE_CONST(dd, DL);
    fe_mul<FT>(rhs, xx, yy);
    fe_mul<FT>(rhs, rhs, dd);
    fe_set_one<FT>(one);
    fe_add<FT>(rhs, rhs, one);
    fe_sub_4p<FT>(lhs, lhs, rhs);
    fe_cond_sub<FT, 4>(lhs);
    if (!fe_is_zero_mod_p<FT>(lhs)) {
      report(err, i, R_NOT_ON_CURVE);
      return;
    }
  }
  if (!subgroup) return;
  constexpr int QB = order_bits(FRED_Q);
  te::Ext acc;
  te::te_set_identity(acc);
#pragma unroll 1
  for (int bit = QB - 1; bit >= 0; bit--) {
    te::Ext D = acc;
    te::te_add(acc, D, D);
    if ((FRED_Q[bit / 32] >> (bit % 32)) & 1u) {
      D = acc;
      te::te_add(acc, D, P);
    }
  }
  Fe<FT> d;
  fe_sub_2p<FT>(d, acc.Y, acc.Z);
  if (!fe_is_zero_mod_p<FT>(acc.X) || !fe_is_zero_mod_p<FT>(d)) report(err, i, R_SUBGROUP);
}

// the uncompressed Edwards upload's tests (k_te_points_from_wire), with the index
__global__ void __launch_bounds__(256) k_te_wire_locate(const uint32_t* wire, uint64_t n, int check_curve, unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t xw[TW], yw[TW];
  te::load_words8(xw, wire + i * 16);
  te::load_words8(yw, wire + i * 16 + 8);
  if (te::words8_ge_p(xw) || te::words8_ge_p(yw)) {
    report(err, i, R_COORD);
    return;
  }
  if (!check_curve) return;
  Fe<FT> x, y, r2, xx, yy, lhs, rhs, dd, one;
  fe_unpack<FT>(x, xw);
  fe_unpack<FT>(y, yw);
  TE_CONST(r2, R2);
  fe_mul<FT>(x, x, r2);
  fe_mul<FT>(y, y, r2);
  fe_sqr<FT>(xx, x);
  fe_sqr<FT>(yy, y);
  fe_sub_2p<FT>(lhs, yy, xx);
  TE_CONST(dd, DL);
  fe_mul<FT>(rhs, xx, yy);
  fe_mul<FT>(rhs, rhs, dd);
  fe_set_one<FT>(one);
  fe_add<FT>(rhs, rhs, one);
  fe_sub_4p<FT>(lhs, lhs, rhs);
  fe_cond_sub<FT, 4>(lhs);
  fe_reduce_4p<FT>(lhs);
  if (!fe_is_zero_canonical<FT>(lhs)) report(err, i, R_NOT_ON_CURVE);
}

}  // namespace ingest
}  // namespace msm
