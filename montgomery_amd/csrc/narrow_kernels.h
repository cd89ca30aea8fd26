// Digit kernels of narrow scalars (msm_run_narrow, msm_narrow.hip): 1-, 2-, 4-, 8- and 16-byte little-endian integers, or
// 32-byte field elements declared to hold small values, cut into the signed window digits k_digits / k_te_digits write for
// full-width scalars -- without the endomorphism split, so that K = ceil((bits + 1) / c) windows are all there is.
//   k_digits_narrow<W>      Weierstrass curves: dig[window][2 n], entry 2 i = the digit of point i, entry 2 i + 1 = 0 (as
//                           k_digits under msm_opts.no_glv: the endomorphism entry is never sorted)
//   k_te_digits_narrow<W>   Ed-on-BLS12-377: dig[window][n]
//   k_*_digits_narrow_batch the same for the elements of a fused batch (virtual window b K + k, as k_digits_batch)
//   k_scalar_bits           the bit lengths a set of 32-byte scalars needs (msm_scalar_bits)
// The kernels do not depend on the curve: widths 1 .. 16 never meet q (2^128 < q on all four curves) and width 32 gets q as an
// argument.  The reference has no counterpart (its fromPackedBytesSmall, src/scalar-glv.ts:44, is the codec of a GLV half).
#pragma once
#include "msm_kernels.h"

namespace msm {

// the scalar format of a narrow call; `bits` is already resolved (1 .. 128)
struct NarrowFmt {
  int32_t bits, is_signed;
  uint32_t q[8];   // width 32 only
};

constexpr int NARROW_BATCH_MAX = 64;   // elements of one fused group: K is 1 .. 5 for most narrow plans, 128 windows hold many
struct NarrowBatchScalars {
  const void* p[NARROW_BATCH_MAX];   // n x W bytes each, aligned to max(4, min(W, 16)) bytes
};

constexpr uint32_t NARROW_ERR_RANGE = 16u;   // bit of ctx->errflag: a value outside the declared range

// scalars one lane takes: a lane always loads at least a dword
template <int W>
struct NarrowLane {
  static constexpr int PER = W == 1 ? 4 : W == 2 ? 2 : 1;
  static constexpr int NW = W < 4 ? 1 : W / 4;   // words of one scalar in registers
};

#ifdef MSM_NARROW_TU

// the PER scalars of group g (scalars [g PER, (g + 1) PER) counted from `base`) as loaded; scalar j of them -> words
template <int W>
struct NarrowLoad {
  uint32_t w[NarrowLane<W>::NW];
  MSM_DEV void load(const void* base, uint64_t g) {
    if constexpr (W <= 4) {
      w[0] = reinterpret_cast<const uint32_t*>(base)[g];
    } else if constexpr (W == 8) {
      const uint2 a = reinterpret_cast<const uint2*>(base)[g];
      w[0] = a.x; w[1] = a.y;
    } else if constexpr (W == 16) {
      const uint4 a = reinterpret_cast<const uint4*>(base)[g];
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    } else {
      const uint4* p4 = reinterpret_cast<const uint4*>(base) + 2 * g;
      const uint4 a = p4[0], b = p4[1];
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    }
  }
};

// m < 2^bits, or m == 2^bits where the negative extreme is allowed (bits 1 .. 128, m of five words)
MSM_DEV bool narrow_in_range(const uint32_t (&m)[5], int bits, bool allow_equal) {
  uint32_t over = 0, rest = 0;
  const int tw = bits >> 5;
  const uint32_t tbit = 1u << (bits & 31);
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int lo = 32 * i;
    const uint32_t mask = bits <= lo ? 0xFFFFFFFFu : bits >= lo + 32 ? 0u : ~((1u << (bits - lo)) - 1u);
    over |= m[i] & mask;
    rest |= i == tw ? m[i] ^ tbit : m[i];
  }
  return over == 0 || (allow_equal && rest == 0);
}

// Scalar j of a lane's load -> magnitude (five words, at most 2^128) and sign.  A value outside the declared range sets
// NARROW_ERR_RANGE in *err (the call then fails with MSM_ERR_SCALAR) and becomes 0, so that no digit leaves its buckets.
template <int W>
MSM_DEV void narrow_value(uint32_t (&m)[5], uint32_t& neg, const NarrowLoad<W>& ld, int j, const NarrowFmt& f, uint32_t* err) {
  constexpr int NW = NarrowLane<W>::NW;
  neg = 0;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 5; i++) m[i] = 0;
  if constexpr (W == 32) {
    uint32_t s[8], q[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { s[i] = ld.w[i]; q[i] = f.q[i]; }
    bad = words8_ge(s, q);
    // s >= 2^129 can only be a negative value stored as q - |v|: |v| <= 2^128 and q > 2^250 on all four curves.  (Values in
    // [2^128, 2^129) stay positive here and are refused by the range check below.)
    if (f.is_signed && (s[5] | s[6] | s[7] | (s[4] & ~1u))) {
      uint32_t t[8];
#pragma unroll
      for (int i = 0; i < 8; i++) t[i] = q[i];
      bn_addsub<8, 8>(t, s, true);
#pragma unroll
      for (int i = 0; i < 8; i++) s[i] = t[i];
      neg = 1;
    }
    bad |= (s[5] | s[6] | s[7]) != 0;
#pragma unroll
    for (int i = 0; i < 5; i++) m[i] = s[i];
  } else {
    uint32_t v[NW];
    if constexpr (W == 1) {
      const uint32_t b = (ld.w[0] >> (8 * j)) & 0xFFu;
      v[0] = f.is_signed ? (uint32_t)(int32_t)(int8_t)b : b;
    } else if constexpr (W == 2) {
      const uint32_t h = (ld.w[0] >> (16 * j)) & 0xFFFFu;
      v[0] = f.is_signed ? (uint32_t)(int32_t)(int16_t)h : h;
    } else {
#pragma unroll
      for (int i = 0; i < NW; i++) v[i] = ld.w[i];
    }
    if (f.is_signed && (v[NW - 1] >> 31)) {
      bn_negate<NW>(v);   // two's complement: |-2^(8 W - 1)| keeps its top bit
      neg = 1;
    }
#pragma unroll
    for (int i = 0; i < NW; i++) m[i] = v[i];
  }
  bad |= !narrow_in_range(m, f.bits, neg != 0);
  if (bad) {
    atomicOr(err, NARROW_ERR_RANGE);
#pragma unroll
    for (int i = 0; i < 5; i++) m[i] = 0;
    neg = 0;
  }
}

// The K signed digits of one magnitude, as the no-GLV branch of k_digits emits them: window k takes c bits (a folded top
// window c + 1 and no recoding), a digit above L = 2^(c-1) becomes 2 L - l with a carry into the next window, and the sign of
// the value rides in bit 31 XORed with that carry.  The top window never carries out: the magnitude is at most 2^bits and
// K c >= bits + 1.  Where K c = bits + 1 its raw digit is at most L - 1, plus the carry L -- or L itself for the extreme 2^bits,
// whose lower bits are all 0, so no carry arrives.  A short top window of t < c bits holds at most 2^t - 1 plus the carry,
// 2^t <= L.  A folded one (c + 1 bits, bits + 1 = K c + 1) at most 2^c - 1 plus the carry, or 2^c for the extreme: 2 L, its
// last bucket.
template <bool TE>
MSM_DEV void narrow_emit(uint32_t* dig, uint64_t stride, uint64_t i, uint32_t (&m)[5], uint32_t neg, int c, int k_total, int k_lo,
                         int k_cnt, bool fold, uint32_t* err, uint32_t* lds_hist, uint32_t hb, uint64_t fbp) {
  const uint32_t L = 1u << (c - 1);
  uint32_t carry = 0;
  for (int k = 0; k < k_total; k++) {
    const bool top = fold && k == k_total - 1;
    bool over = false;
    const uint32_t l = window_step(bn_take_bits<5>(m, top ? c + 1 : c), carry, L, top, over);
    if (over) atomicOr(err, 8u);
    const uint32_t sgn = l ? carry ^ neg : 0u;
    const int kk = k - k_lo;
    if (kk >= 0 && kk < k_cnt) {
      if constexpr (TE) dig[(uint64_t)kk * stride + i] = l | (sgn << 31);
      else *reinterpret_cast<uint2*>(dig + (uint64_t)kk * stride + 2ull * i) = make_uint2(l | (sgn << 31), 0u);
      digit_note(lds_hist, hb, fbp, kk, l);
    }
  }
}

// Block b owns the points [b pps, (b + 1) pps) of the launch, as in k_digits; `scalars` is the array of the whole CALL rounded
// down to the alignment of a lane's load, and point i of this launch is its scalar first + i: a lane takes the aligned group of
// PER scalars and skips those of other blocks or launches (ranges of the points start anywhere).
template <int W, bool TE>
MSM_DEV void digits_narrow(uint32_t* dig, const void* scalars, uint64_t first, uint32_t n, int c, int k_total, int k_lo, int k_cnt,
                           int fold, const NarrowFmt& f, uint32_t* err, uint32_t pps, uint32_t* slice_hist, uint32_t hb, uint64_t fbp) {
  constexpr int PER = NarrowLane<W>::PER;
  uint32_t* lds_hist = slice_hist_begin(slice_hist, (uint32_t)k_cnt * hb);
  const uint64_t r_lo = (uint64_t)blockIdx.x * pps, r_hi = min(r_lo + pps, (uint64_t)n);
  const uint64_t a_lo = first + r_lo, a_hi = first + r_hi;
  const uint64_t stride = TE ? (uint64_t)n : 2ull * n;
  if (r_lo < r_hi) {
    for (uint64_t g = a_lo / PER + threadIdx.x; g * PER < a_hi; g += blockDim.x) {
      NarrowLoad<W> ld;
      ld.load(scalars, g);
#pragma unroll
      for (int j = 0; j < PER; j++) {
        const uint64_t a = g * PER + j;
        if (a < a_lo || a >= a_hi) continue;
        uint32_t m[5], neg;
        narrow_value<W>(m, neg, ld, j, f, err);
        narrow_emit<TE>(dig, stride, a - first, m, neg, c, k_total, k_lo, k_cnt, fold != 0, err, lds_hist, hb, fbp);
      }
    }
  }
  slice_hist_end(slice_hist, lds_hist, (uint32_t)k_cnt * hb, hb);
}

// one lane per group of PER points, its scalars of the b_cnt elements one after the other; no slice histogram (a fused batch
// takes the one-level sort)
template <int W, bool TE>
MSM_DEV void digits_narrow_batch(uint32_t* dig, const NarrowBatchScalars& sc, uint32_t b_cnt, uint32_t n, int c, int k_total, int fold,
                                 const NarrowFmt& f, uint32_t* err) {
  constexpr int PER = NarrowLane<W>::PER;
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g * PER >= n) return;
  const uint64_t stride = TE ? (uint64_t)n : 2ull * n;
#pragma unroll 1
  for (uint32_t b = 0; b < b_cnt; b++) {
    NarrowLoad<W> ld;
    ld.load(sc.p[b], g);   // (the last group reads the whole dword its scalars end in: the host sizes the buffers for it)
    uint32_t* db = dig + (uint64_t)b * k_total * stride;
#pragma unroll
    for (int j = 0; j < PER; j++) {
      const uint64_t i = g * PER + j;
      if (i >= n) continue;
      uint32_t m[5], neg;
      narrow_value<W>(m, neg, ld, j, f, err);
      narrow_emit<TE>(db, stride, i, m, neg, c, k_total, 0, k_total, fold != 0, err, nullptr, 0, 0);
    }
  }
}
#endif   // MSM_NARROW_TU

#ifdef MSM_NARROW_TU
#define MSM_NARROW_BODY(...) { __VA_ARGS__ }
#else
#define MSM_NARROW_BODY(...) ;
#endif

template <int W>
__global__ void __launch_bounds__(1024) k_digits_narrow(uint32_t* dig, const void* scalars, uint64_t first, uint32_t n, int c,
                                                       int k_total, int k_lo, int k_cnt, int fold, NarrowFmt f, uint32_t* err,
                                                       uint32_t pps, uint32_t* slice_hist, uint32_t hb, uint64_t fbp)
    MSM_NARROW_BODY(digits_narrow<W, false>(dig, scalars, first, n, c, k_total, k_lo, k_cnt, fold, f, err, pps, slice_hist, hb, fbp);)

template <int W>
__global__ void __launch_bounds__(1024) k_te_digits_narrow(uint32_t* dig, const void* scalars, uint64_t first, uint32_t n, int c,
                                                          int k_total, int k_lo, int k_cnt, int fold, NarrowFmt f, uint32_t* err,
                                                          uint32_t pps, uint32_t* slice_hist, uint32_t hb, uint64_t fbp)
    MSM_NARROW_BODY(digits_narrow<W, true>(dig, scalars, first, n, c, k_total, k_lo, k_cnt, fold, f, err, pps, slice_hist, hb, fbp);)

template <int W>
__global__ void __launch_bounds__(256) k_digits_narrow_batch(uint32_t* dig, NarrowBatchScalars sc, uint32_t b_cnt, uint32_t n, int c,
                                                            int k_total, int fold, NarrowFmt f, uint32_t* err)
    MSM_NARROW_BODY(digits_narrow_batch<W, false>(dig, sc, b_cnt, n, c, k_total, fold, f, err);)

template <int W>
__global__ void __launch_bounds__(256) k_te_digits_narrow_batch(uint32_t* dig, NarrowBatchScalars sc, uint32_t b_cnt, uint32_t n, int c,
                                                               int k_total, int fold, NarrowFmt f, uint32_t* err)
    MSM_NARROW_BODY(digits_narrow_batch<W, true>(dig, sc, b_cnt, n, c, k_total, fold, f, err);)

// k_scalar_bits: out[0] = the largest unsigned bit length of n 32-byte scalars, out[1] = the largest signed one (the smallest
// `bits` with the value, read as v or as v - q, in [-2^bits, 2^bits)); 255 for a scalar that needs more than 128 bits or is
// >= q.  One pass, a wave-level maximum, one atomicMax per wave and word.
__global__ void __launch_bounds__(256) k_scalar_bits(uint32_t* out, const uint32_t* scalars, uint64_t n, NarrowFmt f)
#ifndef MSM_NARROW_TU
    ;
#else
{
  const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
  uint32_t ub = 0, sb = 0;
  uint32_t q[8];
#pragma unroll
  for (int j = 0; j < 8; j++) q[j] = f.q[j];
  auto bit_len = [](const uint32_t (&x)[8]) -> uint32_t {   // 255 above 128 bits
    if (x[4] | x[5] | x[6] | x[7]) return 255u;
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x[j]) r = 32u * j + (32u - (uint32_t)__clz(x[j]));
    return r;
  };
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    uint32_t s[8];
    const uint4* p4 = reinterpret_cast<const uint4*>(scalars + i * 8);
    const uint4 a = p4[0], b = p4[1];
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    uint32_t u = 255u, g = 255u;
    if (!words8_ge(s, q)) {
      u = bit_len(s);
      // v - q = -(q - v) lies in [-2^bits, 0) when q - v - 1 < 2^bits
      uint32_t t[8], one[1] = {1u};
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = q[j];
      bn_addsub<8, 8>(t, s, true);
      bn_addsub<8, 1>(t, one, true);
      g = min(u, bit_len(t));
    }
    ub = max(ub, u);
    sb = max(sb, g);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    ub = max(ub, (uint32_t)__shfl_xor((int)ub, d, 64));
    sb = max(sb, (uint32_t)__shfl_xor((int)sb, d, 64));
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicMax(&out[0], ub);
    atomicMax(&out[1], sb);
  }
}
#endif

#define MSM_NARROW_WIDTHS(X) X(1) X(2) X(4) X(8) X(16) X(32)
#define MSM_NARROW_SIG_ (uint32_t*, const void*, uint64_t, uint32_t, int, int, int, int, int, NarrowFmt, uint32_t*, uint32_t, uint32_t*, uint32_t, uint64_t)
#define MSM_NARROW_BSIG_ (uint32_t*, NarrowBatchScalars, uint32_t, uint32_t, int, int, int, NarrowFmt, uint32_t*)
#ifdef MSM_NARROW_TU
#define MSM_NARROW_INST(W)                                             \
  template __global__ void k_digits_narrow<W> MSM_NARROW_SIG_;        \
  template __global__ void k_te_digits_narrow<W> MSM_NARROW_SIG_;     \
  template __global__ void k_digits_narrow_batch<W> MSM_NARROW_BSIG_; \
  template __global__ void k_te_digits_narrow_batch<W> MSM_NARROW_BSIG_;
#else
#define MSM_NARROW_INST(W)                                                    \
  extern template __global__ void k_digits_narrow<W> MSM_NARROW_SIG_;        \
  extern template __global__ void k_te_digits_narrow<W> MSM_NARROW_SIG_;     \
  extern template __global__ void k_digits_narrow_batch<W> MSM_NARROW_BSIG_; \
  extern template __global__ void k_te_digits_narrow_batch<W> MSM_NARROW_BSIG_;
#endif
MSM_NARROW_WIDTHS(MSM_NARROW_INST)

}  // namespace msm
