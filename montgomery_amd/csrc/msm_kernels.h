// HIP kernels of the batched-affine Pippenger MSM for short Weierstrass curves y^2 = x^3 + b with a
// GLV endomorphism (BLS12-377 G1, BLS12-381 G1) on gfx950.
//
// Phase map (reference: src/msm-batched-affine.ts:69-340):
//   k_points_from_wire   pointsFromBytes + toMontgomery + endomorphism      src/parallel.ts:97-116, src/wasm/curve.ts:90-103
//   k_digits             decompose + signed slices + bucket histogram       :350-421 (scalars), :175-203
//   k_scan               integrateBucketCounts                              :423-447
//   k_scatter            sortPoints (indices, not 116-byte points)          :456-502
//   k_batch_add          bucket accumulation tree, one inversion per lane   :243-282, src/curve-affine.ts:376-522
//   k_bucket_reduce      normalizeBucketsStorage + reduceBucketsColumnProjective :504-583
//   k_window_sum         partition sums                                     :312-319
// The Horner combination of the K partition sums (:322-333) runs on the host (msm_api.hip).
//
// Data layout in HBM
//   point rows     : N x 64 words (256 B): two 128-byte lines [x | y | pad] and [beta*x | y | pad], canonical
//                    Montgomery (R = 2^390).  A gather of either GLV half touches exactly one 128-byte
//                    line (x alone = its first 64-byte sector): random 64-byte sectors are what bounds
//                    round 1, so no window may straddle sectors it does not need.
//   digits         : Kg x 2N words, magnitude | sign << 31, entry j = 2*point + half
//   slots          : bucket-sorted entry payloads ((j << 1) | neg), every bucket padded with
//                    SLOT_EMPTY to a multiple of G = 2^g so that g tree rounds need no index math
//   tree buffers   : "plane" layout, 16-byte piece c of element e at uint4 index c*cap + e
//                    (planes 0-2 = x, 3-5 = y): consecutive lanes read consecutive 16-byte pieces
//   prefix scratch : dword planes [(step*13 + limb)*T + thread]
// The identity is encoded with x = all-ones words (never canonical), y = 0.
#pragma once
#include "curve.h"
#include "glv.h"
#include "packed.h"

namespace msm {

// curve configurations: every curve-dependent kernel is a template over one of these and takes its limb and word counts from
// the field (the reference sizes limbs per field too, src/parallel.ts:53-57, src/field-msm.ts:20-56): 13 x 30-bit limbs in
// registers and 12 x 32-bit words (3 pieces of 16 bytes) in memory for the 377- / 381-bit primes, 9 limbs and 8 words (2 pieces)
// for Pallas.  Point rows are 256 bytes for all of them (two 128-byte lines), the curve-independent sort / scan kernels are shared.
struct CvBls377 { using F = Fp377; using G = GlvBls377; };   // src/concrete/bls12-377.params.ts
struct CvBls381 { using F = Fp381; using G = GlvBls381; };   // src/concrete/bls12-381.params.ts
struct CvPallas { using F = FpPallas; using G = GlvPallas; }; // src/concrete/pasta.params.ts (255-bit p)
// the two curve cycles (not in the reference), on the 9-limb / 8-word layout of Pallas: BN254 G1 and Grumpkin (254-bit fields,
// p != 1 mod 2^30: the general row of fe_reduce_row; 126-bit GLV halves like BLS12-377), Vesta (Pallas' arithmetic, other constants)
struct CvBn254 { using F = FpBn254; using G = GlvBn254; };
struct CvGrumpkin { using F = FpGrumpkin; using G = GlvGrumpkin; };
struct CvVesta { using F = FpVesta; using G = GlvVesta; };
// every Weierstrass configuration with its curve id (include/msm_hip.h): the one list the host's dispatch, its per-curve
// constants and the extern templates are made from.  X(curve id, configuration)
#define MSM_W_CURVES(X)             \
  X(MSM_CURVE_BLS12_377_G1, CvBls377) \
  X(MSM_CURVE_BLS12_381_G1, CvBls381) \
  X(MSM_CURVE_PALLAS, CvPallas)       \
  X(MSM_CURVE_BN254_G1, CvBn254)      \
  X(MSM_CURVE_GRUMPKIN, CvGrumpkin)   \
  X(MSM_CURVE_VESTA, CvVesta)
constexpr int NL = 13;   // the wide layout; kernels use F::NL / F::NW
constexpr int NW = 12;
static_assert(Fp377::NL == NL && Fp377::NW == NW && Fp381::NL == NL && Fp381::NW == NW, "the 12-word layout");
constexpr int PART_WORDS = 36;   // a window sum on its way to the host: X, Y, Z at word 0, 12, 24 (8-word fields: upper words zero)
constexpr int ROW_WORDS = 64;   // 256 B per point
constexpr int ROW_HALF = 32;    // word offset of the endomorphism image (second 128-byte line)
constexpr int ROW_Y = 12;       // word offset of y inside a line of the 12-word fields (in general: F::NW)
constexpr uint32_t SLOT_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t INF_WORD = 0xFFFFFFFFu;

// How window kk's bucket index (l - 1) is cut for the LDS-staged passes of the sort (sort_kernels.h):
// | ab coarse bits | mb mid bits | fb fine bits |.  Two-pass radix split (c <= 16): mb = 0, fb = 7.  Bin split (c > 16): mb = 0,
// the cut is made on the window's EFFECTIVE bits (a short top window fills only the low end of its bucket range).
struct WinSplit {
  uint8_t ab[16], mb[16], fb[16];
};

}  // namespace msm
#include "batch_add.h"   // k_batch_add: the accumulation tree round
namespace msm {

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------

template <int W>
MSM_DEV void load_words12(uint32_t (&w)[W], const uint32_t* p) {
  const uint4* p4 = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int j = 0; j < W / 4; j++) {
    uint4 v = p4[j];
    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
  }
}

// one coordinate (W / 4 pieces) of element e; x starts at plane 0, y at plane W / 4
template <int W>
MSM_DEV void load_planes3(uint32_t (&w)[W], const uint4* base, uint64_t cap, int first_plane, uint64_t e) {
#pragma unroll
  for (int j = 0; j < W / 4; j++) {
    uint4 v = base[(uint64_t)(first_plane + j) * cap + e];
    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
  }
}

template <int W>
MSM_DEV void store_planes3(uint4* base, uint64_t cap, int first_plane, uint64_t e, const uint32_t (&w)[W]) {
#pragma unroll
  for (int j = 0; j < W / 4; j++)
    base[(uint64_t)(first_plane + j) * cap + e] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

template <class F>
MSM_DEV bool words_ge_p(const uint32_t (&w)[F::NW]) {  // w >= p ?
  constexpr int NW = F::NW;
  bool gt = false, lt = false;
#pragma unroll
  for (int j = NW - 1; j >= 0; j--) {
    if (!gt && !lt) {
      if (w[j] > F::PW[j]) gt = true;
      else if (w[j] < F::PW[j]) lt = true;
    }
  }
  return !lt;
}

template <class F>
MSM_DEV bool fe_equal(const Fe<F>& a, const Fe<F>& b) {
  constexpr int NL = F::NL;
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) o |= a.l[i] ^ b.l[i];
  return o == 0;
}

template <class F>
MSM_DEV void store_row(uint32_t* row, const Fe<F>& x, const Fe<F>& y, const Fe<F>& bx) {   // y follows x: word F::NW of a line
  fe_store<F>(row, x);
  fe_store<F>(row + F::NW, y);
  fe_store<F>(row + ROW_HALF, bx);
  fe_store<F>(row + ROW_HALF + F::NW, y);
}

template <int NP>   // NP = pieces per coordinate
MSM_DEV void store_row_identity(uint32_t* row) {
  uint4* r4 = reinterpret_cast<uint4*>(row);
  const uint4 ones = make_uint4(INF_WORD, INF_WORD, INF_WORD, INF_WORD), zeros = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int j = 0; j < NP; j++) {
      r4[h * (ROW_HALF / 4) + j] = ones;
      r4[h * (ROW_HALF / 4) + NP + j] = zeros;
    }
}

// ---------------------------------------------------------------------------------------------
// k_points_from_wire: N x (x || y), 48-byte little-endian canonical integers -> point rows
// ---------------------------------------------------------------------------------------------

template <class CV>
__global__ void __launch_bounds__(256) k_points_from_wire(uint32_t* rows, const uint32_t* wire, uint64_t n,
                                                          int check_curve, uint32_t* err) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t xw[NW], yw[NW];
  load_words12(xw, wire + i * (2 * NW));
  load_words12(yw, wire + i * (2 * NW) + NW);
  uint32_t* row = rows + i * ROW_WORDS;
  uint32_t any = 0;
#pragma unroll
  for (int j = 0; j < NW; j++) any |= xw[j] | yw[j];
  if (any == 0) {  // (0, 0) is not on y^2 = x^3 + 1: used as the wire encoding of the identity
    store_row_identity<NW / 4>(row);
    return;
  }
  if (words_ge_p<F>(xw) || words_ge_p<F>(yw)) atomicOr(err, 1u);
  Fe<F> x, y, r2, beta, bx;
  fe_unpack<F>(x, xw);
  fe_unpack<F>(y, yw);
#pragma unroll
  for (int l = 0; l < NL; l++) { r2.l[l] = F::R2[l]; beta.l[l] = F::BETAL[l]; }
  fe_mul<F>(x, x, r2);
  fe_reduce_2p<F>(x);
  fe_mul<F>(y, y, r2);
  fe_reduce_2p<F>(y);
  fe_mul<F>(bx, x, beta);
  fe_reduce_2p<F>(bx);
  if (check_curve) {
    Fe<F> lhs, rhs, bb;
#pragma unroll
    for (int l = 0; l < NL; l++) bb.l[l] = F::BL[l];
    fe_sqr<F>(lhs, y);
    fe_sqr<F>(rhs, x);
    fe_mul<F>(rhs, rhs, x);
    fe_add<F>(rhs, rhs, bb);          // < 3p
    fe_sub_4p<F>(lhs, lhs, rhs);      // < 6p: reduce by 4p first
    fe_cond_sub<F, 4>(lhs);
    if (!fe_is_zero_mod_p<F>(lhs)) atomicOr(err, 2u);
  }
  store_row(row, x, y, bx);
}

// ---------------------------------------------------------------------------------------------
// k_table_next: window tables.  Row i of table k holds 2^(c k) P_i (with its beta x line), so that the digit of window k
// addresses a point that already carries the window's weight: all K windows of an MSM then share ONE set of buckets
// (sum_k 2^(c k) sum_i d_ik P_i = sum_(i,k) d_ik T_k[i]) -- K times fewer buckets to finish and reduce, no Horner step.
// The reference keeps no such tables (its memory is 4 GiB of wasm heap); 288 GB of HBM hold six of them for 2^26 points.
// One launch makes table k from table k - 1: c projective doublings (dbl-1998-cmo-2, src/curve-projective.ts:202-253) and
// one inversion per point.  Built once per point set and plan, like the beta x of k_points_from_wire.
// ---------------------------------------------------------------------------------------------

template <class CV>
__global__ void __launch_bounds__(256) k_table_next(uint32_t* rows_out, const uint32_t* rows_in, uint64_t n, int c) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t xw[NW], yw[NW];
  load_words12(xw, rows_in + i * ROW_WORDS);
  load_words12(yw, rows_in + i * ROW_WORDS + NW);
  uint32_t* out = rows_out + i * ROW_WORDS;
  if (xw[NW - 1] == INF_WORD) {
    store_row_identity<NW / 4>(out);
    return;
  }
  Proj<F> P;
  fe_unpack<F>(P.X, xw);
  fe_unpack<F>(P.Y, yw);
  fe_set_one<F>(P.Z);
#pragma unroll 1
  for (int j = 0; j < c; j++) proj_double<F>(P, P);
  if (proj_is_zero<F>(P)) {   // a point of even order (outside the prime-order subgroup) doubled to the identity
    store_row_identity<NW / 4>(out);
    return;
  }
  Fe<F> zi, x, y, bx, beta;
  fe_reduce_4p<F>(P.Z);
  fe_inv<F>(zi, P.Z);
  fe_mul<F>(x, P.X, zi);
  fe_reduce_2p<F>(x);
  fe_mul<F>(y, P.Y, zi);
  fe_reduce_2p<F>(y);
#pragma unroll
  for (int l = 0; l < NL; l++) beta.l[l] = F::BETAL[l];
  fe_mul<F>(bx, x, beta);
  fe_reduce_2p<F>(bx);
  store_row(out, x, y, bx);
}

// ---------------------------------------------------------------------------------------------
// k_digits: scalars (N x 32 B LE) -> signed window digits of both GLV halves
// ---------------------------------------------------------------------------------------------

MSM_DEV bool words8_ge(const uint32_t (&a)[8], const uint32_t* q) {
  bool gt = false, lt = false;
#pragma unroll
  for (int j = 7; j >= 0; j--) {
    if (!gt && !lt) {
      if (a[j] > q[j]) gt = true;
      else if (a[j] < q[j]) lt = true;
    }
  }
  return !lt;
}

// windows [k_lo, k_lo + k_cnt) of K_total are emitted (window groups / multi-GPU window shards)
// glv: bit 0 = endomorphism split, bit 1 = folded top window (Plan::fold, msm_api.hip): window K_total - 1 is c + 1 bits wide
// and keeps its value as it is -- at most 2^c, it cannot carry out.
// Slices: block b owns the points [b * pps, (b + 1) * pps).  slice_hist != nullptr (the bin split of big windows): the block also
// counts, per window, the coarse bins ((l - 1) >> ws.fb[kk]) of the digits it writes -- in the LDS, `hb` counters per window -- and
// leaves them in slice_hist[(kk * gridDim.x + b) * hb + bin]: the digits are in registers here, a separate histogram pass would
// read all of them again.
// b_lo, b_n: the bucket-range shard of a multi-GPU run -- only digits whose bucket index l - 1 lies in [b_lo, b_lo + b_n) are
// kept, the others become "no entry" (0) and are never sorted (the whole range: 0, 0xFFFFFFFF); bt_lo, bt_n: the same for the
// TOP window, whose digits cover another range than the recoded ones (twice as many buckets when folded, fewer when short).
// fbp: the fine bits of the group's windows, four bits each (WinSplit::fb packed: a register shift instead of a load from the
// kernel arguments per digit)
// cache policy of the digit stream k_digits writes (mem_policy.h): written once, read once by the sort.  Non-temporal: +0.1 ms of
// 127.4 at 2^26 points, inside the noise (profiles/stream_policy_time.txt)
struct DigPol {
  static constexpr MemPol OUT = MemPol::DEFAULT;
};
MSM_DEV void digit_note(uint32_t* lds_hist, uint32_t hb, uint64_t fbp, int kk, uint32_t l) {
  if (lds_hist && l) atomicAdd(&lds_hist[(uint32_t)kk * hb + ((l - 1) >> ((uint32_t)(fbp >> (4 * kk)) & 15u))], 1u);
}
inline uint64_t pack_fine_bits(const WinSplit& ws) {
  uint64_t v = 0;
  for (int kk = 0; kk < 16; kk++) v |= (uint64_t)(ws.fb[kk] & 15u) << (4 * kk);
  return v;
}
// The frame of the slice histogram around a digit kernel's loop: the block's `cells` = k_cnt * hb LDS counters zeroed (nullptr:
// the launch wants no histogram), and after the loop written to their row of slice_hist.
__device__ __forceinline__ uint32_t* slice_hist_begin(const uint32_t* slice_hist, uint32_t cells) {
  extern __shared__ uint32_t lds_dig_hist[];
  if (!slice_hist) return nullptr;
  for (uint32_t j = threadIdx.x; j < cells; j += blockDim.x) lds_dig_hist[j] = 0;
  __syncthreads();
  return lds_dig_hist;
}
__device__ __forceinline__ void slice_hist_end(uint32_t* slice_hist, const uint32_t* lds_hist, uint32_t cells, uint32_t hb) {
  if (!lds_hist) return;
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < cells; j += blockDim.x) {
    const uint32_t kk = j / hb, h = j - kk * hb;
    slice_hist[((uint64_t)kk * gridDim.x + blockIdx.x) * hb + h] = lds_hist[j];
  }
}
// s = the 32-byte scalar at src.  Inputs are specified < q (src/curve-random.ts:151-194); larger values are reduced mod q -- the
// group element is the same, MAX_SUB subtractions suffice (2^256 < 16 q on the Weierstrass curves, < 56 q on the Edwards one)
// -- unless the caller asked for strict checking (msm_opts.strict), in which case the call fails with MSM_ERR_SCALAR.
// k_te_digits and k_te_digits_batch call it; k_digits and k_digits_batch spell the same five lines out, because behind the call
// their BN254 instances were allocated two more VGPRs than the kernels they replace.
template <int MAX_SUB>
__device__ __forceinline__ void load_scalar_mod_q(uint32_t (&s)[8], const uint32_t* src, const uint32_t (&q)[8], int strict, uint32_t* err) {
  load_words12<8>(s, src);
  if (words8_ge(s, q)) {
    if (strict) atomicOr(err, 4u);
    for (int it = 0; it < MAX_SUB && words8_ge(s, q); it++) bn_addsub<8, 8>(s, q, true);
  }
}
// One step of the signed-window recoding, L = 2^(c-1): `raw` = the window's c bits plus `carry` from the window below; a digit
// above L becomes 2 L - l with a carry into the next window.  A folded top window (Plan::fold: raw = c + 1 bits) is not
// recoded -- at most 2^c, it cannot carry out; its value stays within its 2^c buckets only while the scalar (the GLV half) stays
// below its bound, so a larger one sets `over` (the caller flags err bit 8: MSM_ERR_INTERNAL) and is clamped to the last bucket.
MSM_DEV uint32_t window_step(uint32_t raw, uint32_t& carry, uint32_t L, bool folded_top, bool& over) {
  uint32_t l = raw + carry;
  if (!folded_top && l > L) { l = 2 * L - l; carry = 1; } else { carry = 0; }
  if (folded_top) { over |= l > 2 * L; l = l > 2 * L ? 2 * L : l; }
  return l;
}

template <class CV>
__global__ void __launch_bounds__(1024) k_digits(uint32_t* dig, const uint32_t* scalars, uint32_t n, int c, int k_total,
                                                int k_lo, int k_cnt, int glv_flags, int strict, uint32_t* err, uint32_t pps,
                                                uint32_t* slice_hist, uint32_t hb, uint64_t fbp, uint32_t b_lo, uint32_t b_n, uint32_t bt_lo,
                                                uint32_t bt_n) {
  uint32_t* lds_hist = slice_hist_begin(slice_hist, (uint32_t)k_cnt * hb);
  const int glv = glv_flags & 1;
  const bool fold = glv_flags & 2;
  const uint64_t p_end = min((uint64_t)(blockIdx.x + 1) * pps, (uint64_t)n);
  for (uint64_t i64 = (uint64_t)blockIdx.x * pps + threadIdx.x; i64 < p_end; i64 += blockDim.x) {
  const uint32_t i = (uint32_t)i64;
  uint32_t s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; j++) q[j] = CV::G::Q[j];
  load_words12<8>(s, scalars + (uint64_t)i * 8);
  if (words8_ge(s, q)) {   // (load_scalar_mod_q<16>, spelt out: see there)
    if (strict) atomicOr(err, 4u);
    for (int it = 0; it < 16 && words8_ge(s, q); it++) bn_addsub<8, 8>(s, q, true);
  }

  const uint32_t L = 1u << (c - 1);
  const uint64_t two_n = 2ull * n;
  if (!glv) {
    // msmBasic / msmProjective window structure (src/msm-basic.ts:72-91): signed digits of the whole scalar on the
    // first entry of the point; the endomorphism entry stays empty (digit 0 is never sorted)
    uint32_t carry = 0;
    for (int k = 0; k < k_total; k++) {
      const bool top = fold && k == k_total - 1;
      bool over = false;
      uint32_t l = window_step(bn_take_bits<8>(s, top ? c + 1 : c), carry, L, top, over);
      if (over) atomicOr(err, 8u);
      uint32_t sgn = carry;
      if (l - 1 - (k == k_total - 1 ? bt_lo : b_lo) >= (k == k_total - 1 ? bt_n : b_n)) { l = 0; sgn = 0; }
      int kk = k - k_lo;
      if (kk >= 0 && kk < k_cnt) {
        *reinterpret_cast<uint2*>(dig + (uint64_t)kk * two_n + 2ull * i) = make_uint2(l | (sgn << 31), 0u);
        digit_note(lds_hist, hb, fbp, kk, l);
      }
    }
    continue;
  }
  GlvHalf h[2];
  glv_decompose<typename CV::G>(h[0], h[1], s);
  // both halves of a window leave as ONE 8-byte store (entries 2 i and 2 i + 1 are neighbours): 4-byte stores a dword apart
  // ran the kernel at half the streaming rate
  uint32_t carry0 = 0, carry1 = 0;
  for (int k = 0; k < k_total; k++) {
    const bool top = fold && k == k_total - 1;
    bool over = false;
    const uint32_t l0 = window_step(bn_take_bits<4>(h[0].mag, top ? c + 1 : c), carry0, L, top, over);
    const uint32_t l1 = window_step(bn_take_bits<4>(h[1].mag, top ? c + 1 : c), carry1, L, top, over);
    if (over) atomicOr(err, 8u);
    const int kk = k - k_lo;
    if (kk >= 0 && kk < k_cnt) {
      uint32_t neg0 = carry0 ^ (h[0].neg ? 1u : 0u), neg1 = carry1 ^ (h[1].neg ? 1u : 0u);
      uint32_t e0 = l0, e1 = l1;
      const uint32_t f_lo = k == k_total - 1 ? bt_lo : b_lo, f_n = k == k_total - 1 ? bt_n : b_n;
      if (e0 - 1 - f_lo >= f_n) { e0 = 0; neg0 = 0; }
      if (e1 - 1 - f_lo >= f_n) { e1 = 0; neg1 = 0; }
      mem_store8<DigPol::OUT>(dig + (uint64_t)kk * two_n + 2ull * i, make_uint2(e0 | (neg0 << 31), e1 | (neg1 << 31)));
      digit_note(lds_hist, hb, fbp, kk, e0);
      digit_note(lds_hist, hb, fbp, kk, e1);
    }
  }
  }
  slice_hist_end(slice_hist, lds_hist, (uint32_t)k_cnt * hb, hb);
}

// ---------------------------------------------------------------------------------------------
// k_digits_batch: the digits of several scalar vectors over the same points (msm_run_batch, msm_batch.hip)
// ---------------------------------------------------------------------------------------------

// the scalar vectors of one fused group, passed in the kernel arguments: a group holds at most 128 windows of K >= 8
// (c <= 16), so at most 16 elements
constexpr int BATCH_MAX = 16;
struct BatchScalars {
  const uint32_t* p[BATCH_MAX];   // n x 8 words each
};

// Element b's window k is "virtual window" b K + k of the group: dig[(b K + k) * 2n + 2 i + {0, 1}], the [window][entry] layout
// k_digits writes, so the sort and the tree take the group as b_cnt K ordinary windows.  The top-window rules (fold, err) are
// those of window k of its own element.  One thread per point, its scalars decomposed one after the other.  No slice histogram
// and no bucket-range shard: a fused batch always takes the one-level sort over the whole bucket range.
template <class CV>
__global__ void __launch_bounds__(256) k_digits_batch(uint32_t* dig, BatchScalars sc, uint32_t b_cnt, uint32_t n, int c, int k_total,
                                                      int glv_flags, int strict, uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int glv = glv_flags & 1;
  const bool fold = glv_flags & 2;
  const uint32_t L = 1u << (c - 1);
  const uint64_t two_n = 2ull * n;
  uint32_t q[8];
#pragma unroll
  for (int j = 0; j < 8; j++) q[j] = CV::G::Q[j];
#pragma unroll 1
  for (uint32_t b = 0; b < b_cnt; b++) {
    uint32_t s[8];
    load_words12<8>(s, sc.p[b] + (uint64_t)i * 8);
    if (words8_ge(s, q)) {   // (load_scalar_mod_q<16>, spelt out: see there)
      if (strict) atomicOr(err, 4u);
      for (int it = 0; it < 16 && words8_ge(s, q); it++) bn_addsub<8, 8>(s, q, true);
    }
    uint32_t* db = dig + (uint64_t)b * k_total * two_n + 2ull * i;
    if (!glv) {
      uint32_t carry = 0;
      for (int k = 0; k < k_total; k++) {
        const bool top = fold && k == k_total - 1;
        bool over = false;
        const uint32_t l = window_step(bn_take_bits<8>(s, top ? c + 1 : c), carry, L, top, over);
        if (over) atomicOr(err, 8u);
        *reinterpret_cast<uint2*>(db + (uint64_t)k * two_n) = make_uint2(l | ((l ? carry : 0u) << 31), 0u);
      }
      continue;
    }
    GlvHalf h[2];
    glv_decompose<typename CV::G>(h[0], h[1], s);
    uint32_t carry0 = 0, carry1 = 0;
    for (int k = 0; k < k_total; k++) {
      const bool top = fold && k == k_total - 1;
      bool over = false;
      const uint32_t l0 = window_step(bn_take_bits<4>(h[0].mag, top ? c + 1 : c), carry0, L, top, over);
      const uint32_t l1 = window_step(bn_take_bits<4>(h[1].mag, top ? c + 1 : c), carry1, L, top, over);
      if (over) atomicOr(err, 8u);
      const uint32_t neg0 = l0 ? carry0 ^ (h[0].neg ? 1u : 0u) : 0u, neg1 = l1 ? carry1 ^ (h[1].neg ? 1u : 0u) : 0u;
      *reinterpret_cast<uint2*>(db + (uint64_t)k * two_n) = make_uint2(l0 | (neg0 << 31), l1 | (neg1 << 31));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// projective points in raw limb form (3 x 13 words) between the reduction kernels: what k_bucket_finish writes and
// tools/ubench_bt.hip reads (the reduction kernels go through ProjPT below)
// ---------------------------------------------------------------------------------------------

template <class F>
MSM_DEV void proj_store(uint32_t* dst, const Proj<F>& P) {
  constexpr int NL = F::NL;
#pragma unroll
  for (int l = 0; l < NL; l++) { dst[l] = P.X.l[l]; dst[NL + l] = P.Y.l[l]; dst[2 * NL + l] = P.Z.l[l]; }
}

// "planar" form for arrays that consecutive lanes walk together: word w of element j at base[w * stride + j]
template <class F>
MSM_DEV void proj_load_planar(Proj<F>& P, const uint32_t* base, uint64_t stride, uint64_t j) {
  constexpr int NL = F::NL;
#pragma unroll
  for (int l = 0; l < NL; l++) {
    P.X.l[l] = base[(uint64_t)l * stride + j];
    P.Y.l[l] = base[(uint64_t)(NL + l) * stride + j];
    P.Z.l[l] = base[(uint64_t)(2 * NL + l) * stride + j];
  }
}

// ---------------------------------------------------------------------------------------------
// k_bucket_finish: once every bucket is down to a handful of elements the remaining tree rounds are pure
// latency (one shared inversion per launch for a few additions per lane).  This kernel ends the accumulation
// in one launch instead: one lane per bucket sums its remaining affine elements with mixed projective
// additions -- no inversion at all -- and leaves the bucket sum in projective form for k_bucket_reduce.
// ---------------------------------------------------------------------------------------------

template <class CV>
__global__ void __launch_bounds__(256) k_bucket_finish(uint32_t* bucket_proj, const uint4* in, uint64_t in_cap,
                                                       const uint32_t* off, uint32_t nb, const uint32_t* perm) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW, NP = F::NW / 4;
  uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  if (perm) b = perm[b];   // buckets ordered by remaining count (k_finish_perm): equal trip counts inside a wave
  const uint32_t o0 = off[b], o1 = off[b + 1];
  Proj<F> acc;
  proj_set_zero<F>(acc);
  // the next element's words are in flight while the current one is added (lanes read 16-byte pieces a bucket
  // length apart: nothing coalesces, so the latency has to be covered by arithmetic)
  uint32_t nx[NW], ny[NW];
  if (o0 < o1) {
    load_planes3(nx, in, in_cap, 0, o0);
    load_planes3(ny, in, in_cap, NP, o0);
  }
#pragma unroll 1
  for (uint32_t o = o0; o < o1; o++) {
    Proj<F> Q;
    const bool qinf = nx[NW - 1] == INF_WORD;
    fe_unpack<F>(Q.X, nx);
    fe_unpack<F>(Q.Y, ny);
    if (o + 1 < o1) {
      load_planes3(nx, in, in_cap, 0, o + 1);
      load_planes3(ny, in, in_cap, NP, o + 1);
    }
    proj_add_mixed<F>(acc, acc, Q, qinf);
  }
  proj_store(bucket_proj + (uint64_t)b * (3 * NL), acc);
}

// ---------------------------------------------------------------------------------------------
// The bucket reduction P_k = sum_l l B_(k,l) over the bucket sums of k_bucket_finish, for both kinds of point: every stage is
// one body over a point-kind policy PT, and a kernel per kind around it with its own __shared__ array.  What a kind of point
// offers: the point P, its W raw words between the reduction kernels (word w = limb w of the point as it sits in registers),
// the identity, the group addition and doubling, and the packed window sum of PW words the host reads.
// ProjPT<F>: projective points of a Weierstrass curve; TePT (te_kernels.h): extended points of the Edwards curve.
// ---------------------------------------------------------------------------------------------

template <class F>
struct ProjPT {
  using P = Proj<F>;
  static constexpr int W = 3 * F::NL;
  static constexpr int PW = PART_WORDS;
  static MSM_DEV void zero(P& p) { proj_set_zero<F>(p); }
  static MSM_DEV void add(P& r, const P& a, const P& b) { proj_add<F>(r, a, b); }
  static MSM_DEV void dbl(P& r, const P& a) { proj_double<F>(r, a); }
  static MSM_DEV uint32_t& word(P& p, int w) { return w < F::NL ? p.X.l[w] : w < 2 * F::NL ? p.Y.l[w - F::NL] : p.Z.l[w - 2 * F::NL]; }
  // 3 x 12 packed canonical Montgomery words (X, Y, Z)
  static MSM_DEV void pack(uint32_t* dst, P& acc) {
    constexpr int NW = F::NW;
    fe_reduce_2p<F>(acc.X);
    fe_reduce_2p<F>(acc.Y);
    fe_reduce_2p<F>(acc.Z);
    uint32_t w[NW];
#pragma unroll
    for (int j = 0; j < PART_WORDS; j++) dst[j] = 0;
    fe_pack<F>(w, acc.X);
#pragma unroll
    for (int j = 0; j < NW; j++) dst[j] = w[j];
    fe_pack<F>(w, acc.Y);
#pragma unroll
    for (int j = 0; j < NW; j++) dst[12 + j] = w[j];
    fe_pack<F>(w, acc.Z);
#pragma unroll
    for (int j = 0; j < NW; j++) dst[24 + j] = w[j];
  }
};

// a point as W raw words in a row ...
template <class PT>
MSM_DEV void pt_load(typename PT::P& p, const uint32_t* src) {
#pragma unroll
  for (int w = 0; w < PT::W; w++) PT::word(p, w) = src[w];
}
template <class PT>
MSM_DEV void pt_store(uint32_t* dst, typename PT::P& p) {
#pragma unroll
  for (int w = 0; w < PT::W; w++) dst[w] = PT::word(p, w);
}
// ... and in the planar form of arrays that consecutive lanes walk together
template <class PT>
MSM_DEV void pt_load_planar(typename PT::P& p, const uint32_t* base, uint64_t stride, uint64_t j) {
#pragma unroll
  for (int w = 0; w < PT::W; w++) PT::word(p, w) = base[(uint64_t)w * stride + j];
}
template <class PT>
MSM_DEV void pt_store_planar(uint32_t* base, uint64_t stride, uint64_t j, typename PT::P& p) {
#pragma unroll
  for (int w = 0; w < PT::W; w++) base[(uint64_t)w * stride + j] = PT::word(p, w);
}

// k_bucket_reduce / k_te_bucket_reduce (normalizeBucketsStorage + reduceBucketsColumnProjective; Edwards: reduceBucketsChunk,
// src/msm-basic.ts:180-211): lane (kk, ch) walks the TC buckets of chunk ch of window kk from the top; `row` is the running
// sum of the bucket sums, `tri` the sum of the running sums = sum_l (l - lstart + 1) B_l, the chunk's local triangle.
// rows == nullptr: the lane applies the weight (lstart - 1) = ch * TC to `row` by double-and-add and writes the chunk's
// column to columns[id].
// rows != nullptr: "bit-sliced" mode -- the chunk's plain sum is written to rows and its local triangle to columns, both
// planar ([window][word][chunk]: lanes = consecutive chunks write and k_bit_tree reads coalesced); the weight is applied
// later through per-bit sums (k_bit_tree) instead of a double-and-add chain in every lane.
template <class PT>
MSM_DEV void bucket_reduce_body(uint32_t* columns, uint32_t* rows, const uint32_t* bucket_sums, uint32_t L, uint32_t TC,
                                uint32_t nchunks, uint32_t k_cnt) {
  using P = typename PT::P;
  constexpr int W = PT::W;
  uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nchunks * k_cnt) return;
  uint32_t kk = id / nchunks, ch = id - kk * nchunks;
  uint32_t lstart = ch * TC + 1;                       // bucket indices l are 1-based
  uint32_t lend = min(lstart + TC - 1, L);
  P row, tri;
  PT::zero(row);
  PT::zero(tri);
#pragma unroll 1
  for (uint32_t l = lend; l >= lstart; l--) {
    P Q;
    pt_load<PT>(Q, bucket_sums + ((uint64_t)kk * L + (l - 1)) * W);
    PT::add(row, row, Q);
    PT::add(tri, tri, row);
  }
  if (rows) {
    pt_store_planar<PT>(rows + (uint64_t)kk * W * nchunks, nchunks, ch, row);
    pt_store_planar<PT>(columns + (uint64_t)kk * W * nchunks, nchunks, ch, tri);
    return;
  }
  uint32_t ls = lstart - 1;
  if (ls) {
#pragma unroll 1
    while (true) {
      if (ls & 1) PT::add(tri, tri, row);
      ls >>= 1;
      if (ls == 0) break;
      PT::dbl(row, row);
    }
  }
  pt_store<PT>(columns + (uint64_t)id * W, tri);
}

template <class CV>
__global__ void __launch_bounds__(64) k_bucket_reduce(uint32_t* columns, uint32_t* rows, const uint32_t* bucket_proj, uint32_t L,
                                                       uint32_t TC, uint32_t nchunks, uint32_t k_cnt) {
  bucket_reduce_body<ProjPT<typename CV::F>>(columns, rows, bucket_proj, L, TC, nchunks, k_cnt);
}

// k_window_sum / k_te_window_sum: P_k = sum of the window's columns (the partition sums, :312-319); one workgroup per
// window, the packed sum to partials[kk]
constexpr int WS_THREADS = 256;

template <class PT>
MSM_DEV void window_sum_body(uint32_t* partials, const uint32_t* columns, uint32_t nchunks, uint32_t* lds) {
  using P = typename PT::P;
  constexpr int W = PT::W;
  const uint32_t kk = blockIdx.x, tid = threadIdx.x;
  P acc;
  PT::zero(acc);
#pragma unroll 1
  for (uint32_t j = tid; j < nchunks; j += WS_THREADS) {
    P Q;
    pt_load<PT>(Q, columns + ((uint64_t)kk * nchunks + j) * W);
    PT::add(acc, acc, Q);
  }
#pragma unroll 1
  for (uint32_t s = WS_THREADS / 2; s >= 1; s >>= 1) {
    if (tid >= s && tid < 2 * s) pt_store_planar<PT>(lds, WS_THREADS, tid, acc);
    __syncthreads();
    if (tid < s) {
      P Q;
      pt_load_planar<PT>(Q, lds, WS_THREADS, tid + s);
      PT::add(acc, acc, Q);
    }
    __syncthreads();
  }
  if (tid == 0) PT::pack(partials + (uint64_t)kk * PT::PW, acc);
}

template <class CV>
__global__ void __launch_bounds__(WS_THREADS) k_window_sum(uint32_t* partials, const uint32_t* columns, uint32_t nchunks) {
  __shared__ uint32_t lds[ProjPT<typename CV::F>::W * WS_THREADS];
  window_sum_body<ProjPT<typename CV::F>>(partials, columns, nchunks, lds);
}

// Bit-sliced weighting of the chunk sums:  sum_ch (ch * TC) * row_ch = TC * sum_b 2^b * S_b  with S_b = sum of row_ch over
// the chunks whose index has bit b set; a window has nchunks = 2^nbits chunks, nbits >= 6 (reduce_buckets).  The nbits sums
// S_b and the sum of the local triangles go to the host, which applies the 2^b weights with nbits doublings per window -- one
// chain per window instead of one per lane (the reference applies the same weight by double-and-add per chunk,
// src/msm-batched-affine.ts:574-580).
//
// Adding every row to half of the nbits sums would take nchunks * nbits / 2 additions.  With the chunk index cut as
// ch = hi * M_lo + lo,  sum_ch ch * row_ch = M_lo * sum_hi hi * A_hi + sum_lo lo * B_lo  with A_hi = sum_lo row (a run of M_lo
// rows) and B_lo = sum_hi row (a column of M_hi rows): 2 * nchunks additions, and the bit-sliced weighting then runs over the
// M_hi + M_lo sums only -- S_b = masked sum over B for the low bits, over A for the high ones.
//   stage 0: grid (M_hi + M_lo + nblk_out, 1, kc): block -> A_hi | B_lo | a share of the n_in local triangles; raw points to
//            out[kk][M_hi + M_lo + nblk_out]
//   stage 1: grid (1, nbits + 1, kc) over those (`rows` = the first stage's output): y < h0: bit y of lo over B;
//            y < nbits: bit y - h0 of hi over A; y == nbits: the nblk_out triangle shares; packed sums to out[kk][nbits + 1]
//
// One wave per block: every lane adds a few elements serially, then the lane sums are folded through LDS in log2 steps.  A
// projective addition is ~7000 dependent VALU instructions (15 us for a lone wave), so what matters is the number of
// additions in sequence, not their count.
// Every lane takes part in every addition: a wave whose EXEC mask is down to a few lanes runs this arithmetic up to 3.5x
// slower per instruction when the chip is busy (tools/ubench_exec.hip), so the usual halving tree -- 32, 16, ... 1 active
// lanes -- is the worst shape.  Instead the lanes form groups of m = min(64, 2^ceil(log2 count)) lanes, each group sums all
// elements of the block (64 / m groups do the same work redundantly), and the fold is a cyclic all-reduce inside the group:
// after log2 m steps every lane holds the total.
constexpr int BT_THREADS = 64;

template <class PT>
MSM_DEV void bit_tree_body(uint32_t* out, const uint32_t* rows, const uint32_t* tris, uint32_t n_in, uint32_t nbits, int stage,
                           uint32_t nblk_out, uint32_t* lds) {
  using P = typename PT::P;
  constexpr int W = PT::W;
  const uint32_t blk = blockIdx.x, y = blockIdx.y, kk = blockIdx.z, tid = threadIdx.x;
  const uint32_t h1 = nbits / 2, h0 = nbits - h1, M_lo = 1u << h0, M_hi = 1u << h1, per_kk = M_hi + M_lo + nblk_out;
  uint32_t count, kind;   // kind 0: A run, 1: B column, 2: triangle share (stage 0); 3: masked over stage-0 slots, 4: plain over slots
  uint32_t a0 = 0, a1 = 0;
  if (stage == 0) {
    if (blk < M_hi) { kind = 0; count = M_lo; a0 = blk * M_lo; }
    else if (blk < M_hi + M_lo) { kind = 1; count = M_hi; a0 = blk - M_hi; }
    else {
      kind = 2;
      const uint32_t t = blk - M_hi - M_lo, span = (n_in + nblk_out - 1) / nblk_out;
      a0 = min(t * span, n_in);
      count = min(a0 + span, n_in) - a0;
    }
  } else {
    if (y < h0) { kind = 3; count = M_lo >> 1; a0 = M_hi; a1 = y; }
    else if (y < nbits) { kind = 3; count = M_hi >> 1; a0 = 0; a1 = y - h0; }
    else { kind = 4; count = nblk_out; a0 = M_hi + M_lo; }
  }
  uint32_t m = 1;
  while (m < count && m < BT_THREADS) m <<= 1;
  const uint32_t gl = tid & (m - 1);
  P acc;
  PT::zero(acc);
#pragma unroll 1
  for (uint32_t i = gl; i < count; i += m) {
    P Q;
    if (kind <= 2) {
      const uint32_t j = kind == 1 ? i * M_lo + a0 : a0 + i;
      pt_load_planar<PT>(Q, (kind == 2 ? tris : rows) + (uint64_t)kk * W * n_in, n_in, j);
    } else {
      // i-th index with bit a1 set: insert a one at bit position a1
      const uint32_t j = kind == 3 ? ((((i >> a1) << 1) | 1u) << a1) | (i & ((1u << a1) - 1u)) : i;
      pt_load<PT>(Q, rows + ((uint64_t)kk * per_kk + a0 + j) * W);
    }
    PT::add(acc, acc, Q);
  }
#pragma unroll 1
  for (uint32_t s = m >> 1; s >= 1; s >>= 1) {
    pt_store_planar<PT>(lds, BT_THREADS, tid, acc);
    __syncthreads();
    const uint32_t partner = (tid & ~(m - 1)) | ((gl + s) & (m - 1));
    P Q;
    pt_load_planar<PT>(Q, lds, BT_THREADS, partner);
    __syncthreads();
    PT::add(acc, acc, Q);
  }
  if (tid == 0) {
    if (stage == 0) pt_store<PT>(out + ((uint64_t)kk * per_kk + blk) * W, acc);
    else PT::pack(out + ((uint64_t)kk * (nbits + 1) + y) * PT::PW, acc);
  }
}

// amdgpu_waves_per_eu(1, 1): one wave per SIMD.  The work is a chain of dependent additions per wave; a second wave on
// the same SIMD halves the speed of both, and the dispatcher fills a SIMD before it moves to the next one (measured:
// 40 us per addition in sequence with two resident waves against 19 us alone).
template <class CV>
__global__ void __launch_bounds__(BT_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) k_bit_tree(uint32_t* out, const uint32_t* rows, const uint32_t* tris,
                                                         uint32_t n_in, uint32_t nbits, int stage, uint32_t nblk_out) {
  __shared__ uint32_t lds[ProjPT<typename CV::F>::W * BT_THREADS];
  bit_tree_body<ProjPT<typename CV::F>>(out, rows, tris, n_in, nbits, stage, nblk_out, lds);
}


// ---------------------------------------------------------------------------------------------
// test kernels: element-wise field / curve / GLV operations for parity tests against the oracle
// (the fine-grained operator table of src/field-msm.ts:86-123 as a GPU debug surface)
// ---------------------------------------------------------------------------------------------

enum : int { OP_MUL = 0, OP_SQR = 1, OP_ADD = 2, OP_SUB = 3, OP_INV = 4, OP_TO_MONT = 5, OP_FROM_MONT = 6,
             OP_INV_FERMAT = 7, OP_INV_KALISKI = 8, OP_INV_WORDSLICED = 9 };

// a, b, out: n x 12 packed words; values are canonical Montgomery form unless the op says otherwise
template <class CV>
__global__ void __launch_bounds__(256) k_test_fp(uint32_t* out, const uint32_t* a, const uint32_t* b, uint32_t n, int op) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW, NP = F::NW / 4;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<F> x, y, r;
  fe_load<F>(x, a + (uint64_t)i * NW);
  fe_load<F>(y, b + (uint64_t)i * NW);
  switch (op) {
    case OP_MUL: fe_mul<F>(r, x, y); break;
    case OP_SQR: fe_sqr<F>(r, x); break;
    case OP_ADD: fe_add<F>(r, x, y); break;
    case OP_SUB: fe_sub_p<F>(r, x, y); break;
    case OP_INV: fe_inv<F>(r, x); break;
    case OP_INV_FERMAT: fe_inv_fermat<F>(r, x); break;     // the inversion variants of SURVEY section 8(f)-3
    case OP_INV_KALISKI: fe_inv_kaliski<F>(r, x); break;
    case OP_INV_WORDSLICED: fe_inv_wordsliced<F>(r, x); break;   // src/inverse/faster-inverse-wasm.ts:133-343
    case OP_TO_MONT: {
      Fe<F> r2;
#pragma unroll
      for (int l = 0; l < NL; l++) r2.l[l] = F::R2[l];
      fe_mul<F>(r, x, r2);
      break;
    }
    default: {
      Fe<F> one;
      fe_set_zero<F>(one);
      one.l[0] = 1;
      fe_mul<F>(r, x, one);
      break;
    }
  }
  fe_reduce_4p<F>(r);
  fe_store<F>(out + (uint64_t)i * NW, r);
}

// `batchInverse` (src/wasm/inverse.ts:220-271, JS twin src/curve-affine.ts:692-727): Montgomery's trick over a
// contiguous array; lane t inverts elements [t * per_lane, (t + 1) * per_lane) with ONE fe_inv.
// Operands and results are canonical Montgomery-form words; zeros are not allowed (as in the reference).
template <class CV>
__global__ void __launch_bounds__(256) k_test_batch_inverse(uint32_t* out, const uint32_t* xs, uint32_t n, uint32_t per_lane) {
  using F = typename CV::F;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t beg = (uint64_t)t * per_lane, end = min(beg + per_lane, (uint64_t)n);
  if (beg >= end) return;
  Fe<F> acc, x;
  fe_set_one<F>(acc);
  for (uint64_t i = beg; i < end; i++) {            // out[i] temporarily holds the prefix product before x_i
    fe_reduce_2p<F>(acc);
    fe_store<F>(out + i * F::NW, acc);
    fe_load<F>(x, xs + i * F::NW);
    fe_mul<F>(acc, acc, x);
  }
  Fe<F> inv, pre, r;
  fe_inv<F>(inv, acc);
  for (uint64_t i = end; i-- > beg;) {
    fe_load<F>(pre, out + i * F::NW);
    fe_load<F>(x, xs + i * F::NW);
    fe_mul<F>(r, inv, pre);
    fe_mul<F>(inv, inv, x);
    fe_reduce_2p<F>(r);
    fe_store<F>(out + i * F::NW, r);
  }
}

// Raw-limb multiplier test: operands are NL 30-bit limbs exactly as given -- unreduced sums, all-ones limbs -- and the
// result limbs are stored as they leave fe_mul / fe_sqr (no reduction): the worst-case side of src/field.test.ts:27-155.
template <class CV>
__global__ void __launch_bounds__(256) k_test_fp_raw(uint32_t* out, const uint32_t* a, const uint32_t* b, uint32_t n, int op) {
  using F = typename CV::F;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<F> x, y, r;
#pragma unroll
  for (int l = 0; l < F::NL; l++) { x.l[l] = a[(uint64_t)i * F::NL + l]; y.l[l] = b[(uint64_t)i * F::NL + l]; }
  if (op == OP_SQR) fe_sqr<F>(r, x);
  else fe_mul<F>(r, x, y);
#pragma unroll
  for (int l = 0; l < F::NL; l++) out[(uint64_t)i * F::NL + l] = r.l[l];
}

// Curve operators on projective points (X, Y, Z: 3 x 12 canonical plain-integer words each, any representative):
// op 0 = proj_add (general, every edge case), 1 = proj_double, 2 = proj_add_mixed (Q affine: Q.Z ignored, Q == (0, 0) is
// the identity).  Operator-level counterpart of src/curve-projective.test.ts:77-208.
enum : int { CURVE_OP_ADD = 0, CURVE_OP_DOUBLE = 1, CURVE_OP_ADD_MIXED = 2 };
template <class CV>
__global__ void __launch_bounds__(64) k_test_curve_op(uint32_t* out, const uint32_t* pp, const uint32_t* qq, uint32_t n, int op) {
  using F = typename CV::F;
  constexpr int NL = F::NL, NW = F::NW, NP = F::NW / 4;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<F> r2, one;
#pragma unroll
  for (int l = 0; l < NL; l++) r2.l[l] = F::R2[l];
  fe_set_zero<F>(one);
  one.l[0] = 1;
  Proj<F> P, Q, R;
  Fe<F>* co[6] = {&P.X, &P.Y, &P.Z, &Q.X, &Q.Y, &Q.Z};
  bool q_zero_xy = true;
  for (int j = 0; j < 6; j++) {
    const uint32_t* src = (j < 3 ? pp : qq) + (uint64_t)i * (3 * NW) + (j % 3) * NW;
    fe_load<F>(*co[j], src);
    if (j == 3 || j == 4) q_zero_xy = q_zero_xy && fe_is_zero_canonical<F>(*co[j]);
    fe_mul<F>(*co[j], *co[j], r2);      // to Montgomery form, < 1.5 p
  }
  if (op == CURVE_OP_DOUBLE) proj_double<F>(R, P);
  else if (op == CURVE_OP_ADD_MIXED) proj_add_mixed<F>(R, P, Q, q_zero_xy);
  else proj_add<F>(R, P, Q);
  Fe<F>* ro[3] = {&R.X, &R.Y, &R.Z};
  for (int j = 0; j < 3; j++) {
    fe_mul<F>(*ro[j], *ro[j], one);     // leave Montgomery form
    fe_reduce_4p<F>(*ro[j]);
    fe_store<F>(out + (uint64_t)i * (3 * NW) + j * NW, *ro[j]);
  }
}

// out: n x 10 words: |s0| (4), |s1| (4), neg0, neg1
template <class CV>
__global__ void __launch_bounds__(256) k_test_glv(uint32_t* out, const uint32_t* scalars, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = scalars[(uint64_t)i * 8 + j];
  GlvHalf h0, h1;
  glv_decompose<typename CV::G>(h0, h1, s);
  uint32_t* o = out + (uint64_t)i * 10;
#pragma unroll
  for (int j = 0; j < 4; j++) { o[j] = h0.mag[j]; o[4 + j] = h1.mag[j]; }
  o[8] = h0.neg; o[9] = h1.neg;
}

}  // namespace msm
