// Resident sumcheck over multilinear tables (msm_scalars_sumcheck_round, msm_scalars_bind, msm_scalars_eq; msm_mle.hip): the round
// polynomial of a product of tables, the binding of one variable, and the table eq(r, .), mod the group order q over the vectors of
// scalar_vec.h -- plain 32-byte little-endian integers in device memory, any value below 2^256, every element written canonical.
// The reference has no counterpart.  Templates over the scalar FIELD S (MSM_SCALAR_FIELDS), 9 limbs of 30 bits, R = 2^270.
//
// A vector of n = 2^log2n elements is a multilinear table; variable j is bit j of the index.  Pair i < n / 2 of variable `var` is
// the two rows lo(i) = ((i >> var) << (var + 1)) | (i & (2^var - 1)) and hi(i) = lo(i) + 2^var.
//
// Value bounds.  Nothing is canonicalised on load in the round kernel: the chain below is proven instead, which saves the four
// reductions per pair and vector that canonicalising would cost (about 30 instructions each, an eighth of a multiplication).
// Let q > 2^250 (the smallest modulus, Ed-on-BLS12-377's, has 251 bits), q < 2^255, and M q the smallest multiple of q that is
// >= 2^256 (M <= 55), so M q < 2^256 + q.  fe_mul takes any operands with normalised limbs and returns a value below q + a b / R.
//   lo, hi                raw, < 2^256
//   delta = hi - lo + M q in (0, 2^256 + M q), < 2^257 + q              congruent to hi - lo; never negative
//   f(t) = lo + t delta   = (1 - t) lo + t hi + t M q <= t (2^257 + q) for t >= 1: below 4 (2^257 + q) < 1.25 * 2^259 at t = 4
//                         and below 2^259 at t = 3.  Limbs stay normalised (fe_add carries), the top limb stays below 2^20.
//   first product         f f' / R < q + 1.5625 * 2^518 / 2^270 = q + 1.5625 * 2^248 < 1.4 q
//   every further product (< 2 q) f / R < q + 2 q * 1.25 * 2^259 / 2^270 < q (1 + 2^-9)
// so every term of MSM_SUMCHECK_PROD is below 2 q, and a term of m factors owes R^-(m-1).  MSM_SUMCHECK_R1CS, f0 (f1 f2 - f3):
//   P = f1 f2 / R < q + 2^518 / 2^270 < 1.25 q    (owes 1/R);   T = f3 * 1 / R <= q   (the plain constant 1: f3 owing 1/R too)
//   D = P - T + 2 q in (0, 4 q)                    f0 D / R < q + 2^259 * 4 q / 2^270 < 2 q      (owes R^-2)
// The one multiplication of f3 by a constant is what keeps the bookkeeping of the difference honest.  With m = 1 the term is
// f itself and nothing is multiplied: reduce_wide brings it below 2 q and nothing is owed.
// reduce_wide: a < 2^262 -> a - qh q in [0, 2 q), qh = (top limb * C) >> 30 with C <= 2^270 / q < C + 2: the quotient estimate is
// low by less than 2^22 * 2 / 2^30 + 2^240 / q < 1, so qh is floor(a / q) or one less.  Nine multiply-adds and a borrow chain.
// Accumulators stay below 2 q (inner_combine of scalar_vec.h); a partial is canonical; the finish multiplies by R^2 once per owed R.
// bind: delta * (r R) / R < q + (2^257 + q) q / 2^270 < 2 q, plus reduce_wide(lo) < 2 q: below 4 q, one multiplication per output.
// eq: table entries are canonical; a low-table entry is plain, a high-table entry carries s R, so their one product is plain.
#pragma once
#include "scalar_vec.h"

namespace msm {
namespace mle {

constexpr int BLOCK = 256;                   // lanes per block
constexpr uint32_t ROUND_MAX_BLOCKS = 1024;  // grid cap of k_mle_round: one partial per block and value
constexpr int MAX_VECS = 4;                  // vectors of a round
constexpr int MAX_BIND = 8;                  // vectors of a bind
constexpr int MAX_VARS = 29;                 // log2n, and the variables of an eq table

// ---------------------------------------------------------------- index maps

MSM_DEV uint64_t pair_lo(uint64_t i, uint32_t var) { return ((i >> var) << (var + 1)) | (i & ((1ull << var) - 1)); }
MSM_DEV uint64_t pair_hi(uint64_t i, uint32_t var) { return pair_lo(i, var) + (1ull << var); }

// the values a round returns: the degree of the round polynomial plus one
constexpr int round_values(int shape, int m) { return (shape == MSM_SUMCHECK_R1CS ? 3 : m) + 1; }
// factors R the sum of the terms owes
constexpr int round_owed(int shape, int m) { return shape == MSM_SUMCHECK_R1CS ? 2 : m - 1; }

// the low half-table of eq over v variables covers the variables [0, k): k = ceil(v / 2)
MSM_DEV uint32_t eq_split(uint32_t v) { return (v + 1) / 2; }

// ---------------------------------------------------------------- constants of the field

template <class S>
struct Limbs {
  uint32_t l[S::NL];
};

// M q, the smallest multiple of q that is >= 2^256, as limbs (the top limb takes what is above 2^240)
template <class S>
constexpr Limbs<S> mq_limbs() {
  Limbs<S> acc = {};
  for (int m = 0; m < 64; m++) {
    uint32_t c = 0;
    for (int i = 0; i < S::NL; i++) {
      const uint32_t t = acc.l[i] + S::P[i] + c;
      if (i + 1 < S::NL) {
        acc.l[i] = t & LMASK;
        c = t >> LB;
      } else {
        acc.l[i] = t;
      }
    }
    if (acc.l[S::NL - 1] >> 16) return acc;
  }
  return acc;
}

// C of reduce_wide: floor(2^78 / (floor(q / 2^192) + 1)) <= 2^270 / q, short of it by less than 2
template <class S>
constexpr uint32_t wide_quotient_const() {
  const unsigned __int128 top = (((unsigned __int128)S::PW[7] << 32) | S::PW[6]) + 1;
  return (uint32_t)((((unsigned __int128)1) << 78) / top);
}

// ---------------------------------------------------------------- lane bodies (host and device)

// a (normalised limbs, < 2^262) -> congruent, < 2 q
template <class S>
MSM_DEV void reduce_wide(Fe<S>& a) {
  constexpr uint32_t C = wide_quotient_const<S>();
  const uint32_t qh = (uint32_t)(((uint64_t)a.l[S::NL - 1] * C) >> LB);
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < S::NL; i++) {
    const int64_t t = (int64_t)a.l[i] - (int64_t)((uint64_t)qh * S::P[i]) + c;
    if (i + 1 < S::NL) {
      a.l[i] = (uint32_t)t & LMASK;
      c = t >> LB;   // arithmetic
    } else {
      a.l[i] = (uint32_t)t;
    }
  }
}

// r = hi - lo + M q for raw hi, lo < 2^256: never negative, < 2^257 + q
template <class S>
MSM_DEV void raw_delta(Fe<S>& r, const Fe<S>& hi, const Fe<S>& lo) {
  constexpr Limbs<S> MQ = mq_limbs<S>();
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < S::NL; i++) {
    const int32_t t = (int32_t)(hi.l[i] + MQ.l[i]) - (int32_t)lo.l[i] + c;
    if (i + 1 < S::NL) {
      c = t >> LB;  // arithmetic
      r.l[i] = (uint32_t)t & LMASK;
    } else {
      r.l[i] = (uint32_t)t;
    }
  }
}

// the rows lo and hi of one pair of one vector: f = a[lo] (the value at t = 0) and the step to t + 1
template <class S>
MSM_DEV void pair_load(Fe<S>& f, Fe<S>& delta, const uint32_t* lo, const uint32_t* hi) {
  Fe<S> h;
  fe_load<S>(f, lo);
  fe_load<S>(h, hi);
  raw_delta<S>(delta, h, f);
}

// g at the current t, below 2 q, owing round_owed(SHAPE, M) factors R
template <class S, int SHAPE, int M>
MSM_DEV void round_term(Fe<S>& g, const Fe<S> (&f)[M]) {
  if constexpr (SHAPE == MSM_SUMCHECK_R1CS) {
    static_assert(M == 4, "f0 (f1 f2 - f3)");
    Fe<S> one, t;
    fe_set_zero<S>(one);
    one.l[0] = 1;
    fe_mul<S>(g, f[1], f[2]);   // P < 1.25 q
    fe_mul<S>(t, f[3], one);    // T <= q
    fe_sub_2p<S>(g, g, t);      // D < 4 q
    fe_mul<S>(g, f[0], g);
  } else if constexpr (M == 1) {
    g = f[0];
    reduce_wide<S>(g);
  } else {
    fe_mul<S>(g, f[0], f[1]);
#pragma unroll
    for (int j = 2; j < M; j++) fe_mul<S>(g, g, f[j]);
  }
}

// the values t = T .. d of one pair: f steps from t - 1 to t without a multiplication.  T is a template parameter, not a loop
// counter: a loop over five multiplications is left rolled, and an accumulator array indexed at run time goes to scratch.
template <class S, int SHAPE, int M, int T>
MSM_DEV void round_steps(Fe<S> (&acc)[round_values(SHAPE, M)], Fe<S> (&f)[M], const Fe<S> (&delta)[M]) {
  if constexpr (T < round_values(SHAPE, M)) {
    if constexpr (T > 0) {
#pragma unroll
      for (int j = 0; j < M; j++) fe_add<S>(f[j], f[j], delta[j]);
    }
    Fe<S> g;
    round_term<S, SHAPE, M>(g, f);
    sv::inner_combine<S>(acc[T], g);
    round_steps<S, SHAPE, M, T + 1>(acc, f, delta);
  }
}

// one pair: acc[t] += g(f_0(t), ..) for t = 0 .. d; rows[j] and rows[M + j]: the rows lo and hi of vector j
template <class S, int SHAPE, int M>
MSM_DEV void round_pair(Fe<S> (&acc)[round_values(SHAPE, M)], const uint32_t* const (&rows)[2 * M]) {
  Fe<S> f[M], delta[M];
#pragma unroll
  for (int j = 0; j < M; j++) pair_load<S>(f[j], delta[j], rows[j], rows[M + j]);
  round_steps<S, SHAPE, M, 0>(acc, f, delta);
}

// the sum of the terms (< 2 q) -> the plain canonical value
template <class S, int SHAPE, int M>
MSM_DEV void round_finish(Fe<S>& r, const Fe<S>& acc) {
  Fe<S> r2;
  sv::set_const<S>(r2, S::R2);
  r = acc;
#pragma unroll
  for (int k = 0; k < round_owed(SHAPE, M); k++) fe_mul<S>(r, r, r2);   // times R each, < 2 q
  fe_reduce_2p<S>(r);
}

// dst = lo + r (hi - lo); rm: the Montgomery form of r.  Both loads come before the store: dst may be the row lo.
template <class S>
MSM_DEV void bind_lane(uint32_t* dst, const uint32_t* lo, const uint32_t* hi, const Fe<S>& rm) {
  Fe<S> f, delta;
  pair_load<S>(f, delta, lo, hi);
  fe_mul<S>(delta, delta, rm);   // r (hi - lo), < 2 q
  reduce_wide<S>(f);             // < 2 q
  fe_add<S>(f, f, delta);        // < 4 q
  fe_reduce_4p<S>(f);
  fe_store<S>(dst, f);
}

// Montgomery forms of (1 - r_j, r_j), j < MAX_VARS, as limbs: a kernel argument of k_mle_eq_tables (read with scalar loads)
template <class S>
struct EqFactors {
  uint32_t l[MAX_VARS][2][S::NL];
};

// entry a of a half-table over the variables [first, first + count): start * prod_j (bit_j(a) ? r_(first+j) : 1 - r_(first+j)),
// canonical; `count` multiplications.  start plain gives a plain entry, start in Montgomery form an entry in Montgomery form.
template <class S>
MSM_DEV void eq_entry(Fe<S>& r, const Fe<S>& start, const EqFactors<S>& fac, uint32_t first, uint32_t count, uint32_t a) {
  r = start;
#pragma unroll 1
  for (uint32_t j = 0; j < count; j++) {
    const bool bit = (a >> j) & 1u;
    Fe<S> t;
#pragma unroll
    for (int i = 0; i < S::NL; i++) t.l[i] = bit ? fac.l[first + j][1][i] : fac.l[first + j][0][i];
    fe_mul<S>(r, r, t);            // < 2 q
  }
  fe_reduce_2p<S>(r);
}

// dst = T_hi[i >> k] * T_lo[i & (2^k - 1)]: one multiplication, one store
template <class S>
MSM_DEV void eq_lane(uint32_t* dst, const uint32_t* t_lo, const uint32_t* t_hi) {
  Fe<S> a, b;
  fe_load<S>(a, t_lo);
  fe_load<S>(b, t_hi);
  fe_mul<S>(a, a, b);
  fe_reduce_2p<S>(a);
  fe_store<S>(dst, a);
}

// ---------------------------------------------------------------- kernels

template <int M>
struct RoundVecs {
  const uint32_t* a[M];
};

// the sums of the block's accumulators (each < 2 q), valid in thread 0: down the wave by shuffles, across the waves through the LDS
template <class S, int NV>
__device__ __forceinline__ void block_sums(Fe<S> (&acc)[NV]) {
  constexpr int NL = S::NL, WAVES = BLOCK / 64;
  __shared__ uint32_t part[NV][WAVES][NL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < NV; v++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      Fe<S> o;
#pragma unroll
      for (int j = 0; j < NL; j++) o.l[j] = (uint32_t)__shfl_down((int)acc[v].l[j], off, 64);
      sv::inner_combine<S>(acc[v], o);   // (lanes whose partner lies outside the wave add their own value: never read)
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < NL; j++) part[v][wave][j] = acc[v].l[j];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < NV; v++) {
#pragma unroll 1
      for (int w = 1; w < WAVES; w++) {
        Fe<S> o;
#pragma unroll
        for (int j = 0; j < NL; j++) o.l[j] = part[v][w][j];
        sv::inner_combine<S>(acc[v], o);
      }
    }
  }
}

// partials[t * gridDim.x + block] = the block's share of value t over a grid-stride walk of the h pairs, canonical, still owing
// its factors R.  A lane whose first pair index is >= h contributes zeros.
template <class S, int SHAPE, int M>
__global__ void __launch_bounds__(BLOCK) k_mle_round(uint32_t* partials, RoundVecs<M> vecs, uint64_t h, uint32_t var) {
  constexpr int NV = round_values(SHAPE, M);
  Fe<S> acc[NV];
#pragma unroll
  for (int t = 0; t < NV; t++) fe_set_zero<S>(acc[t]);
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < h; i += stride) {
    const uint64_t lo = pair_lo(i, var), hi = lo + (1ull << var);
    const uint32_t* rows[2 * M];
#pragma unroll
    for (int j = 0; j < M; j++) {
      rows[j] = vecs.a[j] + 8 * lo;
      rows[M + j] = vecs.a[j] + 8 * hi;
    }
    round_pair<S, SHAPE, M>(acc, rows);
  }
  block_sums<S, NV>(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int t = 0; t < NV; t++) {
      fe_reduce_2p<S>(acc[t]);
      fe_store<S>(partials + 8 * ((uint64_t)t * gridDim.x + blockIdx.x), acc[t]);
    }
  }
}

// out[t] = round_finish(acc[t]) for t = T .. d (a template parameter for the reason given at round_steps)
template <class S, int SHAPE, int M, int T>
MSM_DEV void finish_values(uint32_t* out, const Fe<S> (&acc)[round_values(SHAPE, M)]) {
  if constexpr (T < round_values(SHAPE, M)) {
    Fe<S> r;
    round_finish<S, SHAPE, M>(r, acc[T]);
    fe_store<S>(out + 8 * T, r);
    finish_values<S, SHAPE, M, T + 1>(out, acc);
  }
}

// one block: out[t] = the sum of the `count` partials of value t, times the factors R they owe: plain and canonical, 8 words each
template <class S, int SHAPE, int M>
__global__ void __launch_bounds__(BLOCK) k_mle_round_finish(uint32_t* out, const uint32_t* partials, uint32_t count) {
  constexpr int NV = round_values(SHAPE, M);
  Fe<S> acc[NV];
#pragma unroll
  for (int t = 0; t < NV; t++) fe_set_zero<S>(acc[t]);
#pragma unroll 1
  for (uint32_t i = threadIdx.x; i < count; i += BLOCK) {
#pragma unroll
    for (int t = 0; t < NV; t++) {
      Fe<S> p;
      fe_load<S>(p, partials + 8 * ((uint64_t)t * count + i));
      sv::inner_combine<S>(acc[t], p);
    }
  }
  block_sums<S, NV>(acc);
  if (threadIdx.x == 0) finish_values<S, SHAPE, M, 0>(out, acc);
}

struct BindVecs {
  uint32_t* dst[MAX_BIND];
  const uint32_t* a[MAX_BIND];
};

// blockIdx.y: the vector; one pair per lane
template <class S>
__global__ void __launch_bounds__(BLOCK) k_mle_bind(BindVecs vecs, uint64_t h, uint32_t var, Fe<S> rm) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= h) return;
  const uint64_t lo = pair_lo(i, var), hi = lo + (1ull << var);
  const uint32_t* a = vecs.a[blockIdx.y];
  bind_lane<S>(vecs.dst[blockIdx.y] + 8 * i, a + 8 * lo, a + 8 * hi, rm);
}

// tab: 2^k plain entries over the variables [0, k), then 2^(v - k) entries over [k, v) that carry `start_hi` (s in Montgomery form)
template <class S>
__global__ void __launch_bounds__(BLOCK) k_mle_eq_tables(uint32_t* tab, EqFactors<S> fac, uint32_t v, uint32_t k, Fe<S> start_hi) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x, n_lo = 1u << k, n_hi = 1u << (v - k);
  if (e >= n_lo + n_hi) return;
  const bool high = e >= n_lo;
  Fe<S> start, r;
  fe_set_zero<S>(start);
  start.l[0] = 1;
  fe_select<S>(start, high, start_hi, start);
  eq_entry<S>(r, start, fac, high ? k : 0u, high ? v - k : k, high ? e - n_lo : e);
  fe_store<S>(tab + 8 * (uint64_t)e, r);
}

template <class S>
__global__ void __launch_bounds__(BLOCK) k_mle_eq(uint32_t* dst, const uint32_t* tab, uint64_t n, uint32_t k) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t mask = (1ull << k) - 1;
  eq_lane<S>(dst + 8 * i, tab + 8 * (i & mask), tab + 8 * ((1ull << k) + (i >> k)));
}
}  // namespace mle
}  // namespace msm
