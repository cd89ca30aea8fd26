// Resident number-theoretic transform over vectors of 32-byte scalars (msm_scalars_ntt; msm_ntt.hip): B transforms of n = 2^L
// elements mod the group order q, natural order in and out, on any coset shift <omega>.  The reference has no counterpart.
// Templates over the scalar FIELD, as scalar_vec.h; the lane bodies are MSM_DEV functions of a lane number, which the kernel
// calls between barriers and tests/csrc/ntt_host.hip calls in loops over the lanes, on the same plan, index and exponent functions.
//
// Plan.  The L radix-2 stages are cut into P = ceil(L / T) passes of t_0 >= t_1 >= ... stages (ntt_plan: as even as the division
// allows), one kernel launch each.  With S_i = t_0 + ... + t_(i-1) and rem_i = L - S_i - t_i, pass i sees an element's position as
//     [ k_0 | k_1 | ... | k_(i-1) | d | jrem ]        (k_0 in the top t_0 bits, d: t_i bits, jrem: the rem_i low bits)
// where the k are the output digits of the passes before it and (d, jrem) are bits of the INPUT index still untransformed.  It
// runs, for every (k_0 .. k_(i-1), jrem), the 2^t_i-point transform over d with the root omega^(2^(L - t_i)), leaves digit k_i
// where d was, and multiplies by omega^(2^S_i jrem k_i) -- Cooley-Tukey with N = N1 N2, applied P - 1 times:
//     X[k2 + N2 k1] = sum_j1 w_N1^(j1 k1) [ w_N^(j1 k2) sum_j2 x[j1 + N1 j2] w_N2^(j2 k2) ].
// The output index is k = k_0 + 2^S_1 k_1 + ... + 2^S_(P-1) k_(P-1): the digits in reverse.  Passes 0 .. P-2 write where they
// read; the LAST pass writes every element to its natural place, so no permutation pass exists.  Passes 0 .. P-2 work in a scratch
// vector of the context (the first reads the caller's a), the last reads the scratch and writes dst: dst may be a.  A single
// pass (L <= T) holds whole vectors in its tile, reads all of them before a barrier and writes after it: again dst may be a.
//
// Tiles.  A block of 256 lanes keeps 2^t rows x 2^c columns, at most 2^LDS_LOG elements, in the LDS.  The columns are 2^c
// independent sub-transforms chosen so that global accesses cover adjacent elements:
//   pass i < P - 1:  columns = the low c bits of jrem; reads and writes are runs of 2^c adjacent elements, rows 2^rem apart
//   last pass:       reads are rows of 2^t adjacent elements (d is the low digit); columns = the low c bits of k_0, the LOW bits of
//                    the output index, so writes are runs of 2^c adjacent elements, 2^S_(P-1) apart
//   single pass:     columns = vectors of the batch; reads and writes are whole vectors
// Inside the tile the transform is the textbook decimation in time: rows enter at the bit reversal of d, stage k pairs rows 2^k
// apart with the twiddle omega^(m 2^(L-k-1)), m = row mod 2^k, and rows leave in natural order of k_i.
//
// LDS layout: eight word planes of 2^LDS_LOG + 2^LDS_LOG / 32 words, element `slot` at word slot + slot / 32 of each plane.  A
// 32-byte record per element would put lane-consecutive 16-byte accesses on the same banks four lanes apart; in word planes
// lane-consecutive slots are bank-consecutive for every 4-byte access.  The one word of padding per 32 takes apart the power-of-two
// row strides of the bit-reversed load and of the row-fast accesses of the last pass (a stride of 32 words would be one bank).
//
// Twiddles: two-level tables, never a table of n / 2 entries.  omega^e = WA[e mod 2^h] WB[e >> h], h = ceil(L / 2) (h = L and no
// second level up to L = LDS_LOG), each entry the canonical Montgomery form, so data * WA[..] * WB[..] are two multiplications whose
// product stays plain.  The butterflies of a tile take omega^(m 2^(L-k-1)) from a third table G of 2^(g-1) entries,
// g = min(L, LDS_LOG), with one multiplication.  The same two-level shape serves shift^j (forward, on the first load) and
// n^-1 shift^-k (inverse, on the last store; n^-1 sits in the low table).  Without a shift the forward transform multiplies nothing
// outside butterflies and inter-pass twiddles, and the inverse multiplies once by the constant n^-1.
//
// Value bounds (scalar_vec.h derives the products).  Elements of the caller are raw, < 2^256.  A first load either multiplies by
// a Montgomery constant (shift table: result < 2 q) or brings the raw value below 2 q by conditional subtractions (reduce_raw:
// the count is fixed per field from the top word of q).  Every value in the LDS and in the scratch vector is BELOW 2 q and thus
// fits 256 bits (q < 2^255).  A butterfly forms t = w v < 2 q (or v itself in stage 0, whose twiddle is 1), then u + t < 4 q and
// u - t + 2 q < 4 q, and one conditional subtraction of 2 q returns both below 2 q.  An inter-pass twiddle or a scale is a product
// with a Montgomery constant: < 2 q.  Only the last store subtracts q conditionally: every element written to dst is canonical.
#pragma once
#include "scalar_vec.h"

namespace msm {
namespace ntt {

constexpr int BLOCK = 256;             // lanes per block
constexpr int LDS_LOG = 10;            // log2 of the elements a tile holds: 8 planes x (1024 + 32) words = 33 KiB
constexpr int TILE = 1 << LDS_LOG;
constexpr int PLANE = TILE + TILE / 32;
constexpr int MAX_TILE_LOG = LDS_LOG;  // stages a pass can have
constexpr int DEFAULT_TILE_LOG = 9;    // measured 7 .. 10: 9 and 10 tie, 8 and 7 pay a fourth pass at 2^26
constexpr int MAX_LOG2N = 29;
constexpr int MAX_PASSES = MAX_LOG2N;  // tile_log 1

struct Plan {
  int32_t log2n, passes;
  int32_t stages[MAX_PASSES];
};

// P = ceil(log2n / tile_log) passes, the first log2n mod P of them one stage longer than the rest
inline Plan ntt_plan(int log2n, int tile_log) {
  Plan p = {};
  p.log2n = log2n;
  p.passes = (log2n + tile_log - 1) / tile_log;
  for (int i = 0; i < p.passes; i++) p.stages[i] = log2n / p.passes + (i < log2n % p.passes ? 1 : 0);
  return p;
}

// bits of the low-level table of a two-level power table over exponents below 2^log2n.  -DMSM_NTT_FULL_TABLES (an A/B build:
// `make ab`) makes every table one level of 2^log2n entries, one multiplication per twiddle: the measurement of DESIGN 16.
inline int table_low_bits(int log2n) {
#if defined(MSM_NTT_FULL_TABLES)
  return log2n;
#else
  return log2n <= LDS_LOG ? log2n : (log2n + 1) / 2;
#endif
}

enum PassKind : int32_t { PASS_STRIDED = 0, PASS_LAST = 1, PASS_SINGLE = 2 };
enum ScaleMode : int32_t { SCALE_NONE = 0, SCALE_CONST = 1, SCALE_TABLE = 2 };

// one launch: the geometry of pass `index` of a plan (pass_geometry), a kernel argument
struct Pass {
  int32_t log2n, kind, index;
  int32_t t, c;          // stage count, log2 of the columns
  int32_t S, rem;        // bits transformed before this pass, input bits left after it
  int32_t t0;            // stages of pass 0 (whose low output bits are the columns of the last pass)
  int32_t h, g;          // low bits of the two-level tables, log2 of twice the entries of G
  int32_t first, last;   // reads the caller's vector / writes the result
  int32_t scale;         // ScaleMode of this pass: the load of the first pass scales a forward transform, the store of the last
  int32_t inverse;       //   pass an inverse one (a single pass is both)
  int32_t blocks_log;    // log2 of the blocks per vector (PASS_SINGLE: 0, a block takes 2^c vectors)
  uint32_t B;
  Plan plan;
};

inline int ceil_log2_u32(uint32_t v) {
  int r = 0;
  while ((1ull << r) < v) r++;
  return r;
}

inline Pass pass_geometry(const Plan& pl, int index, uint32_t B, int scale, bool inverse) {
  Pass a = {};
  a.plan = pl;
  a.log2n = pl.log2n;
  a.index = index;
  a.B = B;
  a.h = table_low_bits(pl.log2n);
  a.g = pl.log2n < LDS_LOG ? pl.log2n : LDS_LOG;
  a.t0 = pl.passes ? pl.stages[0] : 0;
  a.first = index == 0;
  a.last = index + 1 >= pl.passes;
  a.t = pl.passes ? pl.stages[index] : 0;   // (n = 1: one launch of no stages)
  for (int i = 0; i < index; i++) a.S += pl.stages[i];
  a.rem = pl.log2n - a.S - a.t;
  if (pl.passes <= 1) {
    a.kind = PASS_SINGLE;
    a.c = LDS_LOG - a.t < ceil_log2_u32(B) ? LDS_LOG - a.t : ceil_log2_u32(B);
    a.blocks_log = 0;
  } else if (a.last) {
    a.kind = PASS_LAST;
    a.c = LDS_LOG - a.t < a.t0 ? LDS_LOG - a.t : a.t0;
    a.blocks_log = pl.log2n - a.t - a.c;
  } else {
    a.kind = PASS_STRIDED;
    a.c = LDS_LOG - a.t < a.rem ? LDS_LOG - a.t : a.rem;
    a.blocks_log = pl.log2n - a.t - a.c;
  }
  // forward: shift^j on the first load; inverse: n^-1 shift^-k on the last store
  a.inverse = inverse;
  a.scale = ((inverse && a.last) || (!inverse && a.first)) ? scale : SCALE_NONE;
  return a;
}

// blocks of the launch
inline uint64_t pass_blocks(const Pass& a) {
  if (a.kind == PASS_SINGLE) return ((uint64_t)a.B + (1u << a.c) - 1) >> a.c;
  return (uint64_t)a.B << a.blocks_log;
}

// canonical Montgomery forms, 8 words an entry (device pointers in the kernel, host arrays in the test shim)
struct Tables {
  const uint32_t *wa, *wb;   // omega^e, e < 2^h; omega^(e 2^h), e < 2^(L-h)          (omega^-1 for an inverse transform)
  const uint32_t *g;         // omega^(e 2^(L-g)), e < 2^(g-1)
  const uint32_t *sa, *sb;   // forward: shift^e and shift^(e 2^h); inverse: n^-1 shift^-e and shift^-(e 2^h)   (SCALE_TABLE only)
};

// ---------------------------------------------------------------- index functions (host and device)

MSM_DEV uint32_t bit_reverse(uint32_t v, int bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return bits ? __brev(v) >> (32 - bits) : 0u;
#else
  uint32_t r = 0;
  for (int i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
  return r;
#endif
}

// word of a plane that holds element `slot` of the tile
MSM_DEV uint32_t lds_word(uint32_t slot) { return slot + (slot >> 5); }

// what a block works on: its vector (PASS_SINGLE: its first vector), the element offsets of its tile inside a vector on the way
// in and on the way out, and the part of jrem / of the output index k that its tile shares
struct BlockBase {
  uint32_t vec;
  uint32_t in, out;
  uint32_t jrem;   // PASS_STRIDED: jrem with the column bits clear
};

MSM_DEV BlockBase block_base(const Pass& a, uint32_t block) {
  BlockBase b;
  if (a.kind == PASS_SINGLE) {
    b.vec = block << a.c;
    b.in = b.out = b.jrem = 0;
    return b;
  }
  b.vec = block >> a.blocks_log;
  const uint32_t id = block & ((1u << a.blocks_log) - 1u);
  if (a.kind == PASS_STRIDED) {
    // id = [ k_0 .. k_(i-1) | jrem >> c ]
    const int jbits = a.rem - a.c;
    const uint32_t kprev = id >> jbits, jhi = id & ((1u << jbits) - 1u);
    b.jrem = jhi << a.c;
    b.in = b.out = (kprev << (a.log2n - a.S)) | b.jrem;
    return b;
  }
  // PASS_LAST: id = [ k_0 >> c | k_1 .. k_(P-2) ], the tile's rows are the low t bits of the position
  const int midw = a.S - a.t0;
  uint32_t mid = id & ((1u << midw) - 1u);
  const uint32_t k0hi = id >> midw;
  b.jrem = 0;
  b.in = ((k0hi << a.c) << (a.log2n - a.t0)) | (mid << a.t);
  uint32_t out = k0hi << a.c;
  int S = a.S;
  for (int i = a.plan.passes - 2; i >= 1; i--) {   // k_(P-2) is the lowest digit of mid
    const int ti = a.plan.stages[i];
    S -= ti;
    out |= (mid & ((1u << ti) - 1u)) << S;
    mid >>= ti;
  }
  b.out = out;
  return b;
}

// element e of the tile on the way in: its row d and column, its offset in the vector, its vector; false: past the batch
MSM_DEV bool load_index(const Pass& a, const BlockBase& b, uint32_t e, uint32_t& d, uint32_t& col, uint32_t& vec, uint32_t& j) {
  vec = b.vec;
  if (a.kind == PASS_STRIDED) {
    col = e & ((1u << a.c) - 1u);
    d = e >> a.c;
    j = b.in + (d << a.rem) + col;
    return true;
  }
  d = e & ((1u << a.t) - 1u);
  col = e >> a.t;
  if (a.kind == PASS_LAST) {
    j = b.in + d + (col << (a.log2n - a.t0));
    return true;
  }
  vec = b.vec + col;
  j = d;
  return vec < a.B;
}

// element e of the tile on the way out: its row k_i and column, its offset in the vector (the OUTPUT index for a last pass)
MSM_DEV bool store_index(const Pass& a, const BlockBase& b, uint32_t e, uint32_t& k, uint32_t& col, uint32_t& vec, uint32_t& j) {
  vec = b.vec;
  if (a.kind == PASS_SINGLE) {
    k = e & ((1u << a.t) - 1u);
    col = e >> a.t;
    vec = b.vec + col;
    j = k;
    return vec < a.B;
  }
  col = e & ((1u << a.c) - 1u);
  k = e >> a.c;
  j = a.kind == PASS_STRIDED ? b.out + (k << a.rem) + col : b.out + col + (k << a.S);
  return true;
}

// exponent of omega an element of a pass before the last is multiplied by on its way out: 2^S jrem k_i, below 2^L
MSM_DEV uint32_t twiddle_exponent(const Pass& a, const BlockBase& b, uint32_t k, uint32_t col) { return ((b.jrem + col) * k) << a.S; }

// butterfly bf of stage k: the slots of u and v and the index into G of its twiddle (0: the twiddle is 1)
MSM_DEV void butterfly_index(const Pass& a, int k, uint32_t bf, uint32_t& su, uint32_t& sv, uint32_t& gi) {
  const uint32_t col = bf & ((1u << a.c) - 1u), bb = bf >> a.c;
  const uint32_t m = bb & ((1u << k) - 1u);
  const uint32_t urow = ((bb >> k) << (k + 1)) | m;
  su = (urow << a.c) + col;
  sv = ((urow + (1u << k)) << a.c) + col;
  gi = m << (a.g - 1 - k);
}

// ---------------------------------------------------------------- lane bodies (host and device)

// a raw element (< 2^256) -> below 2 q, without a multiplication: conditional subtractions of 4 q while the bound is above 4 q,
// then one of 2 q.  2^256 / q <= 2^32 / PW[7]: 3 + 1 subtractions on the 253-bit order, 1 + 1 on the 255-bit ones.
template <class S>
constexpr int raw_bound() { return (int)((1ull << 32) / S::PW[7]) + 1; }
template <class S>
MSM_DEV void reduce_raw(Fe<S>& x) {
#pragma unroll
  for (int bound = raw_bound<S>(); bound > 4; bound -= 4) fe_cond_sub<S, 4>(x);
  fe_cond_sub<S, 2>(x);
}

template <class S>
MSM_DEV void lds_get(Fe<S>& r, const uint32_t* lds, uint32_t slot) {
  uint32_t w[8];
  const uint32_t o = lds_word(slot);
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = lds[j * PLANE + o];
  fe_unpack<S>(r, w);
}
template <class S>
MSM_DEV void lds_put(uint32_t* lds, uint32_t slot, const Fe<S>& a) {   // a < 2^256
  uint32_t w[8];
  fe_pack<S>(w, a);
  const uint32_t o = lds_word(slot);
#pragma unroll
  for (int j = 0; j < 8; j++) lds[j * PLANE + o] = w[j];
}

// x *= T[e] of a two-level table (lo, hi); the product is plain and below 2 q
template <class S>
MSM_DEV void mul_table(Fe<S>& x, const Pass& a, const uint32_t* lo, const uint32_t* hi, uint32_t e) {
  Fe<S> w;
  fe_load<S>(w, lo + 8 * (uint64_t)(e & ((1u << a.h) - 1u)));
  fe_mul<S>(x, x, w);
  if (a.log2n > a.h) {
    fe_load<S>(w, hi + 8 * (uint64_t)(e >> a.h));
    fe_mul<S>(x, x, w);
  }
}

// (u, v) -> (u + w v, u - w v), all below 2 q; wm: the Montgomery form of w, or null for w = 1 (v below 2 q then)
template <class S>
MSM_DEV void butterfly(Fe<S>& u, Fe<S>& v, const Fe<S>* wm) {
  Fe<S> t = v, d;
  if (wm) fe_mul<S>(t, v, *wm);   // < 2 q
  fe_sub_2p<S>(d, u, t);          // u - t + 2 q < 4 q
  fe_add<S>(u, u, t);             // < 4 q
  fe_cond_sub<S, 2>(u);
  fe_cond_sub<S, 2>(d);
  v = d;
}

// the three phases of a block, for lane `lane` of `lanes`; a barrier stands between any two of them
template <class S>
MSM_DEV void load_phase(const Pass& a, const Tables& tb, const uint32_t* src, uint32_t* lds, uint32_t block, uint32_t lane, uint32_t lanes) {
  const BlockBase b = block_base(a, block);
  const uint32_t count = 1u << (a.t + a.c);
  for (uint32_t e = lane; e < count; e += lanes) {
    uint32_t d, col, vec, j;
    if (!load_index(a, b, e, d, col, vec, j)) continue;
    Fe<S> x;
    fe_load<S>(x, src + 8 * (((uint64_t)vec << a.log2n) + j));
    if (a.first) {
      if (!a.inverse && a.scale == SCALE_TABLE) mul_table<S>(x, a, tb.sa, tb.sb, j);
      else reduce_raw<S>(x);
    }
    lds_put<S>(lds, (bit_reverse(d, a.t) << a.c) + col, x);
  }
}

template <class S>
MSM_DEV void stage_phase(const Pass& a, const Tables& tb, uint32_t* lds, int k, uint32_t lane, uint32_t lanes) {
  const uint32_t count = 1u << (a.t - 1 + a.c);
  for (uint32_t bf = lane; bf < count; bf += lanes) {
    uint32_t su, sv, gi;
    butterfly_index(a, k, bf, su, sv, gi);
    Fe<S> u, v, w;
    lds_get<S>(u, lds, su);
    lds_get<S>(v, lds, sv);
    if (k) {
      fe_load<S>(w, tb.g + 8 * (uint64_t)gi);
      butterfly<S>(u, v, &w);
    } else {
      butterfly<S>(u, v, nullptr);
    }
    lds_put<S>(lds, su, u);
    lds_put<S>(lds, sv, v);
  }
}

template <class S>
MSM_DEV void store_phase(const Pass& a, const Tables& tb, const Fe<S>& scale_c, uint32_t* dst, const uint32_t* lds, uint32_t block,
                         uint32_t lane, uint32_t lanes) {
  const BlockBase b = block_base(a, block);
  const uint32_t count = 1u << (a.t + a.c);
  for (uint32_t e = lane; e < count; e += lanes) {
    uint32_t k, col, vec, j;
    if (!store_index(a, b, e, k, col, vec, j)) continue;
    Fe<S> x;
    lds_get<S>(x, lds, (k << a.c) + col);
    if (!a.last) {
      mul_table<S>(x, a, tb.wa, tb.wb, twiddle_exponent(a, b, k, col));   // < 2 q: the scratch vector holds 256-bit values
    } else {
      if (a.inverse && a.scale == SCALE_TABLE) mul_table<S>(x, a, tb.sa, tb.sb, j);
      else if (a.inverse && a.scale == SCALE_CONST) fe_mul<S>(x, x, scale_c);
      fe_reduce_2p<S>(x);
    }
    fe_store<S>(dst + 8 * (((uint64_t)vec << a.log2n) + j), x);
  }
}

// ---------------------------------------------------------------- kernel

#if defined(__HIPCC__)
template <class S>
__global__ void __launch_bounds__(BLOCK) k_ntt_pass(uint32_t* dst, const uint32_t* src, Pass a, Tables tb, Fe<S> scale_c) {
  __shared__ uint32_t lds[8 * PLANE];
  load_phase<S>(a, tb, src, lds, blockIdx.x, threadIdx.x, BLOCK);
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < a.t; k++) {
    stage_phase<S>(a, tb, lds, k, threadIdx.x, BLOCK);
    __syncthreads();
  }
  store_phase<S>(a, tb, scale_c, dst, lds, blockIdx.x, threadIdx.x, BLOCK);
}
#endif

}  // namespace ntt
}  // namespace msm
