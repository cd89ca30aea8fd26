// Resident scans (msm_scalars_scan, msm_scalars_div_linear; msm_scan.hip) and the batch inverse (msm_scalars_inverse) over the
// vectors of scalar_vec.h: plain 32-byte little-endian elements mod the group order q, any value below 2^256 counting as its
// residue, every element written canonical.  A scan carries a value from one element to the next under an associative operator:
//   SUM      v o a = v + a                          running sums (logUp)
//   PRODUCT  v o a = v a                            running products (the grand product of a permutation argument)
//   HORNER   v o a = v z + a, from the top index down: after the coefficients above j it is the quotient coefficient q_j of
//            a(X) = (X - z) q(X) + a(z), and after all of them the remainder a(z)
// The reference has no counterpart.  Templates over the scalar FIELD, as scalar_vec.h.
//
// Reduce-then-scan, one launch per step; no block ever waits for another block (no look-back, no flag, no grid barrier, no
// global atomic).  A vector of more than one tile is reduced to one aggregate per tile (k_scan_reduce); the aggregates are scanned
// exclusively by the same procedure (scan_plan gives the levels); k_scan_apply then rescans every tile from its carry.  A
// vector of one tile is one launch of k_scan_apply.
//
// Positions.  A scan runs over positions p = 0 .. n - 1: p is the element index for SUM and PRODUCT and n - 1 - p for HORNER
// (LV_REVERSE), so that every operator reads "what came before, then this element".  A segment of HORNER is worth
// sum a[p'] z^(e - 1 - p') over its positions [s, e), and a segment A followed by a segment B of length len combines to
// A z^len + B.  Every len that occurs is a power of two: one element, the 2^k lanes of a shuffle step, the 64 lanes of a wave
// times the elements of a lane, and at level L all of these times 2^(L tile_log).  The host passes the Montgomery forms of
// z^(2^k) as a kernel argument (PowTab, as sv::PowTable for powers, with the bits the levels add), and a product of a plain
// value with such a constant is the plain product: HORNER needs no conversion at either end and no per-element power of z.
// Padding lies BEHIND the last position (neutral elements: 0, or 1 for PRODUCT), where it changes no prefix of a real element;
// the call's total is the inclusive value at position n - 1, stored by the lane that owns it, never a tile's aggregate.
//
// Seeding.  The lane that owns the first position of a tile starts its serial accumulation from the tile's carry instead of the
// neutral element; the first lane of every later wave is seeded with what the waves before it hold.  The wave scan then carries
// the seed to every lane, so no element is ever multiplied by "its" carry afterwards.
//
// Value bounds (R = 2^270, q > 2^250, see scalar_vec.h for the products).
//   HORNER   a raw element a < 2^256 enters through one fe_mul: a * (R mod q) / R = a, below q (1 + 2^-14) < 2 q, plain.  v z is
//            (< 2 q) * constant < 2 q, plus an element < 2 q: below 4 q < 2^257 (it fits the limbs), and one conditional
//            subtraction of 2 q returns it below 2 q.
//   PRODUCT  a * (R^2 mod q) / R = a R, below 2 q: Montgomery form, which exists in registers, in the LDS and in the aggregate
//            buffer only; a product of two values below 2 q is below q + 4 q^2 / R < 2 q; one fe_mul by the integer 1 takes a
//            result out of Montgomery form.
//   SUM      raw elements are ADDED AS THEY ARE, without a reduction: the limbs hold 270 bits, a tile has at most 2^10 elements
//            below 2^256 and a carry below 2 q in front of them, so no value of a block passes 2^266 + 2 q < 2^267.  A value
//            leaves through one fe_mul by R mod q, (< 2^267) (R mod q) / R < q / 8, result below 2 q -- fe_mul takes any operand
//            with normalised limbs -- so the reduce kernel multiplies once per TILE and the apply kernel once per element, on
//            the way out.  (The lanes of a tree step that have no partner add their own value, at most 2^6 times: never read.)
// A value below 2 q fits 256 bits, so it packs into the 8 words of an LDS slot or an aggregate (`settle` brings a sum there);
// aggregates and results are made canonical (one subtraction of q) when stored.
// The inverse makes every element canonical in Montgomery form first (fe_inv gives an unspecified value for the representative
// q of zero): a residue of 0 puts 1 into the chain, writes 0 and is counted.
#pragma once
#include <utility>
#include "scalar_vec.h"

namespace msm {
namespace scan {

constexpr int BLOCK = 256;             // lanes per block
constexpr int WAVES = BLOCK / 64;
constexpr int MIN_TILE_LOG = 8;        // one element per lane
constexpr int DEFAULT_TILE_LOG = 10;   // four elements per lane: at most three levels below 2^30 elements
constexpr int MAX_TILE_LOG = DEFAULT_TILE_LOG;
constexpr int MAX_LEVELS = 4;          // ceil(30 / MIN_TILE_LOG)
constexpr int POW_BITS = 40;           // (levels - 1) tile_log < 30, plus the bits inside a tile
#ifndef MSM_SCAN_INV_E
#define MSM_SCAN_INV_E 8               // (an A/B build may set another: DESIGN section 17 has the measurement)
#endif
constexpr int INV_E = MSM_SCAN_INV_E;  // elements per lane of k_inverse: one fe_inv per lane and INV_E elements

enum Op { OP_SUM = 0, OP_PRODUCT = 1, OP_HORNER = 2 };
enum LevelFlags : uint32_t {
  LV_DATA = 1,        // level 0: raw elements in, plain canonical elements out (else: aggregates, in the operator's own form)
  LV_REVERSE = 2,     // position p is element n - 1 - p
  LV_EXCLUSIVE = 4,   // position p gets the value before its element
};

// Montgomery forms of z^(2^k) as limbs (SUM and PRODUCT never read it)
template <class S>
struct PowTab {
  uint32_t l[POW_BITS][S::NL];
};

struct Level {
  uint64_t n;        // elements of this level
  uint32_t e_log;    // 2^e_log elements per lane: tile_log - 8
  uint32_t flags;
  int32_t shift;     // HORNER: one element of this level stands for 2^shift elements of the vector
};

// tiles per level, bottom level first; the top level has one tile.  n == 0: no level.
struct Plan {
  int levels;
  uint32_t tiles[MAX_LEVELS];
};
inline Plan scan_plan(uint64_t n, int tile_log) {
  Plan p = {};
  for (uint64_t m = n; m && p.levels < MAX_LEVELS;) {
    const uint64_t t = (m + (1ull << tile_log) - 1) >> tile_log;
    p.tiles[p.levels++] = (uint32_t)t;
    if (t == 1) break;
    m = t;
  }
  return p;
}

// ---------------------------------------------------------------- lane bodies (host and device)

template <class S, int OP>
MSM_DEV void set_neutral(Fe<S>& v) {
  if (OP == OP_PRODUCT) fe_set_one<S>(v);
  else fe_set_zero<S>(v);
}

// a raw element (any 256-bit value) -> the operator's form: below 2 q, or as it is for SUM
template <class S, int OP>
MSM_DEV void enter(Fe<S>& v) {
  if (OP == OP_SUM) return;
  Fe<S> c;
  if (OP == OP_PRODUCT) sv::set_const<S>(c, S::R2);
  else sv::set_const<S>(c, S::ONE);
  fe_mul<S>(v, v, c);
}

// a value of the operator -> below 2 q, so that it packs into 8 words: a sum (below 2^267) through one multiplication by R mod q
template <class S, int OP>
MSM_DEV void settle(Fe<S>& v) {
  if (OP != OP_SUM) return;
  Fe<S> c;
  sv::set_const<S>(c, S::ONE);
  fe_mul<S>(v, v, c);
}

// a value of the operator -> the plain canonical value
template <class S, int OP>
MSM_DEV void leave(Fe<S>& v) {
  settle<S, OP>(v);
  if (OP == OP_PRODUCT) {
    Fe<S> one;
    fe_set_zero<S>(one);
    one.l[0] = 1;
    fe_mul<S>(v, v, one);
  }
  fe_reduce_2p<S>(v);
}

// r = a o b: a the earlier segment, b the later one of 2^k elements of the level (k is read by HORNER only); PRODUCT and HORNER:
// all below 2 q; SUM: the plain sum
template <class S, int OP>
MSM_DEV void combine(Fe<S>& r, const Fe<S>& a, const Fe<S>& b, const PowTab<S>& pw, int k) {
  if (OP == OP_PRODUCT) {
    fe_mul<S>(r, a, b);
    return;
  }
  if (OP == OP_SUM) {
    fe_add<S>(r, a, b);            // < 2^267 within a block
    return;
  }
  Fe<S> c, t;
#pragma unroll
  for (int j = 0; j < S::NL; j++) c.l[j] = pw.l[k][j];
  fe_mul<S>(t, a, c);              // < 2 q, plain
  fe_add<S>(r, t, b);              // < 4 q
  fe_cond_sub<S, 2>(r);            // < 2 q
}

// a raw element -> canonical Montgomery form for the chain of the inverse; zero: its residue is 0, and 1 takes its place
template <class S>
MSM_DEV void inv_enter(Fe<S>& m, bool& zero, const uint32_t* p) {
  Fe<S> one;
  fe_load<S>(m, p);
  enter<S, OP_PRODUCT>(m);
  fe_reduce_2p<S>(m);
  zero = fe_is_zero_canonical<S>(m);
  fe_set_one<S>(one);
  fe_select<S>(m, zero, one, m);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop the compiler cannot leave rolled, so that an array
// indexed by the step stays in registers
template <class F, int... I>
MSM_DEV void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
MSM_DEV void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Montgomery's trick over the E elements first, first + stride, ...: dst[i] = a[i]^-1, 0 where the residue is 0; returns how many
// of those there were.  One fe_inv.  The way back reads an element again before it writes it: dst may be a.
template <class S, int E>
MSM_DEV uint32_t inverse_lane(uint32_t* dst, const uint32_t* a, uint64_t first, uint64_t stride, uint64_t n) {
  Fe<S> pre[E], acc, inv, m;
  uint32_t zeros = 0;
  fe_set_one<S>(acc);
  static_for<E>([&](auto step) {
    constexpr int t = decltype(step)::value;
    const uint64_t i = first + (uint64_t)t * stride;
    if (i < n) {
      bool zero;
      inv_enter<S>(m, zero, a + 8 * i);
      zeros += zero ? 1u : 0u;
      if (t == 0) acc = m;
      else fe_mul<S>(acc, acc, m);   // < 2 q
    }
    pre[t] = acc;
  });
  fe_reduce_2p<S>(acc);              // canonical and not 0: what fe_inv asks for
  fe_inv<S>(inv, acc);               // < 2 q
  static_for<E>([&](auto step) {
    constexpr int t = E - 1 - decltype(step)::value;
    const uint64_t i = first + (uint64_t)t * stride;
    if (i < n) {
      bool zero;
      Fe<S> r, zero_fe;
      inv_enter<S>(m, zero, a + 8 * i);
      if (t > 0) fe_mul<S>(r, inv, pre[t > 0 ? t - 1 : 0]);
      else r = inv;
      fe_mul<S>(inv, inv, m);
      leave<S, OP_PRODUCT>(r);
      fe_set_zero<S>(zero_fe);
      fe_select<S>(r, zero, zero_fe, r);
      fe_store<S>(dst + 8 * i, r);
    }
  });
  return zeros;
}

MSM_DEV uint64_t element_of(const Level& lv, uint64_t p) { return (lv.flags & LV_REVERSE) ? lv.n - 1 - p : p; }

// 16-byte unit of LDS slot j: 32 bytes per element and 16 bytes of padding behind each lane's 2^e_log elements, so that the lanes'
// 16-byte reads of their own elements fall on different banks
MSM_DEV uint32_t lds_unit(uint32_t j, uint32_t e_log) { return 2 * j + (j >> e_log); }
constexpr uint32_t LDS_UNITS = (2u << MAX_TILE_LOG) + BLOCK;

// ---------------------------------------------------------------- kernels

#if defined(__HIPCC__)

template <class S>
__device__ __forceinline__ void shfl_fe(Fe<S>& o, const Fe<S>& v, int off, bool up) {
#pragma unroll
  for (int j = 0; j < S::NL; j++) o.l[j] = (uint32_t)(up ? __shfl_up((int)v.l[j], off, 64) : __shfl_down((int)v.l[j], off, 64));
}

// the wave's lanes combined in lane order, valid in lane 0: step k joins neighbouring segments of 2^k lanes, each lane standing for
// 2^lane_k elements of the level.  (A lane whose partner lies outside the wave combines its own value: never read.)
template <class S, int OP>
__device__ __forceinline__ void wave_reduce(Fe<S>& v, const PowTab<S>& pw, int lane_k) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<S> o;
    shfl_fe<S>(o, v, 1 << k, false);
    combine<S, OP>(v, v, o, pw, lane_k + k);
  }
}

// agg[tile] = the tile's elements combined in position order, canonical in the operator's form.  Lane l takes the positions
// l, l + 256, ... of the tile (coalesced loads); HORNER joins them with z^256 and the lanes with z^1, z^2, ... as above.
template <class S, int OP>
__global__ void __launch_bounds__(BLOCK) k_scan_reduce(uint32_t* agg, const uint32_t* src, Level lv, PowTab<S> pw) {
  __shared__ uint32_t part[WAVES][S::NL];
  const uint32_t tid = threadIdx.x, trips = 1u << lv.e_log;
  const uint64_t base = (uint64_t)blockIdx.x << (8 + lv.e_log);
  Fe<S> acc;
#pragma unroll 1
  for (uint32_t t = 0; t < trips; t++) {
    const uint64_t p = base + (uint64_t)t * BLOCK + tid;
    Fe<S> a;
    set_neutral<S, OP>(a);
    if (p < lv.n) {
      fe_load<S>(a, src + 8 * element_of(lv, p));
      if (lv.flags & LV_DATA) enter<S, OP>(a);
    }
    if (t == 0) acc = a;
    else combine<S, OP>(acc, acc, a, pw, lv.shift + 8);
  }
  wave_reduce<S, OP>(acc, pw, lv.shift);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < S::NL; j++) part[tid >> 6][j] = acc.l[j];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll 1
    for (int w = 1; w < WAVES; w++) {
      Fe<S> o;
#pragma unroll
      for (int j = 0; j < S::NL; j++) o.l[j] = part[w][j];
      combine<S, OP>(acc, acc, o, pw, lv.shift + 6);
    }
    settle<S, OP>(acc);
    fe_reduce_2p<S>(acc);
    fe_store<S>(agg + 8 * (uint64_t)blockIdx.x, acc);
  }
}

// dst = the scan of the tile from its carry (carry[tile], or `init` where carry is null: the top level).  The tile goes through the
// LDS both ways, so global accesses are coalesced 16-byte ones while every lane scans 2^e_log neighbouring positions.  total: where
// the lane that owns position n - 1 stores the inclusive value there, plain and canonical (level 0 only; null elsewhere).
template <class S, int OP>
__global__ void __launch_bounds__(BLOCK) k_scan_apply(uint32_t* dst, const uint32_t* src, const uint32_t* carry, Fe<S> init, uint32_t* total,
                                                      Level lv, PowTab<S> pw) {
  __shared__ uint4 tile[LDS_UNITS];
  __shared__ uint32_t wtot[WAVES][S::NL];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e_log = lv.e_log, per_lane = 1u << e_log;
  const uint64_t base = (uint64_t)blockIdx.x << (8 + e_log);
  const bool data = (lv.flags & LV_DATA) != 0, exclusive = (lv.flags & LV_EXCLUSIVE) != 0;

#pragma unroll 1
  for (uint32_t t = 0; t < per_lane; t++) {
    const uint32_t j = t * BLOCK + tid;
    const uint64_t p = base + j;
    if (p < lv.n) {
      const uint4* g = reinterpret_cast<const uint4*>(src + 8 * element_of(lv, p));
      const uint4 lo = g[0], hi = g[1];
      tile[lds_unit(j, e_log)] = lo;
      tile[lds_unit(j, e_log) + 1] = hi;
    }
  }
  __syncthreads();

  // every lane over its own positions; the first lane of the tile from the carry.  The elements go back to the LDS in the
  // operator's form for the second walk.
  const uint32_t first = tid << e_log;
  Fe<S> start, v;
  set_neutral<S, OP>(start);
  if (tid == 0) {
    if (carry) fe_load<S>(start, carry + 8 * (uint64_t)blockIdx.x);
    else start = init;
  }
  v = start;
#pragma unroll 1
  for (uint32_t e = 0; e < per_lane; e++) {
    const uint32_t j = first + e;
    Fe<S> a;
    set_neutral<S, OP>(a);
    if (base + j < lv.n) {
      uint32_t* slot = reinterpret_cast<uint32_t*>(&tile[lds_unit(j, e_log)]);
      fe_load<S>(a, slot);
      if (data && OP != OP_SUM) {      // (a sum takes its elements as they are)
        enter<S, OP>(a);
        fe_store<S>(slot, a);
      }
    }
    combine<S, OP>(v, v, a, pw, lv.shift);
  }

  // what the waves before this one hold, then the seeded wave scan
  Fe<S> r = v, before;
  wave_reduce<S, OP>(r, pw, lv.shift + (int)e_log);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < S::NL; j++) wtot[wave][j] = r.l[j];
  }
  __syncthreads();
  set_neutral<S, OP>(before);
  if (wave > 0) {                    // (uniform over the wave)
#pragma unroll
    for (int j = 0; j < S::NL; j++) before.l[j] = wtot[0][j];
#pragma unroll 1
    for (uint32_t w = 1; w < wave; w++) {
      Fe<S> o;
#pragma unroll
      for (int j = 0; j < S::NL; j++) o.l[j] = wtot[w][j];
      combine<S, OP>(before, before, o, pw, lv.shift + (int)e_log + 6);
    }
  }
  {
    Fe<S> t;
    combine<S, OP>(t, before, v, pw, lv.shift + (int)e_log);
    fe_select<S>(v, lane == 0 && wave > 0, t, v);
  }
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<S> o, t;
    shfl_fe<S>(o, v, 1 << k, true);
    combine<S, OP>(t, o, v, pw, lv.shift + (int)e_log + k);
    fe_select<S>(v, lane >= (1u << k), t, v);   // a select, not a branch, for the lanes without a partner
  }
  // the value before this lane's first position
  {
    Fe<S> o;
    shfl_fe<S>(o, v, 1, true);
    fe_select<S>(before, wave > 0, before, start);
    fe_select<S>(v, lane == 0, before, o);
  }

#pragma unroll 1
  for (uint32_t e = 0; e < per_lane; e++) {
    const uint32_t j = first + e;
    const uint64_t p = base + j;
    if (p < lv.n) {                  // (the positions behind n - 1 are padding: nothing reads a value past them)
      uint32_t* slot = reinterpret_cast<uint32_t*>(&tile[lds_unit(j, e_log)]);
      Fe<S> a, out;
      fe_load<S>(a, slot);
      out = v;
      combine<S, OP>(v, v, a, pw, lv.shift);
      if (!exclusive) out = v;
      if (data) {
        leave<S, OP>(out);
      } else {
        settle<S, OP>(out);
        fe_reduce_2p<S>(out);
      }
      fe_store<S>(slot, out);
      if (total && p == lv.n - 1) {
        Fe<S> incl = v;
        leave<S, OP>(incl);
        fe_store<S>(total, incl);
      }
    }
  }
  __syncthreads();

#pragma unroll 1
  for (uint32_t t = 0; t < per_lane; t++) {
    const uint32_t j = t * BLOCK + tid;
    const uint64_t p = base + j;
    if (p < lv.n) {
      uint4* g = reinterpret_cast<uint4*>(dst + 8 * element_of(lv, p));
      g[0] = tile[lds_unit(j, e_log)];
      g[1] = tile[lds_unit(j, e_log) + 1];
    }
  }
}

// dst[i] = a[i]^-1 for the block's INV_E x 256 elements, lane l taking l, l + 256, ... of them; zeros[block] = how many residues
// of 0 it met.  No block depends on another.
template <class S, int E>
__global__ void __launch_bounds__(BLOCK) k_inverse(uint32_t* dst, const uint32_t* a, uint64_t n, uint32_t* zeros) {
  __shared__ uint32_t part[WAVES];
  const uint32_t tid = threadIdx.x;
  uint32_t z = inverse_lane<S, E>(dst, a, (uint64_t)blockIdx.x * (E * BLOCK) + tid, BLOCK, n);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) z += (uint32_t)__shfl_down((int)z, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = z;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WAVES; w++) z += part[w];
    zeros[blockIdx.x] = z;
  }
}

#endif  // __HIPCC__

}  // namespace scan
}  // namespace msm
