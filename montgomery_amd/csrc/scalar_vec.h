// Resident scalar-vector operations (msm_scalars_lincomb, _mul, _inner, _powers; msm_scalars.hip): arithmetic mod the group order
// q over vectors of 32-byte little-endian scalars in device memory -- the format msm_run reads.  The scalar half of an
// inner-product argument's round (a' = u a_lo + u^-1 a_hi, <a_lo, b_hi>), powers of an evaluation point, column products.  The
// reference has no counterpart.  Templates over the scalar FIELD (a struct of constants_gen.h), independent of the curve structs.
//
// Elements in memory are PLAIN integers (no Montgomery form), any value below 2^256: an element >= q stands for its residue.
// Every element written is canonical, in [0, q).  Registers hold the 9 limbs of 30 bits of field.h, R = 2^270.
//
// Value bounds.  fe_mul takes operands with normalised limbs -- a raw 256-bit element is one: eight limbs of 30 bits and a top limb
// of 16, and fe_acc_fits proves the accumulators for ALL-ONES limbs, so no operand can overflow a column -- and returns a value
// below q + a b / R that is congruent to a b / R.  With q > 2^250 (the smallest modulus, Ed-on-BLS12-377's, has 251 bits) and
// R = 2^270:
//   raw * Montgomery constant (a < 2^256, c < q):   a c / R < 2^256 q / 2^270 = q / 2^14   -> result < q (1 + 2^-14)  < 2 q
//   raw * raw                 (a, b < 2^256):       a b / R < 2^512 / 2^270 = 2^242 < q / 2^8 -> result < q (1 + 2^-8) < 2 q
//   (< 2 q) * Montgomery constant (c < q):          2 q c / R < 2 q^2 / 2^270 < q / 2^14 (q < 2^255) -> result < 2 q
// so every product is below 2 q whatever the inputs, on the 251-bit modulus as on the 255-bit ones; a sum of two products is
// below 4 q < 2^257 and fits the limbs.  One conditional subtraction of q (of 2 q, then q, after a sum) makes a result canonical.
// Montgomery form never reaches memory: a product with the Montgomery form x R of a host scalar is the plain product,
// a x R / R = a x, so lincomb costs one multiplication per term and powers one per set bit of the index; mul and inner owe a
// factor R (a b / R), which one multiplication by R^2 mod q returns.
#pragma once
#include "field.h"
#include "../../include/msm_hip.h"

namespace msm {

// the scalar field of every curve: X(curve id of include/msm_hip.h, field struct of constants_gen.h).  Five group orders are
// base fields of other curves (the cycles, and the curve built over BLS12-377's scalar field); Fr381 and FrEd377 exist for this.
#define MSM_SCALAR_FIELDS(X)              \
  X(MSM_CURVE_BLS12_377_G1, Fp253)        \
  X(MSM_CURVE_ED_ON_BLS12_377, FrEd377)   \
  X(MSM_CURVE_BLS12_381_G1, Fr381)        \
  X(MSM_CURVE_PALLAS, FpVesta)            \
  X(MSM_CURVE_BN254_G1, FpGrumpkin)       \
  X(MSM_CURVE_GRUMPKIN, FpBn254)          \
  X(MSM_CURVE_VESTA, FpPallas)

namespace sv {

constexpr int BLOCK = 256;                  // lanes per block, one element per lane
constexpr uint32_t INNER_MAX_BLOCKS = 1024; // grid cap of k_sv_inner: 2^18 lanes walk the vectors in strides, one partial per block
constexpr int MAX_POW_BITS = 30;            // n < 2^30: bits of an index

// Montgomery forms of x^(2^k), k < MAX_POW_BITS, as limbs: a kernel argument of k_sv_powers (read with scalar loads)
template <class S>
struct PowTable {
  uint32_t l[MAX_POW_BITS][S::NL];
};

template <class S>
MSM_DEV void set_const(Fe<S>& r, const uint32_t (&c)[S::NL]) {
#pragma unroll
  for (int i = 0; i < S::NL; i++) r.l[i] = c[i];
}

// host scalar (canonical) -> its Montgomery form, canonical
template <class S>
MSM_DEV void to_mont(Fe<S>& r, const Fe<S>& a) {
  Fe<S> r2;
  set_const<S>(r2, S::R2);
  fe_mul<S>(r, a, r2);
  fe_reduce_2p<S>(r);
}

// ---------------------------------------------------------------- lane bodies (host and device)

// dst = x a + y b (TWO) or x a; xm, ym: Montgomery forms of x, y.  Every load comes before the store: dst may be a or b.
template <class S, bool TWO>
MSM_DEV void lincomb_lane(uint32_t* dst, const uint32_t* a, const uint32_t* b, const Fe<S>& xm, const Fe<S>& ym) {
  Fe<S> va, vb, r;
  fe_load<S>(va, a);
  if (TWO) fe_load<S>(vb, b);
  fe_mul<S>(r, va, xm);            // < 2 q, plain
  if (TWO) {
    fe_mul<S>(vb, vb, ym);
    fe_add<S>(r, r, vb);           // < 4 q
    fe_reduce_4p<S>(r);
  } else {
    fe_reduce_2p<S>(r);
  }
  fe_store<S>(dst, r);
}

// dst = a b
template <class S>
MSM_DEV void mul_lane(uint32_t* dst, const uint32_t* a, const uint32_t* b) {
  Fe<S> va, vb, r, r2;
  fe_load<S>(va, a);
  fe_load<S>(vb, b);
  set_const<S>(r2, S::R2);
  fe_mul<S>(r, va, vb);            // a b / R, < 2 q
  fe_mul<S>(r, r, r2);             // a b, < 2 q
  fe_reduce_2p<S>(r);
  fe_store<S>(dst, r);
}

// r = s x^i, canonical; s plain and canonical, pw the Montgomery forms of x^(2^k): every product stays plain.  Bits k >= 6 of i
// are the same for the 64 lanes of a wave (the lanes of a block are consecutive indices from a multiple of 256), so only the
// six low bits diverge.  nbits: bits the indices of the call can have.
template <class S>
MSM_DEV void powers_lane(Fe<S>& r, const Fe<S>& s, const PowTable<S>& pw, uint32_t i, int nbits) {
  r = s;
#pragma unroll 1
  for (int k = 0; k < nbits; k++) {
    if ((i >> k) & 1u) {
      Fe<S> t;
#pragma unroll
      for (int j = 0; j < S::NL; j++) t.l[j] = pw.l[k][j];
      fe_mul<S>(r, r, t);          // < 2 q
    }
  }
  fe_reduce_2p<S>(r);
}

// one term of an inner product: a b / R, < 2 q
template <class S>
MSM_DEV void inner_term(Fe<S>& t, const uint32_t* a, const uint32_t* b) {
  Fe<S> va, vb;
  fe_load<S>(va, a);
  fe_load<S>(vb, b);
  fe_mul<S>(t, va, vb);
}

// the combine step of the reduction: acc (< 2 q) += t (< 2 q), back below 2 q.  Field addition is exact, so the order in which
// lanes, waves and blocks combine does not show in the result.
template <class S>
MSM_DEV void inner_combine(Fe<S>& acc, const Fe<S>& t) {
  fe_add<S>(acc, acc, t);          // < 4 q
  fe_cond_sub<S, 2>(acc);          // < 2 q
}

// the sum of the terms (< 2 q, owing a factor R) -> the plain canonical inner product
template <class S>
MSM_DEV void inner_finish(Fe<S>& r, const Fe<S>& acc) {
  Fe<S> r2;
  set_const<S>(r2, S::R2);
  fe_mul<S>(r, acc, r2);
  fe_reduce_2p<S>(r);
}

// ---------------------------------------------------------------- kernels

template <class S, bool TWO>
__global__ void __launch_bounds__(BLOCK) k_sv_lincomb(uint32_t* dst, const uint32_t* a, const uint32_t* b, uint64_t n, Fe<S> xm, Fe<S> ym) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  lincomb_lane<S, TWO>(dst + 8 * i, a + 8 * i, b + 8 * i, xm, ym);
}

template <class S>
__global__ void __launch_bounds__(BLOCK) k_sv_mul(uint32_t* dst, const uint32_t* a, const uint32_t* b, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  mul_lane<S>(dst + 8 * i, a + 8 * i, b + 8 * i);
}

template <class S>
__global__ void __launch_bounds__(BLOCK) k_sv_powers(uint32_t* dst, uint64_t n, Fe<S> s, PowTable<S> pw, int nbits) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  Fe<S> r;
  powers_lane<S>(r, s, pw, (uint32_t)i, nbits);
  fe_store<S>(dst + 8 * i, r);
}

// the sum of the block's accumulators (each < 2 q), valid in thread 0: down the wave by shuffles, across the waves through the LDS
template <class S>
__device__ __forceinline__ void block_sum(Fe<S>& acc) {
  constexpr int NL = S::NL, WAVES = BLOCK / 64;
  __shared__ uint32_t part[WAVES][NL];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Fe<S> o;
#pragma unroll
    for (int j = 0; j < NL; j++) o.l[j] = (uint32_t)__shfl_down((int)acc.l[j], off, 64);
    inner_combine<S>(acc, o);      // (lanes whose partner lies outside the wave add their own value: never read)
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NL; j++) part[wave][j] = acc.l[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll 1
    for (int w = 1; w < WAVES; w++) {
      Fe<S> o;
#pragma unroll
      for (int j = 0; j < NL; j++) o.l[j] = part[w][j];
      inner_combine<S>(acc, o);
    }
  }
}

// partials[block] = sum of a[i] b[i] / R over the block's share of a grid-stride walk, canonical
template <class S>
__global__ void __launch_bounds__(BLOCK) k_sv_inner(uint32_t* partials, const uint32_t* a, const uint32_t* b, uint64_t n) {
  Fe<S> acc;
  fe_set_zero<S>(acc);
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
    Fe<S> t;
    inner_term<S>(t, a + 8 * i, b + 8 * i);
    inner_combine<S>(acc, t);
  }
  block_sum<S>(acc);
  if (threadIdx.x == 0) {
    fe_reduce_2p<S>(acc);
    fe_store<S>(partials + 8 * (uint64_t)blockIdx.x, acc);
  }
}

// one block: out = R^2 * (sum of the partials) / R, the plain canonical inner product, 8 words
template <class S>
__global__ void __launch_bounds__(BLOCK) k_sv_inner_finish(uint32_t* out, const uint32_t* partials, uint32_t count) {
  Fe<S> acc;
  fe_set_zero<S>(acc);
  for (uint32_t i = threadIdx.x; i < count; i += BLOCK) {
    Fe<S> t;
    fe_load<S>(t, partials + 8 * (uint64_t)i);
    inner_combine<S>(acc, t);
  }
  block_sum<S>(acc);
  if (threadIdx.x == 0) {
    Fe<S> r;
    inner_finish<S>(r, acc);
    fe_store<S>(out, r);
  }
}
}  // namespace sv
}  // namespace msm
