// Host-side unit-test shim of the resident sumcheck: the index maps, the lane bodies and the half-table split of
// montgomery_amd/csrc/scalar_mle.h compiled for the CPU, over the scalar field MSM_SCALAR_FIELDS gives every curve
// (tests/test_mle_host.py).  Elements cross as 8 words, plain little-endian integers below 2^256, as the kernels read them from
// device memory; host scalars cross as 8 canonical words and go to Montgomery form as the entry points do it.
#include "scalar_vec.h"
#include "scalar_host.h"
#include "scalar_mle.h"
#include <cstring>
using namespace msm;
using namespace msmi;

namespace {

using Words8 = const uint32_t[8];

// the `pairs` pairs of m vectors (a: m x pairs x 2 elements, vector j's pair p at a + 8 (2 (j pairs + p)): row lo, then row hi) as one
// lane would walk them, split at `cut` into two accumulator sets that are then combined; out: NV values.  finish = 0: the
// accumulators as they stand (below 2 q, still owing their factors R), as raw words
template <class S, int SHAPE, int M>
int run_round(const uint32_t* a, int pairs, int cut, int finish, uint32_t* out) {
  constexpr int NV = mle::round_values(SHAPE, M);
  Fe<S> acc[2][NV];
  for (auto& set : acc)
    for (auto& v : set) fe_set_zero<S>(v);
  for (int p = 0; p < pairs; p++) {
    alignas(16) uint32_t buf[2 * M][8];
    const uint32_t* rows[2 * M];
    for (int j = 0; j < M; j++) {
      memcpy(buf[j], a + 8 * (2 * ((size_t)j * pairs + p)), 32);
      memcpy(buf[M + j], a + 8 * (2 * ((size_t)j * pairs + p) + 1), 32);
      rows[j] = buf[j];
      rows[M + j] = buf[M + j];
    }
    mle::round_pair<S, SHAPE, M>(acc[p >= cut], rows);
  }
  for (int t = 0; t < NV; t++) {
    sv::inner_combine<S>(acc[0][t], acc[1][t]);
    if (finish) {
      Fe<S> r;
      mle::round_finish<S, SHAPE, M>(r, acc[0][t]);
      alignas(16) uint32_t vo[8];
      fe_store<S>(vo, r);
      memcpy(out + 8 * t, vo, 32);
    } else {
      uint32_t wo[8];
      fe_pack<S>(wo, acc[0][t]);
      memcpy(out + 8 * t, wo, 32);
    }
  }
  return NV;
}

template <class S>
int round_any(int shape, int m, const uint32_t* a, int pairs, int cut, int finish, uint32_t* out) {
  if (shape == MSM_SUMCHECK_R1CS) return m == 4 ? run_round<S, MSM_SUMCHECK_R1CS, 4>(a, pairs, cut, finish, out) : -1;
  if (shape != MSM_SUMCHECK_PROD) return -1;
  switch (m) {
    case 1: return run_round<S, MSM_SUMCHECK_PROD, 1>(a, pairs, cut, finish, out);
    case 2: return run_round<S, MSM_SUMCHECK_PROD, 2>(a, pairs, cut, finish, out);
    case 3: return run_round<S, MSM_SUMCHECK_PROD, 3>(a, pairs, cut, finish, out);
    case 4: return run_round<S, MSM_SUMCHECK_PROD, 4>(a, pairs, cut, finish, out);
  }
  return -1;
}

// the finish step alone on a value below 2 q that owes the shape's factors R, raw words in, canonical words out
template <class S, int SHAPE, int M>
void run_finish(const uint32_t* acc, uint32_t* out) {
  uint32_t w[8];
  memcpy(w, acc, sizeof w);
  Fe<S> a, r;
  fe_unpack<S>(a, w);
  mle::round_finish<S, SHAPE, M>(r, a);
  fe_pack<S>(w, r);
  memcpy(out, w, sizeof w);
}

template <class S>
int finish_any(int shape, int m, const uint32_t* acc, uint32_t* out) {
  if (shape == MSM_SUMCHECK_R1CS) return run_finish<S, MSM_SUMCHECK_R1CS, 4>(acc, out), 0;
  switch (m) {
    case 1: return run_finish<S, MSM_SUMCHECK_PROD, 1>(acc, out), 0;
    case 2: return run_finish<S, MSM_SUMCHECK_PROD, 2>(acc, out), 0;
    case 3: return run_finish<S, MSM_SUMCHECK_PROD, 3>(acc, out), 0;
    case 4: return run_finish<S, MSM_SUMCHECK_PROD, 4>(acc, out), 0;
  }
  return -1;
}

// a wide value (limbs normalised, below 2^262: 9 words, the ninth holding what is above 2^256) -> reduce_wide, 9 words out
template <class S>
void run_reduce_wide(const uint32_t* in9, uint32_t* out9) {
  Fe<S> a;
  for (int i = 0; i < S::NL; i++) {
    const int bit = LB * i, wi = bit / 32, sh = bit % 32;
    const uint64_t two = (uint64_t)in9[wi] | ((uint64_t)(wi + 1 < 9 ? in9[wi + 1] : 0u) << 32);
    a.l[i] = i + 1 < S::NL ? (uint32_t)(two >> sh) & LMASK : (uint32_t)(two >> sh);
  }
  mle::reduce_wide<S>(a);
  uint32_t w[8];
  fe_pack<S>(w, a);
  memcpy(out9, w, sizeof w);
  out9[8] = a.l[S::NL - 1] >> 16;
}

template <class S>
void run_bind(const uint32_t* lo, const uint32_t* hi, const uint32_t* r, uint32_t* out) {
  alignas(16) uint32_t vl[8], vh[8], vo[8];
  memcpy(vl, lo, sizeof vl);
  memcpy(vh, hi, sizeof vh);
  Fe<S> rm;
  m_from_words<S>(rm, *(Words8*)r);
  mle::bind_lane<S>(vo, vl, vh, rm);
  memcpy(out, vo, sizeof vo);
}

// the whole table eq(r, .) scaled by s over v variables as the two kernels build it: the factors as the entry point makes them,
// the half-tables entry by entry, one eq_lane per element.  tab_out (may be null): the 2^k + 2^(v - k) half-table entries
template <class S>
int run_eq(const uint32_t* r, uint32_t v, const uint32_t* s, uint32_t* out, uint32_t* tab_out) {
  static mle::EqFactors<S> fac;
  Fe<S> sm, unit, one;
  m_from_words<S>(sm, *(Words8*)s);
  fe_set_one<S>(unit);
  fe_set_zero<S>(one);
  one.l[0] = 1;
  for (uint32_t j = 0; j < v; j++) {
    Fe<S> rm, om;
    m_from_words<S>(rm, *(Words8*)(r + 8 * j));
    fe_sub_p<S>(om, unit, rm);
    fe_reduce_2p<S>(om);
    for (int i = 0; i < S::NL; i++) {
      fac.l[j][0][i] = om.l[i];
      fac.l[j][1][i] = rm.l[i];
    }
  }
  const uint32_t k = mle::eq_split(v), n_lo = 1u << k, n_hi = 1u << (v - k);
  uint32_t* tab = new uint32_t[8 * (size_t)(n_lo + n_hi) + 4];
  uint32_t* t16 = (uint32_t*)(((uintptr_t)tab + 15) & ~(uintptr_t)15);
  for (uint32_t e = 0; e < n_lo + n_hi; e++) {
    Fe<S> x;
    if (e < n_lo) mle::eq_entry<S>(x, one, fac, 0, k, e);
    else mle::eq_entry<S>(x, sm, fac, k, v - k, e - n_lo);
    fe_store<S>(t16 + 8 * (size_t)e, x);
  }
  if (tab_out) memcpy(tab_out, t16, 32 * (size_t)(n_lo + n_hi));
  for (uint64_t i = 0; i < (1ull << v); i++) {
    alignas(16) uint32_t vo[8];
    mle::eq_lane<S>(vo, t16 + 8 * (i & (n_lo - 1)), t16 + 8 * (n_lo + (i >> k)));
    memcpy(out + 8 * i, vo, sizeof vo);
  }
  delete[] tab;
  return (int)k;
}

}  // namespace

#define MLE_DISPATCH()                                 \
  switch (curve) {                                          \
    MSM_SCALAR_FIELDS(MLE_CASE)                             \
    default: return -1;                                     \
  }

extern "C" {

int mle_block(void) { return mle::BLOCK; }
int mle_round_max_blocks(void) { return (int)mle::ROUND_MAX_BLOCKS; }
uint64_t mle_pair_lo(uint64_t i, uint32_t var) { return mle::pair_lo(i, var); }
uint64_t mle_pair_hi(uint64_t i, uint32_t var) { return mle::pair_hi(i, var); }
int mle_round_values(int shape, int m) { return mle::round_values(shape, m); }
int mle_round_owed(int shape, int m) { return mle::round_owed(shape, m); }
int mle_eq_split(uint32_t v) { return (int)mle::eq_split(v); }

// M q of raw_delta and C of reduce_wide: 9 limbs of 30 bits, then C
int mle_constants(int curve, uint32_t* out10) {
#define MLE_CASE(ID, S) case ID: { constexpr mle::Limbs<S> mq = mle::mq_limbs<S>(); for (int i = 0; i < 9; i++) out10[i] = mq.l[i]; \
                                   out10[9] = mle::wide_quotient_const<S>(); return 0; }
  MLE_DISPATCH()
#undef MLE_CASE
}

// returns the number of values written, -1 for an unknown curve, shape or m
int mle_round(int curve, int shape, int m, const uint32_t* a, int pairs, int cut, int finish, uint32_t* out) {
#define MLE_CASE(ID, S) case ID: return round_any<S>(shape, m, a, pairs, cut, finish, out);
  MLE_DISPATCH()
#undef MLE_CASE
}

int mle_finish(int curve, int shape, int m, const uint32_t* acc, uint32_t* out) {
#define MLE_CASE(ID, S) case ID: return finish_any<S>(shape, m, acc, out);
  MLE_DISPATCH()
#undef MLE_CASE
}

int mle_reduce_wide(int curve, const uint32_t* in9, uint32_t* out9) {
#define MLE_CASE(ID, S) case ID: run_reduce_wide<S>(in9, out9); return 0;
  MLE_DISPATCH()
#undef MLE_CASE
}

int mle_bind(int curve, const uint32_t* lo, const uint32_t* hi, const uint32_t* r, uint32_t* out) {
#define MLE_CASE(ID, S) case ID: run_bind<S>(lo, hi, r, out); return 0;
  MLE_DISPATCH()
#undef MLE_CASE
}

// returns the split k
int mle_eq(int curve, const uint32_t* r, uint32_t v, const uint32_t* s, uint32_t* out, uint32_t* tab_out) {
#define MLE_CASE(ID, S) case ID: return run_eq<S>(r, v, s, out, tab_out);
  MLE_DISPATCH()
#undef MLE_CASE
}
}
