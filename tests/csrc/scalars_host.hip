// Host-side unit-test shim of the resident scalar-vector operations: the lane bodies of montgomery_amd/csrc/scalar_vec.h compiled
// for the CPU, over the scalar field MSM_SCALAR_FIELDS gives every curve (tests/test_scalars_host.py).  Elements cross as 8 words,
// plain little-endian integers below 2^256, as the kernels read them from device memory.
#include "scalar_vec.h"
#include "scalar_host.h"
#include <cstring>
using namespace msm;
using namespace msmi;

namespace {

using Words8 = const uint32_t[8];   // a canonical host scalar as it crosses the C boundary (-> Montgomery form once per call)

template <class S>
void lincomb(const uint32_t* x, const uint32_t* a, const uint32_t* y, const uint32_t* b, uint32_t* out) {
  alignas(16) uint32_t va[8], vb[8], vo[8];
  Fe<S> xm, ym;
  m_from_words<S>(xm, *(Words8*)x);
  memcpy(va, a, sizeof va);
  if (b) {
    m_from_words<S>(ym, *(Words8*)y);
    memcpy(vb, b, sizeof vb);
    sv::lincomb_lane<S, true>(vo, va, vb, xm, ym);
  } else {
    fe_set_zero<S>(ym);
    sv::lincomb_lane<S, false>(vo, va, va, xm, ym);
  }
  memcpy(out, vo, sizeof vo);
}

template <class S>
void mul(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  alignas(16) uint32_t va[8], vb[8], vo[8];
  memcpy(va, a, sizeof va);
  memcpy(vb, b, sizeof vb);
  sv::mul_lane<S>(vo, va, vb);
  memcpy(out, vo, sizeof vo);
}

// the lanes of the given indices of powers(s, x): the table of x^(2^k) as the host builds it, 30 entries
template <class S>
void powers(const uint32_t* s, const uint32_t* x, const uint32_t* idx, int n_idx, uint32_t* out) {
  uint32_t w[8];
  memcpy(w, s, sizeof w);
  Fe<S> sp, xm;
  fe_unpack<S>(sp, w);
  m_from_words<S>(xm, *(Words8*)x);
  static sv::PowTable<S> pw;
  fill_pow_table<S>(pw, xm, sv::MAX_POW_BITS);
  for (int t = 0; t < n_idx; t++) {
    Fe<S> r;
    sv::powers_lane<S>(r, sp, pw, idx[t], sv::MAX_POW_BITS);
    alignas(16) uint32_t vo[8];
    fe_store<S>(vo, r);
    memcpy(out + 8 * t, vo, sizeof vo);
  }
}

// the inner product of n pairs as one lane would form it -- term, combine, ... -- split at `cut` into two accumulators that
// are then combined (a wave's or a block's step), and finished
template <class S>
void inner(const uint32_t* a, const uint32_t* b, int n, int cut, uint32_t* out) {
  Fe<S> acc[2], t, r;
  fe_set_zero<S>(acc[0]);
  fe_set_zero<S>(acc[1]);
  for (int i = 0; i < n; i++) {
    alignas(16) uint32_t va[8], vb[8];
    memcpy(va, a + 8 * i, sizeof va);
    memcpy(vb, b + 8 * i, sizeof vb);
    sv::inner_term<S>(t, va, vb);
    sv::inner_combine<S>(acc[i >= cut], t);
  }
  sv::inner_combine<S>(acc[0], acc[1]);
  sv::inner_finish<S>(r, acc[0]);
  alignas(16) uint32_t vo[8];
  fe_store<S>(vo, r);
  memcpy(out, vo, sizeof vo);
}

// the combine step alone on two values below 2 q, as raw words in and out (the result is below 2 q, not canonical)
template <class S>
void combine(const uint32_t* u, const uint32_t* v, uint32_t* out) {
  uint32_t wu[8], wv[8], wo[8];
  memcpy(wu, u, sizeof wu);
  memcpy(wv, v, sizeof wv);
  Fe<S> fu, fv;
  fe_unpack<S>(fu, wu);
  fe_unpack<S>(fv, wv);
  sv::inner_combine<S>(fu, fv);
  fe_pack<S>(wo, fu);
  memcpy(out, wo, sizeof wo);
}

}  // namespace

#define SV_DISPATCH()                                       \
  switch (curve) {                                          \
    MSM_SCALAR_FIELDS(SV_CASE)                              \
    default: return -1;                                     \
  }                                                         \
  return 0;

extern "C" {

int sv_inner_max_blocks(void) { return (int)sv::INNER_MAX_BLOCKS; }
int sv_block(void) { return sv::BLOCK; }

// the modulus of the field the dispatch gives the curve, 8 words
int sv_modulus(int curve, uint32_t* out) {
#define SV_CASE(ID, S) case ID: for (int j = 0; j < 8; j++) out[j] = S::PW[j]; break;
  SV_DISPATCH()
#undef SV_CASE
}

// out = x a + y b; b null: x a
int sv_lincomb(int curve, const uint32_t* x, const uint32_t* a, const uint32_t* y, const uint32_t* b, uint32_t* out) {
#define SV_CASE(ID, S) case ID: lincomb<S>(x, a, y, b, out); break;
  SV_DISPATCH()
#undef SV_CASE
}

int sv_mul(int curve, const uint32_t* a, const uint32_t* b, uint32_t* out) {
#define SV_CASE(ID, S) case ID: mul<S>(a, b, out); break;
  SV_DISPATCH()
#undef SV_CASE
}

int sv_powers(int curve, const uint32_t* s, const uint32_t* x, const uint32_t* idx, int n_idx, uint32_t* out) {
#define SV_CASE(ID, S) case ID: powers<S>(s, x, idx, n_idx, out); break;
  SV_DISPATCH()
#undef SV_CASE
}

int sv_inner(int curve, const uint32_t* a, const uint32_t* b, int n, int cut, uint32_t* out) {
#define SV_CASE(ID, S) case ID: inner<S>(a, b, n, cut, out); break;
  SV_DISPATCH()
#undef SV_CASE
}

int sv_combine(int curve, const uint32_t* u, const uint32_t* v, uint32_t* out) {
#define SV_CASE(ID, S) case ID: combine<S>(u, v, out); break;
  SV_DISPATCH()
#undef SV_CASE
}
}
