// The host's side of the scalar field, the integers mod the group order q, for the operators over resident scalars and points
// (msm_scalars.hip, msm_scan.hip, msm_ntt.hip, msm_mle.hip, msm_spmv.hip, msm_lincomb.hip) and for the CPU shims under tests/csrc: how a scalar of a call is
// read and refused, the field work a call does once (powers, inverses, roots of unity) and the power tables its kernels take as
// arguments.  Host only: the fe_* templates of field.h run here as they do in a lane, and nothing in this file launches anything.
// Templates over the scalar FIELD S of scalar_vec.h (MSM_SCALAR_FIELDS), 8 words, Fe<S> of 9 limbs, R = 2^270.
// tests/test_scalar_host.py checks all of it against Python integers.
#pragma once
#include "scalar_vec.h"
#include <cstring>

struct msm_ctx;

namespace msmi {
using namespace msm;

int fail(msm_ctx* ctx, int code, const char* fmt, ...);   // msm_plan.hip

// ---------------------------------------------------------------- the scalars of a call: 32 bytes little-endian, below q

// -> words; false: the value is >= q
template <class S>
bool scalar_words(uint32_t (&w)[8], const uint8_t* bytes) {
  for (int j = 0; j < 8; j++)
    w[j] = (uint32_t)bytes[4 * j] | ((uint32_t)bytes[4 * j + 1] << 8) | ((uint32_t)bytes[4 * j + 2] << 16) | ((uint32_t)bytes[4 * j + 3] << 24);
  for (int j = 7; j >= 0; j--) {
    if (w[j] < S::PW[j]) return true;
    if (w[j] > S::PW[j]) return false;
  }
  return false;
}

// -> registers, canonical; false: the value is >= q
template <class S>
bool host_scalar(Fe<S>& r, const uint8_t* bytes) {
  uint32_t w[8];
  if (!scalar_words<S>(w, bytes)) return false;
  fe_unpack<S>(r, w);
  return true;
}

// -> registers, in Montgomery form; false: the value is >= q
template <class S>
bool host_scalar_mont(Fe<S>& r, const uint8_t* bytes) {
  if (!host_scalar<S>(r, bytes)) return false;
  sv::to_mont<S>(r, r);
  return true;
}

inline void words_to_bytes(uint8_t* out, const uint32_t (&w)[8]) {
  for (int j = 0; j < 8; j++)
    for (int b = 0; b < 4; b++) out[4 * j + b] = (uint8_t)(w[j] >> (8 * b));
}

// the refusal of a scalar that is not below q
inline int scalar_too_big(msm_ctx* ctx, const char* who, const char* name) {
  return fail(ctx, MSM_ERR_SCALAR, "%s: %s >= q (scalars of this call are never reduced)", who, name);
}

// ---------------------------------------------------------------- field work: Fe<S> in canonical Montgomery form

template <class S>
void m_mul(Fe<S>& r, const Fe<S>& a, const Fe<S>& b) {
  fe_mul<S>(r, a, b);
  fe_reduce_2p<S>(r);
}

template <class S>
void m_from_words(Fe<S>& r, const uint32_t (&w)[8]) {   // w < q
  fe_unpack<S>(r, w);
  sv::to_mont<S>(r, r);
}

template <class S>
void m_to_words(uint32_t (&w)[8], const Fe<S>& a) {
  Fe<S> one, r;
  fe_set_zero<S>(one);
  one.l[0] = 1;
  m_mul<S>(r, a, one);
  fe_pack<S>(w, r);
}

// base^e, e as 8 words
template <class S>
void m_pow(Fe<S>& r, const Fe<S>& base, const uint32_t (&e)[8]) {
  Fe<S> acc;
  fe_set_one<S>(acc);
  for (int bit = 255; bit >= 0; bit--) {
    m_mul<S>(acc, acc, acc);
    if ((e[bit / 32] >> (bit % 32)) & 1u) m_mul<S>(acc, acc, base);
  }
  r = acc;
}

template <class S>
void m_pow2k(Fe<S>& r, const Fe<S>& a, int k) {   // a^(2^k)
  r = a;
  for (int i = 0; i < k; i++) m_mul<S>(r, r, r);
}

// out = q - v for a small v, as words
template <class S>
void q_minus(uint32_t (&out)[8], uint32_t v) {
  uint64_t borrow = v;
  for (int j = 0; j < 8; j++) {
    const uint64_t d = (uint64_t)S::PW[j] - borrow;
    out[j] = (uint32_t)d;
    borrow = (d >> 32) & 1u;
  }
}

inline void shift_right(uint32_t (&w)[8], int k) {   // k < 32
  if (!k) return;
  for (int j = 0; j < 8; j++) w[j] = (w[j] >> k) | (j + 1 < 8 ? w[j + 1] << (32 - k) : 0u);
}

template <class S>
int two_adicity() {
  uint32_t w[8];
  q_minus<S>(w, 1);
  int s = 0;
  while (!((w[s / 32] >> (s % 32)) & 1u)) s++;
  return s;
}

template <class S>
bool m_is_minus_one(const Fe<S>& a) {
  uint32_t w[8], m1[8];
  m_to_words<S>(w, a);
  q_minus<S>(m1, 1);
  return memcmp(w, m1, sizeof w) == 0;
}

// the smallest positive quadratic non-residue: g^((q-1)/2) = -1
template <class S>
uint32_t non_residue() {
  uint32_t half[8];
  q_minus<S>(half, 1);
  shift_right(half, 1);
  for (uint32_t g = 2;; g++) {
    uint32_t w[8] = {g};
    Fe<S> gm, r;
    m_from_words<S>(gm, w);
    m_pow<S>(r, gm, half);
    if (m_is_minus_one<S>(r)) return g;
  }
}

// g^((q-1) / 2^log2n), log2n <= the two-adicity
template <class S>
void library_root(Fe<S>& r, uint32_t log2n) {
  uint32_t e[8];
  q_minus<S>(e, 1);
  for (uint32_t k = log2n; k;) {
    const int step = k > 31 ? 31 : (int)k;
    shift_right(e, step);
    k -= step;
  }
  uint32_t w[8] = {non_residue<S>()};
  Fe<S> gm;
  m_from_words<S>(gm, w);
  m_pow<S>(r, gm, e);
}

template <class S>
void m_inverse(Fe<S>& r, const Fe<S>& a) {   // a != 0
  uint32_t e[8];
  q_minus<S>(e, 2);
  m_pow<S>(r, a, e);
}

// 2^-log2n
template <class S>
void m_inverse_n(Fe<S>& r, uint32_t log2n) {
  uint32_t w[8];
  uint64_t c = 1;   // (q + 1) / 2
  for (int j = 0; j < 8; j++) {
    c += S::PW[j];
    w[j] = (uint32_t)c;
    c >>= 32;
  }
  shift_right(w, 1);
  Fe<S> half;
  m_from_words<S>(half, w);
  fe_set_one<S>(r);
  for (uint32_t k = 0; k < log2n; k++) m_mul<S>(r, r, half);
}

// ---------------------------------------------------------------- power tables

// table.l[k] = the limbs of x^(2^k) in Montgomery form, k < bits: a kernel argument, sv::PowTable<S> or scan::PowTab<S>
template <class S, class Table>
void fill_pow_table(Table& table, Fe<S> x_mont, int bits) {
  for (int k = 0; k < bits; k++) {
    for (int j = 0; j < S::NL; j++) table.l[k][j] = x_mont.l[j];
    m_mul<S>(x_mont, x_mont, x_mont);
  }
}

}  // namespace msmi
