// Host-side unit-test shim of montgomery_amd/csrc/scalar_host.h -- how a call's scalars are read, the field work of the scalar
// fields, the power tables -- over the field MSM_SCALAR_FIELDS gives every curve, and of the range and row rules of
// operator_checks.h over a default-constructed context (compiled together with msm_plan.hip, whose fail() the refusals go
// through), for tests/test_scalar_host.py.  Field elements cross as 8 little-endian words.  No GPU is touched.
#include "operator_checks.h"
#include "scalar_host.h"
#include "scalar_scan.h"
using namespace msmi;

namespace {

using Words8 = const uint32_t[8];

// the limbs as they stand (a Montgomery form stays one) -> words
template <class S>
void raw_words(uint32_t* out, const Fe<S>& a) {
  uint32_t w[8];
  fe_pack<S>(w, a);
  memcpy(out, w, sizeof w);
}

template <class S>
int parse(const uint8_t* bytes, uint32_t* words, uint32_t* canonical, uint32_t* mont, uint8_t* bytes_back) {
  uint32_t w[8];
  Fe<S> c, m;
  const bool ok = scalar_words<S>(w, bytes);
  if (ok != host_scalar<S>(c, bytes) || ok != host_scalar_mont<S>(m, bytes)) return -1;   // the three forms agree on the refusal
  memcpy(words, w, sizeof w);
  words_to_bytes(bytes_back, w);
  if (ok) {
    raw_words<S>(canonical, c);
    raw_words<S>(mont, m);
  }
  return ok ? 1 : 0;
}

template <class S>
void root(uint32_t log2n, uint32_t* out) {
  Fe<S> r;
  uint32_t w[8];
  library_root<S>(r, log2n);
  m_to_words<S>(w, r);
  memcpy(out, w, sizeof w);
}

template <class S>
void inverse(const uint32_t* a, uint32_t* out) {
  Fe<S> am, r;
  uint32_t w[8];
  m_from_words<S>(am, *(Words8*)a);
  m_inverse<S>(r, am);
  m_to_words<S>(w, r);
  memcpy(out, w, sizeof w);
}

template <class S>
void inverse_n(uint32_t k, uint32_t* out) {
  Fe<S> r;
  uint32_t w[8];
  m_inverse_n<S>(r, k);
  m_to_words<S>(w, r);
  memcpy(out, w, sizeof w);
}

template <class S, class Table>
void table_entries(const uint32_t* x, int bits, uint32_t* out) {
  Fe<S> xm, e;
  m_from_words<S>(xm, *(Words8*)x);
  static Table table;
  fill_pow_table<S>(table, xm, bits);
  for (int k = 0; k < bits; k++) {
    for (int j = 0; j < S::NL; j++) e.l[j] = table.l[k][j];
    raw_words<S>(out + 8 * k, e);
  }
}

// bits: 30, the table of k_sv_powers; 40, that of the scans
template <class S>
int pow_table(const uint32_t* x, int bits, uint32_t* out) {
  if (bits == sv::MAX_POW_BITS) table_entries<S, sv::PowTable<S>>(x, bits, out);
  else if (bits == scan::POW_BITS) table_entries<S, scan::PowTab<S>>(x, bits, out);
  else return -1;
  return 0;
}

}  // namespace

#define SH_DISPATCH()                                       \
  switch (curve) {                                          \
    MSM_SCALAR_FIELDS(SH_CASE)                              \
    default: return -2;                                     \
  }

extern "C" {

int sh_modulus(int curve, uint32_t* out) {
#define SH_CASE(ID, S) case ID: for (int j = 0; j < 8; j++) out[j] = S::PW[j]; return 0;
  SH_DISPATCH()
#undef SH_CASE
}

// 1: below q (words, canonical limbs and Montgomery limbs as words); 0: refused (words only); bytes_back: the words as bytes again
int sh_parse(int curve, const uint8_t* bytes, uint32_t* words, uint32_t* canonical, uint32_t* mont, uint8_t* bytes_back) {
#define SH_CASE(ID, S) case ID: return parse<S>(bytes, words, canonical, mont, bytes_back);
  SH_DISPATCH()
#undef SH_CASE
}

int sh_two_adicity(int curve) {
#define SH_CASE(ID, S) case ID: return two_adicity<S>();
  SH_DISPATCH()
#undef SH_CASE
}

int64_t sh_non_residue(int curve) {
#define SH_CASE(ID, S) case ID: return (int64_t)non_residue<S>();
  SH_DISPATCH()
#undef SH_CASE
}

int sh_library_root(int curve, uint32_t log2n, uint32_t* out) {
#define SH_CASE(ID, S) case ID: root<S>(log2n, out); return 0;
  SH_DISPATCH()
#undef SH_CASE
}

int sh_inverse(int curve, const uint32_t* a, uint32_t* out) {
#define SH_CASE(ID, S) case ID: inverse<S>(a, out); return 0;
  SH_DISPATCH()
#undef SH_CASE
}

int sh_inverse_n(int curve, uint32_t k, uint32_t* out) {
#define SH_CASE(ID, S) case ID: inverse_n<S>(k, out); return 0;
  SH_DISPATCH()
#undef SH_CASE
}

// out: bits entries of 8 words, entry k = the Montgomery form of x^(2^k)
int sh_pow_table(int curve, const uint32_t* x, int bits, uint32_t* out) {
#define SH_CASE(ID, S) case ID: return pow_table<S>(x, bits, out);
  SH_DISPATCH()
#undef SH_CASE
}

// the refusal of a scalar `name` of the call `who`: its code, and its text into msg
int sh_scalar_too_big(const char* who, const char* name, char* msg, int msg_cap) {
  msm_ctx ctx;
  const int rc = scalar_too_big(&ctx, who, name);
  snprintf(msg, (size_t)msg_cap, "%s", ctx.err.c_str());
  return rc;
}

// dst_ranges_ok of dst against one source "a", both given as addresses that nothing reads: its code, and its text into msg
int sh_dst_ranges_ok(uint64_t dst, uint64_t src, uint64_t bytes, char* msg, int msg_cap) {
  msm_ctx ctx;
  const int rc = dst_ranges_ok(&ctx, "sh", (const void*)(uintptr_t)dst, bytes, {{(const void*)(uintptr_t)src, "a"}});
  snprintf(msg, (size_t)msg_cap, "%s", ctx.err.c_str());
  return rc;
}

int sh_rows_overlap_ok(uint64_t lo, uint64_t count) { return rows_overlap_ok(lo, count) ? 1 : 0; }

}  // extern "C"
