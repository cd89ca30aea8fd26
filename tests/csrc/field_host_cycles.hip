// Host-side unit-test shim of the cycle curves (BN254 G1, Grumpkin, Vesta): the product's field, square-root and GLV templates
// (montgomery_amd/csrc/field.h, packed.h, points_ingest.h, glv.h) compiled for the CPU (tests/test_cycle_curves.py).  The
// packed-word operations (pk_sub_mod, pk_cond_sub_p, pk_add) run here with the plain C++ carry chains packed.h has for a CPU
// build: their modular logic on a 254- / 255-bit modulus.  The device's v_subb / v_addc chains themselves are reached through
// k_batch_add only: tests/test_gpu_cycle_curves.py steers edge operands through them (test_packed_chains_on_edge_operands).
#include "points_ingest.h"
using namespace msm;

template <class C>
static void load(Fe<C>& r, const uint32_t* w) {
  uint32_t t[C::NW];
  for (int i = 0; i < C::NW; i++) t[i] = w[i];
  fe_unpack<C>(r, t);
}
template <class C>
static void store(uint32_t* w, Fe<C> a) {
  fe_reduce_4p<C>(a);
  uint32_t t[C::NW];
  fe_pack<C>(t, a);
  for (int i = 0; i < C::NW; i++) w[i] = t[i];
}

// operands: packed words, any value < 2p (the inversions' and the square root's contract; the others take more)
template <class C>
static int op(int which, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  Fe<C> x, y, r;
  int flag = 1;
  load<C>(x, a);
  load<C>(y, b);
  switch (which) {
    case 0: fe_mul<C>(r, x, y); break;
    case 1: fe_sqr<C>(r, x); break;
    case 2: fe_add<C>(r, x, y); break;
    case 3: fe_sub_2p<C>(r, x, y); break;
    case 4: fe_inv<C>(r, x); break;
    case 5: fe_inv_fermat<C>(r, x); break;
    case 6: fe_inv_kaliski<C>(r, x); break;
    case 7: fe_inv_wordsliced<C>(r, x); break;
    case 8: flag = ingest::fe_sqrt<C>(r, x) ? 1 : 0; break;
    case 9: { uint32_t w[C::NW]; ingest::fe_plain_words<C>(w, x); for (int i = 0; i < C::NW; i++) out[i] = w[i]; return 1; }
    default: r = x;
  }
  store<C>(out, r);
  return flag;
}

// packed.h on packed words: 0 = pk_sub_mod (a < 2^256, b < p), 1 = pk_cond_sub_p, 2 = pk_add (mod 2^256); returns pk_sub's borrow mask
template <class C>
static uint32_t op_packed(int which, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  PkW<C::NW> x, y, r;
  for (int i = 0; i < C::NW; i++) { x.w[i] = a[i]; y.w[i] = b[i]; }
  uint32_t m = 0;
  if (which == 0) pk_sub_mod<C>(r, x, y);
  else if (which == 1) { r = x; pk_cond_sub_p<C>(r); }
  else if (which == 2) pk_add(r, x, y);
  else m = pk_sub(r, x, y);
  for (int i = 0; i < C::NW; i++) out[i] = r.w[i];
  return m;
}

template <class C>
static void op_raw(int which, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  Fe<C> x, y, r;
  for (int i = 0; i < C::NL; i++) { x.l[i] = a[i]; y.l[i] = b[i]; }
  if (which == 1) fe_sqr<C>(r, x); else fe_mul<C>(r, x, y);
  for (int i = 0; i < C::NL; i++) out[i] = r.l[i];
}

extern "C" {
// curve 4 = BN254 G1, 5 = Grumpkin, 6 = Vesta (the ids of include/msm_hip.h): the curve's BASE field and its GLV lattice
int cyc_fp_op(int curve, int which, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (curve == 4) return op<FpBn254>(which, a, b, out);
  if (curve == 5) return op<FpGrumpkin>(which, a, b, out);
  if (curve == 6) return op<FpVesta>(which, a, b, out);
  return -1;
}
int cyc_fp_raw(int curve, int which, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (curve == 4) op_raw<FpBn254>(which, a, b, out);
  else if (curve == 5) op_raw<FpGrumpkin>(which, a, b, out);
  else if (curve == 6) op_raw<FpVesta>(which, a, b, out);
  else return -1;
  return 0;
}
int cyc_packed(int curve, int which, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* borrow) {
  if (curve == 4) *borrow = op_packed<FpBn254>(which, a, b, out);
  else if (curve == 5) *borrow = op_packed<FpGrumpkin>(which, a, b, out);
  else if (curve == 6) *borrow = op_packed<FpVesta>(which, a, b, out);
  else return -1;
  return 0;
}
int cyc_glv(int curve, const uint32_t* s8, uint32_t* out10) {
  uint32_t s[8];
  for (int i = 0; i < 8; i++) s[i] = s8[i];
  GlvHalf h0, h1;
  if (curve == 4) glv_decompose<GlvBn254>(h0, h1, s);
  else if (curve == 5) glv_decompose<GlvGrumpkin>(h0, h1, s);
  else if (curve == 6) glv_decompose<GlvVesta>(h0, h1, s);
  else return -1;
  for (int i = 0; i < 4; i++) { out10[i] = h0.mag[i]; out10[4 + i] = h1.mag[i]; }
  out10[8] = h0.neg; out10[9] = h1.neg;
  return 0;
}
}
