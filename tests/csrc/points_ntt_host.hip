// Host-side unit-test shim of msm_points_ntt: the index maps and the butterfly lane of montgomery_amd/csrc/points_ntt.h compiled
// for the CPU, on the five curves whose scalar field has transforms of more than two points (tests/test_points_ntt_host.py).
// The per-lane table is a plain array of the caller's, laid out as on the device (cap lanes, this lane = g); rows are made by
// the shim of points_mul.h (tests/csrc/points_mul_host.hip).
#include "points_ntt.h"
#include <cstring>
using namespace msm;

namespace {

template <class CV>
void lane(const uint32_t* row_a, const uint32_t* row_b, const uint32_t* twiddle, bool mul, uint4* tbl, uint64_t cap, uint64_t g, uint32_t* out_a,
          uint32_t* out_b) {
  alignas(16) uint32_t a[ROW_WORDS], b[ROW_WORDS], w[8] = {0};
  memcpy(a, row_a, sizeof a);
  memcpy(b, row_b, sizeof b);
  if (twiddle) memcpy(w, twiddle, sizeof w);
  pntt::butterfly_lane<CV, pmul::W_VAR>(a, b, w, mul, tbl, cap, g);   // in place, as a stage runs it
  memcpy(out_a, a, sizeof a);
  memcpy(out_b, b, sizeof b);
}

}  // namespace

// X(curve id of include/msm_hip.h, configuration)
#define PN_CURVES(X) X(0, CvBls377) X(2, CvBls381) X(3, CvPallas) X(4, CvBn254) X(6, CvVesta)

extern "C" {

uint32_t pn_bit_reverse(uint32_t i, int log2n) { return pntt::bit_reverse(i, log2n); }

// butterfly t of stage s: out = {row a, row b, position j, twiddle index}
void pn_butterfly(uint32_t t, int log2n, int s, uint32_t* out) {
  const pntt::Fly f = pntt::butterfly(t, log2n, s);
  out[0] = f.a;
  out[1] = f.b;
  out[2] = f.j;
  out[3] = f.tw;
}

uint64_t pn_multiplications(int log2n) { return pntt::multiplications(log2n); }

// one butterfly: (out_a, out_b) = (A + w B, A - w B); mul = 0: w = 1, twiddle and table unread (both may be NULL)
int pn_lane(int curve, const uint32_t* row_a, const uint32_t* row_b, const uint32_t* twiddle, int mul, void* tbl, uint64_t cap, uint64_t g,
            uint32_t* out_a, uint32_t* out_b) {
  if (mul && (!tbl || !twiddle || g >= cap)) return -1;
  switch (curve) {
#define PN_CASE(ID, CV) case ID: lane<CV>(row_a, row_b, twiddle, mul != 0, (uint4*)tbl, cap, g, out_a, out_b); return 0;
    PN_CURVES(PN_CASE)
#undef PN_CASE
  }
  return -1;
}
}
