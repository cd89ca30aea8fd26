// Host-side unit-test shim of the resident scans: the plan, the three combine operators with their way in and out, and the lane body
// of the batch inverse of montgomery_amd/csrc/scalar_scan.h compiled for the CPU (tests/test_scans_host.py), and the tile constants,
// so that the GPU tests take their sizes from the library.  No GPU work.
#include "scalar_scan.h"
#include "scalar_host.h"
#include <cstring>
#include <vector>
using namespace msm;
using namespace msmi;

namespace {

// enter(a) o enter(b) with b a segment of 2^k elements, then leave: a, b raw (any 256-bit value), z below q (HORNER only)
template <class S, int OP>
void combine_one(const uint32_t* a, const uint32_t* b, const uint32_t* z, int k, uint32_t* out) {
  alignas(16) uint32_t wa[8], wb[8], wz[8], wo[8];
  memcpy(wa, a, sizeof wa);
  memcpy(wb, b, sizeof wb);
  memcpy(wz, z, sizeof wz);
  Fe<S> fa, fb, zm, r;
  fe_load<S>(fa, wa);
  fe_load<S>(fb, wb);
  scan::enter<S, OP>(fa);
  scan::enter<S, OP>(fb);
  scan::PowTab<S> pw = {};
  fe_load<S>(zm, wz);
  sv::to_mont<S>(zm, zm);
  fill_pow_table<S>(pw, zm, scan::POW_BITS);
  scan::combine<S, OP>(r, fa, fb, pw, k);
  scan::leave<S, OP>(r);
  fe_store<S>(wo, r);
  memcpy(out, wo, sizeof wo);
}

template <class S>
void combine_op(int op, const uint32_t* a, const uint32_t* b, const uint32_t* z, int k, uint32_t* out) {
  if (op == scan::OP_SUM) combine_one<S, scan::OP_SUM>(a, b, z, k, out);
  else if (op == scan::OP_PRODUCT) combine_one<S, scan::OP_PRODUCT>(a, b, z, k, out);
  else combine_one<S, scan::OP_HORNER>(a, b, z, k, out);
}

// the chain of n elements as the kernel's lanes walk it: `lanes` lanes, lane l over the elements l, l + lanes, ... of each group of
// INV_E x lanes elements
template <class S>
uint64_t inverse_chain(const uint32_t* in, uint64_t n, uint32_t lanes, uint32_t* out) {
  std::vector<uint4> src(2 * n + 2), dst(2 * n + 2);
  memcpy(src.data(), in, n * 32);
  uint64_t zeros = 0;
  const uint64_t group = (uint64_t)scan::INV_E * lanes;
  for (uint64_t base = 0; base < n; base += group)
    for (uint32_t l = 0; l < lanes; l++)
      zeros += scan::inverse_lane<S, scan::INV_E>((uint32_t*)dst.data(), (const uint32_t*)src.data(), base + l, lanes, n);
  memcpy(out, dst.data(), n * 32);
  return zeros;
}

}  // namespace

#define SCANS_DISPATCH()                                    \
  switch (curve) {                                          \
    MSM_SCALAR_FIELDS(SCANS_CASE)                           \
    default: return -1;                                     \
  }                                                         \
  return 0;

extern "C" {

int scans_default_tile_log(void) { return scan::DEFAULT_TILE_LOG; }
int scans_min_tile_log(void) { return scan::MIN_TILE_LOG; }
int scans_block(void) { return scan::BLOCK; }
int scans_inverse_e(void) { return scan::INV_E; }
int scans_max_levels(void) { return scan::MAX_LEVELS; }

// tiles per level into tiles_out (room for scans_max_levels()); returns the level count
int scans_plan(uint64_t n, int tile_log, int32_t* tiles_out) {
  const scan::Plan p = scan::scan_plan(n, tile_log);
  for (int i = 0; i < p.levels; i++) tiles_out[i] = (int32_t)p.tiles[i];
  return p.levels;
}

int scans_modulus(int curve, uint32_t* out) {
#define SCANS_CASE(ID, S) case ID: for (int j = 0; j < 8; j++) out[j] = S::PW[j]; break;
  SCANS_DISPATCH()
#undef SCANS_CASE
}

// op: 0 sum, 1 product, 2 Horner (a z^(2^k) + b)
int scans_combine(int curve, int op, const uint32_t* a, const uint32_t* b, const uint32_t* z, int k, uint32_t* out) {
#define SCANS_CASE(ID, S) case ID: combine_op<S>(op, a, b, z, k, out); break;
  SCANS_DISPATCH()
#undef SCANS_CASE
}

int scans_inverse(int curve, const uint32_t* in, uint64_t n, uint32_t lanes, uint32_t* out, uint64_t* zeros_out) {
#define SCANS_CASE(ID, S) case ID: *zeros_out = inverse_chain<S>(in, n, lanes, out); break;
  SCANS_DISPATCH()
#undef SCANS_CASE
}
}
