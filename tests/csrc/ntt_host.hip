// Host-side unit-test shim of the resident NTT: the plan, the pass geometry, the index and exponent functions and the lane bodies of
// montgomery_amd/csrc/scalar_ntt.h compiled for the CPU (tests/test_ntt_host.py).  The executor runs a whole transform as the
// kernels do -- per pass, per block, the load phase for every lane, each stage for every lane, the store phase for every lane,
// on a tile image of the LDS -- with tables filled on the host by plain multiplications (the field helpers are those of
// scalar_host.h).  No GPU work.
#include "scalar_ntt.h"
#include "scalar_host.h"
#include <cstring>
#include <vector>
using namespace msm;
using namespace msmi;

namespace {

using Words8 = const uint32_t[8];   // a canonical host scalar as it crosses the C boundary

// out[8 i ..] = s x^i in Montgomery form (s, x Montgomery), i < count, 16-byte aligned storage
template <class S>
void fill_powers(std::vector<uint4>& store, uint32_t count, Fe<S> s, const Fe<S>& x) {
  store.assign(2 * (size_t)count, make_uint4(0, 0, 0, 0));
  uint32_t* out = (uint32_t*)store.data();
  for (uint32_t i = 0; i < count; i++) {
    fe_store<S>(out + 8 * (size_t)i, s);
    m_mul<S>(s, s, x);
  }
}

// reduce_raw on both operands (the first load of a transform), then the butterfly; results below 2 q, as raw words
template <class S>
void butterfly(const uint32_t* u, const uint32_t* v, const uint32_t* w, int with_w, uint32_t* out_u, uint32_t* out_v) {
  uint32_t wu[8], wv[8], wo[8];
  memcpy(wu, u, sizeof wu);
  memcpy(wv, v, sizeof wv);
  Fe<S> fu, fv, fw;
  fe_unpack<S>(fu, wu);
  fe_unpack<S>(fv, wv);
  ntt::reduce_raw<S>(fu);
  ntt::reduce_raw<S>(fv);
  if (with_w) {
    m_from_words<S>(fw, *(Words8*)w);
    ntt::butterfly<S>(fu, fv, &fw);
  } else {
    ntt::butterfly<S>(fu, fv, nullptr);
  }
  fe_pack<S>(wo, fu);
  memcpy(out_u, wo, sizeof wo);
  fe_pack<S>(wo, fv);
  memcpy(out_v, wo, sizeof wo);
}

// w: omega, or omega^-1 for an inverse transform.  scale: ntt::ScaleMode; SCALE_CONST multiplies the last store by s;
// SCALE_TABLE multiplies by s x^j (forward: the first load, j the input index; inverse: the last store, j the output index)
template <class S>
void exec(int log2n, uint32_t B, int tile_log, const uint32_t* w, int scale, const uint32_t* s, const uint32_t* x, int inverse,
          const uint32_t* in, uint32_t* out) {
  const int L = log2n, h = ntt::table_low_bits(L), g = L < ntt::LDS_LOG ? L : ntt::LDS_LOG;
  Fe<S> one, wm, t, sm, xm;
  fe_set_one<S>(one);
  m_from_words<S>(wm, *(Words8*)w);
  std::vector<uint4> wa, wb, gt, sa, sb;
  fill_powers<S>(wa, 1u << h, one, wm);
  m_pow2k<S>(t, wm, h);
  fill_powers<S>(wb, 1u << (L - h), one, t);
  m_pow2k<S>(t, wm, L - g);
  fill_powers<S>(gt, g ? 1u << (g - 1) : 1u, one, t);
  fe_set_zero<S>(sm);
  if (scale != ntt::SCALE_NONE) m_from_words<S>(sm, *(Words8*)s);
  if (scale == ntt::SCALE_TABLE) {
    m_from_words<S>(xm, *(Words8*)x);
    fill_powers<S>(sa, 1u << h, sm, xm);
    m_pow2k<S>(t, xm, h);
    fill_powers<S>(sb, 1u << (L - h), one, t);
  }
  ntt::Tables tb = {(const uint32_t*)wa.data(), (const uint32_t*)wb.data(), (const uint32_t*)gt.data(),
                    sa.empty() ? nullptr : (const uint32_t*)sa.data(), sb.empty() ? nullptr : (const uint32_t*)sb.data()};

  const uint64_t total = (uint64_t)B << L;
  std::vector<uint4> src(2 * total), scratch(2 * total), dst(2 * total);
  memcpy(src.data(), in, total * 32);
  const ntt::Plan plan = ntt::ntt_plan(L, tile_log);
  const int launches = plan.passes ? plan.passes : 1;
  std::vector<uint32_t> lds(8 * ntt::PLANE);
  for (int i = 0; i < launches; i++) {
    const ntt::Pass ps = ntt::pass_geometry(plan, i, B, scale, inverse != 0);
    const uint32_t* from = ps.first ? (const uint32_t*)src.data() : (const uint32_t*)scratch.data();
    uint32_t* to = ps.last ? (uint32_t*)dst.data() : (uint32_t*)scratch.data();
    const uint64_t blocks = ntt::pass_blocks(ps);
    for (uint64_t blk = 0; blk < blocks; blk++) {
      std::fill(lds.begin(), lds.end(), 0u);
      for (uint32_t lane = 0; lane < ntt::BLOCK; lane++) ntt::load_phase<S>(ps, tb, from, lds.data(), (uint32_t)blk, lane, ntt::BLOCK);
      for (int k = 0; k < ps.t; k++)
        for (uint32_t lane = 0; lane < ntt::BLOCK; lane++) ntt::stage_phase<S>(ps, tb, lds.data(), k, lane, ntt::BLOCK);
      for (uint32_t lane = 0; lane < ntt::BLOCK; lane++) ntt::store_phase<S>(ps, tb, sm, to, lds.data(), (uint32_t)blk, lane, ntt::BLOCK);
    }
  }
  memcpy(out, dst.data(), total * 32);
}

}  // namespace

#define NTT_DISPATCH()                                      \
  switch (curve) {                                          \
    MSM_SCALAR_FIELDS(NTT_CASE)                             \
    default: return -1;                                     \
  }                                                         \
  return 0;

extern "C" {

int ntt_default_tile_log(void) { return ntt::DEFAULT_TILE_LOG; }
int ntt_max_tile_log(void) { return ntt::MAX_TILE_LOG; }
int ntt_max_log2n(void) { return ntt::MAX_LOG2N; }

// stages per pass into stages_out (room for 29); returns the pass count
int ntt_plan(int log2n, int tile_log, int32_t* stages_out) {
  const ntt::Plan p = ntt::ntt_plan(log2n, tile_log);
  for (int i = 0; i < p.passes; i++) stages_out[i] = p.stages[i];
  return p.passes;
}

int ntt_modulus(int curve, uint32_t* out) {
#define NTT_CASE(ID, S) case ID: for (int j = 0; j < 8; j++) out[j] = S::PW[j]; break;
  NTT_DISPATCH()
#undef NTT_CASE
}

// u, v raw (any 256-bit value), w below q; with_w == 0: the stage-0 form (w = 1, no multiplication)
int ntt_butterfly(int curve, const uint32_t* u, const uint32_t* v, const uint32_t* w, int with_w, uint32_t* out_u, uint32_t* out_v) {
#define NTT_CASE(ID, S) case ID: butterfly<S>(u, v, w, with_w, out_u, out_v); break;
  NTT_DISPATCH()
#undef NTT_CASE
}

int ntt_exec(int curve, int log2n, uint32_t B, int tile_log, const uint32_t* w, int scale, const uint32_t* s, const uint32_t* x,
             int inverse, const uint32_t* in, uint32_t* out) {
#define NTT_CASE(ID, S) case ID: exec<S>(log2n, B, tile_log, w, scale, s, x, inverse, in, out); break;
  NTT_DISPATCH()
#undef NTT_CASE
}
}
