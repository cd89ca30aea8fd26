// Bucket reduction of a window group (P_k = sum_l l B_(k,l): reduceBucketsColumnProjective + partition sums,
// src/msm-batched-affine.ts:556-583, :312-319) and the host tail over window sums: their sum as group elements, the Horner
// combination, projective -> affine (:322-333, src/curve-projective.ts:335-349), the wire form, msm_combine.  The fork
// between the Weierstrass and the Edwards form of a window sum is taken here and nowhere else on the host: the two point
// kinds below, and with_kind, which picks one.
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

namespace msmi {

void words_to_fe6(msm_host::Fe6& r, const uint32_t* w, int nw) {   // nw packed words, zero-extended
  for (int i = 0; i < 6; i++)
    r.v[i] = (2 * i < nw ? (uint64_t)w[2 * i] : 0) | ((2 * i + 1 < nw ? (uint64_t)w[2 * i + 1] : 0) << 32);
}

void fe6_to_bytes(uint8_t* out, const msm_host::Fe6& a) {
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 8; j++) out[8 * i + j] = (uint8_t)(a.v[i] >> (8 * j));
}

// ---- the two kinds of point on the host: zero, dbl, add, a slot in, a slot out, the affine result -------------------------

// Window sums travel as slots of packed coordinates (device Montgomery form, below 2p): X, Y, Z of 12 words each on the
// Weierstrass curves, X, Y, Z, T of 8 words each on the Edwards curve.  A projective point is a class of triples, so the host
// neither converts them on the way in nor on the way out: read as host Montgomery values the words of a device point carry one
// common factor (2^6 for 13 limbs), which is the same point, and so is every sum the host forms of such points -- an extended
// point (X, Y, Z, T) with T = X Y / Z stays valid too when all four carry one factor.  Only affine values need the exact radix
// (to_result divides the factor out with Z).
template <int N>
static void coords_from_slot(const msm_host::Field6& F, const uint32_t* w, int cw, msm_host::Fe6* const (&co)[N]) {
  for (int j = 0; j < N; j++) {
    words_to_fe6(*co[j], w + cw * j, cw);
    while (msm_host::Field6::ge(*co[j], F.p)) F.sub_raw(*co[j], *co[j], F.p);
  }
}
template <int N>
static void coords_to_slot(uint32_t* out, int cw, const msm_host::Fe6* const (&co)[N]) {   // canonical values; see above for the radix
  for (int j = 0; j < N; j++)
    for (int q = 0; q < cw / 2; q++) {
      out[cw * j + 2 * q] = (uint32_t)co[j]->v[q];
      out[cw * j + 2 * q + 1] = (uint32_t)(co[j]->v[q] >> 32);
    }
}

// x = X/Z, y = Y/Z as canonical integers (src/curve-projective.ts:335-349)
static void affine_to_result(const msm_host::Field6& F, const msm_host::Fe6& X, const msm_host::Fe6& Y, const msm_host::Fe6& Z,
                             msm_result* out) {
  msm_host::Fe6 zi, x, y, one = {{1, 0, 0, 0, 0, 0}};
  F.inv(zi, Z);
  F.mul(x, X, zi);
  F.mul(y, Y, zi);
  F.mul(x, x, one);  // leave Montgomery form
  F.mul(y, y, one);
  memset(out->x, 0, 48);
  memset(out->y, 0, 48);
  fe6_to_bytes(out->x, x);
  fe6_to_bytes(out->y, y);
  out->is_infinity = 0;
}

struct WKind {   // projective points of a Weierstrass curve
  using P = msm_host::Proj6;
  const msm_host::Curve6& C;
  static constexpr int SLOT_WORDS = W_SUM_WORDS;
  P zero() const { return C.zero(); }
  P dbl(const P& a) const { return C.dbl(a); }
  P add(const P& a, const P& b) const { return C.add(a, b); }
  P from_slot(const uint32_t* w) const {
    P r;
    coords_from_slot(C.F, w, 12, {&r.X, &r.Y, &r.Z});
    return r;
  }
  void to_slot(const P& a, uint32_t* out) const { coords_to_slot(out, 12, {&a.X, &a.Y, &a.Z}); }
  P from_wire(const msm_host::Fe6 (&t)[3]) const {
    P r;
    r.X = t[0]; r.Y = t[1]; r.Z = t[2];
    return r;
  }
  void to_result(const P& a, msm_result* out) const {
    if (C.is_zero(a)) {
      memset(out->x, 0, 48);
      memset(out->y, 0, 48);
      out->is_infinity = 1;
      return;
    }
    affine_to_result(C.F, a.X, a.Y, a.Z, out);
  }
};

struct TeKind {   // extended points of the twisted Edwards curve, unified additions (src/msm-basic.ts:142-158)
  using P = msm_host::Ext6;
  const msm_host::TeCurve6& C;
  static constexpr int SLOT_WORDS = TE_SUM_WORDS;
  P zero() const { return C.zero(); }
  P dbl(const P& a) const { return C.add(a, a); }
  P add(const P& a, const P& b) const { return C.add(a, b); }
  P from_slot(const uint32_t* w) const {
    P r;
    coords_from_slot(C.F, w, 8, {&r.X, &r.Y, &r.Z, &r.T});
    return r;
  }
  void to_slot(const P& a, uint32_t* out) const { coords_to_slot(out, 8, {&a.X, &a.Y, &a.Z, &a.T}); }
  // (X : Y : Z) in, T rebuilt as (X Z : Y Z : Z^2 : X Y)
  P from_wire(const msm_host::Fe6 (&t)[3]) const {
    P r;
    C.F.mul(r.X, t[0], t[2]);
    C.F.mul(r.Y, t[1], t[2]);
    C.F.mul(r.Z, t[2], t[2]);
    C.F.mul(r.T, t[0], t[1]);
    return r;
  }
  // the identity is the affine point (0, 1): is_infinity stays 0
  void to_result(const P& a, msm_result* out) const { affine_to_result(C.F, a.X, a.Y, a.Z, out); }
};

template <class Fn>
static void with_kind(const msm_ctx* ctx, Fn&& fn) {
  if (ctx->is_te()) fn(TeKind{ctx->hte});
  else fn(WKind{ctx->hc});
}

// S = sum_k 2^(ck) P_k (src/msm-batched-affine.ts:322-333)
template <class KD>
static typename KD::P horner_points(const KD& kd, const std::vector<typename KD::P>& P, int c) {
  const int K = (int)P.size();
  typename KD::P acc = P[K - 1];
  for (int k = K - 2; k >= 0; k--) {
    for (int j = 0; j < c; j++) acc = kd.dbl(acc);
    acc = kd.add(acc, P[k]);
  }
  return acc;
}
template <class KD>
static typename KD::P slots_horner(const KD& kd, const uint32_t* words, int K, int c) {
  std::vector<typename KD::P> P(K);
  for (int k = 0; k < K; k++) P[k] = kd.from_slot(words + (size_t)k * KD::SLOT_WORDS);
  return horner_points(kd, P, c);
}

// one launch per stage of the reduction: the Edwards kernel, or the curve's instance of the Weierstrass one
#define REDUCE_LAUNCH(X, ...)                                     \
  do {                                                            \
    if (te) hipLaunchKernelGGL(te::k_te_##X, __VA_ARGS__);        \
    else W_LAUNCH(ctx, k_##X, __VA_ARGS__);                       \
  } while (0)

// Bucket reduction of kc windows of L buckets each (L a power of two): P_k = sum_l l * B_(k,l) (reduceBucketsColumnProjective +
// the partition sums, src/msm-batched-affine.ts:556-583, :312-319) -> h_partials_out, kc slots.  bucket_proj: the bucket sums
// of finish_buckets, one raw projective (Edwards: extended) point per bucket.  Runs on w.stream, records w.ev[4] behind its last
// kernel and returns when the sums are on the host.
// stride: bits a window advances by (Plan::c); 0 = log2(L) + 1, the plain plan's c.
// tc_force: buckets per lane in place of the rule below, a power of two in 2 .. 32 -- the values the rule can give; 0: the rule
// (the operator test msm_test_bucket_sums reaches every one of them at small sizes with it; the pipeline never passes it).
void reduce_buckets(msm_ctx* ctx, msm_ctx::Workspace& w, const uint32_t* bucket_proj, uint32_t L, int kc, uint32_t* h_partials_out,
                    bool merged, int stride, uint32_t tc_force) {
  if (L == 0 || (L & (L - 1))) throw MsmFail{MSM_ERR_INTERNAL, "reduce_buckets: L must be a power of two"};
  hipStream_t s = w.stream;
  const bool te = ctx->is_te();
  const uint64_t nb = (uint64_t)kc * L;
  const int part_words = ctx->sum_words();
  // buckets per lane: enough lanes to fill the chip, but never more than 16 buckets deep (2 additions each)
  // (millions of buckets -- the big windows -- go 32 deep: 2^26 at c = 22, with the two policies below, 150.6 -> 149.3 ms)
  uint32_t TC = 2;
  const uint32_t tc_cap = nb >= (1ull << 22) ? 32 : 16;
  while (TC < tc_cap && nb / TC > 65536) TC *= 2;
  MSM_KNOB(TC, "MSM_TC", 1);
  while (TC & (TC - 1)) TC &= TC - 1;   // the knob (tuning builds only) is rounded down to a power of two; the rule gives no other value
  if (tc_force) TC = tc_force;
  TC = std::min<uint32_t>(TC, L);
  // L and TC are powers of two, so a window is cut into exactly 2^nbits chunks: what the two-dimensional bit tree needs
  const uint32_t nchunks = L / TC, nbits = ceil_log2_u64(nchunks);
  // bit-sliced weighting (enough chunks to matter)
  // (the host finishes every window with ~2 c additions and doublings: on the Edwards path, whose plain plans have 13 - 28
  // windows, that tail costs more than the weighting chains it replaces -- 0.28 against 0.05 ms at 2^20 -- so it takes the
  // bit-sliced form only for the one or two merged windows of a run on window tables)
  const bool bit_sliced = nchunks >= 64 && (!te || kc <= 2);
  const size_t raw_words = te ? (size_t)4 * te::TL : (size_t)3 * NL;   // raw limb words of one point between the reduction kernels
  const uint32_t threads = nchunks * (uint32_t)kc;
  ctx->ensure(w.columns, (size_t)kc * nchunks * 4 * NL * 4);
  ctx->ensure(w.partials, (size_t)kc * (bit_sliced ? nbits + 1 : 1) * W_SUM_WORDS * 4);
  if (bit_sliced) ctx->ensure(w.rows_sum, (size_t)kc * nchunks * raw_words * 4);
  REDUCE_LAUNCH(bucket_reduce, dim3((threads + 63) / 64), dim3(64), 0, s, (uint32_t*)w.columns.p,
                bit_sliced ? (uint32_t*)w.rows_sum.p : (uint32_t*)nullptr, bucket_proj, L, TC, nchunks, (uint32_t)kc);
  if (!bit_sliced) {
    // (fewer than 64 chunks per window, or many Edwards windows: one block per window sums its columns)
    REDUCE_LAUNCH(window_sum, dim3(kc), dim3(WS_THREADS), 0, s, (uint32_t*)w.partials.p, (const uint32_t*)w.columns.p, nchunks);
    HIPCHK(hipMemcpyAsync(w.h_part, w.partials.p, (size_t)kc * part_words * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(w.ev[4], s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    memcpy(h_partials_out, w.h_part, (size_t)kc * part_words * 4);
    return;
  }
  // The two-dimensional bit tree (msm_kernels.h, bit_tree_body): row sums A_hi and column sums B_lo of the chunk matrix first --
  // 2 additions per chunk instead of nbits / 2 -- then the nbits masked sums over those 2^(nbits / 2) + ... points.  Measured
  // (profiles/r06_experiments.txt): 2^20 on tables 0.42 -> 0.2x ms for the two launches, 2^26 0.5 -> 0.3x per window group.
  // First stage: the local triangles go to nblk blocks of one wave per 512 elements (8 per lane; at 2^20 that is about one wave
  // per SIMD); second stage: one wave per (window, bit) over the sums it finds.
  const uint32_t nblk = std::max<uint32_t>(2, nchunks / (8 * BT_THREADS));
  const uint32_t per_kk = (1u << (nbits / 2)) + (1u << (nbits - nbits / 2)) + nblk;
  ctx->ensure(w.columns2, (size_t)kc * per_kk * raw_words * 4);
  REDUCE_LAUNCH(bit_tree, dim3(per_kk, 1, kc), dim3(BT_THREADS), 0, s, (uint32_t*)w.columns2.p, (const uint32_t*)w.rows_sum.p,
                (const uint32_t*)w.columns.p, nchunks, nbits, 0, nblk);
  REDUCE_LAUNCH(bit_tree, dim3(1, nbits + 1, kc), dim3(BT_THREADS), 0, s, (uint32_t*)w.partials.p, (const uint32_t*)w.columns2.p,
                (const uint32_t*)nullptr, nchunks, nbits, 1, nblk);
  // read the (nbits + 1) sums per window back and finish P_k = tri + TC * sum_b 2^b S_b on the host
  HIPCHK(hipMemcpyAsync(w.h_part, w.partials.p, (size_t)kc * (nbits + 1) * part_words * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(w.ev[4], s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  const uint32_t lt = ceil_log2_u64(TC), cbits = ceil_log2_u64(L) + 1;
  const int adv = stride ? stride : (int)cbits;
  with_kind(ctx, [&](const auto& kd) {
    if (merged) {
      // The caller only wants S_g = sum_kk 2^(c kk) P_kk of the whole group (a full MSM on this device: the Horner step over
      // the windows follows anyway).  One double-and-add pass over the c kc bit positions then does both jobs -- inside window
      // kk the sum S_b sits at bit log2(TC) + b, the triangle sum at bit 0 -- with c kc doublings instead of (c - 1) kc for
      // the windows plus c (kc - 1) for their combination.  S_g goes into the slot of the group's first window, the identity
      // into the others: sum_k 2^(c k) (slot k) is the same group element as with one P_k per slot.
      // With a folded top window (Plan::fold) a window has one bit position more than it advances by: position `stride` of
      // window kk coincides with position 0 of window kk + 1, so the pass walks GLOBAL bit positions and adds what every
      // window has there.
      auto acc = kd.zero();
      for (int gpos = (kc - 1) * adv + (int)cbits - 1; gpos >= 0; gpos--) {
        acc = kd.dbl(acc);
        for (int kk = kc - 1; kk >= 0; kk--) {
          const int pos = gpos - kk * adv;
          if (pos < 0 || pos >= (int)cbits) continue;
          const uint32_t* base = w.h_part + (size_t)kk * (nbits + 1) * part_words;
          const int b = pos - (int)lt;
          if (b >= 0 && b < (int)nbits) acc = kd.add(acc, kd.from_slot(base + (size_t)b * part_words));
          if (pos == 0) acc = kd.add(acc, kd.from_slot(base + (size_t)nbits * part_words));
        }
      }
      for (int kk = 1; kk < kc; kk++) sum_set_identity(ctx, h_partials_out + (size_t)kk * part_words);
      kd.to_slot(acc, h_partials_out);
      return;
    }
    for (int kk = 0; kk < kc; kk++) {
      const uint32_t* base = w.h_part + (size_t)kk * (nbits + 1) * part_words;
      auto acc = kd.zero();
      for (int b = (int)nbits - 1; b >= 0; b--) {
        acc = kd.dbl(acc);
        acc = kd.add(acc, kd.from_slot(base + (size_t)b * part_words));
      }
      for (uint32_t t = TC; t > 1; t >>= 1) acc = kd.dbl(acc);
      acc = kd.add(acc, kd.from_slot(base + (size_t)nbits * part_words));
      kd.to_slot(acc, h_partials_out + (size_t)kk * part_words);
    }
  });
}
#undef REDUCE_LAUNCH

void device_coord_to_wire(const msm_host::Field6& F, const msm_host::Fe6& k_to_host, const uint32_t* w, int nw, uint8_t* out) {
  const msm_host::Fe6 one = {{1, 0, 0, 0, 0, 0}};
  msm_host::Fe6 t;
  words_to_fe6(t, w, nw);
  F.mul(t, t, k_to_host);   // host Montgomery
  F.mul(t, t, one);         // plain
  uint8_t b48[48];
  fe6_to_bytes(b48, t);
  memcpy(out, b48, (size_t)nw * 4);
}

void plane_element_to_wire(const msm_ctx* ctx, const uint32_t* planes, uint64_t cap, uint64_t e, uint8_t* out_xy) {
  const int nw = ctx->nw(), np = nw / 4;
  const size_t cb = ctx->coord_bytes();
  uint32_t w[24];
  for (int cpl = 0; cpl < 2 * np; cpl++)
    for (int q = 0; q < 4; q++) w[4 * cpl + q] = planes[((uint64_t)cpl * cap + e) * 4 + q];
  memset(out_xy, 0, 2 * cb);
  if (w[nw - 1] == INF_WORD) return;
  for (int j = 0; j < 2; j++) device_coord_to_wire(ctx->hc.F, ctx->k_dev_to_host, w + nw * j, nw, out_xy + cb * j);
}

// ---- the host tail over slots ------------------------------------------------------------------------------------------

// the Weierstrass identity is the all-zero slot (Z = 0), the Edwards identity the extended point (0, 1, 1, 0)
void sum_set_identity(const msm_ctx* ctx, uint32_t* slot) {
  if (ctx->is_te()) TeKind{ctx->hte}.to_slot(ctx->hte.zero(), slot);
  else memset(slot, 0, W_SUM_WORDS * 4);
}

void sum_slots(const msm_ctx* ctx, const std::vector<const uint32_t*>& parts, uint32_t* out) {
  with_kind(ctx, [&](const auto& kd) {
    auto acc = kd.zero();
    for (const uint32_t* p : parts) acc = kd.add(acc, kd.from_slot(p));
    kd.to_slot(acc, out);
  });
}

void sums_horner(const msm_ctx* ctx, const uint32_t* words, int K, int c, uint32_t* out_slot) {
  with_kind(ctx, [&](const auto& kd) { kd.to_slot(slots_horner(kd, words, K, c), out_slot); });
}

void sums_finish(const msm_ctx* ctx, const uint32_t* words, int K, int c, msm_result* out) {
  with_kind(ctx, [&](const auto& kd) { kd.to_result(slots_horner(kd, words, K, c), out); });
}

void identity_to_result(const msm_ctx* ctx, msm_result* out) {
  memset(out->x, 0, 48);
  memset(out->y, 0, 48);
  out->y[0] = ctx->is_te();
  out->is_infinity = !ctx->is_te();
}

void sum_to_wire(const msm_ctx* ctx, const uint32_t* slot, uint8_t* out) {
  const msm_host::Fe6 one = {{1, 0, 0, 0, 0, 0}};
  msm_host::Fe6 X, Y, Z;
  const msm_host::Field6* F;
  if (ctx->is_te()) {
    // extended point (X : Y : Z : T) sent as X || Y || Z; the receiver rebuilds T (msm_combine: T Z = X Y)
    const msm_host::Ext6 P = slot ? TeKind{ctx->hte}.from_slot(slot) : ctx->hte.zero();
    X = P.X; Y = P.Y; Z = P.Z;
    F = &ctx->hte.F;
  } else {
    bool zero_z = true;
    for (int j = 0; slot && j < 12; j++) zero_z &= slot[24 + j] == 0;
    const msm_host::Proj6 P = zero_z ? ctx->hc.zero() : WKind{ctx->hc}.from_slot(slot);
    X = P.X; Y = P.Y; Z = P.Z;
    F = &ctx->hc.F;
  }
  // to 48-byte canonical integers (leave Montgomery form on the host)
  const msm_host::Fe6* co[3] = {&X, &Y, &Z};
  for (int j = 0; j < 3; j++) {
    msm_host::Fe6 t;
    F->mul(t, *co[j], one);
    fe6_to_bytes(out + 48 * j, t);
  }
}

// host curve constants without a context (rank 0 of a sharded run may combine without touching a GPU)
const msm_host::Curve6* static_host_curve(int curve) {
  constexpr int N_IDS = MSM_CURVE_VESTA + 1;
  static msm_host::Curve6 hc[N_IDS];
  static std::atomic<int> ready[N_IDS];
  if (curve < 0 || curve >= N_IDS || curve == MSM_CURVE_ED_ON_BLS12_377) return nullptr;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (!ready[curve].load()) {
    hc[curve].F.init(curve_info(curve).pw);
    ready[curve].store(1);
  }
  return &hc[curve];
}

// msm_combine: G groups of K wire sums (X || Y || Z, 48-byte canonical integers) -> sum over the groups, then the Horner
// combination.  MSM_ERR_ARG: a coordinate is not below p.
template <class KD>
static int combine_kind(const KD& kd, const uint8_t* partials, int32_t K, int32_t c, msm_result* out, int32_t G) {
  const msm_host::Field6& F = kd.C.F;
  std::vector<typename KD::P> P(K);
  for (int k = 0; k < K; k++) {
    P[k] = kd.zero();
    for (int g = 0; g < G; g++) {   // group g's sum of window k
      msm_host::Fe6 t[3];
      for (int j = 0; j < 3; j++) {
        const uint8_t* b = partials + ((size_t)g * K + k) * SUM_WIRE_BYTES + 48 * j;
        for (int i = 0; i < 6; i++) {
          uint64_t v = 0;
          for (int q = 0; q < 8; q++) v |= (uint64_t)b[8 * i + q] << (8 * q);
          t[j].v[i] = v;
        }
        if (msm_host::Field6::ge(t[j], F.p)) return MSM_ERR_ARG;
        F.mul(t[j], t[j], F.r2);  // to host Montgomery form
      }
      const typename KD::P Q = kd.from_wire(t);
      P[k] = G == 1 ? Q : kd.add(P[k], Q);
    }
  }
  memset(out, 0, sizeof(*out));
  kd.to_result(horner_points(kd, P, c), out);
  out->c = c;
  out->K = K;
  return MSM_OK;
}

// twisted Edwards: the curve's constants without a context
int te_combine_impl(const uint8_t* partials, int32_t K, int32_t c, msm_result* out, int32_t G) {
  static msm_host::TeCurve6 C;
  static std::once_flag once;
  std::call_once(once, [] {
    uint32_t pw[12] = {0};
    for (int i = 0; i < 8; i++) pw[i] = Fp253::PW[i];
    C.init(pw, 3021);
  });
  return combine_kind(TeKind{C}, partials, K, c, out, G);
}

int combine_impl(msm_ctx* ctx, const msm_host::Curve6& C, const uint8_t* partials, int32_t K, int32_t c, msm_result* out, int32_t G) {
  const int rc = combine_kind(WKind{C}, partials, K, c, out, G);
  return rc == MSM_OK ? rc : fail(ctx, rc, "msm_combine: coordinate >= p");
}

}  // namespace msmi
