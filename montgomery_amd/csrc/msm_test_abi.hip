// Operator-level test entries of the C ABI (msm_test_*: the fine-grained operator table of src/field-msm.ts:86-123 as a GPU
// debug surface) and the synthetic input generators.
#include "msm_internal.h"

using namespace msm;
using namespace msmi;

extern "C" {

int msm_test_fp(msm_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, uint64_t n) {
  if (!ctx || !a || !b || !out) return fail(ctx, MSM_ERR_ARG, "msm_test_fp: null argument");
  const size_t nb = ctx->coord_bytes();
  try {
    HIPCHK(hipSetDevice(ctx->device));
    ctx->ensure(ctx->misc, n * nb * 3 + 64);
    uint8_t* d = (uint8_t*)ctx->misc.p;
    HIPCHK(hipMemcpyAsync(d, a, n * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d + n * nb, b, n * nb, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->is_te())
      hipLaunchKernelGGL(te::k_te_test_fp, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t*)(d + 2 * n * nb),
                         (const uint32_t*)d, (const uint32_t*)(d + n * nb), (uint32_t)n, op);
    else
      W_LAUNCH(ctx, k_test_fp, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t*)(d + 2 * n * nb),
                         (const uint32_t*)d, (const uint32_t*)(d + n * nb), (uint32_t)n, op);
    HIPCHK(hipMemcpyAsync(out, d + 2 * n * nb, n * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_test_batch_inverse(msm_ctx* ctx, const uint8_t* xs, uint8_t* out, uint64_t n, uint32_t per_lane) {
  if (!ctx || !xs || !out || per_lane == 0) return fail(ctx, MSM_ERR_ARG, "msm_test_batch_inverse: bad argument");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nb = ctx->coord_bytes();
    ctx->ensure(ctx->misc, n * 2 * nb + 64);
    uint8_t* d = (uint8_t*)ctx->misc.p;
    HIPCHK(hipMemcpyAsync(d, xs, n * nb, hipMemcpyHostToDevice, ctx->stream));
    uint64_t lanes = (n + per_lane - 1) / per_lane;
    if (ctx->is_te())
      hipLaunchKernelGGL((k_test_batch_inverse<te::CvEdField>), dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, ctx->stream,
                         (uint32_t*)(d + n * nb), (const uint32_t*)d, (uint32_t)n, per_lane);
    else
      W_LAUNCH(ctx, k_test_batch_inverse, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, ctx->stream,
                         (uint32_t*)(d + n * nb), (const uint32_t*)d, (uint32_t)n, per_lane);
    HIPCHK(hipMemcpyAsync(out, d + n * nb, n * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_test_glv(msm_ctx* ctx, const uint8_t* scalars, uint8_t* out, uint64_t n) {
  if (!ctx || !scalars || !out) return fail(ctx, MSM_ERR_ARG, "msm_test_glv: null argument");
  if (ctx->is_te()) return fail(ctx, MSM_ERR_ARG, "msm_test_glv: the twisted Edwards path has no GLV step");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    ctx->ensure(ctx->misc, n * 72 + 64);
    uint8_t* d = (uint8_t*)ctx->misc.p;
    HIPCHK(hipMemcpyAsync(d, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    W_LAUNCH(ctx, k_test_glv, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t*)(d + n * 32),
                       (const uint32_t*)d, (uint32_t)n);
    HIPCHK(hipMemcpyAsync(out, d + n * 32, n * 40, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

int msm_test_batch_add(msm_ctx* ctx, const uint8_t* g, const uint8_t* h, uint8_t* out, uint64_t n) {
  if (!ctx || !g || !h || !out || n == 0) return fail(ctx, MSM_ERR_ARG, "msm_test_batch_add: bad argument");
  if (ctx->is_te()) {
    // unified extended addition of the gather round (te_add_rows, src/curve-twisted-edwards.ts:84-165): n pairs of
    // 64-byte affine points in, n affine sums out
    try {
      HIPCHK(hipSetDevice(ctx->device));
      DevBuf rows, wire, slots, outb;
      ctx->ensure(wire, 2 * n * 64);
      ctx->ensure(rows, 2 * n * te::TE_ROW_WORDS * 4);
      ctx->ensure(slots, 2 * n * 4);
      ctx->ensure(outb, n * 128);
      std::vector<uint8_t> inter(2 * n * 64);
      std::vector<uint32_t> sl(2 * n);
      for (uint64_t i = 0; i < n; i++) {
        memcpy(&inter[(2 * i) * 64], g + i * 64, 64);
        memcpy(&inter[(2 * i + 1) * 64], h + i * 64, 64);
        sl[2 * i] = (uint32_t)((2 * i) << 1);
        sl[2 * i + 1] = (uint32_t)((2 * i + 1) << 1);
      }
      HIPCHK(hipMemcpyAsync(wire.p, inter.data(), inter.size(), hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(slots.p, sl.data(), sl.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, ctx->stream));
      hipLaunchKernelGGL(te::k_te_points_from_wire, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, ctx->stream,
                         (uint32_t*)rows.p, (const uint32_t*)wire.p, 2 * n, 0, (uint32_t*)ctx->errflag.p);
      BatchArgs a{};
      a.points = (const uint32_t*)rows.p;
      a.slots = (const uint32_t*)slots.p;
      a.out = (uint4*)outb.p;
      a.out_cap = n;
      a.n_out = n;
      a.steps = 1;
      hipLaunchKernelGGL(te::k_te_add<MODE_GATHER>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, a);
      std::vector<uint32_t> planes(n * 32);
      HIPCHK(hipMemcpyAsync(planes.data(), outb.p, n * 128, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      HIPCHK(hipGetLastError());
      const auto& C = ctx->hte;
      msm_host::Fe6 one = {{1, 0, 0, 0, 0, 0}};
      for (uint64_t e = 0; e < n; e++) {
        msm_host::Fe6 co[3];   // X, Y, Z
        for (int j = 0; j < 3; j++) {
          msm_host::Fe6 t = {{0, 0, 0, 0, 0, 0}};
          for (int pl = 0; pl < 2; pl++)
            for (int q = 0; q < 2; q++) {
              const uint32_t* w = &planes[((uint64_t)(2 * j + pl) * n + e) * 4 + 2 * q];
              t.v[2 * pl + q] = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
            }
          if (msm_host::Field6::ge(t, C.F.p)) C.F.sub_raw(t, t, C.F.p);
          C.F.mul(co[j], t, ctx->k_te_to_host);
        }
        msm_host::Fe6 zi, x, y;
        C.F.inv(zi, co[2]);
        C.F.mul(x, co[0], zi);
        C.F.mul(y, co[1], zi);
        C.F.mul(x, x, one);
        C.F.mul(y, y, one);
        uint8_t xb[48], yb[48];
        fe6_to_bytes(xb, x);
        fe6_to_bytes(yb, y);
        memcpy(out + e * 64, xb, 32);
        memcpy(out + e * 64 + 32, yb, 32);
      }
    } MSM_CATCH_ALL(ctx)
    return MSM_OK;
  }
  try {
    HIPCHK(hipSetDevice(ctx->device));
    // rows for 2n points: pair e = (row 2e, row 2e + 1), gathered through identity payload slots
    DevBuf rows, wire, slots, outb, scr;
    const size_t pb = 2 * ctx->coord_bytes();   // wire point; a tree node has the same size
    ctx->ensure(wire, 2 * n * pb);
    ctx->ensure(rows, 2 * n * ROW_WORDS * 4);
    ctx->ensure(slots, 2 * n * 4);
    ctx->ensure(outb, n * pb);
    std::vector<uint8_t> inter(2 * n * pb);
    std::vector<uint32_t> sl(2 * n);
    for (uint64_t i = 0; i < n; i++) {
      memcpy(&inter[(2 * i) * pb], g + i * pb, pb);
      memcpy(&inter[(2 * i + 1) * pb], h + i * pb, pb);
      sl[2 * i] = (uint32_t)((2 * i) << 2);
      sl[2 * i + 1] = (uint32_t)((2 * i + 1) << 2);
    }
    HIPCHK(hipMemcpyAsync(wire.p, inter.data(), 2 * n * pb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(slots.p, sl.data(), 2 * n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, ctx->stream));
    W_LAUNCH(ctx, k_points_from_wire, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t*)rows.p,
                       (const uint32_t*)wire.p, 2 * n, 0, (uint32_t*)ctx->errflag.p);
    RoundGeom gm = round_geom(ctx, n);
    gm.steps = (uint32_t)std::min<uint64_t>(n, 3);  // exercise the shared inversion with a few pairs per lane
    uint64_t threads = (n + gm.steps - 1) / gm.steps;
    gm.grid = (uint32_t)((threads + 255) / 256);
    gm.T = (uint64_t)gm.grid * 256;
    ctx->ensure(scr, (size_t)gm.steps * NL * gm.T * 4);
    BatchArgs a{};
    a.points = (const uint32_t*)rows.p;
    a.slots = (const uint32_t*)slots.p;
    a.y_off = 4 * ctx->nw();
    a.out = (uint4*)outb.p;
    a.out_cap = n;
    a.scratch = (uint32_t*)scr.p;
    a.sstride = gm.T;
    a.n_out = n;
    a.steps = gm.steps;
    W_LAUNCH_MODE(ctx, k_batch_add, MODE_GATHER, dim3(gm.grid), dim3(256), 0, ctx->stream, a);
    std::vector<uint32_t> planes(n * pb / 4);
    HIPCHK(hipMemcpyAsync(planes.data(), outb.p, n * pb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    for (uint64_t e = 0; e < n; e++) plane_element_to_wire(ctx, planes.data(), n, e, out + e * pb);
  } MSM_CATCH_ALL(ctx)
  return MSM_OK;
}

static int generate_points_one(msm_ctx* ctx, uint64_t n, uint64_t seed, uint8_t* a_out) {
  try {
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->is_te()) return msm_gen::generate_points_te(ctx, n, seed, a_out);
    return msm_gen::generate_points(ctx, n, seed, a_out);
  } MSM_CATCH_ALL(ctx)
}

int msm_test_fp_raw(msm_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n) {
  if (!ctx || !a || !b || !out) return fail(ctx, MSM_ERR_ARG, "msm_test_fp_raw: null argument");
  if (op != MSM_OP_MUL && op != MSM_OP_SQR) return fail(ctx, MSM_ERR_ARG, "msm_test_fp_raw: op must be MSM_OP_MUL or MSM_OP_SQR");
  const size_t nb = (size_t)ctx->nl() * 4;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    ctx->ensure(ctx->misc, n * nb * 3 + 64);
    uint8_t* d = (uint8_t*)ctx->misc.p;
    HIPCHK(hipMemcpyAsync(d, a, n * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d + n * nb, b, n * nb, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((uint32_t)((n + 255) / 256));
    if (ctx->is_te())
      hipLaunchKernelGGL(te::k_te_test_fp_raw, grid, dim3(256), 0, ctx->stream, (uint32_t*)(d + 2 * n * nb), (const uint32_t*)d,
                         (const uint32_t*)(d + n * nb), (uint32_t)n, op);
    else
      W_LAUNCH(ctx, k_test_fp_raw, grid, dim3(256), 0, ctx->stream, (uint32_t*)(d + 2 * n * nb), (const uint32_t*)d,
                         (const uint32_t*)(d + n * nb), (uint32_t)n, op);
    HIPCHK(hipMemcpyAsync(out, d + 2 * n * nb, n * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_curve_op(msm_ctx* ctx, int op, const uint8_t* p, const uint8_t* q, uint8_t* out, uint64_t n) {
  if (!ctx || !p || !q || !out) return fail(ctx, MSM_ERR_ARG, "msm_test_curve_op: null argument");
  if (op < 0 || op > 2) return fail(ctx, MSM_ERR_ARG, "msm_test_curve_op: unknown operator");
  const size_t nb = ctx->is_te() ? 128 : 3 * ctx->coord_bytes();   // extended (X, Y, Z, T) or projective (X, Y, Z)
  try {
    HIPCHK(hipSetDevice(ctx->device));
    ctx->ensure(ctx->misc, n * nb * 3 + 64);
    uint8_t* d = (uint8_t*)ctx->misc.p;
    HIPCHK(hipMemcpyAsync(d, p, n * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d + n * nb, q, n * nb, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((uint32_t)((n + 63) / 64));
    if (ctx->is_te())
      hipLaunchKernelGGL(te::k_te_test_curve_op, grid, dim3(64), 0, ctx->stream, (uint32_t*)(d + 2 * n * nb), (const uint32_t*)d,
                         (const uint32_t*)(d + n * nb), (uint32_t)n, op);
    else
      W_LAUNCH(ctx, k_test_curve_op, grid, dim3(64), 0, ctx->stream, (uint32_t*)(d + 2 * n * nb), (const uint32_t*)d,
                         (const uint32_t*)(d + n * nb), (uint32_t)n, op);
    HIPCHK(hipMemcpyAsync(out, d + 2 * n * nb, n * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_bucket_reduce(msm_ctx* ctx, const uint8_t* buckets, int32_t K, uint32_t L, int mode, int c0, uint8_t* partials_out,
                           float* ms_out) {
  if (!ctx || !buckets || !partials_out || K <= 0 || L == 0 || (L & (L - 1)) || (mode != 0 && mode != 1))
    return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_reduce: bad argument");
  if (ctx->is_te()) return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_reduce: Weierstrass curves only");
  int cl = 0;
  while ((1u << cl) < L) cl++;
  if (c0 < 0 || c0 > cl) return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_reduce: c0 must be in [0, log2 L]");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    msm_ctx::Workspace& w = ctx->ws[0];
    hipStream_t s = w.stream;
    const uint64_t nb = (uint64_t)K * L;
    const uint64_t cap = nb + 2 * 257 * 512 + 256;   // plane capacity: idle lanes read (and ignore) past the end
    DevBuf wire, rows, planes, desc, scr;
    const size_t pb = 2 * ctx->coord_bytes();
    const int nw = ctx->nw(), np = nw / 4;
    ctx->ensure(wire, nb * pb);
    ctx->ensure(rows, nb * ROW_WORDS * 4);
    ctx->ensure(planes, cap * pb);
    HIPCHK(hipMemcpyAsync(wire.p, buckets, nb * pb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, s));
    HIPCHK(hipMemsetAsync(planes.p, 0, cap * pb, s));
    W_LAUNCH(ctx, k_points_from_wire, dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, s, (uint32_t*)rows.p, (const uint32_t*)wire.p,
             nb, 0, (uint32_t*)ctx->errflag.p);
    ROWS_TO_PLANES(ctx, dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, s, (uint4*)planes.p, cap, (const uint32_t*)rows.p,
                   (uint32_t)nb);
    std::vector<uint32_t> parts((size_t)K * W_SUM_WORDS, 0);
    float ms = 0;
    if (mode == 0) {
      // every bucket holds exactly one element of the tree buffer: offsets 0, 1, 2, ...
      std::vector<uint32_t> off(nb + 1);
      for (uint64_t b = 0; b <= nb; b++) off[b] = (uint32_t)b;
      ctx->ensure(desc, (nb + 1) * 4);
      HIPCHK(hipMemcpyAsync(desc.p, off.data(), (nb + 1) * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipEventRecord(w.ev[3], s));   // in front of the finish: *ms_out spans affine buckets to window sums
      reduce_buckets(ctx, w, finish_buckets(ctx, w, (const uint4*)planes.p, cap, (const uint32_t*)desc.p, nb), L, K, parts.data());
      HIPCHK(hipEventElapsedTime(&ms, w.ev[3], w.ev[4]));
    } else {
      // The rounds of reduceBucketsAffine as (first operand, second operand) element lists; the sum replaces the first.
      // e(k, l) = k L + l - 1 for the 1-based bucket index l of the reference.
      const uint32_t L0 = 1u << c0, D = L / L0;
      std::vector<std::vector<uint32_t>> ga, gb;
      auto e = [&](int k, uint64_t l) { return (uint32_t)((uint64_t)k * L + l - 1); };
      auto round = [&](const std::function<void(int, std::vector<uint32_t>&, std::vector<uint32_t>&)>& fill) {
        std::vector<uint32_t> A, B;
        for (int k = 0; k < K; k++) fill(k, A, B);
        if (!A.empty()) { ga.push_back(std::move(A)); gb.push_back(std::move(B)); }
      };
      // linear part: suffix sums inside every chunk of L0 buckets (:563-588)
      for (uint32_t l = L0 - 1; l >= 1; l--)
        round([&](int k, std::vector<uint32_t>& A, std::vector<uint32_t>& B) {
          for (uint32_t d = 0; d < D; d++) { A.push_back(e(k, (uint64_t)d * L0 + l)); B.push_back(e(k, (uint64_t)d * L0 + l + 1)); }
        });
      // logarithmic part: chunk heads collect the chunks to their right, power-of-two spans (:590-615)
      for (uint64_t L1 = L0, D1 = D >> 1; D1 > 0; L1 <<= 1, D1 >>= 1)
        round([&](int k, std::vector<uint32_t>& A, std::vector<uint32_t>& B) {
          for (uint64_t d = 0; d < D1; d++) { A.push_back(e(k, d * 2 * L1 + 1)); B.push_back(e(k, (d * 2 + 1) * L1 + 1)); }
        });
      // doublings: every head is weighted with the number of buckets it stands for (:616-641)
      if (D > 1)
        for (int j = 0; j < c0; j++)
          round([&](int k, std::vector<uint32_t>& A, std::vector<uint32_t>& B) {
            for (uint32_t d = 1; d < D; d++) { A.push_back(e(k, (uint64_t)d * L0 + 1)); B.push_back(e(k, (uint64_t)d * L0 + 1)); }
          });
      for (uint64_t L1 = 2ull * L0, D1 = D >> 1; D1 > 1; L1 <<= 1, D1 >>= 1)
        round([&](int k, std::vector<uint32_t>& A, std::vector<uint32_t>& B) {
          for (uint64_t d = 1; d < D1; d++) { A.push_back(e(k, d * L1 + 1)); B.push_back(e(k, d * L1 + 1)); }
        });
      // the buckets now fill the triangle: one addition tree over all of them (:643-662)
      for (uint64_t m = 1; m < L; m *= 2)
        round([&](int k, std::vector<uint32_t>& A, std::vector<uint32_t>& B) {
          for (uint64_t l = 1; l < L; l += 2 * m) { A.push_back(e(k, l)); B.push_back(e(k, l + m)); }
        });
      size_t total = 0, biggest = 0;
      for (auto& v : ga) { total += v.size(); biggest = std::max(biggest, v.size()); }
      ctx->ensure(desc, std::max<size_t>(total, 1) * 8);
      std::vector<uint32_t> flat(2 * total);
      {
        size_t o = 0;
        for (size_t r = 0; r < ga.size(); r++) {
          for (size_t i = 0; i < ga[r].size(); i++) { flat[o + i] = (ga[r][i] << 1) | 1u; flat[total + o + i] = gb[r][i]; }
          o += ga[r].size();
        }
      }
      HIPCHK(hipMemcpyAsync(desc.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, s));
      {
        const RoundGeom g = round_geom(ctx, std::max<uint64_t>(biggest, 1));
        ctx->ensure(scr, (size_t)g.steps * NL * g.T * 4);
      }
      HIPCHK(hipEventRecord(w.ev[3], s));
      size_t o = 0;
      for (size_t r = 0; r < ga.size(); r++) {
        const uint64_t np = ga[r].size();
        const RoundGeom g = round_geom(ctx, np);
        BatchArgs a{};
        a.in = (const uint4*)planes.p;
        a.in_cap = cap;
        a.out = (uint4*)planes.p;
        a.out_cap = cap;
        a.scratch = (uint32_t*)scr.p;
        a.sstride = g.T;
        a.n_out = np;
        a.steps = g.steps;
        a.desc = (const uint32_t*)desc.p + o;
        a.desc_b = (const uint32_t*)desc.p + total + o;
        a.inplace = 1;
        W_LAUNCH_MODE(ctx, k_batch_add, MODE_SEARCH, dim3(g.grid), dim3(256), 0, s, a);
        o += np;
      }
      HIPCHK(hipEventRecord(w.ev[4], s));
      // element e(k, 1) -> partial (X, Y, Z = 1 in device Montgomery form; all-zero = the identity)
      std::vector<uint32_t> el((size_t)K * 24);
      for (int k = 0; k < K; k++)
        for (int cpl = 0; cpl < 2 * np; cpl++)
          HIPCHK(hipMemcpyAsync(&el[(size_t)k * 24 + 4 * cpl], (const uint4*)planes.p + (uint64_t)cpl * cap + (uint64_t)k * L, 16,
                                hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventElapsedTime(&ms, w.ev[3], w.ev[4]));
      for (int k = 0; k < K; k++) {
        const uint32_t* q = &el[(size_t)k * 24];
        if (q[nw - 1] == INF_WORD) continue;   // identity: the partial stays all-zero
        uint32_t* part = &parts[(size_t)k * W_SUM_WORDS];
        memcpy(part, q, nw * 4);            // X, Y at words 0 and 12 of the partial (upper words zero)
        memcpy(part + 12, q + nw, nw * 4);
        const msm_host::Fe6 one_dev = ctx->hc.F.pow2(30 * ctx->nl());   // Z = 1 in the form x and y are in: device Montgomery
        for (int q2 = 0; q2 < 6; q2++) {
          part[24 + 2 * q2] = (uint32_t)one_dev.v[q2];
          part[24 + 2 * q2 + 1] = (uint32_t)(one_dev.v[q2] >> 32);
        }
      }
    }
    for (int k = 0; k < K; k++) sum_to_wire(ctx, &parts[(size_t)k * W_SUM_WORDS], partials_out + (size_t)k * SUM_WIRE_BYTES);
    if (ms_out) *ms_out = ms;
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_bucket_sums(msm_ctx* ctx, const uint8_t* pool, uint64_t n_pool, const uint32_t* off, const uint32_t* elems, int32_t K,
                         uint32_t L, int merged, int stride, uint32_t tc, uint8_t* sums_out, uint32_t* perm_out) {
  if (!ctx || !pool || !off || !sums_out || n_pool == 0 || K <= 0 || L == 0 || (L & (L - 1)) || stride < 0)
    return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_sums: bad argument");
  if (tc && (tc < 2 || tc > 32 || (tc & (tc - 1)))) return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_sums: tc must be 0 or a power of two in 2 .. 32");
  const uint64_t nb = (uint64_t)K * L;
  // the reduction hands the host up to log2(L) sums per window through the pinned buffer of a workspace (128 * 20 slots)
  if (nb >= (1ull << 31) || (uint64_t)K * (ceil_log2_u64(L) + 1) > 128 * 20)
    return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_sums: too many buckets or windows");
  const uint64_t n_el = off[nb];
  if (off[0] != 0 || (n_el && !elems) || n_el >= (1ull << 31)) return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_sums: bad offsets");
  for (uint64_t b = 0; b < nb; b++)
    if (off[b] > off[b + 1]) return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_sums: offsets must ascend");
  for (uint64_t e = 0; e < n_el; e++)
    if (elems[e] >= n_pool) return fail(ctx, MSM_ERR_ARG, "msm_test_bucket_sums: element %llu names no pool point", (unsigned long long)e);
  try {
    HIPCHK(hipSetDevice(ctx->device));
    msm_ctx::Workspace& w = ctx->ws[0];
    hipStream_t s = w.stream;
    const bool te = ctx->is_te();
    const uint64_t cap = n_el + 2 * 257 * 512 + 256;   // plane capacity: idle lanes read (and ignore) past the end
    const size_t pb = 2 * ctx->coord_bytes();          // wire point
    const size_t elem_bytes = te ? 128 : pb;           // tree node: extended (X, Y, Z, T), or affine (x, y)
    DevBuf wire, rows, planes, d_off, slots;
    ctx->ensure(planes, cap * elem_bytes);
    ctx->ensure(d_off, (nb + 1) * 4);
    HIPCHK(hipMemsetAsync(planes.p, 0, cap * elem_bytes, s));
    HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(d_off.p, off, (nb + 1) * 4, hipMemcpyHostToDevice, s));
    std::vector<uint8_t> h_wire;     // (both live until the stream has been waited for)
    std::vector<uint32_t> h_slots;
    if (n_el && te) {
      // the pool as point rows; element e = pool[elems[e]] + the absent operand, through one gather round of the tree
      ctx->ensure(wire, n_pool * pb);
      ctx->ensure(rows, n_pool * te::TE_ROW_WORDS * 4);
      ctx->ensure(slots, 2 * n_el * 4);
      h_slots.resize(2 * n_el);
      for (uint64_t e = 0; e < n_el; e++) { h_slots[2 * e] = elems[e] << 1; h_slots[2 * e + 1] = SLOT_EMPTY; }
      HIPCHK(hipMemcpyAsync(wire.p, pool, n_pool * pb, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(slots.p, h_slots.data(), h_slots.size() * 4, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(te::k_te_points_from_wire, dim3((uint32_t)((n_pool + 255) / 256)), dim3(256), 0, s, (uint32_t*)rows.p,
                         (const uint32_t*)wire.p, n_pool, 0, (uint32_t*)ctx->errflag.p);
      BatchArgs a{};
      a.points = (const uint32_t*)rows.p;
      a.slots = (const uint32_t*)slots.p;
      a.out = (uint4*)planes.p;
      a.out_cap = cap;
      a.n_out = n_el;
      a.steps = 1;
      hipLaunchKernelGGL(te::k_te_add<MODE_GATHER>, dim3((uint32_t)((n_el + 255) / 256)), dim3(256), 0, s, a);
    } else if (n_el) {
      // element e = wire point pool[elems[e]] -> row e -> element e of the planes
      h_wire.resize(n_el * pb);
      for (uint64_t e = 0; e < n_el; e++) memcpy(&h_wire[e * pb], pool + (size_t)elems[e] * pb, pb);
      ctx->ensure(wire, n_el * pb);
      ctx->ensure(rows, n_el * ROW_WORDS * 4);
      HIPCHK(hipMemcpyAsync(wire.p, h_wire.data(), n_el * pb, hipMemcpyHostToDevice, s));
      W_LAUNCH(ctx, k_points_from_wire, dim3((uint32_t)((n_el + 255) / 256)), dim3(256), 0, s, (uint32_t*)rows.p,
               (const uint32_t*)wire.p, n_el, 0, (uint32_t*)ctx->errflag.p);
      ROWS_TO_PLANES(ctx, dim3((uint32_t)((n_el + 255) / 256)), dim3(256), 0, s, (uint4*)planes.p, cap, (const uint32_t*)rows.p,
                     (uint32_t)n_el);
    }
    // the pipeline's own finish, over bucket sums that start out as garbage: a bucket the finish skips cannot come out right
    const uint32_t* perm = nullptr;
    ctx->ensure(w.bucket_proj, bucket_proj_bytes(ctx, nb));
    HIPCHK(hipMemsetAsync(w.bucket_proj.p, 0x2A, bucket_proj_bytes(ctx, nb), s));
    const uint32_t* bucket_proj = finish_buckets(ctx, w, (const uint4*)planes.p, cap, (const uint32_t*)d_off.p, nb, &perm);
    if (perm_out) {
      if (perm) HIPCHK(hipMemcpyAsync(perm_out, perm, nb * 4, hipMemcpyDeviceToHost, s));
      else for (uint64_t b = 0; b < nb; b++) perm_out[b] = (uint32_t)b;   // no ordering: the buckets are taken as they lie
    }
    const int sw = ctx->sum_words();
    std::vector<uint32_t> parts((size_t)K * sw, 0);
    reduce_buckets(ctx, w, bucket_proj, L, K, parts.data(), merged != 0, stride, tc);
    HIPCHK(hipMemcpyAsync(w.h_info, ctx->errflag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (w.h_info[0] & 1) return fail(ctx, MSM_ERR_POINT, "msm_test_bucket_sums: coordinate >= p");
    for (int k = 0; k < K; k++) sum_to_wire(ctx, &parts[(size_t)k * sw], sums_out + (size_t)k * SUM_WIRE_BYTES);
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_tree_sums(msm_ctx* ctx, const uint8_t* pool, uint64_t n_pool, const uint32_t* off, const uint32_t* elems,
                       const uint8_t* flags, int32_t K, uint32_t L, int32_t c, uint32_t logG, uint32_t reported_max, uint8_t* sums_out,
                       uint64_t* plan_out, uint32_t* cursor_out, uint32_t* tail_off_out, uint32_t tail_tables_cap,
                       uint64_t* round_log_out, uint32_t round_log_cap) {
  if (!ctx || !pool || !off || !sums_out || !plan_out || n_pool == 0 || K <= 0 || L == 0 || (L & (L - 1)) || (round_log_cap && !round_log_out))
    return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: bad argument");
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: not on a device-list context");
  if (c < 1 || c > 24) return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: c must be in 1 .. 24");
  if (logG < 1 || logG > 10) return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: logG must be in 1 .. 10");
  const uint64_t nb = (uint64_t)K * L;
  if (nb >= (1ull << 31) || (uint64_t)K * (ceil_log2_u64(L) + 1) > 128 * 20)
    return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: too many buckets or windows");
  const uint64_t n_el = off[nb];
  if (off[0] != 0 || (n_el && !elems) || n_el >= (1ull << 31)) return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: bad offsets");
  const bool te = ctx->is_te();
  const uint32_t G = 1u << logG;
  uint32_t true_max = 0;
  uint64_t padded = 0;   // the slots the scans owe: every bucket rounded up to a multiple of G
  for (uint64_t b = 0; b < nb; b++) {
    if (off[b] > off[b + 1]) return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: offsets must ascend");
    const uint32_t cnt = off[b + 1] - off[b];
    true_max = std::max(true_max, cnt);
    padded += ((uint64_t)cnt + G - 1) / G * G;
  }
  if (padded >= (1ull << 31)) return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: too many padded slots");
  if (reported_max && reported_max < true_max)
    return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: reported_max %u lies below the largest bucket, %u", reported_max, true_max);
  for (uint64_t e = 0; e < n_el; e++) {
    if (elems[e] >= n_pool) return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: element %llu names no pool point", (unsigned long long)e);
    if (flags && (flags[e] > 3 || (te && (flags[e] & 2))))
      return fail(ctx, MSM_ERR_ARG, "msm_test_tree_sums: element %llu: flags are bit 0 (negate) and, on the Weierstrass curves, bit 1 (beta x)",
                  (unsigned long long)e);
  }
  try {
    HIPCHK(hipSetDevice(ctx->device));
    msm_ctx::Workspace& w = ctx->ws[0];
    hipStream_t s = w.stream;
    const size_t pb = 2 * ctx->coord_bytes();   // wire point
    // 1. the pool as point rows of its own (the resident set stays as it is), the bucket sizes where the sort leaves them
    DevBuf wire, rows;
    ctx->ensure(wire, n_pool * pb);
    ctx->ensure(rows, n_pool * ctx->row_words() * 4);
    ctx->ensure(w.counts, nb * 4);
    ctx->ensure(w.cursor, (nb + 1) * 4);
    ctx->ensure(w.tail_off, (size_t)34 * (nb + 1) * 4);
    ctx->ensure(w.info, 64 * 4);
    std::vector<uint32_t> h_counts(nb);
    for (uint64_t b = 0; b < nb; b++) h_counts[b] = off[b + 1] - off[b];
    HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(wire.p, pool, n_pool * pb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.counts.p, h_counts.data(), nb * 4, hipMemcpyHostToDevice, s));
    if (te)
      hipLaunchKernelGGL(te::k_te_points_from_wire, dim3((uint32_t)((n_pool + 255) / 256)), dim3(256), 0, s, (uint32_t*)rows.p,
                         (const uint32_t*)wire.p, n_pool, 0, (uint32_t*)ctx->errflag.p);
    else
      W_LAUNCH(ctx, k_points_from_wire, dim3((uint32_t)((n_pool + 255) / 256)), dim3(256), 0, s, (uint32_t*)rows.p,
               (const uint32_t*)wire.p, n_pool, 0, (uint32_t*)ctx->errflag.p);
    // 2. the pipeline's scans; a reported maximum stands in `info` where the count pass of the bin split leaves its own
    if (reported_max) {
      std::vector<uint32_t> h_info(64, 0);
      h_info[1] = reported_max;
      HIPCHK(hipMemcpyAsync(w.info.p, h_info.data(), 64 * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));   // (h_info leaves the scope)
    }
    scan_bucket_sizes(ctx, w, nb, logG, reported_max == 0);
    const ScanTotals tot = read_scan_totals(w, logG);
    // 3. the padded slots from the device's cursor
    std::vector<uint32_t> h_cursor(nb + 1);
    HIPCHK(hipMemcpyAsync(h_cursor.data(), w.cursor.p, (nb + 1) * 4, hipMemcpyDeviceToHost, s));
    const uint32_t tables = std::min<uint32_t>((uint32_t)tot.RT + 1, tail_tables_cap);
    if (tail_off_out && tables)
      HIPCHK(hipMemcpyAsync(tail_off_out, w.tail_off.p, (size_t)tables * (nb + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (cursor_out) memcpy(cursor_out, h_cursor.data(), (nb + 1) * 4);
    plan_out[0] = (uint64_t)tot.RT;
    plan_out[2] = tot.total_slots;
    plan_out[3] = tot.max_bucket;
    plan_out[1] = plan_out[4] = plan_out[5] = plan_out[6] = plan_out[7] = 0;
    // (slots are written, and the tree sized, from what the device reports: a cursor that would leave them is a finding of its own)
    if (tot.total_slots != padded || h_cursor[nb] != padded)
      throw MsmFail{MSM_ERR_INTERNAL, "msm_test_tree_sums: the scans report " + std::to_string(tot.total_slots) + " padded slots, the buckets need " + std::to_string(padded)};
    for (uint64_t b = 0; b < nb; b++)
      if ((uint64_t)h_cursor[b] + h_counts[b] > padded)
        throw MsmFail{MSM_ERR_INTERNAL, "msm_test_tree_sums: the cursor of bucket " + std::to_string(b) + " leaves the padded slots"};
    std::vector<uint32_t> h_slots(std::max<uint64_t>(padded, 2), SLOT_EMPTY);
    for (uint64_t b = 0; b < nb; b++)
      for (uint32_t i = 0; i < h_counts[b]; i++) {
        const uint64_t e = (uint64_t)off[b] + i;
        const uint32_t f = flags ? flags[e] : 0u;
        // the payloads k_batch_add<MODE_GATHER> / k_te_add<MODE_GATHER> decode: (entry << 1) | negate, entry = 2 row + line, or the row
        const uint32_t entry = te ? elems[e] : 2 * elems[e] + ((f >> 1) & 1u);
        h_slots[h_cursor[b] + i] = (entry << 1) | (f & 1u);
      }
    ctx->ensure(w.slots, h_slots.size() * 4);
    HIPCHK(hipMemcpyAsync(w.slots.p, h_slots.data(), h_slots.size() * 4, hipMemcpyHostToDevice, s));
    // 4. what the sort leaves for its tree, 5. the tree itself
    SortOut so;
    so.logG = logG;
    so.RT = tot.RT;
    so.total_slots = tot.total_slots;
    so.max_bucket = tot.max_bucket;
    so.round1_slots = (const uint32_t*)w.slots.p;
    Plan pl{};
    pl.c = c;
    pl.K = K;
    pl.L = L;
    pl.L_log = (int)ceil_log2_u64(L);
    pl.no_glv = false;
    pl.tables = true;   // (the payloads count the rows of a buffer of the plan's own)
    pl.tab_rows = (const uint32_t*)rows.p;
    pl.tab_n = n_pool;
    ctx->ensure(w.bucket_proj, bucket_proj_bytes(ctx, nb));
    HIPCHK(hipMemsetAsync(w.bucket_proj.p, 0x2A, bucket_proj_bytes(ctx, nb), s));   // a bucket the finish skips cannot come out right
    GroupStats st;
    TreeOut to;
    TreeLog log;
    accumulate_window_group(ctx, w, pl, K, 0, so, st, to, &log);
    // 6. the bucket reduction
    const int sw = ctx->sum_words();
    std::vector<uint32_t> parts((size_t)K * sw, 0);
    reduce_buckets(ctx, w, to.bucket_proj, L, K, parts.data());
    HIPCHK(hipMemcpyAsync(w.h_info, ctx->errflag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (w.h_info[0] & 1) return fail(ctx, MSM_ERR_POINT, "msm_test_tree_sums: coordinate >= p");
    plan_out[1] = (uint64_t)log.r_stop;
    plan_out[4] = (uint64_t)st.rounds;
    plan_out[5] = st.n_pairs;
    plan_out[6] = log.rounds.size();
    for (size_t i = 0; i < log.rounds.size() && i < round_log_cap; i++) {
      round_log_out[3 * i] = (uint64_t)log.rounds[i].mode;
      round_log_out[3 * i + 1] = log.rounds[i].n_out;
      round_log_out[3 * i + 2] = log.rounds[i].steps;
    }
    for (int k = 0; k < K; k++) sum_to_wire(ctx, &parts[(size_t)k * sw], sums_out + (size_t)k * SUM_WIRE_BYTES);
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_batch_add_mode(msm_ctx* ctx, const uint8_t* g, const uint8_t* h, uint8_t* out, uint64_t n, int mode, uint32_t steps) {
  if (!ctx || !g || !h || !out || n == 0 || steps == 0) return fail(ctx, MSM_ERR_ARG, "msm_test_batch_add_mode: bad argument");
  if (ctx->is_te() || (mode != MODE_REGULAR && mode != MODE_SEARCH))
    return fail(ctx, MSM_ERR_ARG, "msm_test_batch_add_mode: Weierstrass curves, mode 1 (regular) or 2 (search)");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    // element 2e = G_e, 2e + 1 = H_e in plane layout; search mode: an all-zero H_e is passed as "no second operand"
    const uint64_t T = ((n + steps - 1) / steps + 255) / 256 * 256;
    const uint64_t in_cap = 2 * (uint64_t)steps * T;     // idle lanes of the last step read (and ignore) up to here
    const size_t pb = 2 * ctx->coord_bytes();            // wire point = tree node
    DevBuf rows, wire, planes, outb, scr, desc;
    ctx->ensure(wire, 2 * n * pb);
    ctx->ensure(rows, 2 * n * ROW_WORDS * 4);
    ctx->ensure(planes, in_cap * pb);
    ctx->ensure(outb, (uint64_t)steps * T * pb);
    ctx->ensure(scr, (size_t)steps * NL * T * 4);
    std::vector<uint8_t> inter(2 * n * pb);
    std::vector<uint32_t> hd(n);
    for (uint64_t i = 0; i < n; i++) {
      memcpy(&inter[(2 * i) * pb], g + i * pb, pb);
      memcpy(&inter[(2 * i + 1) * pb], h + i * pb, pb);
      bool hz = true;
      for (size_t j = 0; j < pb; j++) hz = hz && h[i * pb + j] == 0;
      hd[i] = (uint32_t)((2 * i) << 1) | (hz ? 0u : 1u);
    }
    HIPCHK(hipMemcpyAsync(wire.p, inter.data(), inter.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(planes.p, 0, in_cap * pb, ctx->stream));
    W_LAUNCH(ctx, k_points_from_wire, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t*)rows.p,
                       (const uint32_t*)wire.p, 2 * n, 0, (uint32_t*)ctx->errflag.p);
    ROWS_TO_PLANES(ctx, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, ctx->stream, (uint4*)planes.p, in_cap,
                   (const uint32_t*)rows.p, (uint32_t)(2 * n));
    BatchArgs a{};
    a.in = (const uint4*)planes.p;
    a.in_cap = in_cap;
    a.out = (uint4*)outb.p;
    a.out_cap = (uint64_t)steps * T;
    a.scratch = (uint32_t*)scr.p;
    a.sstride = T;
    a.n_out = n;
    a.steps = steps;
    if (mode == MODE_SEARCH) {
      ctx->ensure(desc, n * 4);
      HIPCHK(hipMemcpyAsync(desc.p, hd.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
      a.desc = (const uint32_t*)desc.p;
      W_LAUNCH_MODE(ctx, k_batch_add, MODE_SEARCH, dim3((uint32_t)(T / 256)), dim3(256), 0, ctx->stream, a);
    } else {
      W_LAUNCH_MODE(ctx, k_batch_add, MODE_REGULAR, dim3((uint32_t)(T / 256)), dim3(256), 0, ctx->stream, a);
    }
    std::vector<uint32_t> pl(a.out_cap * pb / 4);
    HIPCHK(hipMemcpyAsync(pl.data(), outb.p, pl.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    for (uint64_t e = 0; e < n; e++) plane_element_to_wire(ctx, pl.data(), a.out_cap, e, out + e * pb);
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_set_chunk_rows_log(msm_ctx* ctx, int32_t log2_rows) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_chunk_rows_log: not on a device-list context");
  if (log2_rows < 0 || log2_rows > 40) return fail(ctx, MSM_ERR_ARG, "msm_test_set_chunk_rows_log: log2_rows must be 0 (default) or 1 .. 40");
  ctx->chunk_rows_log = log2_rows ? log2_rows : msm_ctx::CHUNK_ROWS_LOG;
  return MSM_OK;
}

int msm_test_last_sort_paths(msm_ctx* ctx, int32_t* out, int cap) {
  if (!ctx || !ctx->children.empty() || cap < 0 || (cap && !out)) return -1;
  const int count = (int)ctx->last_sort_paths.size();
  for (int i = 0; i < count && i < cap; i++) out[i] = ctx->last_sort_paths[i];
  return count;
}

int msm_test_set_points_mul_grid(msm_ctx* ctx, int32_t blocks) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_points_mul_grid: not on a device-list context");
  if (blocks < 0 || blocks > 65536) return fail(ctx, MSM_ERR_ARG, "msm_test_set_points_mul_grid: blocks must be 0 (default) or 1 .. 65536");
  ctx->pmul_grid = blocks;
  return MSM_OK;
}

int msm_test_set_points_mul_base_path(msm_ctx* ctx, int32_t path) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_points_mul_base_path: not on a device-list context");
  if (path < 0 || path > 2) return fail(ctx, MSM_ERR_ARG, "msm_test_set_points_mul_base_path: path must be 0 (auto), 1 (table) or 2 (broadcast)");
  ctx->pmul_base_path = path;
  return MSM_OK;
}

int msm_test_last_points_mul(msm_ctx* ctx, int32_t* out, int cap) {
  if (!ctx || !ctx->children.empty() || cap < 0 || (cap && !out)) return -1;
  for (int i = 0; i < 4 && i < cap; i++) out[i] = ctx->last_pmul[i];
  return 4;
}

int msm_test_set_points_ntt_grid(msm_ctx* ctx, int32_t blocks) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_points_ntt_grid: not on a device-list context");
  if (blocks < 0 || blocks > 65536) return fail(ctx, MSM_ERR_ARG, "msm_test_set_points_ntt_grid: blocks must be 0 (default) or 1 .. 65536");
  ctx->pntt_grid = blocks;
  return MSM_OK;
}

int msm_test_last_points_ntt(msm_ctx* ctx, int32_t* out, int cap) {
  if (!ctx || !ctx->children.empty() || cap < 0 || (cap && !out)) return -1;
  for (int i = 0; i < 7 && i < cap; i++) out[i] = ctx->last_pntt[i];
  return 7;
}

int msm_test_set_ntt_tile_log(msm_ctx* ctx, int32_t tile_log) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_ntt_tile_log: not on a device-list context");
  if (tile_log < 0 || tile_log > 10) return fail(ctx, MSM_ERR_ARG, "msm_test_set_ntt_tile_log: tile_log must be 0 (default) or 1 .. 10");
  ctx->ntt_tile_log = tile_log;
  return MSM_OK;
}

int msm_test_last_ntt_plan(msm_ctx* ctx, int32_t* stages_out, int cap) {
  if (!ctx || !ctx->children.empty() || cap < 0 || (cap && !stages_out)) return -1;
  const int count = (int)ctx->last_ntt_plan.size();
  for (int i = 0; i < count && i < cap; i++) stages_out[i] = ctx->last_ntt_plan[i];
  return count;
}

int msm_test_digits(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, uint64_t n_array, uint64_t first,
                    int32_t width_bytes, int32_t bits, int32_t is_signed, const msm_opts* opts, int32_t k_lo, int32_t k_hi,
                    uint32_t* digits_out, int32_t* c_out, int32_t* K_out, int32_t* fold_out, int32_t* flags_rc_out) {
  if (!ctx || !scalars || (digits_out && !flags_rc_out) || B == 0 || n == 0 || (n >> 32))
    return fail(ctx, MSM_ERR_ARG, "msm_test_digits: null argument, no element or n outside 1 .. 2^32 - 1");
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_digits: not on a device-list context");
  for (uint32_t b = 0; b < B; b++)
    if (!scalars[b]) return fail(ctx, MSM_ERR_ARG, "msm_test_digits: no scalars for element %u", b);
  if (first + n > n_array || (n_array >> 32)) return fail(ctx, MSM_ERR_ARG, "msm_test_digits: [first, first + n) lies outside the array");
  // the plan, as msm_window_sums / msm_run_narrow / msm_run_batch(_narrow) make it
  Plan pl;
  Plan::Narrow nar;
  if (width_bytes) {
    if (int rc = narrow_format(ctx, width_bytes, bits, is_signed, opts, "msm_test_digits", nar)) return rc;
  }
  if (make_plan(ctx, n, opts, pl, false, width_bytes ? nar.fmt.bits : 0)) return fail(ctx, MSM_ERR_ARG, "msm_test_digits: bad window size");
  pl.nar = nar;
  if (k_lo == 0 && k_hi == 0) k_hi = pl.K;
  if (k_lo < 0 || k_hi > pl.K || k_lo >= k_hi) return fail(ctx, MSM_ERR_ARG, "msm_test_digits: bad window range [%d, %d) of %d", k_lo, k_hi, pl.K);
  if (B > 1) {
    // a fused batch: whole elements from their first scalar, all windows, no shard (the _batch kernels know none of these)
    if (int rc = refuse_shard_opts(ctx, opts, "msm_test_digits", "a batch")) return rc;
    if (!opts || opts->c <= 0) return fail(ctx, MSM_ERR_ARG, "msm_test_digits: a batch needs its window (msm_opts.c)");
    if (first || n_array != n || k_lo != 0 || k_hi != pl.K || B > (uint32_t)(width_bytes ? NARROW_BATCH_MAX : BATCH_MAX))
      return fail(ctx, MSM_ERR_ARG, "msm_test_digits: a batch takes whole arrays, all windows and at most %d elements",
                  width_bytes ? NARROW_BATCH_MAX : BATCH_MAX);
  }
  if (c_out) *c_out = pl.c;
  if (K_out) *K_out = pl.K;
  if (fold_out) *fold_out = pl.fold ? 1 : 0;
  if (!digits_out) return MSM_OK;   // the plan alone: what the caller sizes digits_out from
  *flags_rc_out = MSM_OK;
  try {
    HIPCHK(hipSetDevice(ctx->device));
    msm_ctx::Workspace& w = ctx->ws[0];
    // the scalars where the real calls put them
    const uint32_t* d_scal = nullptr;
    NarrowBatchScalars nbs{};
    int kc = k_hi - k_lo;
    if (B > 1) {
      bind_batch_scalars(pl, nbs, stage_batch_scalars(ctx, scalars, B, n, 0, pl), 0, (int)B);
      k_hi = kc = (int)B * pl.K;   // virtual windows b K + k
    } else if (width_bytes) {
      float up_ms = 0;
      const char* dev = narrow_lane_base(stage_narrow(ctx, scalars[0], (size_t)n_array * width_bytes, 0, &up_ms), width_bytes, pl.nar);
      d_scal = group_scalars((const uint32_t*)dev, first, pl);
    } else {
      stage_scalars(ctx, scalars[0], n_array, 0, &d_scal);
      d_scal = group_scalars(d_scal, first, pl);
    }
    HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, 4, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // scalars and the error flag are in place before the group stream starts
    // the digit launch of sort_window_group under the group's sort geometry, and nothing behind it
    // (the digits of a fused batch need no cuts: the _batch kernels count nothing, whatever the windows)
    const uint64_t two_n_d = ctx->is_te() ? n : 2 * n, words = (uint64_t)kc * two_n_d;
    const SortGeometry g = B > 1 ? SortGeometry::digits_alone(kc, two_n_d) : sort_geometry(ctx, n, pl, k_lo, k_hi);
    const GroupDigits dg = launch_group_digits(ctx, w, d_scal, n, pl, k_lo, g);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(digits_out, dg.dig, words * 4, hipMemcpyDeviceToHost, w.stream));
    HIPCHK(hipStreamSynchronize(w.stream));
    try {
      check_scalar_flags(ctx, pl, "msm_test_digits");
    } catch (const MsmFail& f) {
      *flags_rc_out = fail(ctx, f.code, "%s", f.msg.c_str());
    }
    return MSM_OK;
  } MSM_CATCH_ALL(ctx)
}

int msm_test_set_matvec_geometry(msm_ctx* ctx, uint32_t short_max, uint32_t part_len) {
  if (!ctx) return MSM_ERR_ARG;
  if (!ctx->children.empty()) return fail(ctx, MSM_ERR_ARG, "msm_test_set_matvec_geometry: not on a device-list context");
  ctx->spmv_short_max = short_max;
  ctx->spmv_part_len = part_len;
  return MSM_OK;
}

int msm_test_last_matvec(msm_ctx* ctx, int32_t* out, int cap) {
  if (!ctx || !ctx->children.empty() || cap < 0 || (cap && !out)) return -1;
  for (int i = 0; i < 5 && i < cap; i++) out[i] = ctx->last_spmv[i];
  return 5;
}

int msm_test_live_buffers(uint64_t* count_out, uint64_t* bytes_out) {
  if (!count_out || !bytes_out) return MSM_ERR_ARG;
  *count_out = live_buffers.load();
  *bytes_out = live_buffer_bytes.load();
  return MSM_OK;
}

int msm_generate_points(msm_ctx* ctx, uint64_t n, uint64_t seed, uint8_t* a_out) {
  if (!ctx) return MSM_ERR_ARG;
  if (ctx->children.empty()) return generate_points_one(ctx, n, seed, a_out);
  try {   // the generator is deterministic in (seed, index): every device builds the identical set
    return on_all_devices(ctx, [&](msm_ctx* c) { return generate_points_one(c, n, seed, c == ctx ? a_out : nullptr); });
  } MSM_CATCH_ALL(ctx)
}

int msm_generate_scalars(msm_ctx* ctx, uint64_t n, uint64_t seed, void* dev_dst, uint8_t* host_out) {
  if (!ctx) return MSM_ERR_ARG;
  if (!dev_dst && !host_out) return fail(ctx, MSM_ERR_ARG, "msm_generate_scalars: neither a device nor a host destination");
  try {
    HIPCHK(hipSetDevice(ctx->device));
    return msm_gen::generate_scalars(ctx, n, seed, dev_dst, host_out);
  } MSM_CATCH_ALL(ctx)
}

}  // extern "C"
