/* Plain-C host of the C ABI (include/msm_hip.h): no Python, no torch -- what a cgo / JNI / N-API binding would do.
 *   gcc -O2 -Iinclude examples/msm_demo.c -Lmontgomery_amd -lmsm_hip -Wl,-rpath,'$ORIGIN/../montgomery_amd' -o examples/msm_demo
 *   examples/msm_demo [log2_n] [curve id or name: bls12-377, ed-on-bls12-377, bls12-381, pallas, bn254, grumpkin, vesta]
 * Generates N points and scalars on the GPU, runs the MSM twice with different window sizes (the result is a
 * group element: it must not depend on c), then once more as K one-window shards recombined with
 * msm_combine_curve, the way the ranks of a multi-GPU run do, and once through the indexed entry point (msm_run_indexed) with
 * every point named once.  Exit code 0 = all four agree. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "msm_hip.h"

static void die(msm_ctx* ctx, const char* what, int rc) {
  fprintf(stderr, "%s failed: %d (%s)\n", what, rc, ctx ? msm_last_error(ctx) : "no context");
  exit(1);
}

static int curve_of(const char* s) {
  static const char* names[] = {"bls12-377", "ed-on-bls12-377", "bls12-381", "pallas", "bn254", "grumpkin", "vesta"};   /* by curve id */
  for (int i = 0; i < (int)(sizeof names / sizeof names[0]); i++)
    if (strcmp(s, names[i]) == 0) return i;
  char* end = NULL;
  const long id = strtol(s, &end, 10);
  if (end == s || *end || id < 0 || id >= (long)(sizeof names / sizeof names[0])) {
    fprintf(stderr, "unknown curve '%s': a curve id 0 .. 6 or one of", s);
    for (int i = 0; i < (int)(sizeof names / sizeof names[0]); i++) fprintf(stderr, " %s", names[i]);
    fprintf(stderr, "\n");
    exit(1);
  }
  return (int)id;
}

int main(int argc, char** argv) {
  const int lg = argc > 1 ? atoi(argv[1]) : 16;
  const int curve = argc > 2 ? curve_of(argv[2]) : MSM_CURVE_BLS12_377_G1;
  const uint64_t n = 1ull << lg;
  msm_ctx* ctx = NULL;
  int rc = msm_ctx_create(&ctx, curve, 0);
  if (rc) die(NULL, "msm_ctx_create (no usable GPU? there is no CPU fallback)", rc);
  if ((rc = msm_generate_points(ctx, n, 42, NULL))) die(ctx, "msm_generate_points", rc);
  void* d_scalars = NULL; /* one device buffer per scalar handle, owned by the context until msm_device_free */
  if ((rc = msm_device_alloc(ctx, n * 32, &d_scalars))) die(ctx, "msm_device_alloc", rc);
  if ((rc = msm_generate_scalars(ctx, n, 43, d_scalars, NULL))) die(ctx, "msm_generate_scalars", rc);

  msm_opts opts;
  msm_result a, b, c3;
  memset(&opts, 0, sizeof opts);
  if ((rc = msm_run(ctx, d_scalars, n, 1, &opts, &a))) die(ctx, "msm_run", rc);
  opts.c = 11;
  if ((rc = msm_run(ctx, d_scalars, n, 1, &opts, &b))) die(ctx, "msm_run (c = 11)", rc);
  printf("N = 2^%d  c = %d  K = %d  %.3f ms  (accumulate %.3f ms, %llu pair additions)\n", lg, a.c, a.K, a.phase_ms[MSM_T_TOTAL],
         a.phase_ms[MSM_T_ACCUMULATE], (unsigned long long)a.n_pairs);
  printf("x = 0x");
  for (int i = 47; i >= 0; i--) printf("%02x", a.x[i]);
  printf("\n");
  int ok = memcmp(a.x, b.x, 48) == 0 && memcmp(a.y, b.y, 48) == 0 && a.is_infinity == b.is_infinity;

  { /* window shards: one window at a time, then the host combine */
    int32_t cc = 0, K = 0;
    memset(&opts, 0, sizeof opts);
    if ((rc = msm_plan(ctx, n, &opts, &cc, &K))) die(ctx, "msm_plan", rc);
    uint8_t* parts = (uint8_t*)malloc((size_t)K * 144);
    for (int k = 0; k < K; k++) {
      opts.c = cc; opts.k_lo = k; opts.k_hi = k + 1;
      if ((rc = msm_window_sums(ctx, d_scalars, n, 1, &opts, parts + (size_t)k * 144, NULL))) die(ctx, "msm_window_sums", rc);
    }
    if ((rc = msm_combine_curve(curve, parts, K, cc, &c3))) die(ctx, "msm_combine_curve", rc);
    free(parts);
    ok = ok && memcmp(a.x, c3.x, 48) == 0 && memcmp(a.y, c3.y, 48) == 0;
  }
  { /* the indexed form: scalars[j] belongs to point indices[j]; naming every point once, in order, is the dense MSM */
    msm_result d;
    void* d_indices = NULL;
    uint32_t* indices = (uint32_t*)malloc((size_t)n * 4);
    for (uint64_t j = 0; j < n; j++) indices[j] = (uint32_t)j;
    if ((rc = msm_device_alloc(ctx, n * 4, &d_indices))) die(ctx, "msm_device_alloc", rc);
    if ((rc = msm_device_upload(ctx, d_indices, indices, n * 4))) die(ctx, "msm_device_upload", rc);
    free(indices);
    memset(&opts, 0, sizeof opts);
    if ((rc = msm_run_indexed(ctx, d_scalars, (const uint32_t*)d_indices, n, 1, &opts, &d))) die(ctx, "msm_run_indexed", rc);
    ok = ok && memcmp(a.x, d.x, 48) == 0 && memcmp(a.y, d.y, 48) == 0 && a.is_infinity == d.is_infinity;
  }
  msm_ctx_destroy(ctx);
  printf(ok ? "OK: result independent of the window size and of the sharding\n" : "MISMATCH\n");
  return ok ? 0 : 2;
}
