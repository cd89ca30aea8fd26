// Host-side internals of libmsm_hip.so shared by its translation units (HOST_TUS in the Makefile):
//   msm_plan.hip      window size, plan, launch geometry, workspace budget model, the schedule of a call's window groups
//                     (group_schedule: pure arithmetic, tested on the CPU by tests/test_group_schedule.py), error helpers
//   msm_sort.hip      digits + counting sort of one window group (driver of sort_kernels.h)
//   msm_tree.hip      accumulation tree of one window group (driver of k_batch_add / k_te_add), always ended by k_bucket_finish
//   msm_reduce.hip    bucket reduction over the finished bucket sums, and the host tail over window sums (sum, Horner, to-affine,
//                     wire form, combine): one implementation over the two host point kinds (Weierstrass / Edwards)
//   msm_upload.hip    staged and pipelined host -> device transfers
//   msm_pipeline.hip  runs a schedule: window groups on two streams, their sums added back; multi-device fan-out, call statistics,
//                     and the begin / finish every full-MSM entry point shares (call_begin, call_finish)
//   msm_batch.hip     msm_run_batch, msm_run_batch_narrow: B MSMs over one point set, fused into shared window groups
//   msm_tables.hip    window tables (resident tables 2^(c j) P: one set of buckets for all windows of a group)
//   msm_abi.hip       the C ABI of include/msm_hip.h (contexts, points, msm_run, msm_window_sums, handles)
//   msm_test_abi.hip  the operator-level test entries (msm_test_*)
//   msm_gen.hip       the input generators (msm_generate_points, msm_generate_scalars)
//   msm_ingest.hip    msm_set_points_ex, msm_validate_points, msm_get_points_ex: compressed points, subgroup checks
//   msm_narrow.hip    msm_run_narrow, msm_plan_narrow, msm_scalar_bits (narrow scalars: no endomorphism split, K from the call's bits)
//   msm_indexed.hip   msm_run_indexed, msm_run_indexed_narrow (scalars over a chosen multiset of the resident points), with their
//                     two kernels: the index check and the payload translation
//   msm_lincomb.hip   msm_points_lincomb, msm_pointset_size (resident points from resident points: D = a A + b B), with the
//                     kernels of points_lincomb.h
//   msm_scalars.hip   msm_scalars_lincomb, _mul, _inner, _powers (vectors of scalars in device memory, mod the group order) and
//                     msm_device_download, with the kernels of scalar_vec.h
//   msm_mle.hip       msm_scalars_sumcheck_round, _bind, _eq (the sumcheck over multilinear tables) and the two entries of their
//                     debug surface, with the kernels of scalar_mle.h
//   msm_spmv.hip      msm_matrix_create, _destroy, _info and msm_scalars_matvec (resident sparse matrices in CSR and y = alpha M x
//                     (+ y) mod the group order), with the kernels of scalar_spmv.h
//   msm_points_ntt.hip  msm_points_ntt (the transform over the rows of a point set), with the kernels of points_ntt.h
// The operators over resident vectors and point sets (msm_scalars, msm_ntt, msm_scan, msm_mle, msm_spmv, msm_lincomb, msm_points_mul,
// msm_points_ntt) take their
// argument checks from operator_checks.h and the host side of the scalar field from scalar_host.h.
// Kernels live in kernels_curve.hip (one TU per curve), sort_kernels.hip, te_kernels.hip and narrow_kernels.hip; host TUs see
// declarations.
// Ownership: every device buffer, pinned host block, stream and event is a move-only member or local (msmi::DevBuf, Pinned, Stream,
// Event) that its holder's destructor frees; nothing else frees, and no list of names says what a context, a point set, a matrix
// or a call gives back.
// Orchestration follows `createMsm().msm` (reference src/msm-batched-affine.ts:69-340); the per-thread SPMD phases separated
// by `barrier()` there become kernel launches on one HIP stream here.
#pragma once
#include "kernel_inst.h"   // curve-templated kernels: extern templates, defined in kernels_curve.hip per curve
#include "sort_kernels.h"
#include "tree_kernels.h"
#include "te_kernels.h"
#include "narrow_kernels.h"
#include "host_field.h"
#include "scalar_vec.h"    // the scalar field of every curve (MSM_SCALAR_FIELDS); its kernels are instantiated by msm_scalars.hip
#include "../../include/msm_hip.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

// Policy knobs -- the six thresholds that are re-measured when a plan changes (MSM_GROUPS, MSM_MAX_STEPS, MSM_PBL, MSM_TC,
// MSM_FINISH_MAX, MSM_TAIL_MIN) -- are environment variables ONLY in builds made with -DMSM_TUNING (make ab EXTRA=-DMSM_TUNING,
// tools/knob_sweep.sh); the product never reads the environment.  The knobs of closed experiments left in round 6.
// MSM_TC is rounded down to a power of two where it is read (reduce_buckets): a window is cut into 2^nbits chunks.
#ifdef MSM_TUNING
#define MSM_KNOB(var, name, lo) do { if (const char* _e = getenv(name)) var = std::max<long long>((lo), atoll(_e)); } while (0)
#define MSM_KNOB_SET(name) (getenv(name) != nullptr)
#else
#define MSM_KNOB(var, name, lo) do { } while (0)
#define MSM_KNOB_SET(name) false
#endif

namespace msmi {

struct HipFail {
  hipError_t e;
  const char* what;
  int line;
  const char* file;
};

// non-HIP failure raised inside the pipeline (mapped to its error code at the ABI boundary)
struct MsmFail {
  int code;
  std::string msg;
};


#define HIPCHK(x)                                   \
  do {                                              \
    hipError_t _e = (x);                            \
    if (_e != hipSuccess) throw msmi::HipFail{_e, #x, __LINE__, __FILE__}; \
  } while (0)

// The owner types: move-only, a moved-from owner is empty, and an empty one makes no HIP call.

// live device buffers of the process and their bytes as allocated (msm_test_live_buffers)
inline std::atomic<uint64_t> live_buffers{0}, live_buffer_bytes{0};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf o) noexcept {   // (the source is emptied into o; what this held goes back with o)
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DevBuf() { release(); }
  // room for `bytes`: what is there if it suffices, otherwise a new block with some slack (the old one goes back first)
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    release(/*checked=*/true);
    allocate(bytes + bytes / 16 + 256);
  }
  // a block of exactly `want` bytes into an empty buffer; a failure leaves it empty
  void allocate(size_t want) {
    const hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      (void)hipGetLastError();   // the failure must not stay behind as this thread's "last error": the kernel-launch checks read it
      p = nullptr;
      throw HipFail{e, "hipMalloc(&p, want)", __LINE__, __FILE__};
    }
    cap = want;
    live_buffers++;
    live_buffer_bytes += want;
  }
  // checked: throws what hipFree reports; teardown paths have nothing useful to do with an error
  void release(bool checked = false) {
    if (p) {
      const hipError_t e = hipFree(p);
      if (checked) HIPCHK(e);
      live_buffers--;
      live_buffer_bytes -= cap;
    }
    p = nullptr;
    cap = 0;
  }
};

// a stream, an event or a pinned host block: H the handle (null: nothing here), Destroy what gives it back
template <class H, auto Destroy>
struct Owned {
  Owned() = default;
  Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  ~Owned() {
    if (h) (void)Destroy(h);
  }
  operator H() const { return h; }
  H h = nullptr;
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {   // non-blocking
  void create() { HIPCHK(hipStreamCreateWithFlags(&h, hipStreamNonBlocking)); }
  void create(int priority) { HIPCHK(hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority)); }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  void create(unsigned flags = hipEventDefault) { HIPCHK(hipEventCreateWithFlags(&h, flags)); }
};
template <class T>
struct Pinned : Owned<T*, hipHostFree> {
  void allocate(size_t bytes) { HIPCHK(hipHostMalloc((void**)&this->h, bytes, hipHostMallocDefault)); }
};

inline uint32_t ceil_log2_u64(uint64_t n) {
  uint32_t r = 0;
  while ((1ull << r) < n) r++;
  return r;
}

// host-side view of the per-curve constants (constants_gen.h)
struct CurveInfo {
  const uint32_t* pw;   // base field modulus, 12 words (zero-extended for the 8-word fields)
  const uint32_t* q;    // scalar field order, 8 words
  const uint32_t* gx;   // generator (Weierstrass curves), 12 words each, device Montgomery form
  const uint32_t* gy;
  int glv_max_bits;     // Scalar.maxBits after decomposition, src/wasm/glv.ts:216-226
  int q_bits;           // bit length of q
  int nl, nw;           // 30-bit limbs in registers, packed words per coordinate in memory
};

inline int bit_length8(const uint32_t* w) {   // of an 8-word integer
  for (int b = 255; b >= 0; b--)
    if ((w[b / 32] >> (b % 32)) & 1u) return b + 1;
  return 0;
}

// a Weierstrass configuration's constants, the 8-word fields zero-extended to the 12 words the host side reads
template <class CV>
inline const CurveInfo& weierstrass_info() {
  using F = typename CV::F;
  static uint32_t pw[12], gx[12], gy[12];
  static const CurveInfo info = [] {
    for (int i = 0; i < F::NW; i++) { pw[i] = F::PW[i]; gx[i] = F::GXW[i]; gy[i] = F::GYW[i]; }
    return CurveInfo{pw, CV::G::Q, gx, gy, CV::G::MAX_BITS, bit_length8(CV::G::Q), F::NL, F::NW};
  }();
  return info;
}

// nullptr: no such curve id
inline const CurveInfo* curve_info_or_null(int curve) {
  static const CurveInfo ed377 = {msm::Fp253::PW, msm::FRED_Q, nullptr, nullptr, 251, 251, msm::Fp253::NL, msm::Fp253::NW};
  switch (curve) {
#define MSM_INFO_CASE(ID, CV) case ID: return &weierstrass_info<msm::CV>();
    MSM_W_CURVES(MSM_INFO_CASE)
#undef MSM_INFO_CASE
    case MSM_CURVE_ED_ON_BLS12_377: return &ed377;
  }
  return nullptr;
}
inline const CurveInfo& curve_info(int curve) {
  const CurveInfo* ci = curve_info_or_null(curve);
  return ci ? *ci : *curve_info_or_null(MSM_CURVE_BLS12_377_G1);
}

// A window sum travels through the host pipeline as one "slot" of packed words in device Montgomery form: X, Y, Z of 12 words
// each on the Weierstrass curves, X, Y, Z, T of 8 words each on the Edwards curve (msm_ctx::sum_words()); msm_window_sums
// hands it out as X || Y || Z of 48 bytes each.  Only the helpers of msm_reduce.hip look inside a slot.
constexpr int W_SUM_WORDS = 36, TE_SUM_WORDS = 32, SUM_WIRE_BYTES = 144;

// One helper thread per context, started with it: the second window group of a big MSM runs here (the calling thread
// takes the first), so no thread is created per call.  run() hands over a job, wait() returns when it is done and
// re-raises whatever the job threw.
class HelperThread {
 public:
  HelperThread() : th_([this] { loop(); }) {}
  ~HelperThread() {
    {
      std::lock_guard<std::mutex> l(mu_);
      quit_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  void run(std::function<void()> job) {
    std::lock_guard<std::mutex> l(mu_);
    job_ = std::move(job);
    busy_ = true;
    err_ = nullptr;
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> l(mu_);
    cv_.wait(l, [this] { return !busy_; });
    if (err_) {
      std::exception_ptr e = err_;
      err_ = nullptr;
      std::rethrow_exception(e);
    }
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> l(mu_);
    for (;;) {
      cv_.wait(l, [this] { return quit_ || (busy_ && job_); });
      if (quit_) return;
      std::function<void()> job = std::move(job_);
      job_ = nullptr;
      l.unlock();
      std::exception_ptr e;
      try { job(); } catch (...) { e = std::current_exception(); }
      l.lock();
      err_ = e;
      busy_ = false;
      cv_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::function<void()> job_;
  std::exception_ptr err_;
  bool busy_ = false, quit_ = false;
  std::thread th_;   // last member: the thread starts after everything it touches exists
};

}  // namespace msmi

struct msm_ctx {
  std::unique_ptr<msmi::HelperThread> helper;
  int curve = 0;
  int device = 0;
  msmi::Stream stream;
  msmi::Event ev[12];
  msmi::Event ev_dig[2];   // around the digit kernel that serves both window groups of a call (GroupDigits)
  std::string err;
  int n_cu = 256;

  // Window tables of a point set (msm_tables.hip): T tables of n rows each, table j = 2^(c j) P over the points [lo, lo + n),
  // for a plan of K windows (K = 0: none).  T = K where a run on them is one window group; where it is several, every group
  // reads the same T = ceil(K / groups) tables, relative to its own first window (msmi::window_groups_wanted).  Tables of the
  // WHOLE set live in the set's row buffer, which grows to hold them (table 0 is the plain row table: in_rows); tables of a
  // RANGE of the points -- the share of one rank of a points-split run -- in `buf`, with a copy of the range's rows as table 0.
  // K, T != 0 only while the buffer they name holds all T tables: a build describes them last.
  struct WindowTables {
    int c = 0, K = 0;
    int T = 0;   // tables held
    uint64_t lo = 0, n = 0;
    bool in_rows = false;
    msmi::DevBuf buf;   // (may outlive a description that is cleared: a range build of the same size reuses it)
    bool covers(uint64_t l, uint64_t m) const { return K && lo == l && n == m; }
    bool whole_set_pinned() const { return K && in_rows; }
    void clear() { T = 0; c = K = 0; lo = n = 0; in_rows = false; }
    void drop() { clear(); buf.release(); }   // (the description goes first)
  };
  // A resident point set (msm_pointset_*): its rows, one per point, and its window tables.  `sets` holds them all; the
  // CURRENT one, which every call reads, is sets[cur_set] (pts()).
  struct PointSet {
    msmi::DevBuf rows;
    uint64_t n = 0;
    bool live = false;   // (slot 0, the default set, always is)
    WindowTables tab;
    const uint32_t* table_rows() const { return (const uint32_t*)(tab.in_rows ? rows.p : tab.buf.p); }
    void release() { tab.clear(); *this = PointSet(); }   // (the description goes first, then whatever the set holds)
  };
  std::vector<PointSet> sets = std::vector<PointSet>(1);   // slot 0 = the default set
  int cur_set = 0;
  PointSet& pts() { return sets[cur_set]; }
  const PointSet& pts() const { return sets[cur_set]; }
  // new points replace those of the current set: it forgets them and its window tables, and gets room for n rows
  uint32_t* reset_points(uint64_t n) { return reset_points(pts(), n); }
  // the same for any set of the context (msm_points_lincomb writes into sets that are not current)
  uint32_t* reset_points(PointSet& s, uint64_t n) {
    s.n = 0;
    s.tab.drop();   // window tables belong to the points they were built from
    cand_n = 0;
    ensure(s.rows, std::max<uint64_t>(n, 1) * row_words() * 4);
    return (uint32_t*)s.rows.p;
  }
  // the range the last table-eligible call over a RANGE of the points asked for: range tables are built when a call comes back
  // for the same range (a rank of a sharded run does; a caller walking over the shards of one GPU does not and is spared a build per call)
  uint64_t cand_lo = 0, cand_n = 0;
  int cand_c = 0;
  uint64_t tables_limit = 0;   // bytes the tables of one point set may take (msm_set_tables_limit; default: 20 % of the device)
  std::vector<msmi::DevBuf> allocs; // device buffers handed out by msm_device_alloc
  // multi-device context (msm_ctx_create_multi): this context drives devices[0], one child context per further device
  std::vector<msm_ctx*> children;
  std::vector<std::unique_ptr<msmi::HelperThread>> fan;   // one host thread per child for the window-shard fan-out

  // staging / misc buffers shared by all window groups
  msmi::DevBuf scal, errflag, misc;
  msmi::Pinned<uint32_t> h_info;   // 64 words
  // host -> device staging of big pageable buffers (upload_staged): pinned chunks, a copy stream and an event per chunk slot
  static constexpr int STAGE_THREADS = 4, STAGE_SLOTS = 2;
  static constexpr size_t STAGE_CHUNK = (size_t)16 << 20;
  msmi::Pinned<char> stage_pin;
  bool staging_ready = false;      // pinned slots, copy streams and events all exist (ensure_staging)
  msmi::Stream stage_stream[STAGE_THREADS];
  msmi::Event stage_ev[STAGE_THREADS][STAGE_SLOTS + 1];
  static constexpr int MAX_PIECES = 6;   // ranges of the points a host-scalar MSM is pipelined over (PieceUpload)
  msmi::Event piece_ev[MAX_PIECES][STAGE_THREADS];
  uint64_t ws_budget = 0;          // bytes the per-group workspaces may take in total
  uint64_t ws_limit = 0;           // msm_set_workspace_limit: the caller's cap on ws_budget (0 = automatic)
  // log2 of the table rows above which round 1 of a big window takes the pair form (sort_geometry, where the measurements
  // behind the default are); only msm_test_set_chunk_rows_log moves it, so that tests reach the pair form at small sizes
  static constexpr int CHUNK_ROWS_LOG = 23;
  int chunk_rows_log = CHUNK_ROWS_LOG;
  // MSM_SORT_* of every window group of the last call, in the order of its schedule; cleared when a call starts its groups and
  // written when all of them have run, so a call that failed, or a fused batch, leaves it empty
  std::vector<int32_t> last_sort_paths;
  // msm_scalars_ntt (msm_ntt.hip): the twiddle tables of one (log2n, omega) at a time, both directions; the two-level table of the
  // shift of the last coset call; the vector that the passes before the last work in.
  msmi::DevBuf ntt_tw, ntt_shift, ntt_scratch;
  int ntt_tw_log2n = -1;           // -1: no tables
  uint8_t ntt_tw_omega[32] = {};   // the root the tables are of, 32 bytes little-endian
  bool ntt_tw_library = false;     // ... and it is the library's root of that size (a call without omega then computes no root)
  int ntt_tile_log = 0;            // msm_test_set_ntt_tile_log: stages a pass may have; 0 = ntt::DEFAULT_TILE_LOG
  std::vector<int32_t> last_ntt_plan;   // stages per pass of the last msm_scalars_ntt (msm_test_last_ntt_plan); empty after a refusal
  // msm_scalars_scan / _inverse / _div_linear (msm_scan.hip): the call's total, then one 32-byte aggregate per tile and level (the
  // inverse keeps its per-block zero counts there).
  msmi::DevBuf scan_agg;
  int scan_tile_log = 0;           // msm_test_set_scan_tile_log: elements per tile = 2^it; 0 = scan::DEFAULT_TILE_LOG
  std::vector<int32_t> last_scan_plan;  // tiles per level of the last scan / div_linear (msm_test_last_scan_plan); empty after a refusal

  // msm_points_mul / msm_points_mul_base (msm_points_mul.hip): the per-lane tables of the variable-base kernel's grid; the row of
  // the fixed base and its shared table of rows, cached under the base's bytes.
  msmi::DevBuf pmul_tbl, pmul_row, pmul_base_tbl;
  uint8_t pmul_base_key[97] = {};   // 1 + x || y of the base the table is of (first byte 2, the rest zero: the generator)
  bool pmul_base_cached = false;
  int pmul_blocks_per_cu = 0;       // resident blocks of the variable-base kernel per compute unit (0: not asked yet)
  int pmul_grid = 0;                // msm_test_set_points_mul_grid: blocks of the variable-base grid; 0 = the default
  int pmul_base_path = 0;           // msm_test_set_points_mul_base_path: 0 auto, 1 table, 2 broadcast
  int32_t last_pmul[4] = {};        // grid, w, path, table rows of the last call (msm_test_last_points_mul)

  // msm_points_ntt (msm_points_ntt.hip): the vector w^j, j < n / 2, of one (log2n, omega, direction) at a time, 16 n bytes.  The
  // per-lane tables of its butterflies are pmul_tbl.
  msmi::DevBuf pntt_tw;
  int pntt_tw_log2n = -1;           // -1: no vector
  uint8_t pntt_tw_omega[32] = {};   // the root the vector is of, 32 bytes little-endian
  bool pntt_tw_inverse = false;     // ... and it holds the powers of its inverse
  int pntt_blocks_per_cu = 0;       // resident blocks of the multiplying stage kernel per compute unit (0: not asked yet)
  int pntt_grid = 0;                // msm_test_set_points_ntt_grid: blocks of a stage's grid; 0 = the default
  int32_t last_pntt[7] = {};        // the plan of the last call (msm_test_last_points_ntt); all 0 after a refusal

  // msm_scalars_sumcheck_round / _bind / _eq (msm_mle.hip): the round's results and its partials per block and value; the two
  // half-tables of the last eq.
  msmi::DevBuf mle_part, mle_tab;
  int mle_grid = 0;                 // msm_test_set_sumcheck_grid: blocks of the round kernel; 0 = the default
  int32_t last_mle[4] = {0, 0, 0, -1};   // blocks, pairs, values of the last round; split k of the last eq (msm_test_last_sumcheck)

  // msm_matrix_* / msm_scalars_matvec (msm_spmv.hip): resident sparse matrices in CSR, each the sole owner of its arrays -- the
  // column indices, the coefficients in Montgomery form (none in the all-ones form), and the plan of its long rows with their
  // partials (scalar_spmv.h).  `mats` holds them all; slot 0 is never live, ids start at 1.
  struct Matrix {
    bool live = false, ones = false;
    uint64_t rows = 0, cols = 0, nnz = 0;
    uint32_t short_max = 0, part_len = 0, n_long = 0, n_parts = 0;
    msmi::DevBuf row_ptr, col, val, parts, long_rows, long_first, partials;
    uint64_t bytes() const { return row_ptr.cap + col.cap + val.cap + parts.cap + long_rows.cap + long_first.cap + partials.cap; }
    void release() { *this = Matrix(); }
  };
  std::vector<Matrix> mats = std::vector<Matrix>(1);
  uint32_t spmv_short_max = 0, spmv_part_len = 0;   // msm_test_set_matvec_geometry: for matrices created afterwards; 0 = the default
  int32_t last_spmv[5] = {};        // short_max, part_len, long rows, parts, launches of the last product (msm_test_last_matvec)

  // per-group workspace: two of them, each with its own stream, so that the memory-bound sort of one
  // window group runs under the ALU-bound accumulation of the other
  // (its device buffers are named ONCE, here: the members and for_each_buffer both come from this list)
#define MSM_WS_BUFFERS(X)                                                                                                            \
  X(dig) X(counts) X(cursor) X(tail_off) X(info) X(slots) X(block_hist) X(scan_partial) X(desc) X(columns2) X(rows_sum) X(bucket_proj) \
  X(bufA) X(bufB) X(scratch) X(columns) X(partials) X(part) X(dig2) X(idx2) X(rec) X(blk_tab2) X(slots2) X(dest) X(rows1) X(parts) X(sub)
  struct Workspace {
#define MSM_WS_MEMBER(NAME) msmi::DevBuf NAME;
    MSM_WS_BUFFERS(MSM_WS_MEMBER)
#undef MSM_WS_MEMBER
#define MSM_WS_VISIT(NAME) fn(NAME);
    template <class Fn> void for_each_buffer(Fn&& fn) { MSM_WS_BUFFERS(MSM_WS_VISIT) }
#undef MSM_WS_VISIT
    msmi::Stream stream;
    msmi::Stream side;            // read-backs that the host needs while `stream` goes on (the sort's totals under its last pass)
    msmi::Event ev[8];            // (ev[7]: the scans of the bucket sizes are done)
    msmi::Pinned<uint32_t> h_info;   // 64 words
    msmi::Pinned<uint32_t> h_part;   // window sums read-back
  };
  static constexpr int N_WS = 2;
  Workspace ws[N_WS];

  msm_host::Curve6 hc;
  msm_host::Fe6 k_dev_to_host;  // 2^(2 * 64 nl_host - 30 NL): device Montgomery (radix 2^(30 NL)) -> host Montgomery (2^384 or 2^256)
  msm_host::TeCurve6 hte;       // Ed-on-BLS12-377 over the 253-bit field (same 6-limb host field code)
  msm_host::Fe6 k_te_to_host;   // 2^(512 - 270): device Montgomery (2^270) -> host Montgomery (2^256: four active limbs)
  bool is_te() const { return curve == MSM_CURVE_ED_ON_BLS12_377; }
  // per-field sizes (the reference sizes limbs per field, src/parallel.ts:53-57): 30-bit limbs in registers, packed words
  // per coordinate in memory, and the coordinate bytes at the ABI (wire points, results, test operands)
  int nl() const { return msmi::curve_info(curve).nl; }
  int nw() const { return msmi::curve_info(curve).nw; }
  size_t coord_bytes() const { return (size_t)nw() * 4; }
  uint64_t row_words() const { return is_te() ? (uint64_t)msm::te::TE_ROW_WORDS : (uint64_t)msm::ROW_WORDS; }   // of a point row
  int sum_words() const { return is_te() ? msmi::TE_SUM_WORDS : msmi::W_SUM_WORDS; }                            // of a window-sum slot

  void ensure(msmi::DevBuf& b, size_t bytes) { b.ensure(bytes); }
  void release(msmi::DevBuf& b) { b.release(); }
  // bytes the workspaces hold: what a new budget may count on beside the device's free memory
  uint64_t workspace_bytes() {
    uint64_t held = 0;
    for (auto& w : ws) w.for_each_buffer([&](msmi::DevBuf& b) { held += b.cap; });
    return held;
  }

  // What must happen in order: no thread of the context runs any more, and every stream that exists is idle.  The members free
  // everything else.  (Children go first, by msm_ctx_destroy.)  A context that never created a stream makes no HIP call.
  ~msm_ctx() {
    fan.clear();
    helper.reset();
    if (!stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    for (auto& w : ws) {
      if (w.stream) (void)hipStreamSynchronize(w.stream);
      if (w.side) (void)hipStreamSynchronize(w.side);
    }
    for (auto& st : stage_stream) if (st) (void)hipStreamSynchronize(st);
  }
};

// curve dispatch for the templated Weierstrass kernels
template <class Fn>
inline void for_weierstrass_curve(int curve, Fn&& fn) {
  switch (curve) {
#define MSM_DISPATCH_CASE(ID, CV) case ID: fn(msm::CV{}); break;
    MSM_W_CURVES(MSM_DISPATCH_CASE)
#undef MSM_DISPATCH_CASE
    default: throw msmi::HipFail{hipErrorInvalidValue, "Weierstrass kernel launch for a curve id outside MSM_W_CURVES", __LINE__, __FILE__};
  }
}
// curve dispatch to the SCALAR field, the integers mod the group order q (scalar_vec.h): fn(field struct) for all seven curves, the
// Edwards curve included
template <class Fn>
inline void for_scalar_field(int curve, Fn&& fn) {
  switch (curve) {
#define MSM_DISPATCH_CASE(ID, S) case ID: fn(msm::S{}); break;
    MSM_SCALAR_FIELDS(MSM_DISPATCH_CASE)
#undef MSM_DISPATCH_CASE
    default: throw msmi::HipFail{hipErrorInvalidValue, "scalar-field kernel launch for an unknown curve id", __LINE__, __FILE__};
  }
}
// the same for a body that may refuse the call: fn(field struct) returns the status, and so does this
template <class Fn>
inline int with_scalar_field(const msm_ctx* ctx, Fn&& fn) {
  int rc = MSM_OK;
  for_scalar_field(ctx->curve, [&](auto f) { rc = fn(f); });
  return rc;
}
#define W_LAUNCH(ctx, KERNEL, ...) \
  for_weierstrass_curve((ctx)->curve, [&](auto cv_) { hipLaunchKernelGGL((KERNEL<decltype(cv_)>), __VA_ARGS__); })
#define W_LAUNCH_MODE(ctx, KERNEL, MODE, ...) \
  for_weierstrass_curve((ctx)->curve, [&](auto cv_) { hipLaunchKernelGGL((KERNEL<decltype(cv_), MODE>), __VA_ARGS__); })

// point rows -> tree planes (test ops), by the packed words of the curve's coordinates
#define ROWS_TO_PLANES(ctx, ...)                                                                       \
  do {                                                                                                 \
    if ((ctx)->nw() == 8) hipLaunchKernelGGL((k_test_rows_to_planes<8>), __VA_ARGS__);                 \
    else hipLaunchKernelGGL((k_test_rows_to_planes<12>), __VA_ARGS__);                                 \
  } while (0)

namespace msmi {
using namespace msm;

int fail(msm_ctx* ctx, int code, const char* fmt, ...);
int fail_hip(msm_ctx* ctx, const HipFail& f);

// the first resident point a call covers: its points are [point_lo, point_lo + n)
inline uint64_t point_lo(const msm_opts* opts) { return opts ? opts->point_lo : 0; }
// MSM_OK if the points of the call are resident (and there are some, unless empty_ok); otherwise fails it with `code`
int check_points(msm_ctx* ctx, uint64_t n, const msm_opts* opts, int code, const char* who, bool empty_ok = true);
// MSM_ERR_ARG if `opts` asks for a shard of the call -- window shards, bucket shards, merged sums, by_window; no_point_lo: a range of
// the points too -- which the entry point `who`, `kind` of call ("a narrow", "an indexed", "a batch"), does not run
int refuse_shard_opts(msm_ctx* ctx, const msm_opts* opts, const char* who, const char* kind, bool no_point_lo = false);

// every extern "C" entry point ends its try block with this: no C++ exception crosses the C ABI
#define MSM_CATCH_ALL(ctx)                                                                                  \
  catch (const HipFail& f) { return fail_hip(ctx, f); }                                                     \
  catch (const MsmFail& f) { return fail(ctx, f.code, "%s", f.msg.c_str()); }                               \
  catch (const std::bad_alloc&) { return fail(ctx, MSM_ERR_INTERNAL, "host memory allocation failed"); }    \
  catch (const std::exception& e) { return fail(ctx, MSM_ERR_INTERNAL, "unexpected exception: %s", e.what()); } \
  catch (...) { return fail(ctx, MSM_ERR_INTERNAL, "unexpected exception"); }

// ---- msm_plan.hip -----------------------------------------------------------------------------------------------
int pick_window(bool te, uint64_t n, int glv_max_bits);

struct Plan {
  int c, K, L_log;       // c: bits a window advances by (the weight of window k is 2^(c k)); L_log: bits of a bucket index
  int bits = 0;          // b + 1: scalar bits the windows cover (the top window holds bits - (K - 1) c of them)
  bool fold = false;     // the top window is c + 1 bits wide (see make_plan)
  uint32_t L;            // buckets per window = 2^L_log
  bool no_glv;
  bool strict = false;   // msm_opts.strict: scalars >= q fail the call instead of being reduced
  bool lone = false;   // one window, one group: nothing else shares the GPU (see round_geom)
  uint32_t b_lo = 0, b_n = 0xFFFFFFFFu;   // bucket-range shard (msm_opts.bucket_shard): bucket indices [b_lo, b_lo + b_n) only;
  uint32_t bt_lo = 0, bt_n = 0xFFFFFFFFu; // the top window's range (its digits cover another span than the recoded windows')
  bool tables = false; // the call runs on window tables (msm_tables.hip): the windows of a group share one set of buckets, a
                       // group hands back ONE sum that already carries the windows' weights
  const uint32_t* tab_rows = nullptr;   // tables: first row of table 0; its tables are tab_n rows each and cover the points
  uint64_t tab_lo = 0, tab_n = 0;       //         [tab_lo, tab_lo + tab_n)
  int tab_T = 0;                        //         tables held: a window group on them has at most that many windows
  bool merged = false; // a full MSM (msm_run): a window group may hand back sum_k 2^(c (k - k_first)) P_k in the slot of its
                       // first window instead of one P_k per slot (reduce_buckets); msm_window_sums never sets it
  int batch = 0;       // msm_run_batch (msm_batch.hip): the group's windows are those of `batch` elements, K each (window
  BatchScalars batch_sc{};   // kk = virtual window b K + k), their digits come from k_digits_batch over batch_sc
  // msm_run_narrow (msm_narrow.hip): width != 0 -- the scalars are width-byte integers (32: field elements holding small
  // values) of `fmt.bits` magnitude bits, their digits come from k_digits_narrow.  The scalar pointer a window group gets is
  // then the array of the whole CALL, rounded down to the alignment of a lane's load, and scalar `first` + i belongs to the
  // group's point i (a range of the points may start inside a lane's dword).  nb: the scalars of a fused batch.
  struct Narrow {
    int width = 0;
    uint64_t first = 0;
    NarrowFmt fmt{};
    const NarrowBatchScalars* nb = nullptr;
  } nar;
  // msm_run_indexed (msm_indexed.hip): idx != nullptr -- scalar j of the call belongs to resident point idx[j] (device array of
  // the whole CALL, checked against the resident count before the run).  Digits, sort and pairing run over the call's positions;
  // the payloads of a window group are rewritten to name resident rows before round 1 gathers (run_window_group).
  const uint32_t* idx = nullptr;
};

// for_tables: the window a run on window tables wants (bucket work no longer grows with the number of windows)
// narrow_bits > 0: the plan of a narrow call -- b = narrow_bits instead of the curve's scalar length, no endomorphism split,
// the window from pick_window_narrow, c down to 2
int make_plan(const msm_ctx* ctx, uint64_t n, const msm_opts* opts, Plan& pl, bool for_tables = false, int narrow_bits = 0);
// one_level: the window of a fused batch, which must stay within the one-level sort (msm_batch.hip)
int pick_window_narrow(bool te, uint64_t n, int bits, bool one_level = false);
// the plan of msm_run(n, opts) -- on window tables where the call is eligible and they exist or would be built -- and whether
// it is that plan (msm_tables.hip)
// note_range: the call is real (not msm_plan): a range of the points it asks for is remembered as the candidate for range tables
int make_run_plan(msm_ctx* ctx, uint64_t n, const msm_opts* opts, bool placed, Plan& pl, bool& tables_wanted, bool note_range = false);

// Window groups a call over n points and nwin windows runs as where nothing else (workspace budget, sort limits) asks for more.
// The schedule (group_schedule) and the build of window tables, which holds ceil(K / groups) of them, both ask here.
// Measured on MI355X: two groups win 14 % at 2^23 / 2^24, 3 % at 2^22, nothing at 2^21 -- below that the fixed per-group
// latencies (read-backs, bucket reduction depth) cost more than the overlap returns
// (on window tables from 2^21: 5.87 -> 5.73 ms, Edwards 3.96 -> 3.72; the plain path at 2^21 prefers one group, 6.71 / 6.88; at
// 2^20 one group wins on tables too, 3.24 / 3.33 -- round 5, tools/knob_sweep.sh MSM_GROUPS)
// (round 6: the Edwards path on tables from 2^20 -- fifteen digit windows in one group leave the chip to one stream's ramps:
// 2.19 - 2.24 -> 2.13 - 2.18 ms; BLS12-377 at 2^20 is level, 3.44 / 3.41, and stays on one group)
inline int window_groups_wanted(bool te, uint64_t n, bool tables, int nwin) {
  return (nwin >= 2 && (n >= (1ull << 22) || (tables && n >= (te ? 1ull << 20 : 1ull << 21)))) ? 2 : 1;
}
// entries per window from which the sort leaves its one-level form for the radix split; callers that depend on the one-level
// sort -- 128 windows in a group, a fused batch -- ask here
// measured (round 5, with one ds_add per key as the ranking: tools/sortpath_sweep.sh): the split wins from 2^21 entries per
// window -- 2^20 points: sort 0.31 against 0.36 ms, 2^21: 0.51 / 0.85; 2^19: level, below: the one-level sort (2^16 0.11 / 0.14)
inline uint64_t one_level_entry_limit(bool te) { return te ? 1ull << 22 : 1ull << 21; }
// a window's counters fit the LDS of the one-level and radix sorts (c <= 16)
inline bool window_fits_lds(const Plan& pl) { return (size_t)pl.L * 4 <= 128 * 1024; }
// May a window of `entries` entries under this plan leave the one-level sort for one that describes its windows in a WinSplit
// of 16 entries?  The ONE statement of the rule: group_schedule caps such a group at 16 windows, sort_geometry picks the path.
inline bool leaves_one_level(bool te, const Plan& pl, uint64_t entries) {
  return !window_fits_lds(pl) || (pl.L_log > (int)RX_FINE_BITS && entries >= one_level_entry_limit(te));
}

struct GroupStats {
  uint64_t n_pairs = 0;
  uint64_t n_pairs_algo = 0;
  uint64_t max_bucket = 0;
  int rounds = 0;
  float ms_digits = 0, ms_sort = 0, ms_acc = 0, ms_red = 0, ms_r1 = 0;
  // the groups of a call: everything adds up (tree rounds of ALL window groups, like n_pairs and ms_acc) but the largest bucket
  GroupStats& operator+=(const GroupStats& o) {
    n_pairs += o.n_pairs;
    n_pairs_algo += o.n_pairs_algo;
    max_bucket = std::max(max_bucket, o.max_bucket);
    rounds += o.rounds;
    ms_digits += o.ms_digits; ms_sort += o.ms_sort; ms_acc += o.ms_acc; ms_red += o.ms_red; ms_r1 += o.ms_r1;
    return *this;
  }
};

// launch geometry of one tree round
struct RoundGeom {
  uint32_t steps, grid;
  uint64_t T;
};

RoundGeom round_geom(const msm_ctx* ctx, uint64_t n_out, bool gather = false, bool lone = false);
void release_workspaces(msm_ctx* ctx);   // drops every per-call buffer of both window-group workspaces (they only grow otherwise)
long double window_bytes(const msm_ctx* ctx, uint64_t n, const Plan& pl);
int windows_per_group(const msm_ctx* ctx, uint64_t n, const Plan& pl);
uint64_t point_pieces(const msm_ctx* ctx, uint64_t n, const Plan& pl);

// How one call -- windows [k_lo, k_hi) over n points -- is cut into window groups and ranges of the points: every (window, point)
// pair lies in exactly one group.  The runner (window_sums_once) takes the groups in order, two at a time on the two workspaces.
struct GroupSchedule {
  struct Group {
    int ka, kb;            // windows [ka, kb)
    uint64_t p_lo, p_n;    // points [p_lo, p_lo + p_n) of the call
    int piece;             // pipelined upload: the piece whose arrival the group waits for (-1: the scalars are in place)
  };
  std::vector<Group> groups;
  int wpg = 1;               // windows per group as capped; the Horner step of a run on tables uses c * wpg
  bool tables = false;       // the plan's window tables survive the cut
  bool split_points = false; // several groups contribute to one window: the sums of its ranges are added on the host
  bool piped = false;        // the pipelined upload survives (it does not when the workspace forces its own ranges)
  bool share_digits = false; // one launch of the digit kernel serves both groups (GroupDigits)
  bool lone = false;         // every launch has the chip to itself (Plan.lone)
};
// The schedule of a call: plain arithmetic over the plan, the shape of the call and the context's n_cu and ws_budget -- no HIP
// call, no allocation, no write to the context.  p_off: first resident point of the call; piece_end: the piece ends of host
// scalars that would cross PCIe behind the computation (pipelined_piece_ends; empty: the scalars are staged); serial:
// msm_opts.serial.
GroupSchedule group_schedule(const msm_ctx* ctx, uint64_t n, uint64_t p_off, int k_lo, int k_hi, const Plan& pl,
                             const std::vector<uint64_t>& piece_end, bool serial);

// ---- msm_reduce.hip ---------------------------------------------------------------------------------------------
void words_to_fe6(msm_host::Fe6& r, const uint32_t* w, int nw = 12);
void fe6_to_bytes(uint8_t* out, const msm_host::Fe6& a);
// one packed coordinate of nw words in device Montgomery form -> its value as 4 nw little-endian bytes; k_to_host: the
// context's k_dev_to_host (F = hc.F) or k_te_to_host (F = hte.F)
void device_coord_to_wire(const msm_host::Field6& F, const msm_host::Fe6& k_to_host, const uint32_t* w, int nw, uint8_t* out);
void plane_element_to_wire(const msm_ctx* ctx, const uint32_t* planes, uint64_t cap, uint64_t e, uint8_t* out_xy);
// P_k = sum_l l B_(k,l) of kc windows of L buckets (a power of two) over the bucket sums of finish_buckets -> kc slots on the host
void reduce_buckets(msm_ctx* ctx, msm_ctx::Workspace& w, const uint32_t* bucket_proj, uint32_t L, int kc, uint32_t* h_partials_out,
                    bool merged = false, int stride = 0, uint32_t tc_force = 0);
// The host tail: what happens to window sums between the bucket reduction and the caller.  A slot is ctx->sum_words() words;
// `words` are K slots in a row.  These read the context's curve constants only, so any number of host threads may call them.
void sum_set_identity(const msm_ctx* ctx, uint32_t* slot);
// out = the sum of the slots of `parts` as group elements (none: the identity); out may be one of them
void sum_slots(const msm_ctx* ctx, const std::vector<const uint32_t*>& parts, uint32_t* out);
// out_slot = sum_k 2^(c k) words[k] (src/msm-batched-affine.ts:322-333)
void sums_horner(const msm_ctx* ctx, const uint32_t* words, int K, int c, uint32_t* out_slot);
// the same sum as the canonical affine point: x, y and is_infinity of `out`
void sums_finish(const msm_ctx* ctx, const uint32_t* words, int K, int c, msm_result* out);
// the result of an MSM over no points: infinity on a Weierstrass curve, the affine point (0, 1) on the Edwards curve
void identity_to_result(const msm_ctx* ctx, msm_result* out);
// slot -> X || Y || Z, SUM_WIRE_BYTES of canonical integers (slot = nullptr, or Z = 0 on a Weierstrass curve: the identity)
void sum_to_wire(const msm_ctx* ctx, const uint32_t* slot, uint8_t* out);
const msm_host::Curve6* static_host_curve(int curve);
int combine_impl(msm_ctx* ctx, const msm_host::Curve6& C, const uint8_t* partials, int32_t K, int32_t c, msm_result* out, int32_t G);
int te_combine_impl(const uint8_t* partials, int32_t K, int32_t c, msm_result* out, int32_t G = 1);

// ---- msm_sort.hip / msm_tree.hip: the two halves of one window group --------------------------------------------
// what the sort of a window group leaves behind for its tree
struct SortOut {
  uint32_t logG = 1;            // buckets are padded to multiples of 2^logG slots
  int RT = 0;                   // tail rounds the largest bucket would need
  uint64_t total_slots = 0;
  uint32_t max_bucket = 0;
  const uint32_t* round1_slots = nullptr;   // pairs round 1 walks (bucket order, or the tile order of k_bin_pairs)
  const uint32_t* round1_dest = nullptr;    // tile order: the element index every pair's sum belongs to
  uint64_t rec_y_off = 0;       // 12-word fields: where the y records of round 1's results start inside w.rows1
  bool chunked = false;         // round 1 walks tile-ordered pairs and writes element records, round 2 reads them
  int path = MSM_SORT_ONE_LEVEL;   // the sort path taken (MSM_SORT_*, include/msm_hip.h): what msm_test_last_sort_paths reports
};
// The geometry of the sort of windows [k_lo, k_hi) over n points: every size, cut and path choice sort_window_group acts on,
// from sort_geometry (msm_plan.hip) -- plain arithmetic like group_schedule, checked on the CPU by tests/test_sort_geometry.py.
struct SortGeometry {
  int kc_d = 0, kc = 0;            // windows the digit kernel slices; windows behind it (on window tables ONE: the digit array
  uint64_t two_n_d = 0, two_n = 0; //   [kc_d][two_n_d] read as one run of entries); entries per digit window / per window
  uint64_t n_entries = 0, nb = 0;  // entries and buckets of the group
  uint64_t mean = 1;               // mean bucket population the padding granule is sized from
  uint32_t logG = 1;               // buckets are padded to multiples of 2^logG slots
  // the path as intended before the read-back: neither flag = the one-level sort; pairs: the bin split ends in the pair form
  // (k_bin_pairs) and round 1 walks tile-ordered pairs, otherwise in bucket-ordered slots (k_bin_slots)
  bool bin_split = false, radix = false, pairs = false;
  WinSplit ws{};                   // coarse and fine bits of every window (bin split, radix split)
  uint32_t hb = 1;                 // bin split: coarse bins per window of THIS group's windows; V counts with it
  uint32_t hb_stride = 1;          // ... and the stride of the bin tables and slice histograms: hb, unless the group consumes the
                                   // digits of a producer that sliced wider windows too (sort_window_group takes the producer's)
  uint32_t nbmax = 1;              // bin split: most buckets of one bin
  uint32_t Hn = 1;                 // radix split: coarse bins = blocks of its last pass per window
  uint32_t V = 0;                  // bins of the group
  uint32_t sortB = 1;              // slices: block (b, kk) of the histogram and of the first pass owns entries
  uint64_t pps = 0, chunk = 0;     //   [b * chunk, (b + 1) * chunk) of window kk; pps: points per slice
  uint32_t per_block = 1;          // bin split: consecutive slices one block of pass A takes
  uint32_t part_len = 0, part_grid = 0;   // bin split: records per part of a heavy bin; blocks of the count and last passes
  uint64_t parts_extra = 0;        // pair form: slots the parts of heavy bins may add
  uint64_t slots_bound = 0;        // bound of the padded slots, known before the read-back
  // bin split: every window's digits span all L = 2^cbits buckets at the tables' stride (else `counts` is cleared first)
  bool spans_all(int cbits) const {
    bool all = true;
    for (int kk = 0; kk < kc; kk++) all &= (1u << ws.ab[kk]) == hb_stride && (int)ws.ab[kk] + (int)ws.fb[kk] == cbits;
    return all;
  }
  // the geometry of digits that nothing sorts (msm_test_digits of a fused batch): the digit array and no cuts
  static SortGeometry digits_alone(int kc_d, uint64_t two_n_d) {
    SortGeometry g;
    g.kc_d = g.kc = kc_d;
    g.two_n_d = g.two_n = two_n_d;
    g.n_entries = (uint64_t)kc_d * two_n_d;
    return g;
  }
};
// Reads ctx->is_te(), n_cu and chunk_rows_log; no HIP call, no allocation, no write to the context.  Throws MsmFail for a group
// the sorts cannot describe (more than 16 windows off the one-level sort, a window too wide for the bin split).
SortGeometry sort_geometry(const msm_ctx* ctx, uint64_t n, const Plan& pl, int k_lo, int k_hi);
// The two decisions that wait for the read-back (max_bucket, total_slots).
// Radix split: its last pass gives one block to a coarse bin, and a bucket that holds far more than a bin's share of the entries
// (one scalar repeated: a whole window in one bucket) would make one block walk them all.  The histogram is the one-level
// sort's, so such an input takes the one-level scatter instead, which splits the ENTRIES across the blocks (its partial-line
// writes do not matter when most payloads go to a few long runs): one scalar repeated at 2^20 points, sort phase 1.39 -> 0.4x ms.
inline bool radix_bucket_too_heavy(const SortGeometry& g, uint32_t max_bucket) {
  return max_bucket >= (1u << 16) && (uint64_t)max_bucket * g.Hn >= 16 * g.two_n;
}
// Pair form: no entry at all -- the plain slot form handles the empty tree.
inline bool pair_form_tree_empty(uint64_t total_slots) { return total_slots < 2; }

// Digits and slice histograms that are already there: written by launch_group_digits, for the group itself or -- the two groups
// of a call decompose the same scalars: one GLV decomposition instead of two -- for SEVERAL window groups at once, each of which
// then takes its part of the arrays (bin split only) instead of slicing the scalars again.
struct GroupDigits {
  int k_lo = 0;                   // first window of the arrays
  const uint32_t* dig = nullptr;  // [windows][entries per window]
  uint32_t* hist = nullptr;       // [windows][sortB][hb]; null off the bin split
  uint32_t hb = 0, sortB = 0;
  uint64_t pps = 0, chunk = 0;
  hipEvent_t ready = nullptr;     // behind the digit kernel, on the producing workspace's stream (null: not recorded)
  bool valid = false;
};
// The digit launch of windows [k_lo, k_lo + g.kc_d) on w.stream, into w.dig and (bin split) w.block_hist, which it sizes: the
// wide kernels, those of a narrow call, or the _batch forms of a fused batch, as the plan says.  Records `ready` behind it if given.
GroupDigits launch_group_digits(msm_ctx* ctx, msm_ctx::Workspace& w, const uint32_t* d_scalars, uint64_t n, const Plan& pl, int k_lo,
                                const SortGeometry& g, hipEvent_t ready = nullptr);
// share: digits of this group's windows that a launch over several groups has left (valid); the group takes its part
void sort_window_group(msm_ctx* ctx, msm_ctx::Workspace& w, const uint32_t* d_scalars, uint64_t n, const Plan& pl, int k_lo, int k_hi,
                       GroupStats& st, SortOut& so, const GroupDigits* share = nullptr);
// The scans behind the sort, which sort_window_group and the operator test msm_test_tree_sums both run: the nb bucket sizes in
// w.counts -> w.cursor (padded slot offsets, nb + 1 words), w.tail_off (RT + 1 tables of nb + 1 words) and the totals in w.info.
// find_max: clears w.info and looks for the largest bucket first (k_bucket_max); otherwise info[1] holds it already, or a bound
// on it.  Queued on w.stream; records w.ev[7] behind the last scan.
void scan_bucket_sizes(msm_ctx* ctx, msm_ctx::Workspace& w, uint64_t nb, uint32_t logG, bool find_max);
// the ONE read-back of w.info behind the scans, on w.side while w.stream goes on: the launch geometry of the tree
struct ScanTotals {
  uint64_t total_slots = 0;
  uint32_t max_bucket = 0;
  int RT = 0;                 // tail rounds the largest bucket would need: 2^RT >= ceil(max_bucket / 2^logG)
  uint64_t algo_pairs = 0;    // sum over the non-empty buckets of (size - 1)
};
ScanTotals read_scan_totals(msm_ctx::Workspace& w, uint32_t logG);
// what the tree leaves behind for the bucket reduction
struct TreeOut {
  const uint32_t* bucket_proj = nullptr;   // one bucket sum per bucket from k_bucket_finish (projective / extended, raw limbs)
};
// the round plan as it ran, for msm_test_tree_sums (normal calls pass no log)
struct TreeLog {
  int r_stop = 0;             // tail rounds run
  struct Round {
    int mode;                 // MODE_GATHER / MODE_REGULAR / MODE_SEARCH
    uint64_t n_out;
    uint32_t steps;
  };
  std::vector<Round> rounds;  // one per launched round, in launch order
};
// kc: windows of the group as the tree sees them (1 on window tables); row_off: first row of the point table the payloads count from
// (0 on window tables: every group reads them from table 0)
void accumulate_window_group(msm_ctx* ctx, msm_ctx::Workspace& w, const Plan& pl, int kc, uint64_t row_off, const SortOut& so,
                             GroupStats& st, TreeOut& to, TreeLog* log = nullptr);
// bytes of w.bucket_proj for nb buckets: a projective (Edwards: extended) point of raw limbs each
inline size_t bucket_proj_bytes(const msm_ctx* ctx, uint64_t nb) { return nb * (ctx->is_te() ? 4 * te::TL : 3 * NL) * 4; }
// the last step of accumulate_window_group, which the operator test msm_test_bucket_sums runs on buckets of its own (msm_tree.hip)
const uint32_t* finish_buckets(msm_ctx* ctx, msm_ctx::Workspace& w, const uint4* fin, uint64_t fin_cap, const uint32_t* off_fin,
                               uint64_t nb, const uint32_t** perm_out = nullptr);
void sort_kernel_attributes();   // dynamic-LDS limits of the sort kernels (once per process and device)

// ---- msm_tables.hip ---------------------------------------------------------------------------------------------
// true if the MSM over the resident points [opts->point_lo, + n) under plan `pl` can run on window tables, built here if they
// are not there yet and may be -- `pl` then knows where they are (tab_rows, tab_lo, tab_n)
bool use_window_tables(msm_ctx* ctx, uint64_t n, const msm_opts* opts, Plan& pl);

// ---- msm_upload.hip ---------------------------------------------------------------------------------------------
void ensure_staging(msm_ctx* ctx);
void upload_staged(msm_ctx* ctx, void* dst, const void* src, size_t bytes);
int stage_scalars(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const uint32_t** d_out);
// The same staged transfer running BEHIND the call that consumes it: a host scalar buffer of a big MSM crosses PCIe in the
// background while the MSM already runs over the ranges of the points ("pieces") whose scalars have arrived -- 2 GB take
// ~45 ms at the rate of the link, a 2^26 MSM ~150 ms, and the sort of a window needs every digit of its range, so the
// unit of overlap is a range of the points, not a chunk (pipelined_piece_ends picks growing ranges: the first one is small so the
// GPU starts early, the last one is half the input so most of the work runs at full-size efficiency).
// Chunks go out in address order over the staging threads as in upload_staged; when a thread has queued its last chunk of
// piece q it records piece_ev[q][t] on its copy stream, and wait_piece(q, stream) makes `stream` wait for all of them.
// The reference's counterpart is scalarsFromBytes into shared wasm memory before the call, src/parallel.ts:119-133.
// Host scalars are pipelined from 2^24 points; the ranges end at 1/16, 3/16 and the rest from 2^25 points, 1/8, 3/8 and the
// rest below, rounded down to whole staging chunks: the link moves scalars ~4x as fast as the GPU consumes them (2 GB in ~40 ms
// against ~154 ms of MSM at 2^26), so every range may be ~4x its predecessor and still arrive before the GPU is done with the
// one before.  The first range is what the GPU waits for (2-3 ms); few ranges keep the sub-MSMs near full-size efficiency.
inline bool pipelines_host_scalars(uint64_t n) { return n >= (1ull << 24); }
inline std::vector<uint64_t> pipelined_piece_ends(uint64_t n) {   // point index where piece q ends (the last = n)
  const uint64_t gran = msm_ctx::STAGE_CHUNK / 32;   // scalars per staging chunk
  const int big = n >= (1ull << 25);
  return {((n >> (big ? 4 : 3)) / gran) * gran, ((n >> (big ? 2 : 1)) / gran) * gran, n};
}
class PieceUpload {
 public:
  static constexpr int T = msm_ctx::STAGE_THREADS, S = msm_ctx::STAGE_SLOTS;
  static constexpr size_t CH = msm_ctx::STAGE_CHUNK;
  PieceUpload(msm_ctx* ctx, void* dst, const void* src, size_t bytes, const std::vector<size_t>& piece_end_bytes)
      : ctx_(ctx), dst_((char*)dst), src_((const char*)src), bytes_(bytes), ends_(piece_end_bytes), enq_(piece_end_bytes.size(), 0) {
    ensure_staging(ctx);
    n_streams_ = std::max<long long>(1, std::min<long long>(n_streams_, T));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // dst may still be in use by what the stream holds
    for (int t = 0; t < T; t++) HIPCHK(hipStreamSynchronize(ctx->stage_stream[t]));
    for (int t = 0; t < T; t++) rc_[t] = hipSuccess;
    t0_ = std::chrono::steady_clock::now();
    th_.reserve(T);
    try {
      for (int t = 0; t < T; t++) {
        // a thread that cannot be started (resource limits) must not leave the others unjoined: its share runs here
        try { th_.emplace_back([this, t] { run(t); }); } catch (const std::system_error&) { run(t); }
      }
    } catch (...) {   // anything else: the destructor of a half-built object does not run, so the started threads are joined here
      join();
      throw;
    }
  }
  ~PieceUpload() { join(); }
  // host: blocks until every staging thread has queued its part of piece q; device: `stream` then waits for those copies
  void wait_piece(int q, hipStream_t stream) {
    {
      std::unique_lock<std::mutex> l(mu_);
      cv_.wait(l, [&] { return enq_[q] == T; });
    }
    hipError_t rc[T];
    {
      std::lock_guard<std::mutex> l(mu_);   // the staging threads write rc_ under the mutex
      for (int t = 0; t < T; t++) rc[t] = rc_[t];
    }
    for (int t = 0; t < T; t++) {
      if (rc[t] != hipSuccess) throw HipFail{rc[t], "staged upload of the scalars", __LINE__, __FILE__};
      HIPCHK(hipStreamWaitEvent(stream, ctx_->piece_ev[q][t], 0));
    }
  }
  // joins the staging threads, waits for the last copy and returns the wall time of the whole transfer in ms
  float finish() {
    join();
    for (int t = 0; t < T; t++) HIPCHK(rc_[t]);
    for (int t = 0; t < T; t++) HIPCHK(hipStreamSynchronize(ctx_->stage_stream[t % n_streams_]));
    return ms_;
  }

 private:
  void join() {
    for (auto& x : th_) if (x.joinable()) x.join();
  }
  void run(int t) {
    hipError_t e = hipSetDevice(ctx_->device);
    const size_t n_chunks = (bytes_ + CH - 1) / CH;
    size_t turn = 0;
    int q = 0;
    auto mark = [&](int upto) {   // this thread has nothing more to send for the pieces below `upto`
      for (; q < upto; q++) {
        if (e == hipSuccess) e = hipEventRecord(ctx_->piece_ev[q][t], ctx_->stage_stream[t % n_streams_]);
        std::lock_guard<std::mutex> l(mu_);
        rc_[t] = e;
        enq_[q]++;
        cv_.notify_all();
      }
    };
    for (size_t i = t; i < n_chunks && e == hipSuccess; i += T, turn++) {
      const size_t off = i * CH, len = std::min(CH, bytes_ - off);
      int upto = q;
      while (upto < (int)ends_.size() && ends_[upto] <= off) upto++;   // pieces that end at or before this chunk
      mark(upto);
      const int slot = (int)(turn % S);
      char* pin = ctx_->stage_pin + ((size_t)t * S + slot) * CH;
      if (turn >= (size_t)S) e = hipEventSynchronize(ctx_->stage_ev[t][slot]);
      if (e != hipSuccess) break;
      memcpy(pin, src_ + off, len);
      e = hipMemcpyAsync(dst_ + off, pin, len, hipMemcpyHostToDevice, ctx_->stage_stream[t % n_streams_]);
      if (e == hipSuccess) e = hipEventRecord(ctx_->stage_ev[t][slot], ctx_->stage_stream[t % n_streams_]);
    }
    mark((int)ends_.size());   // on an error too: nobody may wait for ever
    if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stage_stream[t % n_streams_]);
    std::lock_guard<std::mutex> l(mu_);
    rc_[t] = e;
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0_).count();
    ms_ = std::max(ms_, ms);
  }
  msm_ctx* ctx_;
  char* dst_;
  const char* src_;
  size_t bytes_;
  std::vector<size_t> ends_;   // byte offset where piece q ends (multiples of the chunk size, the last = bytes)
  std::vector<int> enq_;
  hipError_t rc_[T];
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::chrono::steady_clock::time_point t0_;
  float ms_ = 0;
  long long n_streams_ = 2;   // copy streams the staging threads queue their chunks on (measured: 1, 2, 4 alike; 2 steadiest)
};

// ---- msm_pipeline.hip -------------------------------------------------------------------------------------------
int window_sums_impl(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, int k_lo, int k_hi,
                     const Plan& pl, std::vector<uint32_t>& words, msm_result* stats, uint64_t p_off = 0);
int any_window_sums(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, const msm_opts* opts, int k_lo, int k_hi,
                    const Plan& pl, std::vector<uint32_t>& words, msm_result* stats, const void* const* placed = nullptr);

// the scalars of the points [p_lo, ...) of a call: 32-byte scalars are addressed; narrow ones (msm_run_narrow) keep the call's
// array and count from `first`, which the digit kernel resolves (a range may start inside the dword a lane loads)
const uint32_t* group_scalars(const uint32_t* d_scalars_all, uint64_t p_lo, Plan& pl);
// The two-stream runner of a call: job(slot, i) for i = 0 .. n_jobs - 1, each on one of the context's two workspaces (slot), the
// second worker on the context's helper thread unless `serial`.  Whatever a job throws is re-raised only after both workers have
// stopped and both group streams are idle.
void run_on_workspaces(msm_ctx* ctx, int n_jobs, bool serial, const std::function<void(int slot, int index)>& job);
// adds the five intervals between the events a window group has recorded on w (sort_window_group .. reduce_buckets) to st
void add_group_times(const msm_ctx::Workspace& w, GroupStats& st);
// phases (digits .. reduce), pairs, rounds and the largest bucket of a call's window groups -> its msm_result
void stats_to_result(const GroupStats& st, msm_result* r);
// tot += the statistics of one call of several that make up an entry: phases, pairs and rounds add up, the largest bucket is
// the largest; side_by_side (the devices of a multi-device call) takes the longest of every phase instead of their sum
void add_call_stats(msm_result& tot, const msm_result& r, bool side_by_side = false);
// error word of the digit kernels (ctx->errflag) after the window groups of a call: throws what the plan does not tolerate.
// `who`: the narrow entry point (it alone declares a range)
constexpr uint32_t ERR_SCALAR_GE_Q = 4u, ERR_FOLD_DIGIT = 8u;   // (bits 1 and 2: the point loaders; NARROW_ERR_RANGE: narrow_kernels.h)
void check_scalar_flags(msm_ctx* ctx, const Plan& pl, const char* who);
// The two ends of every entry point that returns one MSM (msm_run, msm_run_narrow, msm_run_indexed, msm_run_indexed_narrow).
// call_begin: the plan is that of a full MSM (Plan.merged), the result is zeroed and told c and K; an empty call is answered
// with the identity.  Returns whether anything is left to run.
bool call_begin(const msm_ctx* ctx, Plan& pl, uint64_t n, msm_result* out);
// call_finish: the window sums `words` (K slots) -> the affine result, timed as MSM_T_FINAL and added to MSM_T_TOTAL.
// staging_ms >= 0: the entry staged its own input in front of the window sums -- that interval is its MSM_T_UPLOAD and part of its
// total; otherwise the upload time the window sums measured stays.
void call_finish(msm_ctx* ctx, const std::vector<uint32_t>& words, const Plan& pl, msm_result* out, float staging_ms = -1);

// runs f(child) for every child of a multi-device context on the fan-out threads, and f(ctx) on the calling thread;
// returns the first error code
template <class F>
int on_all_devices(msm_ctx* ctx, F f) {
  const int nch = (int)ctx->children.size();
  std::vector<int> rc(nch + 1, MSM_OK);
  // The fan-out jobs write into this frame: whatever the caller's own leg or a wait() throws, every job is waited for
  // before the frame unwinds (the first exception is re-raised afterwards).
  std::exception_ptr err;
  for (int i = 0; i < nch; i++) ctx->fan[i]->run([&, i] { rc[i + 1] = f(ctx->children[i]); });
  try { rc[0] = f(ctx); } catch (...) { err = std::current_exception(); }
  for (int i = 0; i < nch; i++) {
    try { ctx->fan[i]->wait(); } catch (...) { if (!err) err = std::current_exception(); }
  }
  if (err) std::rethrow_exception(err);
  for (int i = 0; i <= nch; i++)
    if (rc[i] != MSM_OK) {
      if (i > 0) ctx->err = ctx->children[i - 1]->err;
      return rc[i];
    }
  return MSM_OK;
}

// ---- msm_batch.hip ----------------------------------------------------------------------------------------------
int pick_window_batch(bool te, uint64_t n, uint32_t B, int glv_max_bits);
// The scalars of the B elements of a fused batch on the device: device pointers as they are; host arrays uploaded into
// ctx->scal one behind the other, every element on a 16-byte boundary (narrow elements: n x width bytes each).
std::vector<const uint32_t*> stage_batch_scalars(msm_ctx* ctx, const void* const* scalars, uint32_t B, uint64_t n, int on_device,
                                                 const Plan& pl);
// pl becomes the plan of the fused group of elements [b0, b0 + cnt) of `sc`: Plan::batch, and their scalars in the form the
// _batch digit kernels take as an argument (narrow elements: in nbs, which must outlive the launch)
void bind_batch_scalars(Plan& pl, NarrowBatchScalars& nbs, const std::vector<const uint32_t*>& sc, int b0, int cnt);

// ---- msm_narrow.hip ---------------------------------------------------------------------------------------------
// checks the format and the options of a narrow call (MSM_ERR_ARG with a message) and resolves it: bits = 0 -> all the width gives
int narrow_format(msm_ctx* ctx, int32_t width_bytes, int32_t bits, int32_t is_signed, const msm_opts* opts, const char* who,
                  Plan::Narrow& out);
// the rest of the argument checks of a narrow entry: n < 2^32 (the digit kernels count points in 32 bits) and device scalars
// aligned to their width (16 bytes for the 16- and 32-byte forms, which lanes load as uint4)
int narrow_scalars_ok(msm_ctx* ctx, const void* scalars, uint64_t n, int on_device, int32_t width_bytes, const char* who);
// The array the pipeline gets for the device scalars `dev` of a narrow call: rounded down to the alignment of a lane's load, with
// nar.first = where the first scalar sits in it (only the 1- and 2-byte formats can start inside a lane's dword)
const char* narrow_lane_base(const char* dev, int32_t width_bytes, Plan::Narrow& nar);
// the scalars of a narrow call on the device: host scalars are uploaded whole before the run (timed as *up_ms), device scalars
// stay where they are
const char* stage_narrow(msm_ctx* ctx, const void* scalars, size_t bytes, int on_device, float* up_ms);

// ---- msm_indexed.hip --------------------------------------------------------------------------------------------
// Queues on `s` the pass that rewrites the n_slots payloads the sort left for round 1 -- (entry << 1) | sign, entry counting the
// positions of the group -- so that they name the entries of the resident points idx[position] with the same half and sign
// (0xFFFFFFFF, the absent marker, stays).  te: one entry per position; otherwise two (2 j and 2 j + 1).
void translate_payloads(hipStream_t s, const msm_ctx* ctx, uint32_t* slots, uint64_t n_slots, const uint32_t* idx);

// ---- msm_lincomb.hip --------------------------------------------------------------------------------------------
// out[i] = a * rows_a[i] + b * rows_b[i], i < count (b null: one term), queued on ctx->stream: the kernel of msm_points_lincomb over
// rows of the caller's.  a, b: 8 words below q.  slot 0 or 1: which of the two program buffers of ctx->misc the launch reads, so
// two launches may be in flight.
void lincomb_launch(msm_ctx* ctx, uint32_t* out, const uint32_t* rows_a, const uint32_t* rows_b, uint64_t count, const uint32_t* a,
                    const uint32_t* b, int slot);
// room for n_rows rows behind the program buffers of ctx->misc
uint32_t* lincomb_scratch_rows(msm_ctx* ctx, uint64_t n_rows);

// ---- msm_points_mul.hip -----------------------------------------------------------------------------------------
// the variable-base kernel of msm_points_mul over `count` rows, queued on ctx->stream: rows + i * row_stride under the scalar at
// d_scal + 8 i -> out + i * row_words.  Returns the blocks of its grid.  pmul_reserve makes the per-lane tables of that launch
// exist, so that a caller can have every allocation behind it before its first launch.
uint64_t pmul_launch_var(msm_ctx* ctx, uint32_t* out, const uint32_t* rows, uint32_t row_stride, const uint32_t* d_scal, uint64_t count);
void pmul_reserve(msm_ctx* ctx, uint64_t count);

// ---- msm_gen.hip ------------------------------------------------------------------------------------------------
}  // namespace msmi
namespace msm_gen {
int generate_scalars(msm_ctx* ctx, uint64_t n, uint64_t seed, void* dev_dst, uint8_t* host_out);
int generate_points(msm_ctx* ctx, uint64_t n, uint64_t seed, uint8_t* a_out);
int generate_points_te(msm_ctx* ctx, uint64_t n, uint64_t seed, uint8_t* a_out);
}  // namespace msm_gen
