// C ABI of the hot path (include/hgemm_mi355x.h): planning (tuned table -> analytic model, the arithmetic of
// hgemm_plan.hip), split-K workspace, launch resolution, launch.  Host-side cost per call is one table probe + one (or two)
// hipLaunchKernelGGL: the reference harness times host wall-clock around each call
// (benchmarking_utils.py:23-31), so a lean host path is part of the hot path.
#include "hgemm_plan.hpp"
#include "hgemm_kernel_nn.hpp"
#include "hgemm_act.hpp"
#include "../../include/hgemm_mi355x.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

using namespace hgemm_mi355x;

namespace {

thread_local int g_last_hip_error = 0;   // per calling thread, like hipGetLastError (calls may come from any thread)
#ifdef HGEMM_ABLATION
int g_debug_flags = 0;  // tuner-only build: hgemm_mi355x_set_debug
#endif
#ifdef HGEMM_TIMELINE
// measurement build (lib_tl/): hgemm_mi355x_set_timeline lends a device buffer of `slots` records, launch n writes record
// n % slots (kTimelineWgs workgroups x HGEMM_TL_WORDS words each)
unsigned long long* g_timeline = nullptr;
int g_timeline_slots = 0;
unsigned g_timeline_count = 0;
constexpr int kTimelineWgs = 1024;
#endif

// ---- split-K workspace ------------------------------------------------------------------------
// One buffer per (device, stream): two GEMMs on different streams (or devices) never share slabs or
// arrival counters.  Layout: [kCounterBytes of tile arrival counters, zero between launches][fp32 slabs].
// Growth happens on first use of a bigger plan only (hipFree of the old buffer synchronises the device,
// so no kernel can still be using it); steady state is a mutex + a short linear search.
// hipGraph capture: a captured launch bakes the workspace address into its kernel node, so (i) nothing is
// allocated while the stream is capturing (a plan that does not fit what is there degrades to splits = 1,
// like a lent buffer that is too small; hgemm_mi355x_reserve_workspace sizes it beforehand) and (ii) a buffer
// that a capture has seen is never freed by growth: it is retired and lives until
// hgemm_mi355x_release_workspaces, so graphs instantiated earlier stay valid.
// (kCounterBytes, kMaxFusedTiles = 65536 tiles: hgemm_plan.hpp)
struct Workspace {
  int device; hipStream_t stream;
  char* ptr; size_t bytes;      // whole allocation (counters + slabs)
  bool captured;                // some hipGraph holds ptr
};
std::mutex g_ws_mutex;
std::vector<Workspace> g_ws;
std::vector<void*> g_ws_retired;   // buffers replaced by growth while a graph may still reference them
// caller-lent buffer (hgemm_mi355x_set_workspace): used for every stream of the device that was current
// when it was lent; the caller promises not to run GEMMs concurrently on several streams then.
char*  g_lent_ptr = nullptr;
size_t g_lent_bytes = 0;
int    g_lent_device = -1;

// the calling thread's stream-capture mode is relaxed while one of these lives (see its uses)
struct RelaxedCapture {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  bool ok;
  RelaxedCapture() { ok = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess; if (!ok) (void)hipGetLastError(); }
  ~RelaxedCapture() { if (ok && hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) (void)hipGetLastError(); }
};

// slab_bytes of fp32 slab space (+ counters) for a launch on `stream`; HGEMM_ERR_NO_WORKSPACE when a lent
// buffer is too small or the allocation fails -- the caller then degrades to a plan that needs none.
constexpr int HGEMM_ERR_NO_WORKSPACE_INTERNAL = -100;
int ensure_workspace(size_t slab_bytes, hipStream_t stream, float** slabs, unsigned** counters) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return HGEMM_ERR_HIP;
  const size_t need = kCounterBytes + slab_bytes;
  std::lock_guard<std::mutex> lk(g_ws_mutex);
  if (g_lent_ptr) {
    if (dev != g_lent_device || need > g_lent_bytes) return HGEMM_ERR_NO_WORKSPACE_INTERNAL;
    *counters = (unsigned*)g_lent_ptr;
    *slabs = (float*)(g_lent_ptr + kCounterBytes);
    return HGEMM_OK;
  }
  Workspace* w = nullptr;
  for (Workspace& e : g_ws)
    if (e.device == dev && e.stream == stream) { w = &e; break; }
  if (!w) {
    g_ws.push_back({dev, stream, nullptr, 0, false});
    w = &g_ws.back();
  }
  // (the legacy default stream cannot capture, and querying it while another stream captures is an error)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool capturing = stream && hipStreamIsCapturing(stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
  if (capturing) {
    if (need > w->bytes) return HGEMM_ERR_NO_WORKSPACE_INTERNAL;
    w->captured = true;
  }
  if (need > w->bytes) {
    // hipMalloc / hipFree are "unsafe" calls for stream capture: made while ANOTHER stream of the process captures in
    // global mode (this call's own stream does not, see above; the legacy stream cannot even be asked) they would
    // invalidate that capture.  The thread's capture mode is switched to relaxed around them, which is the documented
    // way for a library to allocate next to somebody else's capture.
    RelaxedCapture relaxed;
    const size_t old = w->bytes;   // (read before the buffer is let go: the growth below is geometric in the OLD size)
    if (w->ptr && w->captured) {
      g_ws_retired.push_back(w->ptr);
      w->ptr = nullptr; w->bytes = 0; w->captured = false;
    } else if (w->ptr) {
      hipError_t e = hipFree(w->ptr);   // device-synchronising: nothing in flight still reads the old slabs
      if (e != hipSuccess) { g_last_hip_error = (int)e; return HGEMM_ERR_HIP; }
      w->ptr = nullptr; w->bytes = 0;
    }
    // Grow geometrically (first buffer: at least 8 MiB) so a sweep over shapes re-allocates O(log) times, while a
    // process with many short-lived streams does not pin 64 MiB for each of them (round 2 did).
    const size_t want = std::max(need, std::max<size_t>(old * 2, (size_t)8 << 20));
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { (void)hipGetLastError(); g_last_hip_error = (int)e; return HGEMM_ERR_NO_WORKSPACE_INTERNAL; }
    e = hipMemsetAsync(p, 0, kCounterBytes, stream);   // ordered in front of the first launch that uses them
    if (e != hipSuccess) { (void)hipFree(p); g_last_hip_error = (int)e; return HGEMM_ERR_HIP; }
    w->ptr = (char*)p; w->bytes = want;
  }
  *counters = (unsigned*)w->ptr;
  *slabs = (float*)(w->ptr + kCounterBytes);
  return HGEMM_OK;
}

// Plans of off-grid shapes are remembered per thread (the search above / model_plan cost 3-7 us of host time, as much
// as a launch-bound GEMM itself; a harness calls the same shape over and over).
struct PlanMemo { int M, N, K; int cfg, splits, group_m; };
thread_local PlanMemo t_plan_memo[32] = {};

// alignment rules of the LDS-DMA path (the K multiple depends on the geometry: k_ok())
bool mfma_path_ok(const void* a, const void* bt, const void* c, int M, int N, int K, int lda,
                  int ldb, int ldc) {
  if (K % 8 != 0 || (N & 3) != 0) return false;
  if ((lda & 7) || (ldb & 7) || (ldc & 3)) return false;
  if (((uintptr_t)a & 15) || ((uintptr_t)bt & 15) || ((uintptr_t)c & 7)) return false;
  (void)M;
  return true;
}

// ---- launch resolution: the form a hgemm_mi355x_launch call runs as, its workspace and its dispatches -------------------
// Host logic only (no HIP call, allocation or lock): the launch issues what it returns, hgemm_mi355x_plan_workspace_bytes reports
// its request, hgemm_mi355x_selfcheck_launch shows it to the CPU tests.
enum Form { FORM_REFERENCE, FORM_RAGGED, FORM_STREAMK, FORM_SPLITK, FORM_FUSED, FORM_HYBRID, FORM_PLAIN };
enum Thunk { THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_TAIL_REDUCE, THUNK_RAGGED, THUNK_GENERIC,
             // the column sum behind a bgemm_mi355x_nn_dact_dbias call (hgemm_dbias.hpp): row blocks of C to partials, partials to db32, C to db32
             THUNK_COLSUM_BLOCKED, THUNK_COLSUM_FINISH, THUNK_COLSUM_DIRECT };
// one dispatch: its arguments (operand pointers, slabs and counters are the launch's to fill in), grid (0: the thunk sizes it),
// epilogue, and whether it carries the timing hook's start / stop event
struct Dispatch { int thunk; GemmArgs g; int grid, epi; bool start, stop; };
struct LaunchPlan {
  int status = HGEMM_OK, form = FORM_PLAIN, n = 0;
  size_t slab_bytes = 0;   // fp32 slab space the form asks for behind the arrival counters (0: no workspace)
  bool counters = false;   // the form uses the arrival counters
  size_t colsum_off = 0;   // bgemm_mi355x_nn_dact_dbias: where in the slab space the column sum's partials start (behind the K slices' slabs)
  Dispatch d[5];
};
// the selfcheck hooks' view of a plan: out = {form, dispatches, slab bytes, counters}, then per dispatch {thunk, grid, epi, splits,
// k_chunk, items, start, stop}; returns the plan's status
int show_plan(const LaunchPlan& p, long long* out) {
  out[0] = p.form; out[1] = p.n; out[2] = (long long)p.slab_bytes; out[3] = p.counters;
  for (int i = 0; i < p.n; ++i) {
    const Dispatch& d = p.d[i];
    const long long v[8] = {d.thunk, d.grid, d.epi, d.g.splits, d.g.k_chunk, d.g.items, d.start, d.stop};
    std::copy(v, v + 8, out + 4 + 8 * i);
  }
  return p.status;
}
struct DisarmTiming {  // the timing hook is one-shot whatever path (or error return) a launch call takes
  ~DisarmTiming() { hgemm_mi355x::t_launch_timing = hgemm_mi355x::LaunchTiming{}; }
};
constexpr struct { int plan, arg; } kArgFlags[] = {   // plan flags -> GemmArgs::flags
    {HGEMM_PLAN_NT_STORE, ARG_NT_STORE}, {HGEMM_PLAN_RS_XCD_STAGGER, ARG_XCD_STAGGER}, {HGEMM_PLAN_RS_NT_LOADS, ARG_NT_LOADS},
    {HGEMM_PLAN_PHASE_OFFSET, ARG_PHASE_OFFSET}, {HGEMM_PLAN_WAVE_PRIORITY, ARG_WAVE_PRIORITY}, {HGEMM_PLAN_PHASE_OFFSET4, ARG_PHASE_OFFSET4}};

// has_b / has_bt: b / b_col_major given; aligned: the operands pass mfma_path_ok; ruled_out: bits 1 << form of the workspace-backed
// forms that got no workspace
LaunchPlan resolve_launch(int config_id, int splits_arg, int group_m, bool has_b, bool has_bt, bool aligned, int M, int N, int K,
                          int lda, int ldb, int ldc, unsigned ruled_out) {
  LaunchPlan p;
  auto add = [&p](int thunk, const GemmArgs& g, long grid, int epi) {
    if (p.n) p.d[p.n - 1].stop = false;
    p.d[p.n] = Dispatch{thunk, g, (int)grid, epi, p.n == 0, true};
    ++p.n;
  };
  auto fail = [&p](int status) { p.status = status; return p; };
  // rows must not overlap: lda >= K, ldc >= N, ldb >= K where b_col_major is given (the row-major b is read at stride N).  K, N >= 1,
  // so a stride of 0 or below is rejected as well (ldc = 0 would pass mfma_path_ok and write every row over row 0)
  if (lda < K || ldc < N || (has_bt && ldb < K)) return fail(HGEMM_ERR_BAD_ARG);
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.k_chunk = K; g.splits = g.tiles_m = g.tiles_n = g.group_m = g.items = 1;
  for (const auto& f : kArgFlags) g.flags |= (splits_arg & f.plan) ? f.arg : 0;
  g.sk = StreamK{1, 0, 0, 1, FastDiv{0u, 0u, 0u}};
#ifdef HGEMM_ABLATION
  g.debug = g_debug_flags;
#endif
#ifdef HGEMM_TIMELINE
  g.timeline = (g_timeline && g_timeline_slots > 0)   // (hgemm_mi355x_launch has counted this call already)
                   ? g_timeline + (size_t)((g_timeline_count - 1) % (unsigned)g_timeline_slots) * kTimelineWgs * HGEMM_TL_WORDS
                   : nullptr;
#endif
  bool fast = config_id >= 0 && has_bt && aligned;
  if (fast) {
    // 32-bit LDS-DMA offsets: (BM-1) rows * ld * 2 B + K * 2 B must stay below 4 GiB; beyond that the
    // register-staged kernel (64-bit addressing) takes over instead of an error.
    const KernelEntry& e = g_kernel_table[config_id];
    // 2 GiB where bit 31 of an offset is the out-of-range mark: the classic family (its descriptors end at 2 GiB), and a launch that
    // runs a direct K tail (families q / r, K % stage != 0); their whole-stage launches address 4 GiB
    const bool mark31 = e.family == Family::T || (direct_tail(e) && k_ok(e, K) && split_k(e, K, 1).tail_direct);
    const double reach = mark31 ? 2147483648.0 : 4294967296.0;
    if ((double)e.bm * lda * 2.0 + K * 2.0 >= reach || (double)e.bn * ldb * 2.0 + K * 2.0 >= reach) fast = false;
    if (K % BK != 0 && !k_ok(e, K)) fast = false;   // a partial last K-step on a geometry that cannot take it: any-shape kernel
    if (e.family == Family::U && !k_ok(e, K)) fast = false;   // family u: a K that is not whole stages (128 / 256) likewise
    // the LDS-staged epilogue addresses a wave tile through one buffer descriptor with 32-bit offsets
    if ((double)e.bm * ldc * 2.0 + (double)N * 2.0 >= 2147483648.0) fast = false;
  }
  if (!fast) {
    const bool ragged = config_id != HGEMM_CONFIG_GENERIC && has_bt;
    if (ragged && (long)((M + 63) / 64) * ((N + 63) / 64) > 0x7fffffffL) return fail(HGEMM_ERR_TOO_LARGE);
    if (!ragged && !has_b) return fail(HGEMM_ERR_BAD_ARG);
    p.form = ragged ? FORM_RAGGED : FORM_REFERENCE;
    add(ragged ? THUNK_RAGGED : THUNK_GENERIC, g, 0, EPI_C16);
    return p;
  }
  const KernelEntry& e = g_kernel_table[config_id];
  g.tiles_m = (M + e.bm - 1) / e.bm; g.tiles_n = (N + e.bn - 1) / e.bn;
  const long tiles = (long)g.tiles_m * g.tiles_n;
  if (!k_ok(e, K)) return fail(HGEMM_ERR_BAD_ARG);
  const int ksteps = split_k(e, K, 1).steps;   // pipeline stages along K (direct tail: whole stages; the rest rides on the last split)
  // Stream-K (HGEMM_PLAN_STREAMK; the low bits of `splits` are then the number of persistent workgroups): one launch, no
  // combine kernel.  Not available (family without the kernel, too many tiles for the counter block): the plan runs as splits = 1.
  if ((splits_arg & HGEMM_PLAN_STREAMK) && !(ruled_out & (1u << FORM_STREAMK)) && streamk_really_runs(e, M, N, K)) {
    const int min_steps = streamk_min_steps(e);
    const int G = (int)std::max<long>(1, std::min<long>(streamk_grid(e, splits_arg & HGEMM_SPLITK_MASK), std::max<long>(1, tiles * ksteps / min_steps)));
    if ((size_t)2 * G * e.bm * e.bn * sizeof(float) < 2147483648ull) {
      p.form = FORM_STREAMK; p.slab_bytes = (size_t)2 * G * e.bm * e.bn * sizeof(float); p.counters = true;
      g.group_m = std::max(1, std::min(group_m, g.tiles_m)); g.items = (int)tiles;
      g.sk = make_streamk((int)tiles, ksteps, G, min_steps);
      set_raster_div(g);
      add(THUNK_ENTRY, g, G, EPI_STREAMK);
      return p;
    }
  }
  // at most one split per stage, no empty split
  int splits = split_k(e, K, (splits_arg & HGEMM_PLAN_STREAMK) ? 1 : splits_arg & HGEMM_SPLITK_MASK).splits;
  g.group_m = std::max(1, std::min(group_m, g.tiles_m));
  if (tiles * splits > 0x7fffffffL) return fail(HGEMM_ERR_TOO_LARGE);
  if (ruled_out & ((1u << FORM_SPLITK) | (1u << FORM_FUSED))) splits = 1;
  // Split-K: two-pass (slabs + combine kernel) by default; single-launch ("fused") on request, unless the
  // tile count exceeds the counter block or the kernel family has no fused epilogue.
  int epi = EPI_C16;
  if (splits > 1) {
    const bool fused = (splits_arg & HGEMM_SPLITK_FUSED) && tiles <= (long)kMaxFusedTiles && e.has_fused &&
                       (double)tiles * splits * e.bm * e.bn * sizeof(float) < 2147483648.0;   // 32-bit slab offsets
    p.form = fused ? FORM_FUSED : FORM_SPLITK;
    p.slab_bytes = fused ? (size_t)tiles * splits * e.bm * e.bn * sizeof(float) : (size_t)splits * M * N * sizeof(float);
    p.counters = fused;
    epi = fused ? EPI_FUSED : EPI_SLAB;
  }
  g.k_chunk = split_k(e, K, splits).k_chunk; g.splits = splits;
  const long grid = tiles * splits;
  g.items = (int)grid;
  // Hybrid schedule for the persistent family (stream-K's data-parallel + tail form): when the tile
  // count is not a multiple of the resident workgroups, the last partial round would keep most CUs
  // idle for a whole tile time.  Instead the full rounds run as they are and the `tail` leftover
  // tiles are cut along K into floor(G / tail) slices each, one slice per workgroup, combined by a
  // small reduce over compact fp32 slabs.  (7168^3 with 256x256 tiles: 784 = 3 x 256 + 16.)
  const long G = e.persistent_wgs;
#ifdef HGEMM_ABLATION
  if (g_debug_flags & 32) ruled_out |= 1u << FORM_HYBRID;
#endif
  if (G > 0 && splits == 1 && tiles > G && tiles % G != 0 && !(ruled_out & (1u << FORM_HYBRID))) {
    const long tail = tiles % G, full = tiles - tail;
    int S = (int)std::min<long>(G / tail, ksteps / 4);   // >= 4 K-steps per slice
    if (S >= 2) {
      const int per_t = (ksteps + S - 1) / S;
      S = (ksteps + per_t - 1) / per_t;
      // Worth it when it beats the partial round it replaces.  Measured on MI355X: a round with few
      // tiles runs at ~0.6x of a full round's tile time (no contention), and the tail pass costs its
      // K slice plus ~25 us of prologue / epilogue / two extra launches / combine
      // (7168^3: 702 -> 661 us, 4352^2 x 4096: 175 -> 149 us; 10000^2 x 1024 would lose 7 %).
      const double tile_us = model_us(e, e.bm, e.bn, K, 1) - kLaunchUs;
      if (0.6 * tile_us - tile_us / S > 25.0) {
        GemmArgs t = g;
        t.tail_first = (int)full; t.tail_tiles = (int)tail; t.splits = S; t.k_chunk = per_t * e.kgran;
        t.items = (int)tail * S;
        g.items = (int)full; set_raster_div(g); set_raster_div(t);
        p.form = FORM_HYBRID; p.slab_bytes = (size_t)t.items * e.bm * e.bn * sizeof(float);
        add(THUNK_ENTRY, g, std::min<long>(full, G), EPI_C16);
        add(THUNK_ENTRY, t, std::min<long>(t.items, G), EPI_SLAB);
        add(THUNK_TAIL_REDUCE, t, 0, EPI_SLAB);
        return p;
      }
    }
  }
  // persistent families walk their work items themselves: one resident wave of workgroups
  long launch_grid = (e.persistent_wgs > 0) ? std::min<long>(grid, e.persistent_wgs) : grid;
  // A two-resident member (persistent_wgs = 512) whose single-launch split-K variant no longer fits twice into a CU's 160 KiB
  // -- the fused epilogue adds the 64-byte vote word to the stage area: q192x128 / q128x192 with 80 KiB of stages -- is resident
  // once per CU: 512 workgroups would run as two sequential waves of 256, each paying its own prologue.  One wave of 256 walks
  // the same items.
  if (epi == EPI_FUSED && e.persistent_wgs > kCUs && 2L * (e.lds_bytes + 64) > 160L * 1024) launch_grid = std::min<long>(launch_grid, kCUs);
  set_raster_div(g);
  add(THUNK_ENTRY, g, launch_grid, epi);
  if (epi == EPI_SLAB) add(THUNK_SPLITK_REDUCE, g, 0, EPI_SLAB);
  return p;
}

// ---- first-use plan selection on the box the library runs on (opt-in) ---------------------------------------------------------
// The reference's H100 tree re-tunes in situ: a kernel file times its variants on first invocation and keeps the fastest
// (kernels/h100_F32F16F16F32/64_4096_64.cu:623-690, 702-721).  This library ships ONE measured table, and rounds 3-4 showed rows
// whose ranking flips between boxes (the lock-step plans of family q: 40 % across boxes).  With
// HGEMM_MI355X_INSITU=1 in the environment (or hgemm_mi355x_set_insitu(1)) the FIRST call of hgemm_mi355x_fp32 / _fp16 for a
// shape times up to three plans on the call's own operands and stream -- the table's (or the planner's) plan and its
// alternates: for a grid shape the oracle-verified runners-up of the last re-tune (hgemm_tuned_alternates.inc), for any shape the
// plan with family q's K stagger / phase offset toggled (flags that cannot change a result's exactness) -- each once to warm up and
// kInsituReps times under dispatch-attached events, in interleaved rounds, and keeps the fastest for the (process, device); an alternate must beat the plan by
// 3 % to replace it.  The call then runs the winner, so C holds exactly one plan's result.  That first call synchronises the
// stream (it is meant for a warm-up phase: the harness's warm-up seconds, a model's first step); calls on a capturing stream and
// every later call take the recorded choice without timing anything.  Default: off -- the hot path is the table probe.
struct AltRow { int M, N, K; const char* cfg; int splits, group_m; };
const AltRow g_alt_rows[] = {
#include "hgemm_tuned_alternates.inc"
    {0, 0, 0, nullptr, 0, 0}};
struct PlanTriple { int cfg, splits, group_m; };
// One record per (device, shape): boxes rank plans differently and so may the devices of one box.
struct InsituChoice { int dev, M, N, K; PlanTriple plan; };
std::mutex g_insitu_mutex;
std::vector<InsituChoice> g_insitu;      // the process's choices (guarded by g_insitu_mutex)
std::atomic<unsigned> g_insitu_epoch{1}; // bumped when set_insitu(0) forgets them: invalidates the per-thread memos below
std::atomic<int> g_insitu_mode{-1};      // -1: environment not read yet (atomic: calls may come from any thread)
constexpr int kInsituReps = 5;
// Steady state must not take a process-wide lock per GEMM: a thread remembers the choices it has used (direct-mapped on the
// shape key like t_plan_memo; the mutex-guarded vector is only consulted on a memo miss).
struct InsituMemo { unsigned epoch; int dev, M, N, K; PlanTriple plan; };
thread_local InsituMemo t_insitu_memo[32] = {};

bool insitu_enabled() {
  int mode = g_insitu_mode.load(std::memory_order_relaxed);
  if (mode < 0) {
    const char* e = getenv("HGEMM_MI355X_INSITU");
    int expected = -1;
    g_insitu_mode.compare_exchange_strong(expected, (e && *e && *e != '0') ? 1 : 0);   // (a concurrent set_insitu wins)
    mode = g_insitu_mode.load(std::memory_order_relaxed);
  }
  return mode == 1;
}

// the plan + its alternates (at most three, no duplicates, every one launchable on this K)
int insitu_candidates(int M, int N, int K, PlanTriple out[3]) {
  int n = 0;
  PlanTriple p0;
  if (hgemm_mi355x_plan(M, N, K, &p0.cfg, &p0.splits, &p0.group_m) != HGEMM_OK) return 0;
  out[n++] = p0;
  auto add = [&](PlanTriple p) {
    if (n >= 3 || p.cfg < 0 || p.cfg >= g_num_kernels || !k_ok(g_kernel_table[p.cfg], K)) return;
    for (int i = 0; i < n; ++i)
      if (out[i].cfg == p.cfg && out[i].splits == p.splits && out[i].group_m == p.group_m) return;
    out[n++] = p;
  };
  for (const AltRow* r = g_alt_rows; r->cfg; ++r)
    if (r->M == M && r->N == N && r->K == K) add({hgemm_mi355x_config_by_name(r->cfg), r->splits, r->group_m});
  // off the grid (round 6): the runners-up among the tuned plans of the surrounding grid shapes, in the model's order -- every one of
  // them an oracle-verified plan of its own corner, run here through the same edge predication / K tail as the planner's choice
  std::call_once(g_tuned_once, build_tuned_index);
  if (p0.cfg >= 0 && !find_tuned(M, N, K) && K % 8 == 0 && (N & 3) == 0) {
    RankedPlan ranked[8];
    int nr = 0, c0, s0, g0;
    if (neighbour_plan(M, N, K, &c0, &s0, &g0, ranked, &nr)) {
      std::sort(ranked, ranked + nr, [](const RankedPlan& a, const RankedPlan& b) { return a.us < b.us; });
      for (int i = 0; i < nr; ++i) add({ranked[i].cfg, ranked[i].splits, ranked[i].group_m});
    }
  }
  if (p0.cfg >= 0 && !(p0.splits & HGEMM_PLAN_STREAMK)) {
    const KernelEntry& e = g_kernel_table[p0.cfg];
    if (e.family == Family::Q && e.mi == 16 && K % e.kgran == 0) {
      const int s = std::max(1, p0.splits & HGEMM_SPLITK_MASK);
      const long items = (long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn) * s;
      if (K / e.kgran / s >= 8) add({p0.cfg, p0.splits ^ HGEMM_PLAN_XCD_STAGGER, p0.group_m});
      if (items >= 2L * e.persistent_wgs && K <= 1024) add({p0.cfg, p0.splits ^ HGEMM_PLAN_PHASE_OFFSET, p0.group_m});
    }
  }
  return n;
}

inline InsituMemo& insitu_memo_slot(int dev, int M, int N, int K) {
  const uint64_t key = shape_key(M, N, K) * 0x9E3779B97F4A7C15ull + (uint64_t)dev;
  return t_insitu_memo[(key ^ (key >> 21) ^ (key >> 42)) & 31];
}

bool insitu_lookup(int dev, int M, int N, int K, PlanTriple* p) {
  const unsigned epoch = g_insitu_epoch.load(std::memory_order_acquire);
  InsituMemo& m = insitu_memo_slot(dev, M, N, K);
  if (m.epoch == epoch && m.dev == dev && m.M == M && m.N == N && m.K == K) { *p = m.plan; return true; }
  std::lock_guard<std::mutex> lk(g_insitu_mutex);
  for (const InsituChoice& c : g_insitu)
    if (c.dev == dev && c.M == M && c.N == N && c.K == K) {
      *p = c.plan;
      m = InsituMemo{epoch, dev, M, N, K, c.plan};
      return true;
    }
  return false;
}

// times the candidates on the call's operands; false (nothing recorded) when the stream captures or an event call fails
bool insitu_select(int dev, const void* a, const void* b, const void* bt, void* c, int M, int N, int K, void* stream, PlanTriple* choice) {
  hipStream_t s = (hipStream_t)stream;
  // A capture on THIS stream means nothing may be timed.  (The legacy stream is not asked: the query itself would invalidate a
  // global-mode capture of another stream, and so would the caller's launch on it.)  The event calls below would invalidate a
  // global-mode capture that ANOTHER stream of this thread is recording: they run under the relaxed capture mode, as
  // ensure_workspace's hipMalloc does.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return false;
  RelaxedCapture relaxed;
  PlanTriple cand[3];
  const int n = insitu_candidates(M, N, K, cand);
  if (n == 0) return false;
  int best = 0;
  if (n > 1) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { if (e0) (void)hipEventDestroy(e0); (void)hipGetLastError(); return false; }
    // Interleaved rounds: one launch of every candidate per round, so that all of them see the same clock /
    // thermal history -- timing them one after the other right after a cold start favours whoever comes later.
    float t[3][kInsituReps];
    bool ok[3] = {true, true, true};
    for (int r = -1; r < kInsituReps; ++r)   // round -1 warms every candidate up untimed
      for (int i = 0; i < n; ++i) {
        if (!ok[i]) continue;
        if (r >= 0) { hgemm_mi355x::t_launch_timing.start = e0; hgemm_mi355x::t_launch_timing.stop = e1; }   // ride on the plan's own dispatch packets
        ok[i] = hgemm_mi355x_launch(cand[i].cfg, cand[i].splits, cand[i].group_m, a, b, bt, c, M, N, K, K, K, N, stream) == HGEMM_OK;
        if (ok[i] && r >= 0) ok[i] = hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t[i][r], e0, e1) == hipSuccess;
        if (!ok[i]) (void)hipGetLastError();
      }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (!ok[0]) return false;
    double us[3] = {1e30, 1e30, 1e30};
    for (int i = 0; i < n; ++i) {
      if (!ok[i]) continue;
      std::sort(t[i], t[i] + kInsituReps);
      us[i] = (double)t[i][kInsituReps / 2] * 1e3;   // median
    }
    for (int i = 1; i < n; ++i)
      if (us[i] < 0.97 * us[0] && us[i] < us[best]) best = i;   // an alternate has to beat the shipped plan by 3 %
  }
  *choice = cand[best];
  std::lock_guard<std::mutex> lk(g_insitu_mutex);
  for (const InsituChoice& ch : g_insitu)
    if (ch.dev == dev && ch.M == M && ch.N == N && ch.K == K) { *choice = ch.plan; return true; }   // another thread was faster: one choice per (process, device)
  g_insitu.push_back({dev, M, N, K, *choice});
  return true;
}

int run(int acc, const void* a, const void* b, const void* bt, void* c, int M, int N, int K,
        void* stream) {
  (void)acc;  // both accumulate modes use the fp32-accumulating MFMA (header comment)
  if (insitu_enabled() && a && c && bt && M > 0 && N > 0 && K > 0) {
    PlanTriple p;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    if (insitu_lookup(dev, M, N, K, &p) || insitu_select(dev, a, b, bt, c, M, N, K, stream, &p))
      return hgemm_mi355x_launch(p.cfg, p.splits, p.group_m, a, b, bt, c, M, N, K, K, K, N, stream);
  }
  int cfg, splits, group_m;
  int st = hgemm_mi355x_plan(M, N, K, &cfg, &splits, &group_m);
  if (st != HGEMM_OK) return st;
  return hgemm_mi355x_launch(cfg, splits, group_m, a, b, bt, c, M, N, K, K, K, N, stream);
}


// ---- the transposed-read layouts: NN (family n, hgemm_kernel_nn.hpp: B row-major [K][ldb]) and TA (family a, hgemm_kernel_ta.hpp: A given
// as a_col_major [K][lda] as well); and on the same host path TN (family f, hgemm_kernel_tn.hpp: bf16 only, B given as b_col_major
// [N][ldb], no transposed read) ---------------------------------------------------------------------------------------------------------
// The tables and kernel sets of both are built in hgemm_registry.hip (TrTable: hgemm_kernel_nn.hpp); the geometry table,
// hgemm_mi355x_plan and what a b-only call of hgemm_mi355x_launch does know nothing of them.  A layout is described once, here;
// resolution, launch, planner and the queries below are written once and take the description.
// What a call writes: fp16 C (every nn_ / ta_ entry point) or fp32 C (c32: hgemm_mi355x_ta_c32, family a only), stored or -- c32 only --
// added into what C holds.  ldc counts C's own elements.
// bias (bgemm_mi355x_tn_bias, family f only): a 16-bit C with a bf16 bias vector fused into the epilogue -- C = T(sum + float(bias[n])), the
// bias added last and the sum rounded once.  The third output kind: the same tiles, cuts and slabs as the plain 16-bit C.
// act (bgemm_mi355x_tn_bias_act, with bias only): an activation of hgemm_act.hpp behind the bias add -- C = T(act(sum + float(bias[n]))),
// applied to the unrounded fp32 value, never to a slab, the result rounded once.  One more kind per activation, TR_C16_BIAS + act; the
// epilogue ids follow suit, EPI_C16_BIAS + act.
// aux (bgemm_mi355x_tn_bias_act_aux, with bias and act only): the rounded pre-activation as a second 16-bit output z_out at row stride ldz,
// the kinds TR_C16_BIAS_AUX + act and the ids EPI_C16_BIAS_AUX + act.  dact (bgemm_mi355x_nn_dact, family n, no bias): C = T(sum x act'(z)),
// z a 16-bit INPUT at row stride ldz; the kinds TR_C16_DACT + act, the ids EPI_C16_DACT + act.  Either way the second matrix has C's rules
// (ldz >= N; ldz % 8 == 0, 16-byte aligned and (BM ldz + N) 2 bytes below 2 GiB, or the reference kernel answers) and changes nothing else
// of the plan.
// dbias (bgemm_mi355x_nn_dact_dbias, with dact only): the dact call and db32[n] (+)= sum over m of float(C[m][n]), the kinds
// TR_C16_DACT_DBIAS + act.  tr_resolve builds the dact call's plan and adds the column sum to it (see there); db_acc is the call's
// `accumulate`, which is db32's and not C's.
// gated (bgemm_mi355x_tn_gated, family f only): C = T(act(sum_g + bias_g[n]) x (sum_u + bias_u[n])) over two weights of N rows each, the kinds
// TR_C16_GATED + act (HGEMM_ACT_SILU included) and the ids EPI_C16_GATED + act.  N is the OUTPUT width; tiles, cuts, slabs and workspace are
// those of the plain product of width 2 N (a member's tile is BM x BN / 2 outputs; hgemm_gated.hpp has the slab).  Either bias may be null.
// dgated (bgemm_mi355x_nn_dgated, family n only, with dact): the gated layer's input gradient -- two saved 16-bit inputs g (= z) and u at ldz,
// two 16-bit outputs dg (= c) and du at ldc, hgemm_dgated.hpp's dgated_store on the finished sum --, the kinds TR_C16_DGATED + act
// (HGEMM_ACT_SILU included) and the ids EPI_C16_DGATED + act.  The dact call's plan in everything but those ids.
// gaux (bgemm_mi355x_tn_gated_aux, with gated): the gated call with the rounded pre-activations as two more 16-bit outputs g_out (= z) and
// u_out, both at row stride ldz with z_out's rules; the kinds TR_C16_GATED_AUX + act and the ids EPI_C16_GATED_AUX + act.  The gated call's
// plan in everything but those ids.
// add (bgemm_mi355x_tn_bias_add: family f, with bias, which may then be NULL; bgemm_mi355x_nn_add: family n, without): a read-only 16-bit
// residual matrix r (= z) at row stride ldr (= ldz), added to the finished sum in fp32 behind the bias and in front of the one rounding
// (hgemm_residual.hpp); the kinds TR_C16_BIAS_ADD / TR_C16_ADD and the ids EPI_C16_BIAS_ADD / EPI_C16_ADD, no activation.  r has dact's rules
// for z with one difference: r == c is allowed where ldr == ldc (in place) and refused otherwise.  The parent call's plan in everything but
// those ids.
struct TrOut {
  bool c32, accumulate;
  bool bias = false;
  int act = 0;   // 0 (none) or HGEMM_ACT_RELU / _GELU / _GELU_TANH = 1 / 2 / 3
  bool aux = false, dact = false;
  int ldz = 0;   // the row stride of z_out (aux) / z (dact); no part of the kind
  bool dbias = false, db_acc = false;
  bool gated = false;
  bool dgated = false;   // with dact: two saved matrices in (z = g, and u) and two outputs (c = dg, and du); the dact call's plan
  bool gaux = false;     // with gated: two more outputs (z = g_out, and u_out) at ldz; the gated call's plan
  bool add = false;      // the residual matrix r (z = r, ldz = ldr), with bias (family f; the vector may be NULL) or without (family n)
  int elem_bytes() const { return c32 ? 4 : 2; }
  bool has_z() const { return aux || dact || gaux || add; }
  bool has_epi() const { return bias || dact || gated || add; }   // the plain dispatch and the combine dispatch carry an id of their own, epi_bias()
  TrKind kind() const {   // the kernel set's cell in TrRow / TrTable
    return add ? (bias ? TR_C16_BIAS_ADD : TR_C16_ADD) : dgated ? (TrKind)(TR_C16_DGATED + act) : gaux ? (TrKind)(TR_C16_GATED_AUX + act) : gated ? (TrKind)(TR_C16_GATED + act) : dact ? (TrKind)((dbias ? TR_C16_DACT_DBIAS : TR_C16_DACT) + act) : bias ? (TrKind)((aux ? TR_C16_BIAS_AUX : TR_C16_BIAS) + act) : c32 ? TR_C32 : TR_C16;
  }
  int epi_bias() const { return add ? (bias ? EPI_C16_BIAS_ADD : EPI_C16_ADD) : (dgated ? EPI_C16_DGATED : gaux ? EPI_C16_GATED_AUX : gated ? EPI_C16_GATED : dact ? EPI_C16_DACT : aux ? EPI_C16_BIAS_AUX : EPI_C16_BIAS) + act; }
};
constexpr TrOut kOutC16{false, false};
constexpr TrOut kOutC16Bias{false, false, true};
static_assert(HGEMM_ACT_RELU == ACT_RELU && HGEMM_ACT_GELU == ACT_GELU && HGEMM_ACT_GELU_TANH == ACT_GELU_TANH, "the public ids are hgemm_act.hpp's");
static_assert(TR_C16_BIAS + ACT_GELU_TANH == TR_C16_BIAS_GELU_TANH && TR_C16_BIAS_AUX == TR_C16_BIAS_GELU_TANH &&
              TR_C16_DACT == TR_C16_BIAS_AUX + ACT_GELU_TANH && TR_C16_DACT_DBIAS == TR_C16_DACT + ACT_GELU_TANH && TR_C16_DACT_DBIAS + ACT_GELU_TANH + 1 == TR_KINDS,
              "a kind per activation, four times");
constexpr bool act_known(int act) { return act == HGEMM_ACT_RELU || act == HGEMM_ACT_GELU || act == HGEMM_ACT_GELU_TANH; }
static_assert(HGEMM_ACT_SILU == ACT_SILU && TR_C16_GATED + 1 == TR_KINDS && TR_C16_GATED + ACT_SILU == TR_C16_DGATED &&
              TR_C16_DGATED + ACT_SILU == TR_C16_GATED_AUX && TR_C16_GATED_AUX + ACT_SILU + 1 == TR_C16_BIAS_ADD && TR_C16_ADD + 1 == TR_KINDS_ALL &&
              !act_known(HGEMM_ACT_SILU),
              "the gated kinds, the dgated kinds and the gated aux kinds follow; SiLU is theirs alone");
constexpr bool act_known_gated(int act) { return act_known(act) || act == HGEMM_ACT_SILU; }
constexpr TrOut out_gated(int act) { return TrOut{false, false, false, act, false, false, 0, false, false, true}; }   // (act_known_gated(act) checked by the caller)
constexpr TrOut out_gated_aux(int act, int ldz) { return TrOut{false, false, false, act, false, false, ldz, false, false, true, false, true}; }
constexpr TrOut out_bias_act(int act) { return TrOut{false, false, true, act}; }   // (act_known(act) checked by the caller)
constexpr TrOut out_bias_act_aux(int act, int ldz) { return TrOut{false, false, true, act, true, false, ldz}; }
constexpr TrOut out_dact(int act, int ldz) { return TrOut{false, false, false, act, false, true, ldz}; }
constexpr TrOut out_dact_dbias(int act, int ldz, bool db_acc) { return TrOut{false, false, false, act, false, true, ldz, true, db_acc}; }
// (act_known_gated(act) checked by the caller.)  A dact call in every rule and in its plan: z is g, ldz the stride of g and of u alike
constexpr TrOut out_dgated(int act, int ldz) { return TrOut{false, false, false, act, false, true, ldz, false, false, false, true}; }
constexpr TrOut out_bias_add(int ldr) { return TrOut{false, false, true, 0, false, false, ldr, false, false, false, false, false, true}; }
constexpr TrOut out_add(int ldr) { return TrOut{false, false, false, 0, false, false, ldr, false, false, false, false, false, true}; }

// What the operands and a 16-bit C hold (TrElem): fp16 (every hgemm_mi355x_nn_ / _ta_ entry point) or bfloat16 (bgemm_mi355x_).  Elements
// are 2 bytes either way: scope, reach, strides, tables, plans and workspaces do not ask.  (TrElem, c32) selects a kernel set and nothing
// else: the member's launcher in its row, the set's combine and reference kernel in the table's `kernels`.
struct TrLayout {
  const TrTable& t;   // rows by config id and kernels[TrElem][TrKind]; a set the layout does not have is empty, and a call for it is refused
  // How A lies in memory decides every rule in which the two layouts differ.  false (n): [M][lda], rows of K elements, staged and
  // addressed from a tile's first row.  true (a): [K][lda], k-rows of M elements, staged as B is and addressed from row 0 to the end
  // of the matrix; a chunk of a k-row must not straddle M, so M % 8 == 0 joins the scope.
  bool a_col_major;
  // How B lies.  false (n, a): row-major [K][ldb], k-rows of N elements, addressed from row 0 to the end of the matrix.  true (f,
  // hgemm_kernel_tn.hpp): b_col_major [N][ldb], rows of K elements, staged and addressed from a tile's first row, as a row-major A is.
  bool b_col_major = false;
  // the kernel set a query that does not ask for an element kind resolves with (scope, reach, cuts and slabs are the same in every set):
  // one the layout has
  TrElem any_elem = TR_F16;

  // elements in a row of A / of B: the least lda / ldb, and the strides of contiguous operands (the planned calls pass (a_row, b_row, N))
  int a_row(int M, int K) const { return a_col_major ? M : K; }
  int b_row(int N, int K) const { return b_col_major ? K : N; }
  // the kernels' scope; everything else is answered by the reference kernel.  Rows of C start at 16-byte boundaries: ldc % 8 == 0 of
  // a 16-bit C, ldc % 4 == 0 of an fp32 C (next to a_col_major's rule: the output kind changes C's rules only)
  bool path_ok(TrOut out, const void* a, const void* b, const void* c, int M, int N, int K, int lda, int ldb, int ldc) const {
    if (K % BK != 0 || (N & 7) != 0 || (a_col_major && (M & 7) != 0)) return false;
    if ((lda & 7) || (ldb & 7) || (ldc & (out.c32 ? 3 : 7))) return false;
    return !(((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)c & 15));
  }
  // 32-bit offsets with bit 31 to spare: C from a tile's first row -- (BM ldc + N) elements of 2 bytes, of 4 for an fp32 C --, A and B
  // as a_col_major / b_col_major say: an operand of k-rows from row 0 to the end of the matrix, one of K-element rows (BM / BN of them)
  // from a tile's first row
  bool reach_ok(TrOut out, const TrEntry& e, int M, int N, int K, int lda, int ldb, int ldc) const {
    const double a_bytes = a_col_major ? (double)(K - 1) * lda * 2.0 + M * 2.0 : (double)e.bm * lda * 2.0 + K * 2.0;
    // (a gated tile holds BN / 2 rows of each weight)
    const double b_bytes = b_col_major ? (double)(out.gated ? e.bn / 2 : e.bn) * ldb * 2.0 + K * 2.0 : (double)(K - 1) * ldb * 2.0 + N * 2.0;
    const double c_bytes = ((double)e.bm * ldc + N) * out.elem_bytes();
    return a_bytes < 2147483648.0 && b_bytes < 2147483648.0 && c_bytes < 2147483648.0;
  }
};
const TrLayout kLayoutNN{tr_table_nn(), false};
const TrLayout kLayoutTA{tr_table_ta(), true};
const TrLayout kLayoutTN{tr_table_tn(), false, true, TR_BF16};   // the bf16 forward product: no transposed read, the same host path

// (same shape as resolve_launch: host logic only; hgemm_mi355x_selfcheck_launch_nn / _ta show it to the CPU tests)
// out.c32: the same tiles, cuts and slabs; the plain dispatch and the combine carry EPI_C32 (the K slices are the family's EPI_SLAB
// kernels), the least ldc is still N
// out.bias: the plan of the plain 16-bit call in everything but the epi of the plain dispatch and of the combine dispatch, EPI_C16_BIAS;
// the bias pointer is no input (its alignment arrives in `aligned`, as the operands' does).  out.act: the same again with
// EPI_C16_BIAS + act in those two dispatches.
LaunchPlan tr_resolve_gemm(const TrLayout& L, TrElem elem, TrOut out, int config, int splits_arg, bool aligned, int M, int N, int K, int lda, int ldb,
                           int ldc, unsigned ruled_out) {
  LaunchPlan p;
  auto add = [&p](int thunk, const GemmArgs& g, long grid, int epi) {
    if (p.n) p.d[p.n - 1].stop = false;
    p.d[p.n] = Dispatch{thunk, g, (int)grid, epi, p.n == 0, true};
    ++p.n;
  };
  // rows must not overlap: lda >= K (n, f) / >= M, the row stride of a_col_major (a); ldb >= N (n, a: B is row-major) / >= K, the row
  // stride of b_col_major (f); ldc >= N
  if (config < 0 || config >= L.t.count || lda < L.a_row(M, K) || ldb < L.b_row(N, K) || ldc < N || (out.has_z() && out.ldz < N) ||
      (out.gated && N >= (1 << 30))) {   // (2 N is an int)
    p.status = HGEMM_ERR_BAD_ARG;
    return p;
  }
  if (!L.t.kernels[elem][out.kind()].present() || (out.accumulate && !out.c32)) { p.status = HGEMM_ERR_BAD_ARG; return p; }   // no such kernel set in this layout
  const int epi_out = out.c32 ? EPI_C32 : out.has_epi() ? out.epi_bias() : EPI_C16;
  const TrEntry& e = L.t.rows[config].e;
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.k_chunk = K; g.splits = g.tiles_m = g.tiles_n = g.group_m = g.items = 1;
  g.flags = ((splits_arg & HGEMM_PLAN_NT_STORE) ? ARG_NT_STORE : 0) | (out.accumulate ? ARG_ACCUMULATE : 0);
  g.sk = StreamK{1, 0, 0, 1, FastDiv{0u, 0u, 0u}};
  // out.gated: g.N stays the OUTPUT width (what the kernels clamp and predicate with); the tiles and the slabs are the product's, 2 N wide
  const int NP = out.gated ? 2 * N : N;
  const long tiles = (long)((M + e.bm - 1) / e.bm) * ((NP + e.bn - 1) / e.bn);
  const bool z_ok = !out.has_z() || ((out.ldz & 7) == 0 && ((double)e.bm * out.ldz + N) * 2.0 < 2147483648.0);   // z / z_out: C's rules
  if (!aligned || !z_ok || !L.path_ok(out, nullptr, nullptr, nullptr, M, N, K, lda, ldb, ldc) || !L.reach_ok(out, e, M, N, K, lda, ldb, ldc) ||
      tiles > 0x7fffffffL) {
    p.form = FORM_REFERENCE;
    add(THUNK_GENERIC, g, 0, epi_out);
    return p;
  }
  g.tiles_m = (M + e.bm - 1) / e.bm; g.tiles_n = (NP + e.bn - 1) / e.bn;
  g.group_m = std::min(g.tiles_m, 8);
  // at most one split per stage, no empty split (the arithmetic of split_k); the single-launch and stream-K words have no kernel
  // here: their split count runs as the two-pass form / the plain launch
  const int steps = K / BK;
  int splits = (splits_arg & HGEMM_PLAN_STREAMK) ? 1 : std::max(1, std::min(splits_arg & HGEMM_SPLITK_MASK, steps));
  if ((ruled_out & (1u << FORM_SPLITK)) || tiles * splits > 0x7fffffffL) splits = 1;
  const int per = (steps + splits - 1) / splits;
  splits = (steps + per - 1) / per;
  g.k_chunk = per * BK; g.splits = splits; g.items = (int)(tiles * splits);
  set_raster_div(g);
  if (splits > 1) {
    p.form = FORM_SPLITK;
    p.slab_bytes = (size_t)splits * M * NP * sizeof(float);
    add(THUNK_ENTRY, g, tiles * splits, EPI_SLAB);
    add(THUNK_SPLITK_REDUCE, g, 0, out.c32 ? EPI_C32 : out.has_epi() ? out.epi_bias() : EPI_SLAB);
  } else {
    add(THUNK_ENTRY, g, tiles, epi_out);
  }
  return p;
}

// out.dbias: the dact call's plan, dispatch for dispatch, and behind it the column sum (hgemm_dbias.hpp).  ruled_out & 1 << FORM_PLAIN: the
// call got no workspace at all.
//   plain, with a workspace: the plain dispatch carries EPI_C16_DACT_DBIAS + act -- the member's fused kernel, its tile sums in
//     P[tiles_m][N] at the start of the slab space -- and THUNK_COLSUM_FINISH adds the tiles_m rows of P into db32;
//   two-pass: the K slices and the dact combine, then the column sum of the C just written in its own form -- M > COLSUM_DIRECT_ROWS:
//     THUNK_COLSUM_BLOCKED into partials behind the slabs and THUNK_COLSUM_FINISH, otherwise THUNK_COLSUM_DIRECT;
//   reference, and plain without a workspace (the dact kernel of bgemm_mi355x_nn_dact itself): THUNK_COLSUM_DIRECT, which needs none.
// A column-sum dispatch shows epi = EPI_C16_DACT_DBIAS and, in `items`, the partial rows it writes or adds (direct: 0).
LaunchPlan tr_resolve(const TrLayout& L, TrElem elem, TrOut out, int config, int splits_arg, bool aligned, int M, int N, int K, int lda, int ldb, int ldc,
                      unsigned ruled_out) {
  LaunchPlan p = tr_resolve_gemm(L, elem, out, config, splits_arg, aligned, M, N, K, lda, ldb, ldc, ruled_out);
  if (!out.dbias || p.status != HGEMM_OK) return p;
  auto add = [&p](int thunk, GemmArgs g, int rows) {
    g.items = rows;
    p.d[p.n - 1].stop = false;
    p.d[p.n] = Dispatch{thunk, g, 0, EPI_C16_DACT_DBIAS, false, true};
    ++p.n;
  };
  const GemmArgs g = p.d[p.n - 1].g;
  const bool workspace = !(ruled_out & (1u << FORM_PLAIN));
  if (p.form == FORM_PLAIN && workspace) {
    p.d[0].epi = EPI_C16_DACT_DBIAS + out.act;
    p.slab_bytes = (size_t)g.tiles_m * N * sizeof(float);
    add(THUNK_COLSUM_FINISH, g, g.tiles_m);
  } else if (p.form == FORM_SPLITK && M > COLSUM_DIRECT_ROWS) {
    p.colsum_off = p.slab_bytes;
    p.slab_bytes += (size_t)colsum_blocks(M) * N * sizeof(float);
    add(THUNK_COLSUM_BLOCKED, g, colsum_blocks(M));
    add(THUNK_COLSUM_FINISH, g, colsum_blocks(M));
  } else {
    add(THUNK_COLSUM_DIRECT, g, 0);
  }
  return p;
}

// Planner of both families: the largest member whose tiles fill the chip (ties: fewer padded elements, then the taller tile); otherwise
// the 64 x 64 member with as many two-pass splits as bring tiles x splits up to the CU count -- at most one per K stage, at most 32.
void tr_model_plan(const TrLayout& L, int M, int N, int K, int* cfg, int* splits) {
  const TrRow* table = L.t.rows;
  int best = -1;
  long best_area = 0, best_pad = 0;
  for (int i = 0; i < L.t.count; ++i) {
    const TrEntry& e = table[i].e;
    const long tm = (M + e.bm - 1) / e.bm, tn = (N + e.bn - 1) / e.bn, area = (long)e.bm * e.bn, pad = tm * e.bm * tn * e.bn;
    if (tm * tn < kCUs) continue;
    if (best < 0 || area > best_area || (area == best_area && (pad < best_pad || (pad == best_pad && e.bm > table[best].e.bm)))) {
      best = i; best_area = area; best_pad = pad;
    }
  }
  if (best >= 0) { *cfg = best; *splits = 1; return; }
  int small = 0;
  for (int i = 1; i < L.t.count; ++i)
    if (table[i].e.bm * table[i].e.bn < table[small].e.bm * table[small].e.bn) small = i;
  const TrEntry& e = table[small].e;
  const long tiles = (long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn);
  *cfg = small;
  *splits = (int)std::max<long>(1, std::min<long>(std::min<long>((kCUs + tiles - 1) / tiles, K / BK), 32));
}

// GemmArgs as the kernels read it: A = a (n, f: [M][lda], a: [K][lda]), Bt = the row-major B (n, a) / b_col_major (f)
// (out.c32: c is the float pointer; it travels in g.C and the EPI_C32 kernels reinterpret it)
// (elem, out.kind()): the kernel set -- the member's launcher, the combine and the reference kernel; the plan does not depend on elem
// (out.bias: `bias` is the bf16 vector of N elements, required, and joins the kernels' 16-byte alignment rule.  It reaches the combine and
// the reference kernel as an argument and the member's EPI_C16_BIAS kernel in g.counters -- a field the launches of these families leave
// null; GemmArgs keeps its layout, the kernel reinterprets the pointer (hgemm_kernel_tn.hpp).  The EPI_SLAB dispatch of a split call keeps
// counters null: store_tile reads a non-null counters as "compact slabs".)
// (out.aux / out.dact: `z` is the second matrix, required, distinct from c, and joins the alignment rule.  It reaches the combine and the
// reference kernel as an argument and the member's own kernel in fields its non-slab launch leaves idle: z_out in
// g.partial, z in g.counters, the stride out.ldz in g.tail_first -- tail_tiles stays 0, so the raster map never reads it.)
// (out.dgated: z = g as in a dact call; the second input u travels as `bias` and the second output du as `bias2`, both required, with z's
// and c's rules; no output may be the other output or an input.  They reach the combine and the reference kernel under those names and the
// member's kernel behind its GemmArgs, in a DgatedArgs (hgemm_kernel_nn.hpp).)
// (out.gaux: a gated call with z = g_out and `z2` = u_out, both required, each distinct from c and from the other, with z_out's rules.  They
// reach the combine and the reference kernel as a GatedAuxOut pair behind `z` and the member's kernel in a GatedAuxArgs.)
// (out.add: z = r, required, read-only; r == c is the in-place call and needs ldr == ldc -- with another stride the rows of r and c would
// overlap out of step.  With out.bias the vector may be NULL (+0.0).  r reaches the combine and the reference kernel as `z` and the member's
// kernel in g.partial (family f, beside the bias in g.counters) or g.counters (family n), its stride in g.tail_first.)
int tr_launch(const TrLayout& L, TrElem elem, TrOut out, int config, int splits_arg, const void* a, const void* b, const void* bias, void* c, int M,
              int N, int K, int lda, int ldb, int ldc, void* stream, void* z = nullptr, float* db32 = nullptr, const void* b2 = nullptr,
              const void* bias2 = nullptr, void* z2 = nullptr) {
  DisarmTiming disarm_timing;
  if (!a || !b || !c || (out.bias && !out.add && !bias) || (out.gated && !b2) || (out.has_z() && (!z || (z == c && !(out.add && out.ldz == ldc)))) || (out.dbias && !db32) || M <= 0 || N <= 0 || K <= 0)
    return HGEMM_ERR_BAD_ARG;
  if (out.dgated && (!bias || !bias2 || bias2 == c || bias2 == z || bias2 == bias || c == bias)) return HGEMM_ERR_BAD_ARG;
  if (out.gaux && (!z2 || z2 == c || z2 == z)) return HGEMM_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const bool aligned = L.path_ok(out, a, b, c, M, N, K, lda, ldb, ldc) && !(out.bias && ((uintptr_t)bias & 15)) && !(out.has_z() && ((uintptr_t)z & 15)) &&
                       !(out.gated && (((uintptr_t)b2 | (uintptr_t)bias | (uintptr_t)bias2) & 15)) &&   // (a null bias is aligned)
                       !(out.dgated && (((uintptr_t)bias | (uintptr_t)bias2) & 15)) && !(out.gaux && ((uintptr_t)z2 & 15));
  unsigned ruled_out = 0;
  LaunchPlan p = tr_resolve(L, elem, out, config, splits_arg, aligned, M, N, K, lda, ldb, ldc, ruled_out);
  float* slabs = nullptr; unsigned* counters = nullptr;
  // no workspace (lent buffer too small, allocation failed, capturing stream): the plan runs unsplit -- and a dbias call, whose plain form
  // asks for its tile sums' space, then asks once more and without any runs the dact kernel and the direct column sum
  for (int attempt = 0; attempt < 2 && p.status == HGEMM_OK && p.slab_bytes; ++attempt) {
    const int st = ensure_workspace(p.slab_bytes, s, &slabs, &counters);
    if (st == HGEMM_OK) break;
    if (st != HGEMM_ERR_NO_WORKSPACE_INTERNAL) return st;
    ruled_out |= (ruled_out & (1u << FORM_SPLITK)) ? 1u << FORM_PLAIN : 1u << FORM_SPLITK;
    p = tr_resolve(L, elem, out, config, splits_arg, aligned, M, N, K, lda, ldb, ldc, ruled_out);
  }
  if (p.status != HGEMM_OK) return p.status;
  const TrKernels& kern = L.t.kernels[elem][out.kind()];
  const TrLaunch launch = L.t.rows[config].launch[elem][out.kind()];
  // out.gaux alone: what the combine and the reference kernel are handed in the `z` slot, a HOST address that the policy's make() reads
  // before the launch call returns (launch_combine / launch_reference, hgemm_registry.hip); it lives to the end of this function.  Unused
  // by every other kind, whose `z` is the device pointer itself.
  const GatedAuxOut gaux_out{z, z2};
  for (int i = 0; i < p.n; ++i) {
    GemmArgs& g = p.d[i].g;
    g.A = (const f16*)a; g.Bt = (const f16*)b; g.C = (f16*)c;   // (bf16 travels in the same fields: the kernels of its Cfgs reinterpret)
    if (p.d[i].epi != EPI_C16) g.partial = slabs;
    if (out.bias && p.d[i].epi == out.epi_bias()) g.counters = (unsigned*)const_cast<void*>(bias);   // read-only there: the kernel's bf16 bias vector
    if (out.has_z() && !out.gaux && p.d[i].thunk == THUNK_ENTRY &&
        (p.d[i].epi == out.epi_bias() || (out.dbias && p.d[i].epi == EPI_C16_DACT_DBIAS + out.act))) {   // the member's own kernel, never a slab kernel
      if (out.aux || (out.add && out.bias)) g.partial = (float*)z; else g.counters = (unsigned*)z;   // (read-only in the dact and add kernels)
      g.tail_first = out.ldz;
    }
    const TimingSlot ts = timing_slot(p.d[i].start, p.d[i].stop);
    switch (p.d[i].thunk) {
      case THUNK_ENTRY:
        if (out.gaux) {   // the gated aux sets' launchers are handed a GatedAuxArgs (hgemm_kernel_tn_gated.hpp)
          GatedAuxArgs ga;
          static_cast<GemmArgs&>(ga) = g;
          ga.Bu = (const __bf16*)b2; ga.bias_g = (const __bf16*)bias; ga.bias_u = (const __bf16*)bias2;
          ga.G = (__bf16*)z; ga.U = (__bf16*)z2; ga.ldz = out.ldz;
          launch(ga, p.d[i].grid, s, p.d[i].epi, ts);
        } else if (out.gated) {   // the gated sets' launchers are handed a GatedArgs (hgemm_kernel_tn_gated.hpp)
          GatedArgs ga;
          static_cast<GemmArgs&>(ga) = g;
          ga.Bu = (const __bf16*)b2; ga.bias_g = (const __bf16*)bias; ga.bias_u = (const __bf16*)bias2;
          launch(ga, p.d[i].grid, s, p.d[i].epi, ts);
        } else if (out.dgated) {   // the dgated sets' launchers are handed a DgatedArgs (hgemm_kernel_nn.hpp)
          DgatedArgs da;
          static_cast<GemmArgs&>(da) = g;
          da.U = (const __bf16*)bias; da.dU = (__bf16*)const_cast<void*>(bias2);
          launch(da, p.d[i].grid, s, p.d[i].epi, ts);
        } else {
          launch(g, p.d[i].grid, s, p.d[i].epi, ts);
        }
        break;
      case THUNK_COLSUM_BLOCKED: launch_colsum_blocked(c, slabs + p.colsum_off / sizeof(float), M, N, ldc, s, ts); break;
      case THUNK_COLSUM_FINISH: launch_colsum_finish(slabs + p.colsum_off / sizeof(float), db32, g.items, N, out.db_acc, s, ts); break;
      case THUNK_COLSUM_DIRECT: launch_colsum_direct(c, db32, M, N, ldc, out.db_acc, s, ts); break;
      case THUNK_SPLITK_REDUCE: kern.combine(g.partial, c, bias, bias2, out.gaux ? (void*)&gaux_out : z, M, N, ldc, out.ldz, g.splits, out.accumulate, s, ts); break;
      default: kern.reference(a, b, b2, c, bias, bias2, out.gaux ? (void*)&gaux_out : z, M, N, K, lda, ldb, ldc, out.ldz, out.accumulate, s, ts); break;
    }
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) { g_last_hip_error = (int)err; return HGEMM_ERR_HIP; }
  return HGEMM_OK;
}

// the planned call on contiguous operands
int tr_run(const TrLayout& L, TrElem elem, TrOut out, const void* a, const void* b, const void* bias, void* c, int M, int N, int K, void* stream,
           void* z = nullptr, float* db32 = nullptr) {
  if (M <= 0 || N <= 0 || K <= 0) return HGEMM_ERR_BAD_ARG;
  int cfg, splits;
  tr_model_plan(L, M, N, K, &cfg, &splits);
  return tr_launch(L, elem, out, cfg, splits, a, b, bias, c, M, N, K, L.a_row(M, K), L.b_row(N, K), N, stream, z, db32);
}

const char* tr_config_name(const TrLayout& L, int id) { return (id >= 0 && id < L.t.count) ? L.t.rows[id].e.name : nullptr; }

int tr_config_by_name(const TrLayout& L, const char* name) {
  if (!name) return -1;
  for (int i = 0; i < L.t.count; ++i)
    if (std::strcmp(name, L.t.rows[i].e.name) == 0) return i;
  return -1;
}

int tr_config_info(const TrLayout& L, int id, int out[8]) {
  if (id < 0 || id >= L.t.count || !out) return HGEMM_ERR_BAD_ARG;
  const TrEntry& e = L.t.rows[id].e;
  out[0] = e.bm; out[1] = e.bn; out[2] = e.wm; out[3] = e.wn; out[4] = 16; out[5] = e.nbuf; out[6] = e.threads; out[7] = e.lds_bytes;
  return HGEMM_OK;
}

int tr_plan(const TrLayout& L, int M, int N, int K, int* config, int* splits) {
  if (M <= 0 || N <= 0 || K <= 0 || !config || !splits) return HGEMM_ERR_BAD_ARG;
  tr_model_plan(L, M, N, K, config, splits);
  return HGEMM_OK;
}

int tr_runs(const TrLayout& L, TrElem elem, TrOut out, int config, int M, int N, int K, int lda, int ldb, int ldc) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const LaunchPlan p = tr_resolve(L, elem, out, config, 1, true, M, N, K, lda, ldb, ldc, 0);
  return p.status == HGEMM_OK && p.form != FORM_REFERENCE ? 1 : 0;
}

size_t tr_plan_workspace_bytes(const TrLayout& L, int config, int splits, int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const LaunchPlan p = tr_resolve(L, L.any_elem, kOutC16, config, splits, true, M, N, K, L.a_row(M, K), L.b_row(N, K), N, 0);   // (the slabs of both output kinds)
  return p.status == HGEMM_OK && p.slab_bytes ? kCounterBytes + p.slab_bytes : 0;
}

int tr_reserve_workspace(const TrLayout& L, int M, int N, int K, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return HGEMM_ERR_BAD_ARG;
  int cfg = 0, splits = 1;
  tr_model_plan(L, M, N, K, &cfg, &splits);
  const size_t ws = tr_plan_workspace_bytes(L, cfg, splits, M, N, K);
  if (!ws) return HGEMM_OK;
  float* slabs = nullptr; unsigned* counters = nullptr;
  const int rc = ensure_workspace(ws - kCounterBytes, (hipStream_t)stream, &slabs, &counters);
  return rc == HGEMM_ERR_NO_WORKSPACE_INTERNAL ? HGEMM_ERR_NO_WORKSPACE : rc;
}

// what tr_launch decides for a call, nothing launched (the twin of hgemm_mi355x_selfcheck_launch; not part of the public header):
// operands = 4 when the pointers are 16-byte aligned, ruled_out = 1 << form of the two-pass form that got no workspace.  Returns the
// call's status; out = {form, dispatches, slab bytes, counters (0)}, then per dispatch {thunk, grid, epi, splits, k_chunk, items,
// start, stop}.
int tr_selfcheck_launch(const TrLayout& L, TrElem elem, TrOut kind, int config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc,
                        int ruled_out, long long out[20]) {
  if (M <= 0 || N <= 0 || K <= 0 || !out) return HGEMM_ERR_BAD_ARG;
  return show_plan(tr_resolve(L, elem, kind, config, splits, (operands & 4) != 0, M, N, K, lda, ldb, ldc, (unsigned)ruled_out), out);
}

}  // namespace

extern "C" {

int hgemm_mi355x_num_configs(void) { return g_num_kernels; }

const char* hgemm_mi355x_config_name(int id) {
  return (id >= 0 && id < g_num_kernels) ? g_kernel_table[id].name : nullptr;
}

int hgemm_mi355x_config_info(int id, int out[8]) {
  if (id < 0 || id >= g_num_kernels || !out) return HGEMM_ERR_BAD_ARG;
  const KernelEntry& e = g_kernel_table[id];
  out[0] = e.bm; out[1] = e.bn; out[2] = e.wm; out[3] = e.wn;
  out[4] = e.mi; out[5] = e.nbuf; out[6] = e.threads; out[7] = e.lds_bytes;
  return HGEMM_OK;
}

int hgemm_mi355x_config_k_granularity(int id) {
  if (id < 0 || id >= g_num_kernels) return 1;
  return g_kernel_table[id].ktail != KTail::NONE ? 8 : g_kernel_table[id].kgran;
}

int hgemm_mi355x_config_accepts_k(int id, int K) {
  if (id < 0 || id >= g_num_kernels) return K > 0 ? 1 : 0;   // the special ids take any K
  return K > 0 && k_ok(g_kernel_table[id], K) ? 1 : 0;
}

int hgemm_mi355x_config_local_splits(int id) {
  if (id < 0 || id >= g_num_kernels) return -1;
  return g_kernel_table[id].family == Family::U ? LU_KS : 1;
}

int hgemm_mi355x_config_by_name(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < g_num_kernels; ++i)
    if (std::strcmp(name, g_kernel_table[i].name) == 0) return i;
  return -1;
}

int hgemm_mi355x_plan(int M, int N, int K, int* config_id, int* splits, int* group_m) {
  if (M <= 0 || N <= 0 || K <= 0 || !config_id || !splits || !group_m) return HGEMM_ERR_BAD_ARG;
  std::call_once(g_tuned_once, build_tuned_index);
  if (const TunedPlan* hit = find_tuned(M, N, K)) {
    *config_id = hit->cfg; *splits = hit->splits; *group_m = hit->group_m;
    return HGEMM_OK;
  }
  if (K % 8 != 0 || (N & 3) != 0) {  // register-staged any-shape MFMA kernel (hgemm_kernel_rg.hpp)
    *config_id = HGEMM_CONFIG_RAGGED; *splits = 1; *group_m = 1;
    return HGEMM_OK;
  }
  const uint64_t key = shape_key(M, N, K);
  PlanMemo& memo = t_plan_memo[(key ^ (key >> 21) ^ (key >> 42)) & 31];
  if (memo.M != M || memo.N != N || memo.K != K) {   // (an empty slot holds M = 0, never a valid shape)
    PlanMemo m{M, N, K, 0, 1, 1};
    if (!neighbour_plan(M, N, K, &m.cfg, &m.splits, &m.group_m)) model_plan(M, N, K, &m.cfg, &m.splits, &m.group_m);
    memo = m;
  }
  *config_id = memo.cfg; *splits = memo.splits; *group_m = memo.group_m;
  return HGEMM_OK;
}

double hgemm_mi355x_model_us(int config_id, int splits, int M, int N, int K) {
  if (config_id < 0 || config_id >= g_num_kernels || splits < 1 || M <= 0 || N <= 0 || K <= 0) return -1.0;
  const KernelEntry& e = g_kernel_table[config_id];
  // `splits` as hgemm_mi355x_launch takes it: the plan flags are not a split count (round 3 passed them through: a row with
  // HGEMM_PLAN_NT_STORE was priced as 131073 splits)
  if ((splits & HGEMM_PLAN_STREAMK) && e.sk_wgs_per_cu > 0)
    return model_us_streamk(e, M, N, K, streamk_grid(e, splits & HGEMM_SPLITK_MASK));
  return model_us(e, M, N, K, std::max(1, splits & HGEMM_SPLITK_MASK));
}

int hgemm_mi355x_streamk_runs(int config_id, int M, int N, int K) {
  if (config_id < 0 || config_id >= g_num_kernels || M <= 0 || N <= 0 || K <= 0) return 0;
  return streamk_really_runs(g_kernel_table[config_id], M, N, K) ? 1 : 0;
}

int hgemm_mi355x_config_streamk(int config_id) {
  return (config_id >= 0 && config_id < g_num_kernels) ? g_kernel_table[config_id].sk_wgs_per_cu : 0;
}

int hgemm_mi355x_default_group(int config_id, int M, int N) {
  if (config_id < 0 || config_id >= g_num_kernels || M <= 0 || N <= 0) return 1;
  const KernelEntry& e = g_kernel_table[config_id];
  return default_group_m(e, (M + e.bm - 1) / e.bm, (N + e.bn - 1) / e.bn);
}

size_t hgemm_mi355x_workspace_bytes(int M, int N, int splits) {
  // upper bound over both split-K forms and every tile size (<= 256): counters + tile-padded fp32 slabs
  if (splits & HGEMM_PLAN_STREAMK) {   // two compact slabs per persistent workgroup; no stream-K kernel beyond 256 x 128 tiles, and
    // the launch never asks for more workgroups than the largest default grid (1024) unless the plan names more
    const int G = std::min(4096, std::max(1024, splits & HGEMM_SPLITK_MASK));
    return kCounterBytes + (size_t)2 * (size_t)G * 256 * 128 * sizeof(float);
  }
  if ((splits & HGEMM_SPLITK_MASK) <= 1) return 0;
  const size_t mp = ((size_t)M + 255) / 256 * 256, np = ((size_t)N + 255) / 256 * 256;
  return kCounterBytes + (size_t)(splits & HGEMM_SPLITK_MASK) * mp * np * sizeof(float);
}

size_t hgemm_mi355x_plan_workspace_bytes(int config_id, int splits, int M, int N, int K) {
  // what hgemm_mi355x_launch asks ensure_workspace for with this plan on the operands run() passes (0: the plan needs none)
  if (config_id < 0 || config_id >= g_num_kernels || M <= 0 || N <= 0 || K <= 0) return 0;
  const bool aligned = mfma_path_ok(nullptr, nullptr, nullptr, M, N, K, K, K, N);   // (null pointers are aligned ones)
  const LaunchPlan p = resolve_launch(config_id, splits, 1, true, true, aligned, M, N, K, K, K, N, 0);
  return p.status == HGEMM_OK && p.slab_bytes ? kCounterBytes + p.slab_bytes : 0;
}

int hgemm_mi355x_set_workspace(void* device_ptr, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_ws_mutex);
  if (device_ptr) {
    if (bytes < kCounterBytes) return HGEMM_ERR_BAD_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return HGEMM_ERR_HIP;
    hipError_t e = hipMemset(device_ptr, 0, kCounterBytes);   // arrival counters start at zero
    if (e != hipSuccess) { g_last_hip_error = (int)e; return HGEMM_ERR_HIP; }
    g_lent_device = dev;
  }
  g_lent_ptr = (char*)device_ptr; g_lent_bytes = device_ptr ? bytes : 0;
  return HGEMM_OK;
}

int hgemm_mi355x_release_workspaces(void) {
  std::lock_guard<std::mutex> lk(g_ws_mutex);
  int rc = HGEMM_OK;
  for (Workspace& w : g_ws)
    if (w.ptr && hipFree(w.ptr) != hipSuccess) rc = HGEMM_ERR_HIP;
  for (void* p : g_ws_retired)
    if (hipFree(p) != hipSuccess) rc = HGEMM_ERR_HIP;
  g_ws.clear();
  g_ws_retired.clear();
  return rc;
}

int hgemm_mi355x_release_stream_workspace(void* stream) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return HGEMM_ERR_HIP;
  std::lock_guard<std::mutex> lk(g_ws_mutex);
  for (size_t i = 0; i < g_ws.size(); ++i) {
    if (g_ws[i].device != dev || g_ws[i].stream != (hipStream_t)stream) continue;
    int rc = HGEMM_OK;
    if (g_ws[i].ptr) {
      if (g_ws[i].captured) g_ws_retired.push_back(g_ws[i].ptr);   // a graph may still hold it: lives until release_workspaces
      else if (hipFree(g_ws[i].ptr) != hipSuccess) rc = HGEMM_ERR_HIP;
    }
    g_ws.erase(g_ws.begin() + (long)i);
    return rc;
  }
  return HGEMM_OK;
}

int hgemm_mi355x_reserve_workspace(int M, int N, int K, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return HGEMM_ERR_BAD_ARG;
  int cfg = 0, splits = 1, group = 1;
  const int st = hgemm_mi355x_plan(M, N, K, &cfg, &splits, &group);
  if (st != HGEMM_OK) return st;
  // what the launch will ask for, and no less than what a hybrid tail can ask for (one 256x256 fp32 tile per resident workgroup)
  const size_t ws = std::max(hgemm_mi355x_plan_workspace_bytes(cfg, splits, M, N, K), kCounterBytes + (size_t)256 * 256 * 256 * sizeof(float));
  float* slabs = nullptr; unsigned* counters = nullptr;
  const int rc = ensure_workspace(ws - kCounterBytes, (hipStream_t)stream, &slabs, &counters);
  return rc == HGEMM_ERR_NO_WORKSPACE_INTERNAL ? HGEMM_ERR_NO_WORKSPACE : rc;
}

int hgemm_mi355x_launch(int config_id, int splits_arg, int group_m, const void* a, const void* b,
                        const void* b_col_major, void* c, int M, int N, int K, int lda, int ldb,
                        int ldc, void* stream) {
  DisarmTiming disarm_timing;
  if (!a || !c || M <= 0 || N <= 0 || K <= 0) return HGEMM_ERR_BAD_ARG;
  if (config_id >= g_num_kernels || config_id < HGEMM_CONFIG_RAGGED) return HGEMM_ERR_BAD_ARG;
#ifdef HGEMM_TIMELINE
  ++g_timeline_count;
#endif
  hipStream_t s = (hipStream_t)stream;
  const bool aligned = mfma_path_ok(a, b_col_major, c, M, N, K, lda, ldb, ldc);
  unsigned ruled_out = 0;
  auto resolve = [&] {
    return resolve_launch(config_id, splits_arg, group_m, b != nullptr, b_col_major != nullptr, aligned, M, N, K, lda, ldb, ldc, ruled_out);
  };
  LaunchPlan p = resolve();
  float* slabs = nullptr; unsigned* counters = nullptr;
  // No workspace (lent buffer too small, allocation failed, capturing stream) runs the plan without the form that needed it;
  // stream-K and split-K return any other error, the hybrid tail runs its plain launch whatever went wrong.
  while (p.status == HGEMM_OK && p.slab_bytes) {
    const int st = ensure_workspace(p.slab_bytes, s, &slabs, &counters);
    if (st == HGEMM_OK) break;
    if (st != HGEMM_ERR_NO_WORKSPACE_INTERNAL && p.form != FORM_HYBRID) return st;
    ruled_out |= 1u << p.form;
    p = resolve();
  }
  if (p.status != HGEMM_OK) return p.status;
  for (int i = 0; i < p.n; ++i) {
    GemmArgs& g = p.d[i].g;
    g.A = (const f16*)a; g.Bt = (const f16*)b_col_major; g.C = (f16*)c;
    if (p.d[i].epi != EPI_C16) {
      g.partial = slabs;
      if (p.counters) g.counters = counters;
    }
    const TimingSlot ts = timing_slot(p.d[i].start, p.d[i].stop);
    switch (p.d[i].thunk) {
      case THUNK_ENTRY: g_kernel_table[config_id].launch(g, p.d[i].grid, s, p.d[i].epi, ts); break;
      case THUNK_SPLITK_REDUCE: launch_splitk_reduce(g.partial, g.C, M, N, ldc, g.splits, s, ts); break;
      case THUNK_TAIL_REDUCE: launch_tail_reduce(g, g_kernel_table[config_id].bm, g_kernel_table[config_id].bn, s, ts); break;
      case THUNK_RAGGED: launch_ragged(g, s, ts); break;
      case THUNK_GENERIC: launch_generic((const f16*)a, (const f16*)b, (f16*)c, M, N, K, lda, N, ldc, s, ts); break;
    }
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) { g_last_hip_error = (int)err; return HGEMM_ERR_HIP; }
  return HGEMM_OK;
}

// q256x256_w2x2's one-tile-per-workgroup kernel (hgemm_kernel_sq_one.hpp; switch, counter and selection rule: hgemm_inst_g13.hip)
int hgemm_mi355x_set_one_item_kernel(int on) { return sq_one_set_enabled(on); }

unsigned long long hgemm_mi355x_one_item_kernel_launches(void) { return sq_one_launch_count(); }

int hgemm_mi355x_one_item_kernel_takes(int config_id, int splits, int group_m, int M, int N, int K, int lda, int ldb, int ldc) {
  if (M <= 0 || N <= 0 || K <= 0 || config_id >= g_num_kernels || config_id < HGEMM_CONFIG_RAGGED) return HGEMM_ERR_BAD_ARG;
  const LaunchPlan p = resolve_launch(config_id, splits, group_m, false, true, true, M, N, K, lda, ldb, ldc, 0);
  if (p.status != HGEMM_OK) return p.status;
  static const int q256 = hgemm_mi355x_config_by_name("q256x256_w2x2");
  if (config_id != q256) return 0;
  for (int i = 0; i < p.n; ++i)   // (the query's C is the null pointer: aligned)
    if (p.d[i].thunk == THUNK_ENTRY && sq_one_takes(p.d[i].g, p.d[i].grid, p.d[i].epi)) return 1;
  return 0;
}

int hgemm_mi355x_set_insitu(int enable) {
  const int old = insitu_enabled() ? 1 : 0;
  g_insitu_mode.store(enable ? 1 : 0);
  if (!enable) {   // a later enable measures again (the epoch retires every thread's memo of the old choices)
    std::lock_guard<std::mutex> lk(g_insitu_mutex);
    g_insitu.clear();
    g_insitu_epoch.fetch_add(1, std::memory_order_release);
  }
  return old;
}

int hgemm_mi355x_insitu_enabled(void) { return insitu_enabled() ? 1 : 0; }

int hgemm_mi355x_insitu_candidates(int M, int N, int K, int config_id[3], int splits[3], int group_m[3]) {
  if (M <= 0 || N <= 0 || K <= 0 || !config_id || !splits || !group_m) return 0;
  PlanTriple c[3];
  const int n = insitu_candidates(M, N, K, c);
  for (int i = 0; i < n; ++i) { config_id[i] = c[i].cfg; splits[i] = c[i].splits; group_m[i] = c[i].group_m; }
  return n;
}

int hgemm_mi355x_insitu_choice(int M, int N, int K, int* config_id, int* splits, int* group_m) {
  PlanTriple p;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
  if (!config_id || !splits || !group_m || !insitu_lookup(dev, M, N, K, &p)) return 0;
  *config_id = p.cfg; *splits = p.splits; *group_m = p.group_m;
  return 1;
}

int hgemm_mi355x_fp32(const void* a, const void* b, const void* bt, void* c, int M, int N, int K,
                      void* stream) {
  return run(HGEMM_ACC_FP32, a, b, bt, c, M, N, K, stream);
}

int hgemm_mi355x_fp16(const void* a, const void* b, const void* bt, void* c, int M, int N, int K,
                      void* stream) {
  return run(HGEMM_ACC_FP16, a, b, bt, c, M, N, K, stream);
}

// ---- NN layout (kLayoutNN) and TA layout (kLayoutTA): forwards to the one host path of the transposed-read layouts ---------------------
int hgemm_mi355x_nn_num_configs(void) { return kLayoutNN.t.count; }
const char* hgemm_mi355x_nn_config_name(int id) { return tr_config_name(kLayoutNN, id); }
int hgemm_mi355x_nn_config_by_name(const char* name) { return tr_config_by_name(kLayoutNN, name); }
int hgemm_mi355x_nn_config_info(int id, int out[8]) { return tr_config_info(kLayoutNN, id, out); }
int hgemm_mi355x_nn_plan(int M, int N, int K, int* nn_config, int* splits) { return tr_plan(kLayoutNN, M, N, K, nn_config, splits); }
int hgemm_mi355x_nn_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc) { return tr_runs(kLayoutNN, TR_F16, kOutC16, nn_config, M, N, K, lda, ldb, ldc); }
size_t hgemm_mi355x_nn_plan_workspace_bytes(int nn_config, int splits, int M, int N, int K) {
  return tr_plan_workspace_bytes(kLayoutNN, nn_config, splits, M, N, K);
}
int hgemm_mi355x_nn_reserve_workspace(int M, int N, int K, void* stream) { return tr_reserve_workspace(kLayoutNN, M, N, K, stream); }
int hgemm_mi355x_launch_nn(int nn_config, int splits_arg, const void* a, const void* b, void* c, int M, int N, int K, int lda, int ldb,
                           int ldc, void* stream) {
  return tr_launch(kLayoutNN, TR_F16, kOutC16, nn_config, splits_arg, a, b, nullptr, c, M, N, K, lda, ldb, ldc, stream);
}
int hgemm_mi355x_nn_fp32(const void* a, const void* b, void* c, int M, int N, int K, void* stream) { return tr_run(kLayoutNN, TR_F16, kOutC16, a, b, nullptr, c, M, N, K, stream); }
int hgemm_mi355x_nn_fp16(const void* a, const void* b, void* c, int M, int N, int K, void* stream) { return tr_run(kLayoutNN, TR_F16, kOutC16, a, b, nullptr, c, M, N, K, stream); }
int hgemm_mi355x_selfcheck_launch_nn(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                     long long out[20]) {
  return tr_selfcheck_launch(kLayoutNN, TR_F16, kOutC16, nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

int hgemm_mi355x_ta_num_configs(void) { return kLayoutTA.t.count; }
const char* hgemm_mi355x_ta_config_name(int id) { return tr_config_name(kLayoutTA, id); }
int hgemm_mi355x_ta_config_by_name(const char* name) { return tr_config_by_name(kLayoutTA, name); }
int hgemm_mi355x_ta_config_info(int id, int out[8]) { return tr_config_info(kLayoutTA, id, out); }
int hgemm_mi355x_ta_plan(int M, int N, int K, int* ta_config, int* splits) { return tr_plan(kLayoutTA, M, N, K, ta_config, splits); }
int hgemm_mi355x_ta_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc) { return tr_runs(kLayoutTA, TR_F16, kOutC16, ta_config, M, N, K, lda, ldb, ldc); }
size_t hgemm_mi355x_ta_plan_workspace_bytes(int ta_config, int splits, int M, int N, int K) {
  return tr_plan_workspace_bytes(kLayoutTA, ta_config, splits, M, N, K);
}
int hgemm_mi355x_ta_reserve_workspace(int M, int N, int K, void* stream) { return tr_reserve_workspace(kLayoutTA, M, N, K, stream); }
int hgemm_mi355x_launch_ta(int ta_config, int splits_arg, const void* a_col_major, const void* b, void* c, int M, int N, int K, int lda,
                           int ldb, int ldc, void* stream) {
  return tr_launch(kLayoutTA, TR_F16, kOutC16, ta_config, splits_arg, a_col_major, b, nullptr, c, M, N, K, lda, ldb, ldc, stream);
}
int hgemm_mi355x_ta_fp32(const void* a_col_major, const void* b, void* c, int M, int N, int K, void* stream) { return tr_run(kLayoutTA, TR_F16, kOutC16, a_col_major, b, nullptr, c, M, N, K, stream); }
int hgemm_mi355x_ta_fp16(const void* a_col_major, const void* b, void* c, int M, int N, int K, void* stream) { return tr_run(kLayoutTA, TR_F16, kOutC16, a_col_major, b, nullptr, c, M, N, K, stream); }
int hgemm_mi355x_selfcheck_launch_ta(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                     long long out[20]) {
  return tr_selfcheck_launch(kLayoutTA, TR_F16, kOutC16, ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// fp32 C (family a, EPI_C32): the same path with the other output kind.  Plan, workspace size and reserve call are the TA layout's own
// (hgemm_mi355x_ta_plan / _ta_plan_workspace_bytes / _ta_reserve_workspace): the tiles and the slabs are the same.
int hgemm_mi355x_launch_ta_c32(int ta_config, int splits_arg, const void* a_col_major, const void* b, float* c32, int M, int N, int K, int lda,
                               int ldb, int ldc, int accumulate, void* stream) {
  if (accumulate != 0 && accumulate != 1) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutTA, TR_F16, TrOut{true, accumulate == 1}, ta_config, splits_arg, a_col_major, b, nullptr, c32, M, N, K, lda, ldb, ldc, stream);
}
int hgemm_mi355x_ta_c32(const void* a_col_major, const void* b, float* c32, int M, int N, int K, int accumulate, void* stream) {
  if (accumulate != 0 && accumulate != 1) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutTA, TR_F16, TrOut{true, accumulate == 1}, a_col_major, b, nullptr, c32, M, N, K, stream);
}
int hgemm_mi355x_ta_c32_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc) {
  return tr_runs(kLayoutTA, TR_F16, TrOut{true, false}, ta_config, M, N, K, lda, ldb, ldc);
}
int hgemm_mi355x_selfcheck_launch_ta_c32(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int accumulate,
                                         int ruled_out, long long out[20]) {
  if (accumulate != 0 && accumulate != 1) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTA, TR_F16, TrOut{true, accumulate == 1}, ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- bfloat16 operands and 16-bit C on the two transposed-read layouts: the same path with the other element kind.  Tables, ids, plans,
// workspace sizes and the reserve calls are the hgemm_mi355x_nn_ / _ta_ functions' (elements are 2 bytes either way); the b_col_major
// families have no bf16 form (the bf16 forward product is the TN layout below, kernels of its own).
int bgemm_mi355x_launch_nn(int nn_config, int splits_arg, const void* a, const void* b, void* c, int M, int N, int K, int lda, int ldb,
                           int ldc, void* stream) {
  return tr_launch(kLayoutNN, TR_BF16, kOutC16, nn_config, splits_arg, a, b, nullptr, c, M, N, K, lda, ldb, ldc, stream);
}
int bgemm_mi355x_nn(const void* a, const void* b, void* c, int M, int N, int K, void* stream) { return tr_run(kLayoutNN, TR_BF16, kOutC16, a, b, nullptr, c, M, N, K, stream); }
int bgemm_mi355x_nn_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc) { return tr_runs(kLayoutNN, TR_BF16, kOutC16, nn_config, M, N, K, lda, ldb, ldc); }
int bgemm_mi355x_launch_ta(int ta_config, int splits_arg, const void* a_col_major, const void* b, void* c, int M, int N, int K, int lda,
                           int ldb, int ldc, void* stream) {
  return tr_launch(kLayoutTA, TR_BF16, kOutC16, ta_config, splits_arg, a_col_major, b, nullptr, c, M, N, K, lda, ldb, ldc, stream);
}
int bgemm_mi355x_ta(const void* a_col_major, const void* b, void* c, int M, int N, int K, void* stream) { return tr_run(kLayoutTA, TR_BF16, kOutC16, a_col_major, b, nullptr, c, M, N, K, stream); }
int bgemm_mi355x_ta_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc) { return tr_runs(kLayoutTA, TR_BF16, kOutC16, ta_config, M, N, K, lda, ldb, ldc); }
int bgemm_mi355x_launch_ta_c32(int ta_config, int splits_arg, const void* a_col_major, const void* b, float* c32, int M, int N, int K, int lda,
                               int ldb, int ldc, int accumulate, void* stream) {
  if (accumulate != 0 && accumulate != 1) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutTA, TR_BF16, TrOut{true, accumulate == 1}, ta_config, splits_arg, a_col_major, b, nullptr, c32, M, N, K, lda, ldb, ldc, stream);
}
int bgemm_mi355x_ta_c32(const void* a_col_major, const void* b, float* c32, int M, int N, int K, int accumulate, void* stream) {
  if (accumulate != 0 && accumulate != 1) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutTA, TR_BF16, TrOut{true, accumulate == 1}, a_col_major, b, nullptr, c32, M, N, K, stream);
}
int bgemm_mi355x_ta_c32_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc) {
  return tr_runs(kLayoutTA, TR_BF16, TrOut{true, false}, ta_config, M, N, K, lda, ldb, ldc);
}
// (the CPU tests' view, not part of the public header: the plan is the fp16 twin's -- the element kind is not an input of tr_resolve)
int bgemm_mi355x_selfcheck_launch_nn(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                     long long out[20]) {
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, kOutC16, nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_ta(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                     long long out[20]) {
  return tr_selfcheck_launch(kLayoutTA, TR_BF16, kOutC16, ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_ta_c32(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int accumulate,
                                         int ruled_out, long long out[20]) {
  if (accumulate != 0 && accumulate != 1) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTA, TR_BF16, TrOut{true, accumulate == 1}, ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}


// ---- the bf16 forward product, Y = X W^T (kLayoutTN, family f): the same path once more.  A table, ids, plan, workspace size and reserve
// call of its own -- the layout has no fp16 twin to borrow them from.
int bgemm_mi355x_tn_num_configs(void) { return kLayoutTN.t.count; }
const char* bgemm_mi355x_tn_config_name(int id) { return tr_config_name(kLayoutTN, id); }
int bgemm_mi355x_tn_config_by_name(const char* name) { return tr_config_by_name(kLayoutTN, name); }
int bgemm_mi355x_tn_config_info(int id, int out[8]) { return tr_config_info(kLayoutTN, id, out); }
int bgemm_mi355x_tn_plan(int M, int N, int K, int* tn_config, int* splits) { return tr_plan(kLayoutTN, M, N, K, tn_config, splits); }
int bgemm_mi355x_tn_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc) { return tr_runs(kLayoutTN, TR_BF16, kOutC16, tn_config, M, N, K, lda, ldb, ldc); }
size_t bgemm_mi355x_tn_plan_workspace_bytes(int tn_config, int splits, int M, int N, int K) {
  return tr_plan_workspace_bytes(kLayoutTN, tn_config, splits, M, N, K);
}
int bgemm_mi355x_tn_reserve_workspace(int M, int N, int K, void* stream) { return tr_reserve_workspace(kLayoutTN, M, N, K, stream); }
int bgemm_mi355x_launch_tn(int tn_config, int splits_arg, const void* a, const void* b_col_major, void* c, int M, int N, int K, int lda,
                           int ldb, int ldc, void* stream) {
  return tr_launch(kLayoutTN, TR_BF16, kOutC16, tn_config, splits_arg, a, b_col_major, nullptr, c, M, N, K, lda, ldb, ldc, stream);
}
int bgemm_mi355x_tn(const void* a, const void* b_col_major, void* c, int M, int N, int K, void* stream) { return tr_run(kLayoutTN, TR_BF16, kOutC16, a, b_col_major, nullptr, c, M, N, K, stream); }
int bgemm_mi355x_selfcheck_launch_tn(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                     long long out[20]) {
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, kOutC16, tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- the forward product with a fused bias, Y = X W^T + b (the layout's third output kind, kOutC16Bias): C = bf16(S + float(bias[n])), S
// the finished fp32 sum, the bias added last and the result rounded once.  Table, ids, names, plan, workspace size and reserve call are
// bgemm_mi355x_tn_*'s: the tiles, cuts and slabs are the same.  bias: bf16, N elements, required (a caller without one has bgemm_mi355x_tn).
int bgemm_mi355x_tn_bias_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc) { return tr_runs(kLayoutTN, TR_BF16, kOutC16Bias, tn_config, M, N, K, lda, ldb, ldc); }
int bgemm_mi355x_launch_tn_bias(int tn_config, int splits_arg, const void* a, const void* b_col_major, const void* bias, void* c, int M, int N,
                                int K, int lda, int ldb, int ldc, void* stream) {
  return tr_launch(kLayoutTN, TR_BF16, kOutC16Bias, tn_config, splits_arg, a, b_col_major, bias, c, M, N, K, lda, ldb, ldc, stream);
}
int bgemm_mi355x_tn_bias(const void* a, const void* b_col_major, const void* bias, void* c, int M, int N, int K, void* stream) {
  if (!bias) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutTN, TR_BF16, kOutC16Bias, a, b_col_major, bias, c, M, N, K, stream);
}
// (operands & 4: a, b_col_major, c AND bias 16-byte aligned.  The NN and TA layouts have no such kernel set: their twins show the refusal.)
int bgemm_mi355x_selfcheck_launch_tn_bias(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                          long long out[20]) {
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, kOutC16Bias, tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_nn_bias(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                          long long out[20]) {
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, kOutC16Bias, nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_ta_bias(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                          long long out[20]) {
  return tr_selfcheck_launch(kLayoutTA, TR_BF16, kOutC16Bias, ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- the forward product with a fused bias and residual add, X_out = X_in + (H W^T + b) (the kind TR_C16_BIAS_ADD): C = bf16((S +
// float(bias[n])) + float(r[m][n])), hgemm_residual.hpp's two fp32 adds in this order and one rounding, in the kernel's epilogue, in the
// combine and in the reference kernel.  A call resolves to the plan of the bgemm_mi355x_launch_tn_bias call with the same arguments; only
// the epi id of the plain dispatch and of the combine dispatch differs.  bias may be NULL (+0.0); r is read-only, has dact's rules for z and
// may be c where ldr == ldc.
int bgemm_mi355x_tn_bias_add_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldr) {
  return tr_runs(kLayoutTN, TR_BF16, out_bias_add(ldr), tn_config, M, N, K, lda, ldb, ldc);
}
int bgemm_mi355x_launch_tn_bias_add(int tn_config, int splits_arg, const void* a, const void* b_col_major, const void* bias, const void* r, void* c,
                                    int M, int N, int K, int lda, int ldb, int ldc, int ldr, void* stream) {
  return tr_launch(kLayoutTN, TR_BF16, out_bias_add(ldr), tn_config, splits_arg, a, b_col_major, bias, c, M, N, K, lda, ldb, ldc, stream, const_cast<void*>(r));
}
int bgemm_mi355x_tn_bias_add(const void* a, const void* b_col_major, const void* bias, const void* r, void* c, int M, int N, int K, void* stream) {
  if (!r) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutTN, TR_BF16, out_bias_add(N), a, b_col_major, bias, c, M, N, K, stream, const_cast<void*>(r));
}
// (bgemm_mi355x_selfcheck_launch_tn_bias_act_aux's output; operands & 4: a, b, c, r and a non-NULL bias are 16-byte aligned.  The NN twin shows
// the refusal: family n has no bias.)
int bgemm_mi355x_selfcheck_launch_tn_bias_add(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldr,
                                              int ruled_out, long long out[20]) {
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, out_bias_add(ldr), tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_nn_bias_add(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldr,
                                              int ruled_out, long long out[20]) {
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_bias_add(ldr), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- the gated forward product, H = act(X Wg^T + bg) (.) (X Wu^T + bu) (the kinds TR_C16_GATED + act): the work of the TN product of width
// 2 N, so the planned call asks bgemm_mi355x_tn_plan(M, 2 N, K) and the workspace is that product's; N is the output width everywhere else.
// act: HGEMM_ACT_RELU / _GELU / _GELU_TANH / _SILU, anything else HGEMM_ERR_BAD_ARG.  Either bias may be NULL: +0.0.
int bgemm_mi355x_tn_gated_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc) {
  return tr_runs(kLayoutTN, TR_BF16, out_gated(HGEMM_ACT_RELU), tn_config, M, N, K, lda, ldb, ldc);   // (no activation changes the answer)
}
int bgemm_mi355x_launch_tn_gated(int tn_config, int splits_arg, const void* a, const void* wg_col_major, const void* wu_col_major, const void* bias_g,
                                 const void* bias_u, void* c, int M, int N, int K, int lda, int ldb, int ldc, int act, void* stream) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutTN, TR_BF16, out_gated(act), tn_config, splits_arg, a, wg_col_major, bias_g, c, M, N, K, lda, ldb, ldc, stream, nullptr, nullptr,
                   wu_col_major, bias_u);
}
int bgemm_mi355x_tn_gated(const void* a, const void* wg_col_major, const void* wu_col_major, const void* bias_g, const void* bias_u, void* c, int M,
                          int N, int K, int act, void* stream) {
  if (!act_known_gated(act) || M <= 0 || N <= 0 || K <= 0 || N >= (1 << 30)) return HGEMM_ERR_BAD_ARG;   // (2 N is an int)
  int cfg, splits;
  tr_model_plan(kLayoutTN, M, 2 * N, K, &cfg, &splits);
  return bgemm_mi355x_launch_tn_gated(cfg, splits, a, wg_col_major, wu_col_major, bias_g, bias_u, c, M, N, K, K, K, N, act, stream);
}
// ---- the gated forward product's training form (the kinds TR_C16_GATED_AUX + act): the call above with g_out = bf16(g) and u_out = bf16(u)
// as two more outputs, both [M][ldz]; the activation and the gate read the unrounded g and u, so C is the gated call's C bit for bit.  Plan,
// workspace and reserve call are the gated call's.
int bgemm_mi355x_tn_gated_aux_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz) {
  return tr_runs(kLayoutTN, TR_BF16, out_gated_aux(HGEMM_ACT_RELU, ldz), tn_config, M, N, K, lda, ldb, ldc);
}
int bgemm_mi355x_launch_tn_gated_aux(int tn_config, int splits_arg, const void* a, const void* wg_col_major, const void* wu_col_major, const void* bias_g,
                                     const void* bias_u, void* c, void* g_out, void* u_out, int M, int N, int K, int lda, int ldb, int ldc, int ldz, int act,
                                     void* stream) {
  if (!act_known_gated(act) || !g_out || !u_out) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutTN, TR_BF16, out_gated_aux(act, ldz), tn_config, splits_arg, a, wg_col_major, bias_g, c, M, N, K, lda, ldb, ldc, stream, g_out, nullptr,
                   wu_col_major, bias_u, u_out);
}
int bgemm_mi355x_tn_gated_aux(const void* a, const void* wg_col_major, const void* wu_col_major, const void* bias_g, const void* bias_u, void* c, void* g_out,
                              void* u_out, int M, int N, int K, int act, void* stream) {
  if (!act_known_gated(act) || M <= 0 || N <= 0 || K <= 0 || N >= (1 << 30)) return HGEMM_ERR_BAD_ARG;   // (2 N is an int)
  int cfg, splits;
  tr_model_plan(kLayoutTN, M, 2 * N, K, &cfg, &splits);
  return bgemm_mi355x_launch_tn_gated_aux(cfg, splits, a, wg_col_major, wu_col_major, bias_g, bias_u, c, g_out, u_out, M, N, K, K, K, N, N, act, stream);
}
// (the gated hook's output; operands & 4: g_out and u_out are 16-byte aligned too)
int bgemm_mi355x_selfcheck_launch_tn_gated_aux(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldz,
                                               int ruled_out, int act, long long out[20]) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, out_gated_aux(act, ldz), tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_nn_gated_aux(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldz,
                                               int ruled_out, int act, long long out[20]) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_gated_aux(act, ldz), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_ta_gated_aux(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldz,
                                               int ruled_out, int act, long long out[20]) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTA, TR_BF16, out_gated_aux(act, ldz), ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
// (bgemm_mi355x_selfcheck_launch_tn_bias_act's output; operands & 4: a, both weights, c and every non-NULL bias are 16-byte aligned.  The NN
// and TA twins show the refusal.)
int bgemm_mi355x_selfcheck_launch_tn_gated(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                           int act, long long out[20]) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, out_gated(act), tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_nn_gated(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                           int act, long long out[20]) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_gated(act), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_ta_gated(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                           int act, long long out[20]) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTA, TR_BF16, out_gated(act), ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- the forward product with a fused bias and activation, Y = act(X W^T + b) (the kinds TR_C16_BIAS + act): C = bf16(act32(z)),
// z = fl32(S + float(bias[n])) exactly bgemm_mi355x_tn_bias's value before its rounding; the activation (hgemm_act.hpp) is applied to the
// unrounded z, never to a slab, and the result is rounded once.  A call resolves to the plan of the bgemm_mi355x_launch_tn call with the
// same arguments; only the epi id of the plain dispatch and of the combine dispatch differs.  act: HGEMM_ACT_RELU / _GELU / _GELU_TANH,
// anything else HGEMM_ERR_BAD_ARG (a caller with no activation has bgemm_mi355x_tn_bias).
int bgemm_mi355x_tn_bias_act_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc) {
  return tr_runs(kLayoutTN, TR_BF16, out_bias_act(HGEMM_ACT_RELU), tn_config, M, N, K, lda, ldb, ldc);   // (no activation changes the answer)
}
int bgemm_mi355x_launch_tn_bias_act(int tn_config, int splits_arg, const void* a, const void* b_col_major, const void* bias, void* c, int M, int N,
                                    int K, int lda, int ldb, int ldc, int act, void* stream) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutTN, TR_BF16, out_bias_act(act), tn_config, splits_arg, a, b_col_major, bias, c, M, N, K, lda, ldb, ldc, stream);
}
int bgemm_mi355x_tn_bias_act(const void* a, const void* b_col_major, const void* bias, void* c, int M, int N, int K, int act, void* stream) {
  if (!act_known(act) || !bias) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutTN, TR_BF16, out_bias_act(act), a, b_col_major, bias, c, M, N, K, stream);
}
// (the output layout of bgemm_mi355x_selfcheck_launch_tn_bias; the NN and TA twins show the refusal)
int bgemm_mi355x_selfcheck_launch_tn_bias_act(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                              int act, long long out[20]) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, out_bias_act(act), tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_nn_bias_act(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                              int act, long long out[20]) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_bias_act(act), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_ta_bias_act(int ta_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ruled_out,
                                              int act, long long out[20]) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTA, TR_BF16, out_bias_act(act), ta_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- the same forward product that also writes the rounded pre-activation (the kinds TR_C16_BIAS_AUX + act): z_out = bf16(z) at row stride
// ldz and C = bf16(act32(z)) of the unrounded z -- C is bgemm_mi355x_launch_tn_bias_act's and z_out bgemm_mi355x_launch_tn_bias's, bit for
// bit, for the same arguments and plan.  z_out has C's rules; NULL and z_out == c are HGEMM_ERR_BAD_ARG.
int bgemm_mi355x_tn_bias_act_aux_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz) {
  return tr_runs(kLayoutTN, TR_BF16, out_bias_act_aux(HGEMM_ACT_RELU, ldz), tn_config, M, N, K, lda, ldb, ldc);
}
int bgemm_mi355x_launch_tn_bias_act_aux(int tn_config, int splits_arg, const void* a, const void* b_col_major, const void* bias, void* c, void* z_out,
                                        int M, int N, int K, int lda, int ldb, int ldc, int ldz, int act, void* stream) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutTN, TR_BF16, out_bias_act_aux(act, ldz), tn_config, splits_arg, a, b_col_major, bias, c, M, N, K, lda, ldb, ldc, stream, z_out);
}
int bgemm_mi355x_tn_bias_act_aux(const void* a, const void* b_col_major, const void* bias, void* c, void* z_out, int M, int N, int K, int act,
                                 void* stream) {
  if (!act_known(act) || !bias || !z_out) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutTN, TR_BF16, out_bias_act_aux(act, N), a, b_col_major, bias, c, M, N, K, stream, z_out);
}
// (bgemm_mi355x_selfcheck_launch_tn_bias_act's output; operands & 4: a, b, bias, c AND z_out are 16-byte aligned)
int bgemm_mi355x_selfcheck_launch_tn_bias_act_aux(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldz,
                                                  int ruled_out, int act, long long out[20]) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, out_bias_act_aux(act, ldz), tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- the input gradient through the activation, dZ = (dY W) (.) act'(Z) (the kinds TR_C16_DACT + act, family n, bf16): C = bf16(S x
// dact32(float(z[m][n]))), one fp32 multiply on the finished sum (ReLU: a select) and one rounding; hgemm_act.hpp's dact_mul in the kernel's
// epilogue, in the combine and in the reference kernel.  A call resolves to the plan of the bgemm_mi355x_launch_nn call with the same
// arguments; only the epi id of the plain dispatch and of the combine dispatch differs.  z is read-only and has C's rules.
int bgemm_mi355x_nn_dact_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz) {
  return tr_runs(kLayoutNN, TR_BF16, out_dact(HGEMM_ACT_RELU, ldz), nn_config, M, N, K, lda, ldb, ldc);
}
int bgemm_mi355x_launch_nn_dact(int nn_config, int splits_arg, const void* a, const void* b, const void* z, void* c, int M, int N, int K, int lda,
                                int ldb, int ldc, int ldz, int act, void* stream) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutNN, TR_BF16, out_dact(act, ldz), nn_config, splits_arg, a, b, nullptr, c, M, N, K, lda, ldb, ldc, stream, const_cast<void*>(z));
}
int bgemm_mi355x_nn_dact(const void* a, const void* b, const void* z, void* c, int M, int N, int K, int act, void* stream) {
  if (!act_known(act) || !z) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutNN, TR_BF16, out_dact(act, N), a, b, nullptr, c, M, N, K, stream, const_cast<void*>(z));
}
// ---- the input gradient with a fused residual add, dX = dZ W + dX_out (the kind TR_C16_ADD, family n, bf16): C = bf16(S + float(r[m][n])),
// hgemm_residual.hpp's one fp32 add on the finished sum and one rounding.  A call resolves to the plan of the bgemm_mi355x_launch_nn call with
// the same arguments; only the epi id of the plain dispatch and of the combine dispatch differs.  r as in bgemm_mi355x_launch_tn_bias_add.
int bgemm_mi355x_nn_add_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldr) {
  return tr_runs(kLayoutNN, TR_BF16, out_add(ldr), nn_config, M, N, K, lda, ldb, ldc);
}
int bgemm_mi355x_launch_nn_add(int nn_config, int splits_arg, const void* a, const void* b, const void* r, void* c, int M, int N, int K, int lda,
                               int ldb, int ldc, int ldr, void* stream) {
  return tr_launch(kLayoutNN, TR_BF16, out_add(ldr), nn_config, splits_arg, a, b, nullptr, c, M, N, K, lda, ldb, ldc, stream, const_cast<void*>(r));
}
int bgemm_mi355x_nn_add(const void* a, const void* b, const void* r, void* c, int M, int N, int K, void* stream) {
  if (!r) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutNN, TR_BF16, out_add(N), a, b, nullptr, c, M, N, K, stream, const_cast<void*>(r));
}
// (not part of the public header; the TN twin shows the refusal: family f's residual call is the bias form)
int bgemm_mi355x_selfcheck_launch_nn_add(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldr,
                                         int ruled_out, long long out[20]) {
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_add(ldr), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
int bgemm_mi355x_selfcheck_launch_tn_add(int tn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldr,
                                         int ruled_out, long long out[20]) {
  return tr_selfcheck_launch(kLayoutTN, TR_BF16, out_add(ldr), tn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
// ---- the gated MLP's input gradient, dG = (dY Wd) (.) U (.) act'(G) and dU = act(G) (.) (dY Wd) (the kinds TR_C16_DGATED + act, family n,
// bf16, HGEMM_ACT_SILU included): hgemm_dgated.hpp's dgated_store on the finished sum in the kernel's epilogue, in the combine and in the
// reference kernel.  A call resolves to the plan of the bgemm_mi355x_launch_nn_dact call with the same arguments (z = g).
int bgemm_mi355x_nn_dgated_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldz, int ldc) {
  return tr_runs(kLayoutNN, TR_BF16, out_dgated(HGEMM_ACT_RELU, ldz), nn_config, M, N, K, lda, ldb, ldc);
}
int bgemm_mi355x_launch_nn_dgated(int nn_config, int splits_arg, const void* a, const void* b, const void* g, const void* u, void* dg, void* du, int M,
                                  int N, int K, int lda, int ldb, int ldz, int ldc, int act, void* stream) {
  if (!act_known_gated(act) || !g || !u || !dg || !du) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutNN, TR_BF16, out_dgated(act, ldz), nn_config, splits_arg, a, b, u, dg, M, N, K, lda, ldb, ldc, stream, const_cast<void*>(g), nullptr,
                   nullptr, du);
}
int bgemm_mi355x_nn_dgated(const void* a, const void* b, const void* g, const void* u, void* dg, void* du, int M, int N, int K, int act, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return HGEMM_ERR_BAD_ARG;
  int cfg, splits;
  tr_model_plan(kLayoutNN, M, N, K, &cfg, &splits);
  return bgemm_mi355x_launch_nn_dgated(cfg, splits, a, b, g, u, dg, du, M, N, K, K, N, N, N, act, stream);
}
// (not part of the public header)
int bgemm_mi355x_selfcheck_launch_nn_dgated(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldz, int ldc,
                                            int ruled_out, int act, long long out[20]) {
  if (!act_known_gated(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_dgated(act, ldz), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}
// ---- the same with the bias gradient (the kinds TR_C16_DACT_DBIAS + act, family n, bf16): C is bgemm_mi355x_launch_nn_dact's C bit for bit
// and db32[n] (+)= sum over m of float(C[m][n]), the rounded values, in fp32 in an order fixed by the plan (tr_resolve; hgemm_dbias.hpp).
int bgemm_mi355x_nn_dact_dbias_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz) {
  return tr_runs(kLayoutNN, TR_BF16, out_dact_dbias(HGEMM_ACT_RELU, ldz, false), nn_config, M, N, K, lda, ldb, ldc);
}
int bgemm_mi355x_launch_nn_dact_dbias(int nn_config, int splits_arg, const void* a, const void* b, const void* z, void* c, float* db32, int M, int N,
                                      int K, int lda, int ldb, int ldc, int ldz, int act, int accumulate, void* stream) {
  if (!act_known(act) || !db32 || (accumulate != 0 && accumulate != 1)) return HGEMM_ERR_BAD_ARG;
  return tr_launch(kLayoutNN, TR_BF16, out_dact_dbias(act, ldz, accumulate == 1), nn_config, splits_arg, a, b, nullptr, c, M, N, K, lda, ldb, ldc, stream,
                   const_cast<void*>(z), db32);
}
int bgemm_mi355x_nn_dact_dbias(const void* a, const void* b, const void* z, void* c, float* db32, int M, int N, int K, int act, int accumulate,
                               void* stream) {
  if (!act_known(act) || !z || !db32 || (accumulate != 0 && accumulate != 1)) return HGEMM_ERR_BAD_ARG;
  return tr_run(kLayoutNN, TR_BF16, out_dact_dbias(act, N, accumulate == 1), a, b, nullptr, c, M, N, K, stream, const_cast<void*>(z), db32);
}
// what the launch asks ensure_workspace for with this plan on contiguous operands: the counter block, the K slices' slabs of a two-pass
// plan and the column sum's partials (0: the plan needs none)
size_t bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes(int nn_config, int splits, int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const LaunchPlan p = tr_resolve(kLayoutNN, TR_BF16, out_dact_dbias(HGEMM_ACT_RELU, N, false), nn_config, splits, true, M, N, K, K, N, N, 0);
  return p.status == HGEMM_OK && p.slab_bytes ? kCounterBytes + p.slab_bytes : 0;
}
int bgemm_mi355x_nn_dact_dbias_reserve_workspace(int M, int N, int K, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return HGEMM_ERR_BAD_ARG;
  int cfg = 0, splits = 1;
  tr_model_plan(kLayoutNN, M, N, K, &cfg, &splits);
  const size_t ws = bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes(cfg, splits, M, N, K);
  if (!ws) return HGEMM_OK;
  float* slabs = nullptr; unsigned* counters = nullptr;
  const int rc = ensure_workspace(ws - kCounterBytes, (hipStream_t)stream, &slabs, &counters);
  return rc == HGEMM_ERR_NO_WORKSPACE_INTERNAL ? HGEMM_ERR_NO_WORKSPACE : rc;
}
// (not part of the public header; out = {form, dispatches, slab bytes, counters (0)} and up to five dispatches: 44 words.  ruled_out:
// 1 << FORM_SPLITK as its siblings, 1 << FORM_PLAIN: no workspace at all)
int bgemm_mi355x_selfcheck_launch_nn_dact_dbias(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldz,
                                                int ruled_out, int act, long long out[44]) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_dact_dbias(act, ldz, false), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// ---- the column sum on its own: out32[n] (+)= sum over m of float(x[m][n]), x bf16 [M][ldx] -- the bias gradient of a layer without an
// activation (db = sum over m of dY) and part 2 of the call above.  M > COLSUM_DIRECT_ROWS and a workspace: row blocks to partials and the
// finish kernel; otherwise one thread per column (hgemm_dbias.hpp).
int bgemm_mi355x_colsum_c32(const void* x, float* out32, int M, int N, int ldx, int accumulate, void* stream) {
  DisarmTiming disarm_timing;
  if (!x || !out32 || M <= 0 || N <= 0 || ldx < N || (accumulate != 0 && accumulate != 1)) return HGEMM_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* partial = nullptr; unsigned* counters = nullptr;
  if (M > COLSUM_DIRECT_ROWS) {
    const int st = ensure_workspace((size_t)colsum_blocks(M) * N * sizeof(float), s, &partial, &counters);
    if (st != HGEMM_OK && st != HGEMM_ERR_NO_WORKSPACE_INTERNAL) return st;
    if (st != HGEMM_OK) partial = nullptr;
  }
  if (partial) {
    launch_colsum_blocked(x, partial, M, N, ldx, s, timing_slot(true, false));
    launch_colsum_finish(partial, out32, colsum_blocks(M), N, accumulate == 1, s, timing_slot(false, true));
  } else {
    launch_colsum_direct(x, out32, M, N, ldx, accumulate == 1, s, timing_slot(true, true));
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) { g_last_hip_error = (int)err; return HGEMM_ERR_HIP; }
  return HGEMM_OK;
}

// (not part of the public header: the byte range of the dact kernels' Z descriptor for the tile at row m0, the kernels' own function)
unsigned bgemm_mi355x_selfcheck_dact_z_range(int M, int N, int ldz, int m0) { return dact_z_range_bytes(M, N, ldz, m0); }
int bgemm_mi355x_selfcheck_launch_nn_dact(int nn_config, int splits, int operands, int M, int N, int K, int lda, int ldb, int ldc, int ldz,
                                          int ruled_out, int act, long long out[20]) {
  if (!act_known(act)) return HGEMM_ERR_BAD_ARG;
  return tr_selfcheck_launch(kLayoutNN, TR_BF16, out_dact(act, ldz), nn_config, splits, operands, M, N, K, lda, ldb, ldc, ruled_out, out);
}

// Host-side self-check hook (tests/test_host_logic.py; not part of the public header): the raster map of the
// kernels evaluated on the host, with true divisions (use_fast = 0) or with the multipliers the launch path would
// pass (use_fast = 1).  out = {split, tile, tile_m, tile_n}.
int hgemm_mi355x_selfcheck_raster(int tiles_m, int tiles_n, int group_m, int tail_first, int tail_tiles, int bid, int use_fast,
                                  int out[4]) {
  if (tiles_m < 1 || tiles_n < 1 || group_m < 1 || bid < 0 || !out) return HGEMM_ERR_BAD_ARG;
  const RasterPos r = use_fast ? raster_fast(bid, tiles_m, tiles_n, group_m, tail_first, tail_tiles,
                                             make_raster_div(tiles_m, tiles_n, group_m, tail_tiles))
                               : raster_ref(bid, tiles_m, tiles_n, group_m, tail_first, tail_tiles);
  out[0] = r.split; out[1] = r.tile; out[2] = r.tile_m; out[3] = r.tile_n;
  return HGEMM_OK;
}
// the stream-K partition as the kernels evaluate it: out[0] = first stage of workgroup w's run (w = G: the total), out[1] = the
// workgroup that owns stage x
int hgemm_mi355x_selfcheck_streamk(int tiles, int steps, int G, int min_steps, int w, int x, int out[2]) {
  if (tiles < 1 || steps < 1 || G < 1 || min_steps < 1 || w < 0 || !out || (long)tiles * steps >= (1L << 30)) return HGEMM_ERR_BAD_ARG;
  const StreamK sk = make_streamk(tiles, steps, G, min_steps);
  out[0] = sk_start(sk, w, G);
  out[1] = (x >= 0 && (long)x < (long)tiles * steps) ? sk_owner(sk, x, G) : -1;
  return HGEMM_OK;
}
// how hgemm_mi355x_launch cuts K for (geometry, K, requested split count): out = {stages, splits, k_chunk, direct tail (0 / 1)}
int hgemm_mi355x_selfcheck_ksplit(int config_id, int K, int splits, int out[4]) {
  if (config_id < 0 || config_id >= g_num_kernels || K <= 0 || splits < 1 || !out || !k_ok(g_kernel_table[config_id], K)) return HGEMM_ERR_BAD_ARG;
  const KSplit r = split_k(g_kernel_table[config_id], K, splits);
  out[0] = r.steps; out[1] = r.splits; out[2] = r.k_chunk; out[3] = r.tail_direct ? 1 : 0;
  return HGEMM_OK;
}
// what hgemm_mi355x_launch decides for a call, nothing launched: operands = 1 (b given) | 2 (b_col_major given) | 4 (pointers
// 16-byte aligned; dimensions and strides are checked as the launch checks them), ruled_out = 1 << form of the workspace-backed forms
// that got no workspace.  Returns the call's status; out = {form, dispatches, slab bytes, counters (0 / 1)}, then for each dispatch
// {thunk, grid, epi, splits, k_chunk, items, start, stop}.
int hgemm_mi355x_selfcheck_launch(int config_id, int splits, int group_m, int operands, int M, int N, int K, int lda, int ldb, int ldc,
                                  int ruled_out, long long out[28]) {
  if (M <= 0 || N <= 0 || K <= 0 || config_id >= g_num_kernels || config_id < HGEMM_CONFIG_RAGGED || !out) return HGEMM_ERR_BAD_ARG;
  const bool aligned = (operands & 4) && mfma_path_ok(nullptr, nullptr, nullptr, M, N, K, lda, ldb, ldc);
  return show_plan(resolve_launch(config_id, splits, group_m, operands & 1, operands & 2, aligned, M, N, K, lda, ldb, ldc, ruled_out), out);
}
unsigned hgemm_mi355x_selfcheck_fastdiv(unsigned n, unsigned d) { return d ? fast_div(n, make_fast_div(d)) : 0xFFFFFFFFu; }

const char* hgemm_mi355x_strerror(int status) {
  switch (status) {
    case HGEMM_OK: return "ok";
    case HGEMM_ERR_BAD_ARG: return "bad argument";
    case HGEMM_ERR_TOO_LARGE: return "operand too large for 32-bit tile addressing";
    case HGEMM_ERR_HIP: return "HIP runtime error";
    case HGEMM_ERR_BACKEND: return "rocBLAS/hipBLASLt error";
    case HGEMM_ERR_NOT_READY: return "baseline not initialised / no algorithm selected";
    case HGEMM_ERR_NO_ALGO: return "hipBLASLt returned no usable algorithm";
    case HGEMM_ERR_NO_WORKSPACE: return "no split-K workspace (lent buffer too small, out of memory, or stream capturing)";
    default: return "unknown status";
  }
}

int hgemm_mi355x_last_hip_error(void) { return g_last_hip_error; }

// ---- measurement helpers (bench.py): kernel-exact timing without marker packets between launches ----
void* hgemm_mi355x_event_create(void) {
  hipEvent_t e = nullptr;
  return hipEventCreate(&e) == hipSuccess ? (void*)e : nullptr;
}
int hgemm_mi355x_event_destroy(void* ev) { return hipEventDestroy((hipEvent_t)ev) == hipSuccess ? HGEMM_OK : HGEMM_ERR_HIP; }
int hgemm_mi355x_time_next_launch(void* start_event, void* stop_event) {
  if ((start_event == nullptr) != (stop_event == nullptr)) return HGEMM_ERR_BAD_ARG;
  hgemm_mi355x::t_launch_timing.start = (hipEvent_t)start_event;
  hgemm_mi355x::t_launch_timing.stop = (hipEvent_t)stop_event;
  return HGEMM_OK;
}
double hgemm_mi355x_event_elapsed_us(void* start_event, void* stop_event) {
  float ms = 0.f;
  if (hipEventSynchronize((hipEvent_t)stop_event) != hipSuccess) return -1.0;
  if (hipEventElapsedTime(&ms, (hipEvent_t)start_event, (hipEvent_t)stop_event) != hipSuccess) return -1.0;
  return (double)ms * 1e3;
}

#ifdef HGEMM_ABLATION
// tuner-only library build (lib_ablation/): results are garbage by construction, never shipped
int hgemm_mi355x_set_debug(int flags) { const int old = g_debug_flags; g_debug_flags = flags; return old; }
#endif

#ifdef HGEMM_TIMELINE
// measurement library build (lib_tl/), never shipped: see HGEMM_TL_* in hgemm_kernel.hpp.  The buffer must hold
// slots * 1024 * 16 eight-byte words; returns the number of launches recorded so far.
int hgemm_mi355x_set_timeline(void* device_ptr, int slots) {
  g_timeline = (unsigned long long*)device_ptr;
  g_timeline_slots = device_ptr ? slots : 0;
  const int n = (int)g_timeline_count;
  g_timeline_count = 0;
  return n;
}
#endif

const char* hgemm_mi355x_version(void) { return "hgemm_mi355x 0.2 (gfx950)"; }

}  // extern "C"
