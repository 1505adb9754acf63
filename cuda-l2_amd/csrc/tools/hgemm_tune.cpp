// hgemm_tune -- native (no torch) checker / autotuner / micro-benchmark for libhgemm_mi355x.so.
//
//   hgemm_tune check [--shapes M_N_K,...] [--configs a,b]   every (or the named) geometry x split-K form, BIT-EXACT against an exact
//                                                     integer reference on the reference's {0,1} inputs
//                                                     (zero_one_correctness_check.py:65-92,263-268)
//   hgemm_tune tune  --shapes M_N_K,... | --shape-file F  [--out F.jsonl] [--keep R] [--baselines] [--fused] [--streamk] [--nt]
//                                                     time candidate plans, print one JSON line per shape
//   hgemm_tune tune  --plan-only --baselines --interleave [--stream] [--autotune] [--also CONFIG:SPLITS:GROUP,...] --shapes ...
//                                                     the library's plan, the vendor baselines and the named explicit plans in the
//                                                     same interleaved rounds (family u: a candidate only by name, --configs / --also)
//   hgemm_tune bench --shape M_N_K [--config NAME --splits S --group G] [--reps N] [--lib]
//                                                     run one plan N times (for rocprofv3)
//   hgemm_tune bench --shape M_N_K --baseline X --isolated [--reps N]   a vendor baseline one launch at a time (for rocprofv3 --pmc)
//   hgemm_tune bench --shape M_N_K --timeline [...]   (measurement library lib_tl/ only) in-kernel clock stamps of back-to-back launches
//   hgemm_tune bench --shape M_N_K --power [--seconds S] [--baseline hipblaslt_tn|hipblaslt_nn|rocblas_tn] [...]
//                                                     back-to-back launches for S seconds (no sync in between); reports
//                                                     us per call and the board's gfx clock / socket power sampled over
//                                                     the timed region (rocm_smi gpu metrics, every 10 ms)
//   hgemm_tune check --layout nn [--shapes ...]       family n (B row-major, hgemm_mi355x_launch_nn): every member x {plain, NT stores,
//                                                     two-pass splits 2 / 5}, bit-exact as above
//   hgemm_tune check --layout ta [--shapes ...]       family a (A given as [K][M], hgemm_mi355x_launch_ta): the same check
//   hgemm_tune bench --layout ta --shapes ... [--out F.jsonl]
//   hgemm_tune check --layout ta --c32 [--shapes ...] fp32 C (hgemm_mi355x_launch_ta_c32): the same forms x {store, accumulate}, exact
//   hgemm_tune bench --layout ta --c32 --shapes ... [--out F.jsonl]   the accumulate call against ta_fp32 + an elementwise add
//                                                     that check first, then per shape interleaved rounds of the planned TA call, the
//                                                     NN call on a pre-transposed A, a copy of A's bytes + that NN call, rocBLAS
//   hgemm_tune check --layout nn|ta [--c32] --bf16 [--shapes ...]   the bfloat16 calls (bgemm_mi355x_launch_nn / _ta / _ta_c32): the same
//                                                     check, the expected 16-bit C rounded to bf16 once (nearest even)
//   hgemm_tune bench --layout nn|ta [--c32] --bf16 --shapes ... [--out F.jsonl]
//                                                     that check first, then per shape interleaved rounds of the planned bf16 call, the
//                                                     fp16 call of the same plan and shape (c32: both accumulate) and -- context only --
//                                                     rocBLAS with bf16 in and out; "bf16_le_fp16": bf16 <= fp16 + the fp16 call's own
//                                                     round-to-round spread (its slowest round minus its median)
//   hgemm_tune check --layout tn --bf16 [--shapes ...] the bf16 forward product (bgemm_mi355x_launch_tn, family f: B given as b_col_major)
//   hgemm_tune bench --layout tn --bf16 --shapes ... [--out F.jsonl]
//   hgemm_tune check --layout tn --bf16 --bias [--shapes ...]   the fused-bias calls (bgemm_mi355x_launch_tn_bias): bf16(S + bias[n])
//   hgemm_tune bench --layout tn --bf16 --bias --shapes ... [--out F.jsonl]   against the same plan without a bias, "bias_le_plain"
//   hgemm_tune check --layout tn --bf16 --bias --act relu|gelu|gelu_tanh [--shapes ...]   the fused bias+activation calls
//                                                     (bgemm_mi355x_launch_tn_bias_act): ReLU bit for bit, the GELUs inside their bar
//   hgemm_tune check|bench --layout tn --bf16 --bias --act A --aux [...]   bgemm_mi355x_tn_bias_act_aux: C to the bars above, z_out = bf16(z)
//                                                     bit for bit; bench against bgemm_mi355x_launch_tn_bias + an element-wise act(Z) kernel
//   hgemm_tune check|bench --layout nn --bf16 --dact relu|gelu|gelu_tanh [...]   bgemm_mi355x_nn_dact: ReLU bit for bit, the GELUs inside
//                                                     1/2 ulp_bf16(S g*) + 2^-19 |S|; bench against bgemm_mi355x_launch_nn + an element-wise kernel
//   hgemm_tune check|bench --layout nn --bf16 --dact A --dbias [...]   bgemm_mi355x_nn_dact_dbias: C to the bars above and bit for bit the
//                                                     dact call's, db32 against the fp64 column sum of the C read back -- ReLU bit for bit, the
//                                                     GELUs inside gamma_(M-1) sum |C| --, accumulate = 1 one fp32 add; bench against
//                                                     bgemm_mi355x_launch_nn_dact + bgemm_mi355x_colsum_c32 at the same member and splits
//   hgemm_tune check|bench --layout tn --bf16 --gated-aux relu|gelu|gelu_tanh|silu [...]   bgemm_mi355x_launch_tn_gated_aux: C as --gated judges it,
//                                                     g_out and u_out bit for bit, sentinel bytes behind each of the three; bench against
//                                                     bgemm_mi355x_launch_tn_bias on the stacked weight at 2N + the element-wise gate kernel
//   hgemm_tune check|bench --layout tn --bf16 --bias-add [...]   bgemm_mi355x_launch_tn_bias_add: C = bf16((S + bias) + r) bit for bit, every run
//                                                     once out of place and once in place (r == c); bench against bgemm_mi355x_launch_tn_bias +
//                                                     an element-wise add at the same member and splits
//   hgemm_tune check|bench --layout nn --bf16 --nn-add [...]     bgemm_mi355x_launch_nn_add: C = bf16(S + r), the same check; bench against
//                                                     bgemm_mi355x_launch_nn + an element-wise add
//   hgemm_tune check|bench --layout nn --bf16 --dgated relu|gelu|gelu_tanh|silu [...]   bgemm_mi355x_launch_nn_dgated: ReLU bit for bit, the
//                                                     others inside the two bars of hgemm_dgated.hpp, sentinel bytes behind both outputs; bench
//                                                     against bgemm_mi355x_launch_nn + an element-wise kernel at the same member and splits
//   hgemm_tune bench --layout tn --bf16 --bias --act A --shapes ... [--out F.jsonl]   against bgemm_mi355x_launch_tn_bias followed by an
//                                                     element-wise activation kernel, "act_le_unfused"
//                                                     that check first, then per shape interleaved rounds of the planned call, of
//                                                     bgemm_mi355x_launch_nn with the same member and splits, and -- context -- rocBLAS
//   hgemm_tune bench --layout nn --shapes ... [--autotune] [--out F.jsonl]
//                                                     that check first, then per shape interleaved rounds of the planned NN call, the
//                                                     reference kernel on the same operands, hipBLASLt _nn and the shipped TN plan
//
// This is the offline replacement for the reference's first-call in-process autotune variants
// (h100 kernels that time several variants on first invocation): plans are
// measured here, committed as csrc/hgemm_tuned_table.inc, and the hot path only does a table probe.
// Timing: HIP events around each launch on the launch stream, operands N(0,1) (never zeros: DVFS,
// MI355X_MICROARCH.md), buffer sets rotated so consecutive launches do not re-hit L2/MALL lines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <fstream>
#include <functional>
#include <sstream>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <rocm_smi/rocm_smi.h>

#include "../../../include/hgemm_mi355x.h"
#include "../hgemm_act.hpp"
#include "../hgemm_dbias.hpp"
#include "../hgemm_dgated.hpp"
#include "../hgemm_gated.hpp"
#include "../hgemm_residual.hpp"

// Ablation switches exist only in the -DHGEMM_ABLATION build of the library (build.py: HGEMM_LIB_SUFFIX=ablation
// HGEMM_EXTRA_HIPFLAGS=-DHGEMM_ABLATION); against the shipping library the symbol is absent and --debug refuses.
extern "C" int hgemm_mi355x_set_debug(int flags) __attribute__((weak));
// Timeline stamps exist only in the -DHGEMM_TIMELINE build (lib_tl/); bench --timeline refuses without it.
extern "C" int hgemm_mi355x_set_timeline(void* device_ptr, int slots) __attribute__((weak));

#define HIP_OK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                            \
    }                                                                                     \
  } while (0)

typedef _Float16 f16;

struct Shape { int M, N, K; };

static std::vector<Shape> parse_shapes(const std::string& s) {
  std::vector<Shape> out;
  std::stringstream ss(s);
  std::string tok;
  while (std::getline(ss, tok, ',')) {
    Shape sh;
    if (sscanf(tok.c_str(), "%d_%d_%d", &sh.M, &sh.N, &sh.K) == 3) out.push_back(sh);
  }
  return out;
}

static std::vector<Shape> read_shape_file(const char* path) {
  std::vector<Shape> out;
  std::ifstream f(path);
  std::string line;
  while (std::getline(f, line)) {
    Shape sh;
    if (sscanf(line.c_str(), "%d_%d_%d", &sh.M, &sh.N, &sh.K) == 3) out.push_back(sh);
  }
  return out;
}

static size_t g_pad_alloc_mib = 0;  // --pad-alloc N: a dummy N-MiB allocation in front of the operand sets (moves their physical placement:
                                    // lock-step K walks over 32-KiB-strided rows are sensitive to which HBM channels the rows land on)
static int g_ld_override = -1;     // --ld N: pass lda = ldb = N (0 = every tile row aliases row 0: cache-hit ablation)
static bool g_zero_fill = false;  // --fill zero: DVFS experiment only (never for quoted numbers)

struct Buffers {
  f16 *a = nullptr, *b = nullptr, *bt = nullptr, *c = nullptr;
};

__global__ void transpose_kernel(const f16* __restrict__ b, f16* __restrict__ bt, int K, int N) {
  // bt[n][k] = b[k][n]; small helper, not on any timed path
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)K * N) return;
  const int n = (int)(idx / K), k = (int)(idx % K);
  bt[idx] = b[(size_t)k * N + n];
}

static void alloc_set(Buffers& s, const Shape& shape, unsigned long long seed, bool need_b) {
  Shape sh = shape;
  if (g_ld_override > sh.K) sh.K = g_ld_override;  // padded-row experiment: rows are ld apart
  HIP_OK(hipMalloc(&s.a, (size_t)sh.M * sh.K * 2));
  HIP_OK(hipMalloc(&s.bt, (size_t)sh.N * sh.K * 2));
  HIP_OK(hipMalloc(&s.c, (size_t)sh.M * sh.N * 2));
  if (g_zero_fill) {
    HIP_OK(hipMemset(s.a, 0, (size_t)sh.M * sh.K * 2));
    HIP_OK(hipMemset(s.bt, 0, (size_t)sh.N * sh.K * 2));
    if (need_b) { HIP_OK(hipMalloc(&s.b, (size_t)sh.K * sh.N * 2)); HIP_OK(hipMemset(s.b, 0, (size_t)sh.K * sh.N * 2)); }
    HIP_OK(hipDeviceSynchronize());
    return;
  }
  hgemm_fill_normal_f16(s.a, (size_t)sh.M * sh.K, seed * 3 + 1, nullptr);
  if (need_b) {
    HIP_OK(hipMalloc(&s.b, (size_t)sh.K * sh.N * 2));
    hgemm_fill_normal_f16(s.b, (size_t)sh.K * sh.N, seed * 3 + 2, nullptr);
    const size_t n = (size_t)sh.K * sh.N;
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, s.b, s.bt, sh.K, sh.N);
  } else {
    hgemm_fill_normal_f16(s.bt, (size_t)sh.N * sh.K, seed * 3 + 2, nullptr);
  }
  HIP_OK(hipDeviceSynchronize());
}

static void free_set(Buffers& s) {
  if (s.a) HIP_OK(hipFree(s.a));
  if (s.b) HIP_OK(hipFree(s.b));
  if (s.bt) HIP_OK(hipFree(s.bt));
  if (s.c) HIP_OK(hipFree(s.c));
  s = Buffers();
}

static double median(std::vector<float> v) {
  if (v.empty()) return 1e30;
  std::sort(v.begin(), v.end());
  const size_t m = v.size() / 2;
  return v.size() % 2 ? v[m] : 0.5 * (v[m] + v[m - 1]);
}

struct Plan { int cfg, splits, group_m; double model_us; };
static bool g_plan_only = false;  // tune --plan-only

// Time one callable over rotating buffer sets; returns median microseconds.
// The callable returns the library status: a candidate that errors (bad geometry for the shape, no
// workspace, backend failure) is reported with 1e30 us and can never win.
constexpr double kFailedUs = 1e30;
static int g_cooldown_ms = 0;   // tune / bench: --cooldown-ms
static double g_stream_box_s = 0;   // tune --stream-seconds: length of a back-to-back box (default 8 / 12 ms)
template <class F>
static double time_us(F&& launch, std::vector<Buffers>& sets, int warm, int reps, hipEvent_t e0, hipEvent_t e1) {
  // --cooldown-ms N (round 5): every isolated timing starts N ms after the previous work has drained -- for every contender alike.
  // Why: the plan report with a 1 s autotune budget times OUR plan first for each shape, i.e. right behind the previous shape's two
  // seconds of sustained hipBLASLt launches, and the board's power management was still throttling: on the >= 1e11-FLOP shapes our
  // isolated launches read 8.8 % above our own back-to-back figure in that run (2.2 % in a run without the autotune search), the
  // heuristic's, timed third and fourth, 0.5 % (tuning/r05_grid_plan_report_autotune_mi355x.jsonl).
  if (g_cooldown_ms > 0) {
    HIP_OK(hipDeviceSynchronize());
    std::this_thread::sleep_for(std::chrono::milliseconds(g_cooldown_ms));
  }
  for (int i = 0; i < warm; ++i)
    if (launch(sets[i % sets.size()]) != HGEMM_OK) return kFailedUs;
  HIP_OK(hipDeviceSynchronize());
  std::vector<float> t;
  for (int i = 0; i < reps; ++i) {
    Buffers& s = sets[i % sets.size()];
    HIP_OK(hipEventRecord(e0, nullptr));
    if (launch(s) != HGEMM_OK) return kFailedUs;
    HIP_OK(hipEventRecord(e1, nullptr));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    t.push_back(ms * 1000.f);
  }
  return median(t);
}

// back-to-back launches between one event pair (what bench.py's timed region and a serving loop do): us per call
template <class F>
static double stream_us(F&& launch, std::vector<Buffers>& sets, double seconds, hipEvent_t e0, hipEvent_t e1, double est_us) {
  const int reps = (int)std::max(8.0, std::min(20000.0, seconds * 1e6 / std::max(1.0, est_us)));
  for (int i = 0; i < std::max(4, reps / 4); ++i)
    if (launch(sets[i % sets.size()]) != HGEMM_OK) return kFailedUs;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipEventRecord(e0, nullptr));
  for (int i = 0; i < reps; ++i) (void)launch(sets[i % sets.size()]);
  HIP_OK(hipEventRecord(e1, nullptr));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  return ms * 1000.0 / reps;
}

// tune --rank both: candidates are ranked by sqrt(isolated x back-to-back) time.  The isolated launch is what the reference's
// harness times (a device sync either side of every call), the back-to-back stream is what a model runs; a plan that is level
// in one and 10 % better in the other should win (16384^2 x 128: 256x128 tiles with streaming C stores 158 / 133 us against
// 157 / 148 for 128x128 tiles).  Candidates slower than 1.25x the best isolated time are dropped unmeasured.
static bool g_rank_both = false;
static bool g_stream_report = false;   // tune --plan-only --baselines --stream
static bool g_try_nt = false;   // tune --nt: streaming C stores for the winner, judged back to back (HGEMM_PLAN_NT_STORE)

// tune --plan-only --baselines --interleave (round 6): the report's contenders -- our plan, rocBLAS nn / tn,
// hipBLASLt-heuristic nn / tn, hipBLASLt-autotune nn / tn -- are timed in INTERLEAVED rounds with one warm history instead of one
// after the other: every round launches every contender once (isolated clock: one event pair around one launch, a sync behind it)
// resp. runs one back-to-back box of each (stream clock), and the order rotates from round to round (--reverse: the opposite
// rotation, for the order-reversal test).  The autotune search runs BEFORE any timing (with HGEMM_AUTOTUNE_CACHE it times nothing)
// and a warm round of every contender separates it from the first sample.  Round 5's report timed contenders sequentially, ours
// first and right behind the previous shape's two seconds of autotune launches: the device-bound decades moved +-5 % with the order
// (DESIGN.md section 6.7).  Same record keys as the sequential report, plus "protocol".
static bool g_interleave = false;
static bool g_reverse = false;
// tune --plan-only --baselines --interleave --also config:splits:group,...: explicit plans timed as further contenders of the SAME
// interleaved rounds as the library's plan and the baselines (how a new family is compared with the shipped plan before any table
// row moves); a plan whose geometry does not take the shape's K is left out.  Recorded under "also".
struct AlsoPlan { std::string cfg; int splits, group; };
static std::vector<AlsoPlan> g_also;
#include <functional>
struct Contender {
  const char* key;                          // JSON key stem
  std::function<int(Buffers&)> launch;
  std::vector<float> iso;                   // one sample per round, us
  std::vector<float> box;                   // one back-to-back box per stream round, us per call
  bool ok = true;
  double iso_us() const { return ok && !iso.empty() ? median(iso) : -1.0; }
  double box_us() const { return ok && !box.empty() ? median(box) : -1.0; }
};
static void time_interleaved(std::vector<Contender>& cs, std::vector<Buffers>& sets, int rounds, int stream_rounds, double box_s, double est_us,
                             hipEvent_t e0, hipEvent_t e1) {
  const int n = (int)cs.size();
  auto order = [&](int round, int i) { return g_reverse ? ((n - 1 - i) + n - round % n) % n : (i + round) % n; };
  // warm round: two launches of everybody (first-call setup of the vendor libraries, clocks up), untimed
  for (int w = 0; w < 2; ++w)
    for (int i = 0; i < n; ++i) {
      Contender& c = cs[order(w, i)];
      if (c.ok && c.launch(sets[w % sets.size()]) != HGEMM_OK) c.ok = false;
    }
  HIP_OK(hipDeviceSynchronize());
  for (int r = 0; r < rounds; ++r)
    for (int i = 0; i < n; ++i) {
      Contender& c = cs[order(r, i)];
      if (!c.ok) continue;
      if (g_cooldown_ms > 0) { HIP_OK(hipDeviceSynchronize()); std::this_thread::sleep_for(std::chrono::milliseconds(g_cooldown_ms)); }
      Buffers& s = sets[(r * n + i) % sets.size()];
      HIP_OK(hipEventRecord(e0, nullptr));
      if (c.launch(s) != HGEMM_OK) { c.ok = false; HIP_OK(hipDeviceSynchronize()); continue; }
      HIP_OK(hipEventRecord(e1, nullptr));
      HIP_OK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      c.iso.push_back(ms * 1000.f);
    }
  if (stream_rounds <= 0) return;
  const int reps = (int)std::max(8.0, std::min(20000.0, box_s * 1e6 / std::max(1.0, est_us)));
  for (int r = 0; r < stream_rounds; ++r)
    for (int i = 0; i < n; ++i) {
      Contender& c = cs[order(r, i)];
      if (!c.ok) continue;
      // (no per-box warm-up: the previous contender's box is this one's warm history -- the same for everybody over the rotation)
      HIP_OK(hipEventRecord(e0, nullptr));
      for (int k = 0; k < reps; ++k) (void)c.launch(sets[k % sets.size()]);
      HIP_OK(hipEventRecord(e1, nullptr));
      HIP_OK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      c.box.push_back((float)(ms * 1000.0 / reps));
    }
}

static int default_group(int cfg, const Shape& sh) { return hgemm_mi355x_default_group(cfg, sh.M, sh.N); }

static std::vector<std::string> g_config_filter;  // --configs a,b,c: only these geometries are candidates
// tune --cand-file F: explicit candidate plans per shape, one line per shape: "M_N_K config:splits:group config:splits:group ..."
// (tools/make_cand_file.py writes it from earlier tuning runs: a targeted re-tune measures a handful of plans per shape
// instead of the model's whole list)
#include <map>
static std::map<std::string, std::vector<Plan>> g_cand_file;
static bool load_cand_file(const char* path) {
  std::ifstream f(path);
  if (!f) return false;
  std::string line;
  while (std::getline(f, line)) {
    std::stringstream ss(line);
    std::string key, tok;
    if (!(ss >> key) || key[0] == '#') continue;
    std::vector<Plan>& v = g_cand_file[key];
    while (ss >> tok) {
      const size_t a = tok.find(':'), b = tok.rfind(':');
      if (a == std::string::npos || b == a) continue;
      const int cfg = hgemm_mi355x_config_by_name(tok.substr(0, a).c_str());
      if (cfg < 0) continue;   // a retired geometry
      v.push_back({cfg, atoi(tok.substr(a + 1, b - a - 1).c_str()), atoi(tok.substr(b + 1).c_str()), 0.0});
    }
  }
  return true;
}
static bool g_with_shipped = false;            // --with-shipped: the library's plan for the shape joins the candidates
static bool g_fused_too = false;               // --fused: also time the single-launch form of every split-K plan
static bool g_streamk_too = false;             // --streamk: also time the stream-K plans (HGEMM_PLAN_STREAMK | workgroups)

static std::vector<Plan> candidates(const Shape& sh, double keep_ratio, int max_cand) {
  std::vector<Plan> all;
  const int nc = hgemm_mi355x_num_configs();
  const int ksteps = sh.K / 64;
  for (int c = 0; c < nc; ++c) {
    int info[8];
    hgemm_mi355x_config_info(c, info);
    if (!g_config_filter.empty() &&
        std::find(g_config_filter.begin(), g_config_filter.end(), std::string(hgemm_mi355x_config_name(c))) == g_config_filter.end())
      continue;
    if (info[0] > sh.M * 2 && info[0] > 32) continue;
    if (info[1] > sh.N * 2 && info[1] > 32) continue;
    if (!hgemm_mi355x_config_accepts_k(c, sh.K)) continue;
    // family u (K split inside the workgroup) is a candidate only when --configs names it: no plan of the table uses it yet
    if (hgemm_mi355x_config_local_splits(c) > 1 && g_config_filter.empty()) continue;
    for (int s = 1; s <= 64; s *= 2) {
      if (s > 1 && ksteps / s < 2) break;
      const long wgs = (long)((sh.M + info[0] - 1) / info[0]) * ((sh.N + info[1] - 1) / info[1]) * s;
      if (s > 1 && wgs > 256L * 12) break;  // split-K only to fill the chip
      all.push_back({c, s, default_group(c, sh), hgemm_mi355x_model_us(c, s, sh.M, sh.N, sh.K)});
      if (s > 1 && g_fused_too)
        all.push_back({c, s | HGEMM_SPLITK_FUSED, default_group(c, sh), hgemm_mi355x_model_us(c, s, sh.M, sh.N, sh.K) * 1.001});
    }
    // stream-K plans of the geometries that have the kernel: one, two, ... resident workgroups per CU
    if (g_streamk_too)
      for (int r = 1; r <= hgemm_mi355x_config_streamk(c) && hgemm_mi355x_streamk_runs(c, sh.M, sh.N, sh.K); ++r) {   // (never a plan that would run data-parallel)
        const int plan = HGEMM_PLAN_STREAMK | (256 * r);
        all.push_back({c, plan, default_group(c, sh), hgemm_mi355x_model_us(c, plan, sh.M, sh.N, sh.K)});
      }
  }
  std::sort(all.begin(), all.end(), [](const Plan& a, const Plan& b) { return a.model_us < b.model_us; });
  std::vector<Plan> out;
  for (const Plan& p : all) {
    if ((int)out.size() >= max_cand) break;
    if (!out.empty() && p.model_us > all[0].model_us * keep_ratio && (int)out.size() >= 4) break;
    out.push_back(p);
  }
  return out;
}

// ------------------------------------------------------------------------------------------------
// Exact reference for the reference's correctness inputs (zero_one_correctness_check.py:65-73: entries are
// 0 or 1, P(1) = 1/2, or 1/3 when max(M,N,K) > 8192).  With 0/1 operands every product and every partial
// sum is a small integer, so C[m][n] = popcount(A_row_bits[m] & Bt_row_bits[n]) EXACTLY, whatever the
// summation order; the expected fp16 value is that integer rounded to nearest-even -- which is what
// (a.float() @ b.float()).half() gives (:85-90).  Outputs must match bit for bit (pass rule :263-268; the
// reference masks |truth| > 2047 because ITS fp16-accumulate kernels round on the way -- fp32 accumulation
// does not, so nothing is masked here).  This is a development self-check of the tool; the parity evidence
// against the CPU oracle lives in tests/ (tests/tools/verify_plans.py, tests/test_gpu_*.py).
struct ZeroOne {
  std::vector<f16> a, bt;             // [M][K], [N][K]
  std::vector<uint64_t> abits, bbits; // bit-packed rows, K/64 words (K rounded up)
  int words;
};
static ZeroOne make_zero_one(const Shape& sh, uint64_t seed) {
  ZeroOne z;
  z.words = (sh.K + 63) / 64;
  z.a.assign((size_t)sh.M * sh.K, (f16)0.f);
  z.bt.assign((size_t)sh.N * sh.K, (f16)0.f);
  z.abits.assign((size_t)sh.M * z.words, 0);
  z.bbits.assign((size_t)sh.N * z.words, 0);
  const bool sparse = std::max(sh.M, std::max(sh.N, sh.K)) > 8192;
  uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1;
  auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
  auto fill = [&](std::vector<f16>& v, std::vector<uint64_t>& bits, int rows) {
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < sh.K; ++k) {
        const uint64_t x = next() >> 11;
        const bool one = sparse ? (x % 3 == 0) : (x & 1);
        if (one) { v[(size_t)r * sh.K + k] = (f16)1.f; bits[(size_t)r * z.words + k / 64] |= 1ull << (k % 64); }
      }
  };
  fill(z.a, z.abits, sh.M);
  fill(z.bt, z.bbits, sh.N);
  return z;
}

static int cmd_check(const std::vector<Shape>& shapes) {
  int failures = 0, runs = 0;
  const int nc = hgemm_mi355x_num_configs();
  for (const Shape& sh : shapes) {
    const ZeroOne z = make_zero_one(sh, 1234 + sh.M + sh.N * 3 + sh.K * 7);
    const size_t cn = (size_t)sh.M * sh.N;
    std::vector<f16> truth(cn), got(cn), b_rm((size_t)sh.K * sh.N);
    for (int m = 0; m < sh.M; ++m)
      for (int n = 0; n < sh.N; ++n) {
        int acc = 0;
        for (int w = 0; w < z.words; ++w) acc += __builtin_popcountll(z.abits[(size_t)m * z.words + w] & z.bbits[(size_t)n * z.words + w]);
        truth[(size_t)m * sh.N + n] = (f16)(float)acc;   // int -> fp32 exact, fp32 -> fp16 round-to-nearest-even
      }
    for (int n = 0; n < sh.N; ++n)
      for (int k = 0; k < sh.K; ++k) b_rm[(size_t)k * sh.N + n] = z.bt[(size_t)n * sh.K + k];
    Buffers s;
    HIP_OK(hipMalloc(&s.a, z.a.size() * 2));
    HIP_OK(hipMalloc(&s.bt, z.bt.size() * 2));
    HIP_OK(hipMalloc(&s.b, b_rm.size() * 2));
    HIP_OK(hipMalloc(&s.c, cn * 2));
    HIP_OK(hipMemcpy(s.a, z.a.data(), z.a.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(s.bt, z.bt.data(), z.bt.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(s.b, b_rm.data(), b_rm.size() * 2, hipMemcpyHostToDevice));
    for (int c = HGEMM_CONFIG_RAGGED; c < nc; ++c) {
      if (c >= 0 && sh.K % 64 == 0 && !hgemm_mi355x_config_accepts_k(c, sh.K)) continue;  // BK=128 member, K = 64 (mod 128): the launch refuses
      const char* cname = c >= 0 ? hgemm_mi355x_config_name(c) : (c == HGEMM_CONFIG_GENERIC ? "generic" : "ragged");
      if (!g_config_filter.empty() && std::find(g_config_filter.begin(), g_config_filter.end(), std::string(cname)) == g_config_filter.end())
        continue;   // --configs: only these (the special ids are "generic" / "ragged")
      // stream-K forms (geometries that have the kernel): one resident wave of workgroups, and small odd grids that cut tiles
      // at odd stages and give every workgroup several segments
      const char fam = c >= 0 ? cname[0] : ' ';
      std::vector<int> forms = {1, 2, 3, 8, 2 | HGEMM_SPLITK_FUSED, 8 | HGEMM_SPLITK_FUSED, HGEMM_PLAN_STREAMK, 5 | HGEMM_PLAN_STREAMK,
                                37 | HGEMM_PLAN_STREAMK, 300 | HGEMM_PLAN_STREAMK};
      // round 6: the last arriver of a single-launch split-K adds the slabs in batches of 32 / 16 / 8 / 4 / 2 / 1 (fused_combine,
      // hgemm_kernel.hpp; family q: 2 or 4 slabs ahead + a tail loop) -- split counts that walk every batch depth and remainder
      // (on the shapes with K >= 2048 only: that is where 13 .. 48 splits of >= one stage exist, and it keeps the check's run count down)
      if (sh.K >= 2048)
        for (int f : {3, 5, 7, 13, 16, 21, 32, 37, 48}) forms.push_back(f | HGEMM_SPLITK_FUSED);
      if (fam == 'r')   // family r's plan flags (K stagger per XCD, non-temporal loads of the streamed operand), alone and combined
        forms.insert(forms.end(), {1 | HGEMM_PLAN_RS_XCD_STAGGER | HGEMM_PLAN_RS_NT_LOADS, 2 | HGEMM_SPLITK_FUSED | HGEMM_PLAN_RS_XCD_STAGGER,
                                   3 | HGEMM_PLAN_RS_NT_LOADS, 37 | HGEMM_PLAN_STREAMK | HGEMM_PLAN_RS_XCD_STAGGER | HGEMM_PLAN_RS_NT_LOADS});
      if (fam == 'q')   // family q's kstagger variant (round 5): plain, with NT stores, two-pass and single-launch split-K
        forms.insert(forms.end(), {1 | HGEMM_PLAN_XCD_STAGGER, 1 | HGEMM_PLAN_XCD_STAGGER | HGEMM_PLAN_NT_STORE, 3 | HGEMM_PLAN_XCD_STAGGER,
                                   4 | HGEMM_SPLITK_FUSED | HGEMM_PLAN_XCD_STAGGER,
                                   // the walk's phase flags (prologue only: a sleep / a priority): alone, together, with a stagger
                                   1 | HGEMM_PLAN_PHASE_OFFSET, 1 | HGEMM_PLAN_PHASE_OFFSET4, 1 | HGEMM_PLAN_PHASE_OFFSET8, 1 | HGEMM_PLAN_WAVE_PRIORITY | HGEMM_PLAN_NT_STORE,
                                   2 | HGEMM_PLAN_PHASE_OFFSET | HGEMM_PLAN_WAVE_PRIORITY | HGEMM_PLAN_XCD_STAGGER});
      if (fam == 'u')   // family u (K split inside the workgroup): external splits 5 and 16 on top of 1 / 2 / 3 / 8, non-temporal stores
        forms.insert(forms.end(), {5, 16, 1 | HGEMM_PLAN_NT_STORE, 2 | HGEMM_PLAN_NT_STORE});
      for (int splits : forms) {
        const bool sk = (splits & HGEMM_PLAN_STREAMK) != 0;
        const int sp = sk ? 2 : (splits & HGEMM_SPLITK_MASK);   // (sp > 1: run twice, one raster group)
        if (sk && (c < 0 || hgemm_mi355x_config_streamk(c) <= 0)) continue;
        if (!sk && sp > 1 && (c < 0 || sh.K / 64 < sp)) continue;
        for (int group : {1, 4}) {
          if (group > 1 && sp > 1 && !sk) continue;
          if (group > 1 && c < 0) continue;
          for (int rep = 0; rep < (sp > 1 ? 2 : 1); ++rep) {   // split-K twice: the arrival counters must come back to zero
            HIP_OK(hipMemset(s.c, 0xff, cn * 2));  // NaN pattern: unwritten outputs are caught
            const int st = hgemm_mi355x_launch(c, splits, group, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr);
            hipError_t e = hipDeviceSynchronize();
            ++runs;
            if (st != HGEMM_OK || e != hipSuccess) {
              printf("FAIL %d_%d_%d %s s=%d%s g=%d: status %d hip %d\n", sh.M, sh.N, sh.K, cname, splits & HGEMM_SPLITK_MASK, sk ? "(stream-K)" : sp != splits ? "(fused)" : "", group, st, (int)e);
              ++failures;
              if (e != hipSuccess) return 3;
              continue;
            }
            HIP_OK(hipMemcpy(got.data(), s.c, cn * 2, hipMemcpyDeviceToHost));
            size_t bad = 0;
            for (size_t i = 0; i < cn; ++i)
              if (memcmp(&got[i], &truth[i], 2) != 0) {
                if (bad < 8 && getenv("HGEMM_CHECK_VERBOSE")) printf("   bad m=%zu n=%zu got 0x%04x want 0x%04x\n", i / sh.N, i % sh.N, got[i], truth[i]);
                ++bad;
              }
            if (bad) {
              printf("FAIL %d_%d_%d %s s=%d%s g=%d: %zu/%zu elements differ from the exact result\n", sh.M, sh.N, sh.K, cname, splits & HGEMM_SPLITK_MASK,
                     sk ? "(stream-K)" : sp != splits ? "(fused)" : "", group, bad, cn);
              ++failures;
            }
          }
        }
      }
    }
    free_set(s);
    printf("checked %d_%d_%d\n", sh.M, sh.N, sh.K);
    fflush(stdout);
  }
  // what this log covers, machine-readable (tests/test_evidence_consistency.py: a tuner result is only committed beside a
  // check log that names every geometry it times)
  printf("one-item-kernel: %llu launches (q256x256_w2x2, --one-item 0 sends them to the general kernel)\n", hgemm_mi355x_one_item_kernel_launches());
  printf("check-configs:");
  for (int c = HGEMM_CONFIG_RAGGED; c < nc; ++c) {
    const char* cname = c >= 0 ? hgemm_mi355x_config_name(c) : (c == HGEMM_CONFIG_GENERIC ? "generic" : "ragged");
    if (g_config_filter.empty() || std::find(g_config_filter.begin(), g_config_filter.end(), std::string(cname)) != g_config_filter.end())
      printf(" %s", cname);
  }
  printf("\ncheck-forms: 1 2 3 8 2|fused 8|fused 3|fused 5|fused 7|fused 13|fused 16|fused 21|fused 32|fused 37|fused 48|fused (3|fused .. 48|fused: K >= 2048) streamk|0 streamk|5 streamk|37 streamk|300 (stream-K on the geometries that have the kernel), family r also 1|xcd-stagger|nt-loads 2|fused|xcd-stagger 3|nt-loads streamk|37|xcd-stagger|nt-loads, family q also 1|xcd-stagger 1|xcd-stagger|nt-store 3|xcd-stagger 4|fused|xcd-stagger 1|phase-offset 1|phase-offset4 1|phase-offset8 1|wave-priority|nt-store 2|phase-offset|wave-priority|xcd-stagger, family u also 5 16 1|nt-store 2|nt-store (its fused / stream-K words run as two-pass / plain), raster groups 1 4\n");
  printf("check: %d runs, %d failures (bit-exact against the exact integer result of 0/1 inputs)\n", runs, failures);
  return failures ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
static int cmd_tune(const std::vector<Shape>& shapes, const char* out_path, double keep_ratio, int max_cand,
                    bool baselines, bool sweep_group, bool autotune) {
  // resumable: shapes already present in --out are skipped
  std::vector<std::string> have;
  if (out_path) {
    std::ifstream prev(out_path);
    std::string line;
    while (std::getline(prev, line)) {
      const size_t p0 = line.find("\"mnk\": \"");
      if (p0 == std::string::npos) continue;
      const size_t p1 = line.find('"', p0 + 8);
      have.push_back(line.substr(p0 + 8, p1 - p0 - 8));
    }
  }
  FILE* out = out_path ? fopen(out_path, "a") : stdout;
  if (!out) { perror("open --out"); return 2; }
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  if (baselines) {
    hgemm_rocblas_init();
    hgemm_hipblaslt_heuristic_init();
    if (autotune) hgemm_hipblaslt_autotune_init();
  }
  for (const Shape& sh : shapes) {
    char key[64];
    snprintf(key, sizeof key, "%d_%d_%d", sh.M, sh.N, sh.K);
    if (std::find(have.begin(), have.end(), std::string(key)) != have.end()) continue;
    const double flops = 2.0 * sh.M * sh.N * (double)sh.K;
    const size_t set_bytes = 2 * ((size_t)sh.M * sh.K + (size_t)sh.N * sh.K * (baselines ? 2 : 1) + (size_t)sh.M * sh.N);
    // rotate enough buffer sets to exceed L2 + MALL (~288 MiB), capped at 6 GiB total
    int nsets = (int)std::min<size_t>(8, std::max<size_t>(1, ((size_t)320 << 20) / set_bytes + 1));
    while (nsets > 1 && (size_t)nsets * set_bytes > ((size_t)6 << 30)) --nsets;
    std::vector<Buffers> sets(nsets);
    for (int i = 0; i < nsets; ++i) alloc_set(sets[i], sh, 77 + i, baselines);

    std::vector<Plan> cands;
    if (g_plan_only) {  // report mode: time the library's own plan (tuned table / model) against the baselines
      Plan p{0, 1, 1, 0.0};
      hgemm_mi355x_plan(sh.M, sh.N, sh.K, &p.cfg, &p.splits, &p.group_m);
      p.model_us = p.cfg >= 0 ? hgemm_mi355x_model_us(p.cfg, p.splits, sh.M, sh.N, sh.K) : 0.0;
      cands.push_back(p);
    } else if (!g_cand_file.empty()) {
      auto it = g_cand_file.find(key);
      if (it != g_cand_file.end())
        for (Plan p : it->second) {
          if (!hgemm_mi355x_config_accepts_k(p.cfg, sh.K)) continue;
          if ((p.splits & HGEMM_PLAN_STREAMK) && !hgemm_mi355x_streamk_runs(p.cfg, sh.M, sh.N, sh.K)) {
            // the launch would degrade to the geometry's plain launch and still return OK: not a stream-K timing, not recorded as one
            fprintf(stderr, "tune: %s %s stream-K plan skipped (would run data-parallel on this shape)\n", key, hgemm_mi355x_config_name(p.cfg));
            continue;
          }
          p.model_us = hgemm_mi355x_model_us(p.cfg, p.splits, sh.M, sh.N, sh.K);   // (takes `splits` as the launch does)
          cands.push_back(p);
        }
      if (cands.empty()) cands = candidates(sh, keep_ratio, std::min(max_cand, 6));   // a shape the file does not know
    } else {
      cands = candidates(sh, keep_ratio, max_cand);
    }
    if (g_with_shipped && !g_plan_only) {   // --with-shipped: the library's own plan (tuned table / planner) is measured beside the candidates
      Plan p{0, 1, 1, 0.0};
      hgemm_mi355x_plan(sh.M, sh.N, sh.K, &p.cfg, &p.splits, &p.group_m);
      p.model_us = p.cfg >= 0 ? hgemm_mi355x_model_us(p.cfg, p.splits, sh.M, sh.N, sh.K) : 0.0;
      bool have = false;
      for (const Plan& c : cands) have = have || (c.cfg == p.cfg && c.splits == p.splits && c.group_m == p.group_m);
      if (!have) cands.insert(cands.begin(), p);
    }
    struct Res { Plan p; double us; double iso_us = -1, stream = -1; };
    std::vector<Res> res;
    for (const Plan& p : cands) {
      const double est_us = std::max(2.0, p.model_us);
      int reps = (int)std::max(3.0, std::min(30.0, 20000.0 / est_us));
      if (flops > 1.5e12) reps = 2;
      auto launch = [&](Buffers& s) {
        return hgemm_mi355x_launch(p.cfg, p.splits, p.group_m, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr);
      };
      const double us = time_us(launch, sets, flops > 1.5e12 ? 1 : 2, reps, e0, e1);
      if (us >= kFailedUs) {
        fprintf(stderr, "tune: %s %s splits=%d rejected (launch status != OK)\n", key, hgemm_mi355x_config_name(p.cfg), p.splits);
        continue;
      }
      res.push_back({p, us});
    }
    if (res.empty()) {
      fprintf(stderr, "tune: %s has no usable candidate\n", key);
      for (auto& s : sets) free_set(s);
      continue;
    }
    std::sort(res.begin(), res.end(), [](const Res& a, const Res& b) { return a.us < b.us; });
    if (g_rank_both && !g_plan_only) {
      std::vector<Res> kept;
      const double box = flops > 1.5e12 ? 0.012 : 0.02;
      for (const Res& r : res) {
        if (r.us > res[0].us * 1.25) break;
        const Plan p = r.p;
        auto launch = [&](Buffers& s) {
          return hgemm_mi355x_launch(p.cfg, p.splits, p.group_m, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr);
        };
        const double st = stream_us(launch, sets, box, e0, e1, r.us);
        if (st >= kFailedUs) continue;
        Res k = r;
        k.iso_us = r.us; k.stream = st; k.us = std::sqrt(r.us * st);
        kept.push_back(k);
      }
      if (!kept.empty()) res = kept;
      std::sort(res.begin(), res.end(), [](const Res& a, const Res& b) { return a.us < b.us; });
    }
    if (sweep_group && !g_rank_both && !res.empty()) {
      Res best = res[0];
      for (int g : {1, 2, 4, 8, 16, 32}) {
        if (flops > 1.5e12 && (g == 1 || g == 32)) continue;
        if (g == best.p.group_m) continue;
        Plan p = best.p;
        p.group_m = g;
        auto launch = [&](Buffers& s) {
          return hgemm_mi355x_launch(p.cfg, p.splits, p.group_m, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr);
        };
        const double us = time_us(launch, sets, 1, flops > 1.5e12 ? 2 : std::max(3, (int)std::min(20.0, 20000.0 / best.us)), e0, e1);
        if (us < kFailedUs) res.push_back({p, us});
      }
      std::sort(res.begin(), res.end(), [](const Res& a, const Res& b) { return a.us < b.us; });
    }
    // Non-temporal C stores for the winner: the effect is at the seam between two launches (dirty lines leave the L2s during
    // the epilogue instead of at the end-of-kernel release), so it is judged in back-to-back mode, plain and NT interleaved
    // twice; adopted when both repetitions agree and the gain is at least 1 %.
    double nt_plain_us = -1, nt_us = -1;
    double nt_iso_us = -1, nt_plain_iso_us = -1;
    if (g_try_nt && !g_plan_only && res[0].p.cfg >= 0 && ((res[0].p.splits & HGEMM_SPLITK_MASK) == 1 || (res[0].p.splits & HGEMM_PLAN_STREAMK)) &&
        (double)sh.M * sh.N >= 512.0 * 512.0) {
      Plan pp = res[0].p, pn = res[0].p;
      pn.splits |= HGEMM_PLAN_NT_STORE;
      auto lp = [&](Buffers& s) { return hgemm_mi355x_launch(pp.cfg, pp.splits, pp.group_m, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr); };
      auto ln = [&](Buffers& s) { return hgemm_mi355x_launch(pn.cfg, pn.splits, pn.group_m, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr); };
      const double box = flops > 1.5e12 ? 0.02 : 0.04;
      const double p1 = stream_us(lp, sets, box, e0, e1, res[0].us), n1 = stream_us(ln, sets, box, e0, e1, res[0].us);
      const double p2 = stream_us(lp, sets, box, e0, e1, res[0].us), n2 = stream_us(ln, sets, box, e0, e1, res[0].us);
      nt_plain_us = std::min(p1, p2); nt_us = std::min(n1, n2);
      if (n1 < p1 * 0.99 && n2 < p2 * 0.99 && std::max(n1, n2) < std::min(p1, p2)) {
        // adopted on the back-to-back figures; the record carries the NT form's own MEASURED isolated time (round 3 wrote a
        // synthetic one: the plain form's time scaled by the stream gain)
        nt_plain_iso_us = res[0].iso_us > 0 ? res[0].iso_us : res[0].us;
        const int reps_nt = flops > 1.5e12 ? 2 : std::max(3, (int)std::min(30.0, 20000.0 / std::max(2.0, nt_plain_iso_us)));
        nt_iso_us = time_us(ln, sets, 2, reps_nt, e0, e1);
        Res rn{pn, g_rank_both ? std::sqrt(nt_iso_us * nt_us) : nt_iso_us};
        rn.iso_us = nt_iso_us; rn.stream = nt_us;
        res.insert(res.begin(), rn);
      }
    }
    double rb_nn = -1, rb_tn = -1, lt_nn = -1, lt_tn = -1;
    double st_ours = -1, st_lt_nn = -1, st_lt_tn = -1;
    double at_nn = -1, at_tn = -1, st_at_nn = -1, st_at_tn = -1;
    int at_cand_nn = 0, at_cand_tn = 0;
    int at_cached[2] = {0, 0};
    const bool interleaved = baselines && g_plan_only && g_interleave;
    int il_rounds = 0, il_stream_rounds = 0;
    std::string also_json;
    if (interleaved) {
      bool have_at_nn = false, have_at_tn = false;
      if (autotune) {   // the search first: nothing of it may sit between two timed samples
        have_at_nn = hgemm_hipblaslt_autotune_find_best_nn(sh.M, sh.N, sh.K, 0) == HGEMM_OK;
        if (have_at_nn) { at_cand_nn = hgemm_hipblaslt_autotune_candidates(0); at_cached[0] = hgemm_hipblaslt_autotune_from_cache(0); }
        have_at_tn = hgemm_hipblaslt_autotune_find_best_tn(sh.M, sh.N, sh.K, 0) == HGEMM_OK;
        if (have_at_tn) { at_cand_tn = hgemm_hipblaslt_autotune_candidates(1); at_cached[1] = hgemm_hipblaslt_autotune_from_cache(1); }
      }
      const Plan p = res[0].p;
      std::vector<Contender> cs;
      cs.push_back({"ours", [&, p](Buffers& b) { return hgemm_mi355x_launch(p.cfg, p.splits, p.group_m, b.a, b.b, b.bt, b.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr); }});
      cs.push_back({"rocblas_nn", [&](Buffers& b) { return hgemm_rocblas_nn(b.a, b.b, b.c, sh.M, sh.N, sh.K, 0, nullptr); }});
      cs.push_back({"rocblas_tn", [&](Buffers& b) { return hgemm_rocblas_tn(b.a, b.bt, b.c, sh.M, sh.N, sh.K, 0, nullptr); }});
      cs.push_back({"heur_nn", [&](Buffers& b) { return hgemm_hipblaslt_heuristic_nn(b.a, b.b, b.c, sh.M, sh.N, sh.K, 0, nullptr); }});
      cs.push_back({"heur_tn", [&](Buffers& b) { return hgemm_hipblaslt_heuristic_tn(b.a, b.bt, b.c, sh.M, sh.N, sh.K, 0, nullptr); }});
      if (have_at_nn) cs.push_back({"auto_nn", [&](Buffers& b) { return hgemm_hipblaslt_autotune_nn(b.a, b.b, b.c, sh.M, sh.N, sh.K, 0, nullptr); }});
      if (have_at_tn) cs.push_back({"auto_tn", [&](Buffers& b) { return hgemm_hipblaslt_autotune_tn(b.a, b.bt, b.c, sh.M, sh.N, sh.K, 0, nullptr); }});
      std::vector<std::string> also_keys;
      also_keys.reserve(g_also.size());
      std::vector<Plan> also_plans;
      for (const AlsoPlan& ap : g_also) {
        const int ac = hgemm_mi355x_config_by_name(ap.cfg.c_str());
        if (ac < 0 || !hgemm_mi355x_config_accepts_k(ac, sh.K)) continue;
        const Plan q{ac, ap.splits, ap.group > 0 ? ap.group : default_group(ac, sh), 0.0};
        also_plans.push_back(q);
        also_keys.push_back("also:" + ap.cfg + ":" + std::to_string(ap.splits));
        cs.push_back({also_keys.back().c_str(), [&, q](Buffers& b) { return hgemm_mi355x_launch(q.cfg, q.splits, q.group_m, b.a, b.b, b.bt, b.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr); }});
      }
      il_rounds = flops > 1.5e12 ? 3 : std::max(5, (int)std::min(30.0, 20000.0 / std::max(2.0, res[0].us)));
      il_stream_rounds = g_stream_report ? 3 : 0;
      const double box = g_stream_box_s > 0 ? g_stream_box_s : (flops > 1.5e12 ? 0.012 : 0.008);
      time_interleaved(cs, sets, il_rounds, il_stream_rounds, box, res[0].us, e0, e1);
      for (const Contender& c : cs) {
        const std::string k = c.key;
        const double iso = c.iso_us(), bx = c.box_us();
        if (k == "ours") { if (iso > 0) { res[0].us = iso; } st_ours = bx; }
        else if (k == "rocblas_nn") rb_nn = iso;
        else if (k == "rocblas_tn") rb_tn = iso;
        else if (k == "heur_nn") { lt_nn = iso; st_lt_nn = bx; }
        else if (k == "heur_tn") { lt_tn = iso; st_lt_tn = bx; }
        else if (k == "auto_nn") { at_nn = iso; st_at_nn = bx; }
        else if (k == "auto_tn") { at_tn = iso; st_at_tn = bx; }
      }
      for (size_t i = 0; i < also_plans.size(); ++i) {
        const Contender& c = cs[cs.size() - also_plans.size() + i];
        char buf[256];
        snprintf(buf, sizeof buf, "%s{\"config\": \"%s\", \"splits\": %d, \"group_m\": %d, \"us\": %.3f, \"stream_us\": %.3f}", i ? ", " : "",
                 hgemm_mi355x_config_name(also_plans[i].cfg), also_plans[i].splits, also_plans[i].group_m, c.iso_us(), c.box_us());
        also_json += buf;
      }
    }
    if (baselines && !interleaved) {
      const int reps = flops > 1.5e12 ? 2 : std::max(3, (int)std::min(30.0, 20000.0 / std::max(2.0, res[0].us)));
      rb_nn = time_us([&](Buffers& s) { return hgemm_rocblas_nn(s.a, s.b, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, 2, reps, e0, e1);
      rb_tn = time_us([&](Buffers& s) { return hgemm_rocblas_tn(s.a, s.bt, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, 2, reps, e0, e1);
      lt_nn = time_us([&](Buffers& s) { return hgemm_hipblaslt_heuristic_nn(s.a, s.b, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, 2, reps, e0, e1);
      lt_tn = time_us([&](Buffers& s) { return hgemm_hipblaslt_heuristic_tn(s.a, s.bt, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, 2, reps, e0, e1);
    }
    // tune --plan-only --baselines --stream: the same comparison back to back (what a model runs: launches queue behind each
    // other, the end-of-kernel release and the clocks of a busy device are part of the figure), short boxes
    if (baselines && g_stream_report && !interleaved) {
      const double box = g_stream_box_s > 0 ? g_stream_box_s : (flops > 1.5e12 ? 0.012 : 0.008);
      const Plan p = res[0].p;
      st_ours = stream_us([&](Buffers& s) { return hgemm_mi355x_launch(p.cfg, p.splits, p.group_m, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr); },
                          sets, box, e0, e1, res[0].us);
      st_lt_tn = stream_us([&](Buffers& s) { return hgemm_hipblaslt_heuristic_tn(s.a, s.bt, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, box, e0, e1, lt_tn);
      st_lt_nn = stream_us([&](Buffers& s) { return hgemm_hipblaslt_heuristic_nn(s.a, s.b, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, box, e0, e1, lt_nn);
    }
    if (baselines && autotune && !interleaved) {
      // the reference's strongest baseline (cublaslt_auto_tuning): per-shape search over the heuristic
      // candidates, time-boxed by HGEMM_AUTOTUNE_MAX_SECONDS, then timed like every other entry
      const int reps = flops > 1.5e12 ? 2 : std::max(3, (int)std::min(30.0, 20000.0 / std::max(2.0, res[0].us)));
      if (hgemm_hipblaslt_autotune_find_best_nn(sh.M, sh.N, sh.K, 0) == HGEMM_OK) {
        at_cand_nn = hgemm_hipblaslt_autotune_candidates(0);
        at_nn = time_us([&](Buffers& s) { return hgemm_hipblaslt_autotune_nn(s.a, s.b, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, 2, reps, e0, e1);
      }
      if (hgemm_hipblaslt_autotune_find_best_tn(sh.M, sh.N, sh.K, 0) == HGEMM_OK) {
        at_cand_tn = hgemm_hipblaslt_autotune_candidates(1);
        at_tn = time_us([&](Buffers& s) { return hgemm_hipblaslt_autotune_tn(s.a, s.bt, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, 2, reps, e0, e1);
      }
      // ... and back to back, like ours and the heuristic (round 5: the north-star comparison is against the autotuned baseline on
      // both clocks; the library keeps one selected algorithm per layout).
      if (g_stream_report) {
        const double box = g_stream_box_s > 0 ? g_stream_box_s : (flops > 1.5e12 ? 0.012 : 0.008);
        if (at_tn > 0) st_at_tn = stream_us([&](Buffers& s) { return hgemm_hipblaslt_autotune_tn(s.a, s.bt, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, box, e0, e1, at_tn);
        if (at_nn > 0) st_at_nn = stream_us([&](Buffers& s) { return hgemm_hipblaslt_autotune_nn(s.a, s.b, s.c, sh.M, sh.N, sh.K, 0, nullptr); }, sets, box, e0, e1, at_nn);
      }
    }
    // "splits" is the value to pass to hgemm_mi355x_launch (split count | HGEMM_SPLITK_FUSED); "fused" repeats the flag
    fprintf(out, "{\"mnk\": \"%d_%d_%d\", \"best\": {\"config\": \"%s\", \"splits\": %d, \"fused\": %d, \"streamk\": %d, \"group_m\": %d, \"us\": %.3f, \"tflops\": %.2f}",
            sh.M, sh.N, sh.K, hgemm_mi355x_config_name(res[0].p.cfg), res[0].p.splits, (res[0].p.splits & HGEMM_SPLITK_FUSED) ? 1 : 0,
            (res[0].p.splits & HGEMM_PLAN_STREAMK) ? 1 : 0, res[0].p.group_m, res[0].us, flops / res[0].us * 1e-6);
    if (g_rank_both && res[0].stream > 0) fprintf(out, ", \"rank\": \"sqrt(isolated_us * stream_us)\"");
    if (baselines)
      fprintf(out, ", \"rocblas_nn_us\": %.3f, \"rocblas_tn_us\": %.3f, \"hipblaslt_heur_nn_us\": %.3f, \"hipblaslt_heur_tn_us\": %.3f",
              rb_nn, rb_tn, lt_nn, lt_tn);
    if (baselines && autotune)
      fprintf(out, ", \"hipblaslt_auto_nn_us\": %.3f, \"hipblaslt_auto_tn_us\": %.3f, \"hipblaslt_auto_candidates\": [%d, %d]", at_nn, at_tn,
              at_cand_nn, at_cand_tn);
    if (st_at_nn > 0 || st_at_tn > 0) fprintf(out, ", \"hipblaslt_auto_nn_stream_us\": %.3f, \"hipblaslt_auto_tn_stream_us\": %.3f", st_at_nn, st_at_tn);
    if (interleaved)
      fprintf(out, ", \"protocol\": {\"interleaved\": 1, \"reverse\": %d, \"rounds\": %d, \"stream_rounds\": %d, \"autotune_from_cache\": [%d, %d]}",
              g_reverse ? 1 : 0, il_rounds, il_stream_rounds, at_cached[0], at_cached[1]);
    if (nt_us > 0) fprintf(out, ", \"stream_plain_us\": %.3f, \"stream_nt_us\": %.3f", nt_plain_us, nt_us);
    if (nt_iso_us > 0) fprintf(out, ", \"nt_adopted_on\": \"stream\", \"isolated_plain_us\": %.3f, \"isolated_nt_us\": %.3f", nt_plain_iso_us, nt_iso_us);
    if (st_ours > 0)
      fprintf(out, ", \"stream_us\": %.3f, \"hipblaslt_heur_tn_stream_us\": %.3f, \"hipblaslt_heur_nn_stream_us\": %.3f", st_ours, st_lt_tn, st_lt_nn);
    if (!also_json.empty()) fprintf(out, ", \"also\": [%s]", also_json.c_str());
    fprintf(out, ", \"candidates\": [");
    for (size_t i = 0; i < res.size(); ++i)
    {
      fprintf(out, "%s{\"config\": \"%s\", \"splits\": %d, \"group_m\": %d, \"us\": %.3f, \"model_us\": %.2f", i ? ", " : "",
              hgemm_mi355x_config_name(res[i].p.cfg), res[i].p.splits, res[i].p.group_m, res[i].us, res[i].p.model_us);
      if (res[i].stream > 0) fprintf(out, ", \"isolated_us\": %.3f, \"stream_us\": %.3f", res[i].iso_us, res[i].stream);
      fprintf(out, "}");
    }
    fprintf(out, "]}\n");
    fflush(out);
    for (auto& s : sets) free_set(s);
  }
  if (out != stdout) fclose(out);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// Board telemetry over a timed region: the compute-bound shapes run power-limited, so what a
// kernel sustains is (cycles per flop) x (clock the board grants it at the power cap).  Sampled from the SMU's
// gpu-metrics table through rocm_smi; the HIP device is matched to its rocm_smi index by PCI address.
struct BoardSampler {
  bool ok = false;
  uint32_t dv = 0;
  std::thread th;
  std::atomic<bool> stop{false};
  double sum_mhz = 0, sum_w = 0, max_w = 0, min_mhz = 1e9;
  int n = 0;
  bool open() {
    if (rsmi_init(0) != RSMI_STATUS_SUCCESS) return false;
    uint32_t num = 0;
    if (rsmi_num_monitor_devices(&num) != RSMI_STATUS_SUCCESS || num == 0) return false;
    int dev = 0, dom = 0, bus = 0, slot = 0;
    HIP_OK(hipGetDevice(&dev));
    (void)hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, dev);
    (void)hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, dev);
    (void)hipDeviceGetAttribute(&slot, hipDeviceAttributePciDeviceId, dev);
    dv = 0;
    for (uint32_t i = 0; i < num; ++i) {
      uint64_t bdf = 0;
      if (rsmi_dev_pci_id_get(i, &bdf) != RSMI_STATUS_SUCCESS) continue;
      if ((int)((bdf >> 8) & 0xff) == bus && (int)((bdf >> 3) & 0x1f) == slot && (int)((bdf >> 32) & 0xffffffff) == dom) { dv = i; break; }
    }
    ok = true;
    return true;
  }
  void sample() {
    rsmi_gpu_metrics_t m;
    memset(&m, 0, sizeof m);
    if (rsmi_dev_gpu_metrics_info_get(dv, &m) != RSMI_STATUS_SUCCESS) return;
    double mhz = 0; int k = 0;
    for (int x = 0; x < RSMI_MAX_NUM_GFX_CLKS; ++x)
      if (m.current_gfxclks[x] != 0 && m.current_gfxclks[x] != 0xFFFF) { mhz += m.current_gfxclks[x]; ++k; }
    if (k) mhz /= k; else if (m.current_gfxclk != 0xFFFF) mhz = m.current_gfxclk;
    double w = (m.current_socket_power != 0xFFFF) ? m.current_socket_power : (m.average_socket_power != 0xFFFF ? m.average_socket_power : 0);
    if (mhz > 0) { sum_mhz += mhz; min_mhz = std::min(min_mhz, mhz); }
    sum_w += w; max_w = std::max(max_w, w);
    ++n;
  }
  void start() {
    if (!ok) return;
    stop = false;
    th = std::thread([this] { while (!stop.load()) { sample(); std::this_thread::sleep_for(std::chrono::milliseconds(10)); } });
  }
  void finish() {
    if (!ok) return;
    stop = true;
    if (th.joinable()) th.join();
  }
};

// back-to-back launches for `seconds` (one event pair around the whole run): us per call in steady state + telemetry
template <class F>
static int power_bench(const Shape& sh, const char* label, F&& launch, std::vector<Buffers>& sets, double seconds) {
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  // calibrate: 20 launches, then size the warm-up (0.5 s) and the timed run
  for (int i = 0; i < 20; ++i)
    if (launch(sets[i % sets.size()]) != HGEMM_OK) { fprintf(stderr, "power: launch failed\n"); return 1; }
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipEventRecord(e0, nullptr));
  for (int i = 0; i < 20; ++i) (void)launch(sets[i % sets.size()]);
  HIP_OK(hipEventRecord(e1, nullptr));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  const double est_us = std::max(1.0, ms * 1000.0 / 20);
  const int warm = (int)std::min(200000.0, 0.5e6 / est_us) + 1, reps = (int)std::min(2000000.0, seconds * 1e6 / est_us) + 1;
  for (int i = 0; i < warm; ++i) (void)launch(sets[i % sets.size()]);
  BoardSampler bs;
  bs.open();
  HIP_OK(hipEventRecord(e0, nullptr));
  bs.start();
  for (int i = 0; i < reps; ++i) {
    if (launch(sets[i % sets.size()]) != HGEMM_OK) { bs.finish(); fprintf(stderr, "power: launch failed\n"); return 1; }
  }
  HIP_OK(hipEventRecord(e1, nullptr));
  HIP_OK(hipEventSynchronize(e1));
  bs.finish();
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  const double us = ms * 1000.0 / reps, flops = 2.0 * sh.M * sh.N * (double)sh.K;
  printf("{\"mnk\": \"%d_%d_%d\", \"what\": \"%s\", \"mode\": \"stream\", \"us\": %.3f, \"tflops\": %.2f, \"reps\": %d, \"seconds\": %.3f, "
         "\"telemetry\": {\"samples\": %d, \"gfx_mhz_mean\": %.1f, \"gfx_mhz_min\": %.1f, \"socket_w_mean\": %.1f, \"socket_w_max\": %.1f}}\n",
         sh.M, sh.N, sh.K, label, us, flops / us * 1e-6, reps, ms * 1e-3, bs.n, bs.n ? bs.sum_mhz / bs.n : 0.0, bs.n ? bs.min_mhz : 0.0,
         bs.n ? bs.sum_w / bs.n : 0.0, bs.max_w);
  fflush(stdout);
  return 0;
}

// bench --timeline (measurement library lib_tl/ only): N back-to-back launches with the in-kernel stamps on, then the
// head / K-loop / epilogue / drain split per workgroup (shader cycles), the kernel's own clock estimate (stamps against
// the 100 MHz wall clock) and the gap between consecutive launches per XCD.
static bool g_timeline = false;
template <class F>
static int timeline_bench(const Shape& sh, const char* label, F&& launch, std::vector<Buffers>& sets) {
  if (!hgemm_mi355x_set_timeline) { fprintf(stderr, "--timeline needs the -DHGEMM_TIMELINE library build (lib_tl/)\n"); return 2; }
  constexpr int kSlots = 8, kWgs = 1024, kWords = 16;
  unsigned long long* dev = nullptr;
  const size_t bytes = (size_t)kSlots * kWgs * kWords * 8;
  HIP_OK(hipMalloc(&dev, bytes));
  for (int i = 0; i < 200; ++i) (void)launch(sets[i % sets.size()]);   // warm: clocks at their steady state
  HIP_OK(hipMemset(dev, 0, bytes));
  HIP_OK(hipDeviceSynchronize());
  for (int i = 0; i < 50; ++i) (void)launch(sets[i % sets.size()]);
  hgemm_mi355x_set_timeline(dev, kSlots);
  for (int i = 0; i < kSlots; ++i)
    if (launch(sets[i % sets.size()]) != HGEMM_OK) { fprintf(stderr, "timeline: launch failed\n"); return 1; }
  hgemm_mi355x_set_timeline(nullptr, 0);
  for (int i = 0; i < 8; ++i) (void)launch(sets[i % sets.size()]);      // the recorded launches are not the stream's last
  HIP_OK(hipDeviceSynchronize());
  std::vector<unsigned long long> h((size_t)kSlots * kWgs * kWords);
  HIP_OK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(dev));
  auto q = [](std::vector<double> v, double f) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[(size_t)(f * (v.size() - 1))]; };
  unsigned long long prev_end[8] = {0}, prev_rend = 0;
  for (int sl = 0; sl < kSlots; ++sl) {
    std::vector<double> head, loop, epi, drain, total, mhz, step_cyc, h_setup, h_issue, h_land, h_prime;
    unsigned long long first[8], last[8], rfirst = ~0ull, rlast = 0;
    for (int x = 0; x < 8; ++x) { first[x] = ~0ull; last[x] = 0; }
    int wgs = 0, items = 0;
    for (int w = 0; w < kWgs; ++w) {
      const unsigned long long* t = &h[((size_t)sl * kWgs + w) * kWords];
      if (t[0] == 0 || t[6] == 0) continue;
      ++wgs;
      const int xcc = (int)((t[8] >> 32) & 7);
      if (t[11] && t[12] && t[13]) {   // head split: setup (arguments, coordinates), issue (2 tiles + clear), first tile lands, pipeline primed
        h_setup.push_back((double)(t[11] - t[0])); h_issue.push_back((double)(t[12] - t[11]));
        h_land.push_back((double)(t[13] - t[12])); h_prime.push_back((double)(t[2] - t[13]));
      }
      head.push_back((double)(t[2] - t[0])); loop.push_back((double)(t[4] - t[3])); epi.push_back((double)(t[5] - t[4]));
      drain.push_back((double)(t[6] - t[5])); total.push_back((double)(t[6] - t[0]));
      if (t[7] > t[1]) mhz.push_back((double)(t[6] - t[0]) / ((double)(t[7] - t[1]) * 0.01));   // cycles per us
      const double it = (double)t[10] > 0 ? (double)t[9] / (double)t[10] : 0;   // K-steps of one item
      if (it > 0) step_cyc.push_back((double)(t[4] - t[3]) / it);
      items += (int)t[10];
      first[xcc] = std::min(first[xcc], t[0]); last[xcc] = std::max(last[xcc], t[6]);
      rfirst = std::min(rfirst, t[1]); rlast = std::max(rlast, t[7]);
    }
    std::vector<double> gap, span;
    for (int x = 0; x < 8; ++x) {
      if (last[x] == 0) continue;
      span.push_back((double)(last[x] - first[x]));
      if (sl > 0 && prev_end[x] != 0) gap.push_back((double)first[x] - (double)prev_end[x]);
      prev_end[x] = last[x];
    }
    printf("{\"mnk\": \"%d_%d_%d\", \"what\": \"%s\", \"mode\": \"timeline\", \"launch\": %d, \"wgs\": %d, \"items\": %d, "
           "\"wall_us\": %.2f, \"gap_wall_us\": %.2f, \"mhz_med\": %.0f, "
           "\"head_split_med\": [%.0f, %.0f, %.0f, %.0f], \"cycles\": {\"head\": [%.0f, %.0f, %.0f], \"loop_last_item\": [%.0f, %.0f, %.0f], \"per_k_step\": [%.0f, %.0f, %.0f], "
           "\"epilogue\": [%.0f, %.0f, %.0f], \"drain\": [%.0f, %.0f, %.0f], \"wg_total\": [%.0f, %.0f, %.0f], "
           "\"xcd_span\": [%.0f, %.0f, %.0f], \"xcd_gap_to_prev\": [%.0f, %.0f, %.0f]}}\n",
           sh.M, sh.N, sh.K, label, sl, wgs, items, (double)(rlast - rfirst) * 0.01,
           sl > 0 && prev_rend ? ((double)rfirst - (double)prev_rend) * 0.01 : 0.0, q(mhz, 0.5),
           q(h_setup, 0.5), q(h_issue, 0.5), q(h_land, 0.5), q(h_prime, 0.5),
           q(head, 0.1), q(head, 0.5), q(head, 0.9), q(loop, 0.1), q(loop, 0.5), q(loop, 0.9), q(step_cyc, 0.1), q(step_cyc, 0.5), q(step_cyc, 0.9),
           q(epi, 0.1), q(epi, 0.5), q(epi, 0.9), q(drain, 0.1), q(drain, 0.5), q(drain, 0.9), q(total, 0.1), q(total, 0.5), q(total, 0.9),
           q(span, 0.0), q(span, 0.5), q(span, 1.0), q(gap, 0.0), q(gap, 0.5), q(gap, 1.0));
    prev_rend = rlast;
  }
  fflush(stdout);
  return 0;
}

static const char* g_baseline = nullptr;   // bench --baseline
static bool g_power = false;               // bench --power
static double g_seconds = 1.5;             // bench --seconds

static int cmd_bench(const Shape& sh, const char* cfg_name, int splits, int group, int reps, bool use_lib_plan) {
  int cfg = -2;
  if (use_lib_plan || !cfg_name) {
    hgemm_mi355x_plan(sh.M, sh.N, sh.K, &cfg, &splits, &group);
  } else {
    cfg = hgemm_mi355x_config_by_name(cfg_name);
    if (cfg < 0) { fprintf(stderr, "unknown config %s\n", cfg_name); return 2; }
    if (group <= 0) group = default_group(cfg, sh);
  }
  const size_t set_bytes = 2 * ((size_t)sh.M * sh.K + (size_t)sh.N * sh.K + (size_t)sh.M * sh.N);
  int nsets = (int)std::min<size_t>(8, std::max<size_t>(1, ((size_t)320 << 20) / set_bytes + 1));
  std::vector<Buffers> sets(nsets);
  for (int i = 0; i < nsets; ++i) alloc_set(sets[i], sh, 5 + i, g_baseline != nullptr);
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  const int ld = g_ld_override >= 0 ? g_ld_override : sh.K;
  auto launch = [&](Buffers& s) {
    return hgemm_mi355x_launch(cfg, splits, group, s.a, s.b, s.bt, s.c, sh.M, sh.N, sh.K, ld, ld, sh.N, nullptr);
  };
  if (g_baseline) {
    const std::string b = g_baseline;
    int rc = 0;
    std::function<int(Buffers&)> base;
    if (b == "rocblas_tn") {
      hgemm_rocblas_init();
      base = [&](Buffers& s) { return hgemm_rocblas_tn(s.a, s.bt, s.c, sh.M, sh.N, sh.K, 0, nullptr); };
    } else if (b == "hipblaslt_tn" || b == "hipblaslt_nn") {
      hgemm_hipblaslt_heuristic_init();
      const bool tn = b == "hipblaslt_tn";
      base = [&, tn](Buffers& s) {
        return tn ? hgemm_hipblaslt_heuristic_tn(s.a, s.bt, s.c, sh.M, sh.N, sh.K, 0, nullptr)
                  : hgemm_hipblaslt_heuristic_nn(s.a, s.b, s.c, sh.M, sh.N, sh.K, 0, nullptr); };
    } else {
      fprintf(stderr, "unknown --baseline %s\n", g_baseline);
      rc = 2;
    }
    if (rc == 0 && g_power) rc = power_bench(sh, g_baseline, base, sets, g_seconds);
    else if (rc == 0) {   // --isolated: one launch at a time, `reps` of them (the form a rocprofv3 --pmc pass can afford)
      const double us = time_us(base, sets, 3, reps, e0, e1);
      printf("{\"mnk\": \"%d_%d_%d\", \"what\": \"%s\", \"mode\": \"isolated\", \"us\": %.3f, \"reps\": %d}\n", sh.M, sh.N, sh.K, g_baseline, us, reps);
    }
    for (auto& s : sets) free_set(s);
    return rc;
  }
  if (g_timeline) {
    const int rc = timeline_bench(sh, cfg >= 0 ? hgemm_mi355x_config_name(cfg) : "generic", launch, sets);
    for (auto& s : sets) free_set(s);
    return rc;
  }
  if (g_power) {
    // (label = the whole plan: the same geometry with and without non-temporal stores are different variants of the energy table)
    const std::string label = std::string(cfg >= 0 ? hgemm_mi355x_config_name(cfg) : "generic") + ":" + std::to_string(splits) + ":" + std::to_string(group) +
                              (use_lib_plan ? " (shipped plan)" : "");
    const int rc = power_bench(sh, label.c_str(), launch, sets, g_seconds);
    for (auto& s : sets) free_set(s);
    return rc;
  }
  const double us = time_us(launch, sets, 3, reps, e0, e1);
  if (us >= kFailedUs) { fprintf(stderr, "bench: launch failed\n"); return 1; }
  const double flops = 2.0 * sh.M * sh.N * (double)sh.K;
  printf("{\"mnk\": \"%d_%d_%d\", \"config\": \"%s\", \"splits\": %d, \"group_m\": %d, \"us\": %.3f, \"tflops\": %.2f, \"reps\": %d}\n",
         sh.M, sh.N, sh.K, cfg >= 0 ? hgemm_mi355x_config_name(cfg) : "generic", splits, group, us, flops / us * 1e-6, reps);
  for (auto& s : sets) free_set(s);
  return 0;
}

// ---- The transposed-read variants: `check --layout nn|ta|tn ...`, `bench --layout nn|ta|tn ...` ------------------------------------------
// Fifteen call kinds -- nn, ta, ta --c32, nn --bf16, ta --bf16, ta --c32 --bf16, tn --bf16, tn --bf16 --bias, tn --bf16 --bias --act A,
// ... --act A --aux, nn --bf16 --dact A, ... --dact A --dbias, tn --bf16 --gated A, nn --bf16 --dgated A, tn --bf16 --gated-aux A, tn --bf16 --bias-add, nn --bf16 --nn-add (seventeen) --, each one row of kVariants that main resolves once from the flags; the
// activation A is a run-time value of the call (TrCall::act), not of the row.  ONE check (tr_check) and ONE bench driver (tr_bench) serve
// them all; a row names what differs: its operand scheme, its judge of one finished run, its closing sentence, its bench description.
// The check: every member x {plain, non-temporal stores, two-pass splits 2 / 5} (fp32 C: x {store, accumulate}) from NaN-filled outputs.
// The NN default shapes hold one tile, ragged M / N, an 8-column sliver, 1 .. 7 K stages, a long K -- and three the kernels do not take
// (K % 64, N % 8: the reference kernel answers); the TA ones (A handed over as a_col_major [K][M], lda = M) add M % 8 != 0 to what the
// kernels do not take and an 8-row sliver to what they do.  Two operand schemes.  operands_zero_one (c16 / c32 / bias): 0/1 inputs, C
// bit-exact.  bf16: operands are converted on the host (0 and 1 are bf16 values), the expected 16-bit C is the integer sum (plus the
// bias) rounded to bf16 once.  fp32 C: exact against the host's integer result, the old C32 integers in +-1000.  operands_small_int (the
// activation kinds): integers in -2 .. 2, A scaled by a power of two, so the sum is exact in fp32 in any order (verified per element)
// and lies in the activations' live range; ReLU is held bit for bit, the GELUs to a bar (within_gelu_bar).
static uint16_t bf16_rne(float x) {   // round to nearest even (finite inputs)
  uint32_t u;
  memcpy(&u, &x, 4);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
enum Elem { kF16, kBF16 };
// An output kind, as TrOut in hgemm_api.hip and the registry's OutC16 / OutC32 / OutBias / OutBiasAux / OutDact describe it.
// c32: C is fp32, stored or accumulated onto (else 16-bit elements); bias: the call takes bias[N]; db32: it also writes the column sum
// db32[N]; act: it takes an activation.
enum ZRole { kZNone, kZRead, kZWritten };   // no z; Z is an input (dact); z_out is a second output (aux)
struct OutKind { bool c32, bias; ZRole z; bool db32, act; bool gated = false;       // gated: two weights, two biases (bgemm_mi355x_tn_gated)
                 bool dgated = false;      // dgated: two saved matrices in, two 16-bit matrices out (bgemm_mi355x_nn_dgated)
                 bool gaux = false;        // gaux (with gated): g_out and u_out as two more 16-bit outputs (bgemm_mi355x_tn_gated_aux)
                 bool add = false; };      // add: a read-only residual matrix r [M][N] (TrCall::z), with a bias (tn) or without (nn); no activation
static const OutKind kOutC16 = {false, false, kZNone, false, false}, kOutC32 = {true, false, kZNone, false, false},
                     kOutBias = {false, true, kZNone, false, false}, kOutBiasAct = {false, true, kZNone, false, true},
                     kOutBiasAux = {false, true, kZWritten, false, true}, kOutDact = {false, false, kZRead, false, true},
                     kOutDactDbias = {false, false, kZRead, true, true}, kOutGated = {false, false, kZNone, false, true, true},
                     kOutDgated = {false, false, kZNone, false, true, false, true}, kOutGatedAux = {false, false, kZNone, false, true, true, false, true},
                     kOutBiasAdd = {false, true, kZNone, false, false, false, false, false, true}, kOutAdd = {false, false, kZNone, false, false, false, false, false, true};
static const char* const kActNames[] = {"", "relu", "gelu", "gelu_tanh", "silu"};   // silu: --gated alone
// fp16 values as fp16 or as bf16 bits, ready for upload
static std::vector<uint16_t> operand_bits(const std::vector<f16>& v, Elem elem) {
  std::vector<uint16_t> o(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    if (elem == kBF16) o[i] = bf16_rne((float)v[i]);
    else memcpy(&o[i], &v[i], 2);
  }
  return o;
}

// What a layout's variants share: its words, how A and B are handed over (ldc = N always), its table.
struct TrLayout {
  const char* label;            // "nn" / "ta" / "tn": --layout, the JSON "layout", the stem of the check's labels
  const char* kernels;
  const char* check_shapes;     // the check's default shapes
  bool a_col_major;             // A handed over as [K][M] with lda = M (else [M][K], lda = K)
  bool b_col_major;             // B handed over as b_col_major [N][K] with ldb = K (else row-major [K][N], ldb = N)
  int (*num_configs)(void);
  const char* (*config_name)(int);
  int (*plan)(int, int, int, int*, int*);
  int (*rocblas_bf16)(const void*, const void*, void*, int, int, int, void*);   // rocBLAS on this layout's operands, bf16 in and out
  int lda(const Shape& sh) const { return a_col_major ? sh.M : sh.K; }
  int ldb(const Shape& sh) const { return b_col_major ? sh.K : sh.N; }
};
static const char kShapesNN[] = "64_64_64,1_8_64,65_72_128,200_264_192,130_8_64,96_136_256,96_136_320,96_136_448,512_1024_2048,64_64_8192,"
                                "200_136_72,200_100_128,33_17_40";
static const TrLayout kLayoutNN = {"nn", "the NN kernels", kShapesNN, false, false,
                                   hgemm_mi355x_nn_num_configs, hgemm_mi355x_nn_config_name, hgemm_mi355x_nn_plan, bgemm_rocblas_nn};
static const TrLayout kLayoutTA = {"ta", "the TA kernels",
                                   "64_64_64,8_8_64,72_72_128,200_264_192,136_8_64,96_136_256,96_136_320,96_136_448,512_1024_2048,64_64_8192,"
                                   "200_136_72,200_100_128,100_136_128,33_17_40", true, false,
                                   hgemm_mi355x_ta_num_configs, hgemm_mi355x_ta_config_name, hgemm_mi355x_ta_plan, bgemm_rocblas_ta};
// the bf16 forward product (family f, hgemm_kernel_tn.hpp): a table of its own; M is free, K % 64 and N % 8 go to the reference kernel,
// so the NN layout's shapes serve
static const TrLayout kLayoutTN = {"tn", "the TN kernels", kShapesNN, false, true,
                                   bgemm_mi355x_tn_num_configs, bgemm_mi355x_tn_config_name, bgemm_mi355x_tn_plan, bgemm_rocblas_tn};

// One call's operands.  Every variant's entry points sit behind the same two signatures; what a variant has no use for (bias,
// accumulate, z, db32, act) its adapter drops.  z: z_out of --aux, Z of --dact; act: HGEMM_ACT_RELU / _GELU / _GELU_TANH
struct TrCall { const void *a, *b, *bias; void* c; int accumulate; void* z = nullptr; float* db32 = nullptr; int act = 0;
                const void *b2 = nullptr, *bias2 = nullptr;      // b2, bias2: Wu and bias_u of a gated call, whose b and bias are the gate's
                void* c2 = nullptr; };   // a dgated call: z = g, b2 = u (both [M][N]), c = dg, c2 = du; a gated aux call: z = g_out, c2 = u_out
template <auto F> static int launch16(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {   // F: a 16-bit-C launch
  return F(cfg, splits, o.a, o.b, o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
}
template <auto F> static int launch32(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {   // F: an fp32-C launch
  return F(cfg, splits, o.a, o.b, (float*)o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, o.accumulate, nullptr);
}
static int launch_bias(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_tn_bias(cfg, splits, o.a, o.b, o.bias, o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
}
template <auto F> static int planned16(const TrCall& o, const Shape& sh) { return F(o.a, o.b, o.c, sh.M, sh.N, sh.K, nullptr); }
template <auto F> static int planned32(const TrCall& o, const Shape& sh) { return F(o.a, o.b, (float*)o.c, sh.M, sh.N, sh.K, o.accumulate, nullptr); }
static int planned_bias(const TrCall& o, const Shape& sh) { return bgemm_mi355x_tn_bias(o.a, o.b, o.bias, o.c, sh.M, sh.N, sh.K, nullptr); }
// the fused bias+activation calls (bgemm_mi355x_tn_bias_act), and --aux: the same call with the pre-activation as a second output
static int launch_bias_act(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_tn_bias_act(cfg, splits, o.a, o.b, o.bias, o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, o.act, nullptr);
}
static int planned_bias_act(const TrCall& o, const Shape& sh) { return bgemm_mi355x_tn_bias_act(o.a, o.b, o.bias, o.c, sh.M, sh.N, sh.K, o.act, nullptr); }
static int launch_bias_act_aux(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_tn_bias_act_aux(cfg, splits, o.a, o.b, o.bias, o.c, o.z, sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, o.act, nullptr);
}
static int planned_bias_act_aux(const TrCall& o, const Shape& sh) { return bgemm_mi355x_tn_bias_act_aux(o.a, o.b, o.bias, o.c, o.z, sh.M, sh.N, sh.K, o.act, nullptr); }
static int aux_runs(int cfg, int M, int N, int K, int lda, int ldb, int ldc) { return bgemm_mi355x_tn_bias_act_aux_runs(cfg, M, N, K, lda, ldb, ldc, N); }
// the activation's derivative at a saved Z (bgemm_mi355x_nn_dact), and --dbias: the same call that also writes db32 (ldz = N throughout)
static int launch_dact(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_nn_dact(cfg, splits, o.a, o.b, o.z, o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, o.act, nullptr);
}
static int planned_dact(const TrCall& o, const Shape& sh) { return bgemm_mi355x_nn_dact(o.a, o.b, o.z, o.c, sh.M, sh.N, sh.K, o.act, nullptr); }
static int dact_runs(int cfg, int M, int N, int K, int lda, int ldb, int ldc) { return bgemm_mi355x_nn_dact_runs(cfg, M, N, K, lda, ldb, ldc, N); }
static int launch_dact_dbias(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_nn_dact_dbias(cfg, splits, o.a, o.b, o.z, o.c, o.db32, sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, o.act, o.accumulate, nullptr);
}
static int planned_dact_dbias(const TrCall& o, const Shape& sh) { return bgemm_mi355x_nn_dact_dbias(o.a, o.b, o.z, o.c, o.db32, sh.M, sh.N, sh.K, o.act, o.accumulate, nullptr); }
static int dact_dbias_runs(int cfg, int M, int N, int K, int lda, int ldb, int ldc) { return bgemm_mi355x_nn_dact_dbias_runs(cfg, M, N, K, lda, ldb, ldc, N); }

// the gated forward product (bgemm_mi355x_tn_gated): sh.N is the OUTPUT width, both weights [N][K]
static int launch_gated(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_tn_gated(cfg, splits, o.a, o.b, o.b2, o.bias, o.bias2, o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, o.act, nullptr);
}
static int planned_gated(const TrCall& o, const Shape& sh) { return bgemm_mi355x_tn_gated(o.a, o.b, o.b2, o.bias, o.bias2, o.c, sh.M, sh.N, sh.K, o.act, nullptr); }

// its training form (bgemm_mi355x_tn_gated_aux; separate g_out and u_out, ldz = N)
static int launch_gated_aux(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_tn_gated_aux(cfg, splits, o.a, o.b, o.b2, o.bias, o.bias2, o.c, o.z, o.c2, sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, o.act, nullptr);
}
static int planned_gated_aux(const TrCall& o, const Shape& sh) {
  return bgemm_mi355x_tn_gated_aux(o.a, o.b, o.b2, o.bias, o.bias2, o.c, o.z, o.c2, sh.M, sh.N, sh.K, o.act, nullptr);
}
static int gated_aux_runs(int cfg, int M, int N, int K, int lda, int ldb, int ldc) { return bgemm_mi355x_tn_gated_aux_runs(cfg, M, N, K, lda, ldb, ldc, N); }

// the fused residual add (bgemm_mi355x_tn_bias_add, bgemm_mi355x_nn_add; z = r, ldr = N; r == c is the in-place call)
static int launch_bias_add(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_tn_bias_add(cfg, splits, o.a, o.b, o.bias, o.z, o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, nullptr);
}
static int planned_bias_add(const TrCall& o, const Shape& sh) { return bgemm_mi355x_tn_bias_add(o.a, o.b, o.bias, o.z, o.c, sh.M, sh.N, sh.K, nullptr); }
static int bias_add_runs(int cfg, int M, int N, int K, int lda, int ldb, int ldc) { return bgemm_mi355x_tn_bias_add_runs(cfg, M, N, K, lda, ldb, ldc, N); }
static int launch_nn_add(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_nn_add(cfg, splits, o.a, o.b, o.z, o.c, sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, nullptr);
}
static int planned_nn_add(const TrCall& o, const Shape& sh) { return bgemm_mi355x_nn_add(o.a, o.b, o.z, o.c, sh.M, sh.N, sh.K, nullptr); }
static int nn_add_runs(int cfg, int M, int N, int K, int lda, int ldb, int ldc) { return bgemm_mi355x_nn_add_runs(cfg, M, N, K, lda, ldb, ldc, N); }

// the gated MLP's input gradient (bgemm_mi355x_nn_dgated; ldz = ldc = N throughout)
static int launch_dgated(int cfg, int splits, const TrCall& o, const Shape& sh, int lda, int ldb) {
  return bgemm_mi355x_launch_nn_dgated(cfg, splits, o.a, o.b, o.z, o.b2, o.c, o.c2, sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, o.act, nullptr);
}
static int planned_dgated(const TrCall& o, const Shape& sh) { return bgemm_mi355x_nn_dgated(o.a, o.b, o.z, o.b2, o.c, o.c2, sh.M, sh.N, sh.K, o.act, nullptr); }
static int dgated_runs(int cfg, int M, int N, int K, int lda, int ldb, int ldc) { return bgemm_mi355x_nn_dgated_runs(cfg, M, N, K, lda, ldb, N, ldc); }

// What tr_bench is told about one bench (the descriptions themselves: bench_nn ... bench_nn_dact_dbias, below).
struct TrBench;
struct BenchDesc {
  unsigned long long seed0;       // operand set i is filled from seed0 + i
  void (*warm)(bool autotune);    // the vendor libraries' set-up, once, before anything is allocated or timed
  void (*shape)(TrBench&);        // per shape: the extra buffers, the contenders in order, the header fields, the verdict
};
static void warm_none(bool) {}
static void warm_rocblas(bool) { hgemm_rocblas_init(); }
static void warm_hipblaslt(bool autotune) {
  hgemm_hipblaslt_heuristic_init();
  if (autotune) hgemm_hipblaslt_autotune_init();
}
static void bench_nn(TrBench&), bench_ta(TrBench&), bench_ta_c32(TrBench&), bench_bf16(TrBench&), bench_tn_bf16(TrBench&), bench_tn_bias(TrBench&),
    bench_tn_bias_act(TrBench&), bench_tn_aux(TrBench&), bench_nn_dact(TrBench&), bench_nn_dact_dbias(TrBench&), bench_tn_gated(TrBench&), bench_nn_dgated(TrBench&), bench_tn_gated_aux(TrBench&), bench_tn_bias_add(TrBench&), bench_nn_add(TrBench&);
static const BenchDesc kBenchNN = {77, warm_hipblaslt, bench_nn}, kBenchTA = {91, warm_none, bench_ta}, kBenchTAC32 = {91, warm_none, bench_ta_c32},
                       kBenchBF16 = {91, warm_rocblas, bench_bf16}, kBenchTN = {91, warm_rocblas, bench_tn_bf16}, kBenchTNBias = {91, warm_none, bench_tn_bias},
                       kBenchTNBiasAct = {91, warm_none, bench_tn_bias_act}, kBenchTNAux = {91, warm_none, bench_tn_aux},
                       kBenchNNDact = {91, warm_none, bench_nn_dact}, kBenchNNDactDbias = {91, warm_none, bench_nn_dact_dbias},
                       kBenchTNGated = {91, warm_none, bench_tn_gated}, kBenchNNDgated = {91, warm_none, bench_nn_dgated},
                       kBenchTNGatedAux = {91, warm_none, bench_tn_gated_aux}, kBenchTNBiasAdd = {91, warm_none, bench_tn_bias_add},
                       kBenchNNAdd = {91, warm_none, bench_nn_add};

// What tr_check is told about one kind (the functions themselves: below, above tr_check).
struct Check;
struct CheckDesc {
  int (*operands)(Check&);        // per shape: the host operands and the exact host result; 0, or the exit status of a refusal
  int (*judge)(Check&);           // per finished run: compares, reports through Check::report; 0, or the exit status that ends the check
  void (*summary)(const Check&);  // the closing line(s)
};
static int operands_zero_one(Check&), operands_small_int(Check&), operands_gated(Check&), judge_exact(Check&), judge_act(Check&), judge_dbias(Check&), judge_gated(Check&),
           operands_dgated(Check&), judge_dgated(Check&), judge_gated_aux(Check&), operands_add(Check&), judge_add(Check&);
static void summary_exact(const Check&), summary_act(const Check&), summary_gated(const Check&), summary_dgated(const Check&), summary_gated_aux(const Check&), summary_add(const Check&);
static const CheckDesc kCheckExact = {operands_zero_one, judge_exact, summary_exact}, kCheckAct = {operands_small_int, judge_act, summary_act},
                       kCheckDbias = {operands_small_int, judge_dbias, summary_act}, kCheckGated = {operands_gated, judge_gated, summary_gated},
                       kCheckDgated = {operands_dgated, judge_dgated, summary_dgated}, kCheckGatedAux = {operands_gated, judge_gated_aux, summary_gated_aux},
                       kCheckAdd = {operands_add, judge_add, summary_add};

struct Variant {
  const TrLayout* L;
  Elem elem;
  const OutKind* out;
  int (*runs)(int cfg, int M, int N, int K, int lda, int ldb, int ldc);   // 1: the family's kernel takes the call
  int (*launch)(int cfg, int splits, const TrCall&, const Shape&, int lda, int ldb);
  int (*planned)(const TrCall&, const Shape&);
  const CheckDesc* check;
  const BenchDesc* bench;
  // "ta-c32-bf16" / "--layout ta --c32 --bf16"; with an activation the check's label, "tn-bf16-bias-gelu-aux" / "nn-bf16-dact-relu-dbias"
  std::string words(const char* layout, const char* sep, int act = 0) const {
    std::string w = std::string(layout) + L->label + (out->c32 ? std::string(sep) + "c32" : "") + (elem == kBF16 ? std::string(sep) + "bf16" : "") +
                    (out->bias ? std::string(sep) + "bias" : "") + (out->add ? std::string(sep) + "add" : "");
    if (act) w += (out->z == kZRead ? std::string(sep) + "dact" : out->gaux ? std::string(sep) + "gated-aux" : out->gated ? std::string(sep) + "gated" : out->dgated ? std::string(sep) + "dgated" : "") + sep + kActNames[act] + (out->z == kZWritten ? std::string(sep) + "aux" : "") +
                  (out->db32 ? std::string(sep) + "dbias" : "");
    return w;
  }
  int runs_at(int cfg, const Shape& sh) const { return runs(cfg, sh.M, sh.N, sh.K, L->lda(sh), L->ldb(sh), sh.N); }
};
static const Variant kVariants[] = {
    {&kLayoutNN, kF16, &kOutC16, hgemm_mi355x_nn_runs, launch16<hgemm_mi355x_launch_nn>, planned16<hgemm_mi355x_nn_fp32>, &kCheckExact, &kBenchNN},
    {&kLayoutTA, kF16, &kOutC16, hgemm_mi355x_ta_runs, launch16<hgemm_mi355x_launch_ta>, planned16<hgemm_mi355x_ta_fp32>, &kCheckExact, &kBenchTA},
    {&kLayoutTA, kF16, &kOutC32, hgemm_mi355x_ta_c32_runs, launch32<hgemm_mi355x_launch_ta_c32>, planned32<hgemm_mi355x_ta_c32>, &kCheckExact, &kBenchTAC32},
    {&kLayoutNN, kBF16, &kOutC16, bgemm_mi355x_nn_runs, launch16<bgemm_mi355x_launch_nn>, planned16<bgemm_mi355x_nn>, &kCheckExact, &kBenchBF16},
    {&kLayoutTA, kBF16, &kOutC16, bgemm_mi355x_ta_runs, launch16<bgemm_mi355x_launch_ta>, planned16<bgemm_mi355x_ta>, &kCheckExact, &kBenchBF16},
    {&kLayoutTA, kBF16, &kOutC32, bgemm_mi355x_ta_c32_runs, launch32<bgemm_mi355x_launch_ta_c32>, planned32<bgemm_mi355x_ta_c32>, &kCheckExact, &kBenchBF16},
    {&kLayoutTN, kBF16, &kOutC16, bgemm_mi355x_tn_runs, launch16<bgemm_mi355x_launch_tn>, planned16<bgemm_mi355x_tn>, &kCheckExact, &kBenchTN},
    {&kLayoutTN, kBF16, &kOutBias, bgemm_mi355x_tn_bias_runs, launch_bias, planned_bias, &kCheckExact, &kBenchTNBias},
    {&kLayoutTN, kBF16, &kOutBiasAct, bgemm_mi355x_tn_bias_act_runs, launch_bias_act, planned_bias_act, &kCheckAct, &kBenchTNBiasAct},
    {&kLayoutTN, kBF16, &kOutBiasAux, aux_runs, launch_bias_act_aux, planned_bias_act_aux, &kCheckAct, &kBenchTNAux},
    {&kLayoutNN, kBF16, &kOutDact, dact_runs, launch_dact, planned_dact, &kCheckAct, &kBenchNNDact},
    {&kLayoutNN, kBF16, &kOutDactDbias, dact_dbias_runs, launch_dact_dbias, planned_dact_dbias, &kCheckDbias, &kBenchNNDactDbias},
    {&kLayoutTN, kBF16, &kOutGated, bgemm_mi355x_tn_gated_runs, launch_gated, planned_gated, &kCheckGated, &kBenchTNGated},
    {&kLayoutNN, kBF16, &kOutDgated, dgated_runs, launch_dgated, planned_dgated, &kCheckDgated, &kBenchNNDgated},
    {&kLayoutTN, kBF16, &kOutGatedAux, gated_aux_runs, launch_gated_aux, planned_gated_aux, &kCheckGatedAux, &kBenchTNGatedAux},
    {&kLayoutTN, kBF16, &kOutBiasAdd, bias_add_runs, launch_bias_add, planned_bias_add, &kCheckAdd, &kBenchTNBiasAdd},
    {&kLayoutNN, kBF16, &kOutAdd, nn_add_runs, launch_nn_add, planned_nn_add, &kCheckAdd, &kBenchNNAdd},
};
// What the command line says of the call; act, dact: 0, or the A of --act A / --dact A as HGEMM_ACT_RELU / _GELU / _GELU_TANH.
struct TrFlags {
  std::string layout;
  bool bf16 = false, c32 = false, bias = false, aux = false, dbias = false;
  bool bias_add = false, nn_add = false;   // --bias-add (a bias kind: sets `bias` too), --nn-add
  int act = 0, dact = 0, gated = 0, dgated = 0, gated_aux = 0;
  int activation() const { return act ? act : dact ? dact : gated ? gated : dgated ? dgated : gated_aux; }
};
// nullptr: no such variant (--layout tn without --bf16 and no --layout at all are the fp16 b_col_major commands)
static const Variant* resolve_variant(const TrFlags& f) {
  for (const Variant& v : kVariants)
    if (f.layout == v.L->label && (v.elem == kBF16) == f.bf16 && v.out->c32 == f.c32 && v.out->bias == f.bias && v.out->db32 == f.dbias &&
        v.out->z == (f.dact ? kZRead : f.aux ? kZWritten : kZNone) && v.out->act == (f.activation() != 0) && v.out->gated == (f.gated != 0 || f.gated_aux != 0) &&
        v.out->dgated == (f.dgated != 0) && v.out->gaux == (f.gated_aux != 0) && !((f.gated || f.dgated || f.gated_aux) && (f.act || f.dact)) &&
        (f.gated != 0) + (f.dgated != 0) + (f.gated_aux != 0) <= 1 && v.out->add == (f.bias_add || f.nn_add))
      return &v;
  return nullptr;
}

struct DevBufs {   // the device allocations of one scope: freed when it ends, on every way out
  std::vector<void*> ptrs;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() { for (void* p : ptrs) (void)hipFree(p); }
  void* alloc(size_t bytes) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, bytes));
    ptrs.push_back(p);
    return p;
  }
  void* upload(const void* src, size_t bytes) {
    void* p = alloc(bytes);
    HIP_OK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    return p;
  }
};

// The fused-bias check's bias is bias[n] = ((n mod 255) - 127) / 2: bf16 values, and with the integer sums S <= K exact in fp32, so the
// expected C is bf16(S + bias[n]), rounded once.
static float check_bias(int n) { return (float)((n % 255) - 127) * 0.5f; }
template <class T> static std::vector<T> transposed(const std::vector<T>& v, int rows, int cols) {   // [rows][cols] -> [cols][rows]
  std::vector<T> t(v.size());
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = v[(size_t)r * cols + c];
  return t;
}

constexpr int DBIAS_GUARD = 8;               // floats behind db32[N - 1] that must keep DBIAS_SENTINEL
constexpr float DBIAS_SENTINEL = -12345.625f;
// db32 as a run finds it: N floats -- NaN, or with `old` a fixed pattern to accumulate onto -- and the sentinels behind them
static std::vector<float> dbias_prefill(int N, bool old) {
  std::vector<float> v(N + DBIAS_GUARD, std::nanf(""));
  for (int n = 0; n < N && old; ++n) v[n] = (float)((n * 37) % 129 - 64) * 0.3f;
  for (int n = 0; n < DBIAS_GUARD; ++n) v[N + n] = DBIAS_SENTINEL;
  return v;
}

// One check as its kind's functions (CheckDesc) see it: the tallies, the shape at hand with what `operands` made of it, the run at hand.
struct Check {
  const Variant& V;
  const int act;
  const std::string lay;                  // the label of every line: V's words and the activation
  int failures = 0, runs = 0;
  double worst = 0.0, worst_db = 0.0;     // the GELU bars: the largest err / bar that passed, of C and of db32
  Shape sh = {};
  size_t cn = 0;                          // M N
  struct Host {
    std::vector<uint16_t> b2, bias2;      // operands_gated: Wu [N][K] and bias_u (b and bias are the gate's)
    std::vector<uint16_t> a, b, bias, z;  // the bits to upload, A and B as the layout takes them; z [M][N]: Z of a dact call, of an aux call what z_out must hold
    std::vector<unsigned char> want[2];   // operands_zero_one: the expected C as bytes: [0] what a store leaves, [1] (fp32 C alone) what accumulating onto `old` leaves
    std::vector<float> old;
    std::vector<uint16_t> relu;           // operands_small_int: ReLU's exact C,
    std::vector<double> y, eps;           //   the GELUs' fp64 target y* and the second term of their bar
                                          // (operands_dgated: 2 M N of each, dg's and behind them du's; z = g and b2 = u, [M][N])
  } h;
  TrCall call = {};
  int cfg = 0, splits = 1;
  const char* cname = "";
  std::vector<unsigned char> got;         // C read back
  void report(size_t bad) {               // the run's elements outside its bar
    if (!bad) return;
    printf("FAIL %s %d_%d_%d %s s=%d%s%s: %zu/%zu elements %s\n", lay.c_str(), sh.M, sh.N, sh.K, cname, splits & HGEMM_SPLITK_MASK,
           (splits & HGEMM_PLAN_NT_STORE) ? "|nt" : "", !V.out->c32 ? "" : call.accumulate ? " accumulate" : " store", bad, cn,
           V.out->act && act != HGEMM_ACT_RELU ? "outside the bar" : "differ from the exact result");
    ++failures;
  }
};

static int operands_zero_one(Check& K) {
  const Variant& V = K.V;
  const Shape& sh = K.sh;
  const bool c32 = V.out->c32, bias = V.out->bias;
  const size_t esz = c32 ? 4 : 2, cn = K.cn;
  const ZeroOne z = make_zero_one(sh, 4321 + sh.M + sh.N * 3 + sh.K * 7);
  K.h.want[0].resize(cn * esz);
  K.h.want[1].resize(c32 ? cn * esz : 0);
  K.h.old.resize(c32 ? cn : 0);
  uint64_t lcg = 88172645463325252ull + cn;
  for (int m = 0; m < sh.M; ++m)
    for (int n = 0; n < sh.N; ++n) {
      int acc = 0;
      for (int w = 0; w < z.words; ++w) acc += __builtin_popcountll(z.abits[(size_t)m * z.words + w] & z.bbits[(size_t)n * z.words + w]);
      const size_t i = (size_t)m * sh.N + n;
      if (c32) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        K.h.old[i] = (float)((int)((lcg >> 33) % 2001) - 1000);
        const float stored = (float)acc, summed = K.h.old[i] + stored;   // integers below 2^24: exact
        memcpy(&K.h.want[0][i * 4], &stored, 4);
        memcpy(&K.h.want[1][i * 4], &summed, 4);
      } else {
        const f16 t16 = (f16)(float)acc;   // int -> fp32 exact, fp32 -> fp16 round-to-nearest-even
        const uint16_t tb = bf16_rne((float)acc + (bias ? check_bias(n) : 0.f));
        memcpy(&K.h.want[0][i * 2], V.elem == kBF16 ? (const void*)&tb : (const void*)&t16, 2);
      }
    }
  K.h.a = operand_bits(V.L->a_col_major ? transposed(z.a, sh.M, sh.K) : z.a, V.elem);   // (z.a: [M][K])
  K.h.b = operand_bits(V.L->b_col_major ? z.bt : transposed(z.bt, sh.N, sh.K), V.elem);   // (z.bt: [N][K])
  for (int n = 0; n < sh.N && bias; ++n) K.h.bias.push_back(bf16_rne(check_bias(n)));
  return 0;
}
static int judge_exact(Check& K) {   // bit for bit
  const size_t esz = K.V.out->c32 ? 4 : 2;
  const unsigned char* w = K.h.want[K.call.accumulate].data();
  size_t bad = 0;
  for (size_t i = 0; i < K.cn; ++i)
    if (memcmp(&K.got[i * esz], &w[i * esz], esz) != 0) {
      if (bad < 8 && getenv("HGEMM_CHECK_VERBOSE")) {
        uint32_t gv = 0, wv = 0;
        memcpy(&gv, &K.got[i * esz], esz);
        memcpy(&wv, &w[i * esz], esz);
        printf("   bad m=%zu n=%zu got 0x%0*x want 0x%0*x\n", i / K.sh.N, i % K.sh.N, (int)esz * 2, gv, (int)esz * 2, wv);
      }
      ++bad;
    }
  K.report(bad);
  return 0;
}
static void summary_exact(const Check& K) {
  printf("check %s: %d runs, %d failures (bit-exact against the exact integer result of 0/1 inputs%s)\n", K.lay.c_str(), K.runs, K.failures,
         K.V.out->c32 ? " and an integer old C32" : K.V.out->bias ? " plus the bias, rounded to bf16 once" : K.V.elem == kBF16 ? ", rounded to bf16 once" : "");
}

// ---- The activation kinds' check ------------------------------------------------------------------------------------------------------------
// --act A (with --layout tn --bf16 --bias; bgemm_mi355x_tn_bias_act): C = bf16(act(S + bias[n])).  A bias of multiples of 2^-8 in [-1, 1]:
// z = S + bias is exact in fp32 in any order.  The bars: ReLU bit for bit against (z > 0 ? bf16(z) : +0); both GELUs
// |C - y*| <= 1/2 ulp_bf16(y*) + 2^-19 |z|, y* the fp64 activation of z.  --aux: z_out = bf16(z), held bit for bit next to C's bars.
// --dact A (with --layout nn --bf16; bgemm_mi355x_nn_dact): C = bf16(S x act'(float(z))).  Z is a seeded matrix of multiples of 1/32 in
// [-4, 4] (bf16 values; both signs, zeros, some -0, the range of a negative derivative).  The bars: ReLU bit for bit against
// (z <= 0 ? +0 : bf16(S)); both GELUs |C - S g*| <= 1/2 ulp_bf16(S g*) + DACT_EPS |S|, g* in fp64.
static double act_fp64(double z, int act) {
  if (act == HGEMM_ACT_RELU) return z > 0 ? z : 0.0;
  if (act == HGEMM_ACT_GELU) return 0.5 * z * erfc(-z / sqrt(2.0));
  if (act == HGEMM_ACT_SILU) return z / (1.0 + exp(-z));
  const double u = sqrt(2.0 / M_PI) * (z + 0.044715 * z * z * z);
  return z / (1.0 + exp(-2.0 * u));
}
static double dact_fp64(double z, int act) {
  if (act == HGEMM_ACT_RELU) return z <= 0 ? 0.0 : 1.0;
  if (act == HGEMM_ACT_GELU) return 0.5 * erfc(-z / sqrt(2.0)) + z * exp(-0.5 * z * z) / sqrt(2.0 * M_PI);
  const double c = sqrt(2.0 / M_PI), s = 1.0 / (1.0 + exp(-2.0 * c * (z + 0.044715 * z * z * z)));
  return s + z * s * (1.0 - s) * 2.0 * c * (1.0 + 3.0 * 0.044715 * z * z);
}
static double bf16_value(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return (double)f;
}
// Integers in -2 .. 2, A scaled by 2^-(floor(log2 K) - 2); drawn in the order A, B (as the layout hands it over), for a dact call then Z.
static int operands_small_int(Check& K) {
  const Shape& sh = K.sh;
  const size_t cn = K.cn;
  const bool dact = K.V.out->z == kZRead;
  int j = 0;
  while ((2 << j) <= sh.K) ++j;   // floor(log2 K)
  const double scale = ldexp(1.0, -std::max(j - 2, 0));
  uint64_t lcg = 0x9E3779B97F4A7C15ull + (uint64_t)sh.M * 1315423911u + (uint64_t)sh.N * 2654435761u + (uint64_t)sh.K;
  auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(lcg >> 33); };
  std::vector<int8_t> ai((size_t)sh.M * sh.K), bi((size_t)sh.K * sh.N);
  for (auto& v : ai) v = (int8_t)((int)(next() % 5) - 2);
  for (auto& v : bi) v = (int8_t)((int)(next() % 5) - 2);
  for (int8_t v : ai) K.h.a.push_back(bf16_rne((float)(v * scale)));   // a small integer times a power of two: a bf16 value
  for (int8_t v : bi) K.h.b.push_back(bf16_rne((float)v));
  std::vector<double> bias(sh.N, 0.0), z(dact ? cn : 0);
  for (int n = 0; n < sh.N && K.V.out->bias; ++n) {
    bias[n] = (double)(((n * 37 + 11) % 513) - 256) / 256.0;   // |q| <= 256: at most 8 significant bits, a bf16 value
    K.h.bias.push_back(bf16_rne((float)bias[n]));
  }
  K.h.z.resize(cn), K.h.relu.resize(cn), K.h.y.resize(cn), K.h.eps.resize(cn);
  for (size_t i = 0; i < z.size(); ++i) {
    z[i] = (double)((int)(next() % 257) - 128) / 32.0;   // |q| <= 128: at most 8 significant bits, a bf16 value
    K.h.z[i] = (i % 29 == 7) ? (uint16_t)0x8000 : bf16_rne((float)z[i]);   // some -0
    if (i % 29 == 7) z[i] = 0.0;
  }
  const std::vector<int8_t> bt = K.V.L->b_col_major ? bi : transposed(bi, sh.K, sh.N);   // [N][K]
  for (int m = 0; m < sh.M; ++m)
    for (int n = 0; n < sh.N; ++n) {
      int acc = 0;
      const int8_t *ar = &ai[(size_t)m * sh.K], *br = &bt[(size_t)n * sh.K];
      for (int k = 0; k < sh.K; ++k) acc += ar[k] * br[k];
      const double s = acc * scale, t = s + bias[n];   // t: the pre-activation of an act call
      if ((double)(float)t != t || (double)(float)s != s) {
        fprintf(stderr, "check %s: %s is not exact in fp32 at %d_%d_%d\n", K.lay.c_str(), dact ? "S" : "z", sh.M, sh.N, sh.K);
        return 2;
      }
      const size_t i = (size_t)m * sh.N + n;
      if (dact) {
        K.h.relu[i] = z[i] <= 0 ? (uint16_t)0 : bf16_rne((float)s);
        K.h.y[i] = s * dact_fp64(z[i], K.act), K.h.eps[i] = (double)hgemm_mi355x::DACT_EPS * fabs(s);
      } else {
        K.h.z[i] = bf16_rne((float)t);
        K.h.relu[i] = t > 0 ? K.h.z[i] : (uint16_t)0;
        K.h.y[i] = act_fp64(t, K.act), K.h.eps[i] = ldexp(fabs(t), -19);
      }
    }
  return 0;
}
// The GELU bar of one element: |c - y| <= 1/2 ulp_bf16(y) + eps (a NaN fails); `worst` keeps the largest err / bar that passed.
static bool within_gelu_bar(uint16_t c, double y, double eps, double& worst) {
  const double bar = (y != 0 ? ldexp(1.0, (int)floor(log2(fabs(y))) - 8) : 0.0) + eps, err = fabs(bf16_value(c) - y);
  if (!(err <= bar)) return false;
  if (bar > 0) worst = std::max(worst, err / bar);
  return true;
}
static int judge_act(Check& K) {   // act, aux, dact; the C of dbias
  const uint16_t* got = (const uint16_t*)K.got.data();
  size_t bad = 0;
  if (K.V.out->z == kZWritten) {   // z_out = bf16(z), bit for bit
    std::vector<uint16_t> got_z(K.cn);
    HIP_OK(hipMemcpy(got_z.data(), K.call.z, K.cn * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < K.cn; ++i) bad += got_z[i] != K.h.z[i];
  }
  for (size_t i = 0; i < K.cn; ++i) bad += K.act == HGEMM_ACT_RELU ? got[i] != K.h.relu[i] : !within_gelu_bar(got[i], K.h.y[i], K.h.eps[i], K.worst);
  K.report(bad);
  return 0;
}
// --dbias: C by the dact bars, then: C is the dact call's at the same plan bit for bit; db32 is the column sum of the C read back, taken in
// fp64 -- ReLU: every C is a multiple of `scale` and every column sum exact in fp32 in any order (verified), so bit for bit; the GELUs:
// inside gamma_(M-1) sum |C|, the bound of an M-term fp32 sum in any order (hgemm_dbias.hpp) --; nothing behind db32[N - 1] is written;
// accumulate = 1 is fl32(old + s).  (Two more launches, not counted as runs.)
static int judge_dbias(Check& K) {
  judge_act(K);
  const Shape& sh = K.sh;
  const size_t cn = K.cn;
  const int lda = K.V.L->lda(sh), ldb = K.V.L->ldb(sh);
  const char* lay = K.lay.c_str();
  const uint16_t* got = (const uint16_t*)K.got.data();
  const std::vector<float> db_old = dbias_prefill(sh.N, true);
  std::vector<float> db_got(db_old.size()), db_acc(db_old.size());
  std::vector<uint16_t> dact_c(cn);
  DevBufs dev;
  TrCall twin = K.call;   // the dact call on the same operands, into a C of its own
  twin.c = dev.alloc(cn * 2);
  HIP_OK(hipMemcpy(db_got.data(), K.call.db32, db_got.size() * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemset(twin.c, 0xff, cn * 2));
  const int st_d = launch_dact(K.cfg, K.splits, twin, sh, lda, ldb);
  HIP_OK(hipMemcpy(K.call.db32, db_old.data(), db_old.size() * 4, hipMemcpyHostToDevice));
  K.call.accumulate = 1;
  const int st_a = K.V.launch(K.cfg, K.splits, K.call, sh, lda, ldb);
  K.call.accumulate = 0;
  const hipError_t e_d = hipDeviceSynchronize();
  if (e_d != hipSuccess) { printf("FAIL %s %d_%d_%d %s s=%d: hip %d\n", lay, sh.M, sh.N, sh.K, K.cname, K.splits & HGEMM_SPLITK_MASK, (int)e_d); return 3; }
  HIP_OK(hipMemcpy(dact_c.data(), twin.c, cn * 2, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(db_acc.data(), K.call.db32, db_acc.size() * 4, hipMemcpyDeviceToHost));
  size_t c_differs = 0, db_bad = 0, acc_bad = 0, guard_bad = 0;
  for (size_t i = 0; i < cn; ++i) c_differs += got[i] != dact_c[i];
  for (int n = 0; n < DBIAS_GUARD; ++n) guard_bad += (db_got[sh.N + n] != DBIAS_SENTINEL) + (db_acc[sh.N + n] != DBIAS_SENTINEL);
  for (int n = 0; n < sh.N; ++n) {
    double sum = 0.0, mag = 0.0;
    for (int m = 0; m < sh.M; ++m) { const double v = bf16_value(got[(size_t)m * sh.N + n]); sum += v; mag += fabs(v); }
    if (K.act == HGEMM_ACT_RELU) {
      if ((double)(float)sum != sum) { fprintf(stderr, "check %s: a column sum is not exact in fp32 at %d_%d_%d\n", lay, sh.M, sh.N, sh.K); return 2; }
      const float want = (float)sum;
      db_bad += memcmp(&want, &db_got[n], 4) != 0;
    } else {
      const double bar = hgemm_mi355x::colsum_gamma(sh.M) * mag, err = fabs((double)db_got[n] - sum);
      if (!(err <= bar)) ++db_bad;   // (a NaN fails)
      else if (bar > 0) K.worst_db = std::max(K.worst_db, err / bar);
    }
    const float want_acc = db_old[n] + db_got[n];
    acc_bad += memcmp(&want_acc, &db_acc[n], 4) != 0;
  }
  if (st_d != HGEMM_OK || st_a != HGEMM_OK || c_differs || db_bad || acc_bad || guard_bad) {
    printf("FAIL %s %d_%d_%d %s s=%d%s: status %d %d, %zu/%zu elements of C differ from the dact call's, %zu/%d columns of db32 %s, %zu not fl32(old + s), "
           "%zu guard floats written\n", lay, sh.M, sh.N, sh.K, K.cname, K.splits & HGEMM_SPLITK_MASK, (K.splits & HGEMM_PLAN_NT_STORE) ? "|nt" : "", st_d, st_a,
           c_differs, cn, db_bad, sh.N, K.act == HGEMM_ACT_RELU ? "differ from the exact sum" : "outside the bar", acc_bad, guard_bad);
    ++K.failures;
  }
  return 0;
}
static void summary_act(const Check& K) {
  const char* lay = K.lay.c_str();
  const bool relu = K.act == HGEMM_ACT_RELU, dact = K.V.out->z == kZRead;
  if (K.V.out->db32 && relu) printf("check-%s-db32: bit-exact against the fp64 column sum of the C read back; C the dact call's bit for bit\n", lay);
  else if (K.V.out->db32) printf("check-%s-db32: every column within gamma_(M-1) sum |C| of the fp64 column sum of the C read back (worst %.3f of it); "
                                 "C the dact call's bit for bit\n", lay, K.worst_db);
  if (relu) printf("check %s: %d runs, %d failures (bit-exact against %s)\n", lay, K.runs, K.failures,
                   dact ? "where(z <= 0, +0, bf16(S)) of the exact S" : "where(z > 0, bf16(z), +0) of the exact z");
  else printf("check %s: %d runs, %d failures (every element within %s; worst %.3f of it)\n", lay, K.runs, K.failures,
              dact ? "1/2 ulp_bf16(S g*) + 2^-19 |S| of the fp64 product" : "1/2 ulp_bf16(y*) + 2^-19 |z| of the fp64 activation of the exact z", K.worst);
}

// ---- The gated kind's check (--gated A with --layout tn --bf16; bgemm_mi355x_tn_gated) --------------------------------------------------------
// C = bf16(act(Sg + bias_g[n]) x (Su + bias_u[n])), sh.N the output width.  Wg and Wu independent integers in -2 .. 2, A scaled as in
// operands_small_int, two bias vectors of multiples of 2^-8 in [-1, 1]: g and u are exact in fp32 in any order (verified per element).
// The bars: ReLU bit for bit against bf16(fl32(relu(g) u)); the other three |C - y*| <= 1/2 ulp_bf16(y*) + GATED_ACT_EPS |g| |u| +
// GATED_MUL_EPS |y*|, y* = act*(g) u in fp64 (hgemm_gated.hpp).  C is followed by GATED_GUARD sentinel bytes that no run may change.
constexpr size_t GATED_GUARD = 64;
constexpr int GATED_SENTINEL = 0x5a;
static int operands_gated(Check& K) {
  const Shape& sh = K.sh;
  int j = 0;
  while ((2 << j) <= sh.K) ++j;   // floor(log2 K)
  const double scale = ldexp(1.0, -std::max(j - 2, 0));
  uint64_t lcg = 0xD1B54A32D192ED03ull + (uint64_t)sh.M * 1315423911u + (uint64_t)sh.N * 2654435761u + (uint64_t)sh.K;
  auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(lcg >> 33); };
  std::vector<int8_t> ai((size_t)sh.M * sh.K), gi((size_t)sh.N * sh.K), ui((size_t)sh.N * sh.K);   // A [M][K], Wg and Wu [N][K]
  for (auto& v : ai) v = (int8_t)((int)(next() % 5) - 2);
  for (auto& v : gi) v = (int8_t)((int)(next() % 5) - 2);
  for (auto& v : ui) v = (int8_t)((int)(next() % 5) - 2);
  for (int8_t v : ai) K.h.a.push_back(bf16_rne((float)(v * scale)));
  for (int8_t v : gi) K.h.b.push_back(bf16_rne((float)v));
  for (int8_t v : ui) K.h.b2.push_back(bf16_rne((float)v));
  std::vector<double> bg(sh.N), bu(sh.N);
  for (int n = 0; n < sh.N; ++n) {
    bg[n] = (double)(((n * 37 + 11) % 513) - 256) / 256.0;   // |q| <= 256: at most 8 significant bits, a bf16 value
    bu[n] = (double)(((n * 101 + 300) % 513) - 256) / 256.0;
    K.h.bias.push_back(bf16_rne((float)bg[n]));
    K.h.bias2.push_back(bf16_rne((float)bu[n]));
  }
  K.h.relu.resize(K.cn), K.h.y.resize(K.cn), K.h.eps.resize(K.cn);
  if (K.V.out->gaux) K.h.z.resize(2 * K.cn);   // what g_out and behind it u_out must hold: bf16(g), bf16(u) of gated_pre's value
  for (int m = 0; m < sh.M; ++m)
    for (int n = 0; n < sh.N; ++n) {
      int sg = 0, su = 0;
      const int8_t *ar = &ai[(size_t)m * sh.K], *gr = &gi[(size_t)n * sh.K], *ur = &ui[(size_t)n * sh.K];
      for (int k = 0; k < sh.K; ++k) sg += ar[k] * gr[k], su += ar[k] * ur[k];
      const double g = sg * scale + bg[n], u = su * scale + bu[n];
      if ((double)(float)g != g || (double)(float)u != u || (double)(float)(sg * scale) != sg * scale || (double)(float)(su * scale) != su * scale) {
        fprintf(stderr, "check %s: g or u is not exact in fp32 at %d_%d_%d\n", K.lay.c_str(), sh.M, sh.N, sh.K);
        return 2;
      }
      const size_t i = (size_t)m * sh.N + n;
      const float gf = (float)g, uf = (float)u;
      if (K.V.out->gaux) {
        K.h.z[i] = bf16_rne(hgemm_mi355x::gated_pre((float)(sg * scale), (float)bg[n]));
        K.h.z[K.cn + i] = bf16_rne(hgemm_mi355x::gated_pre((float)(su * scale), (float)bu[n]));
      }
      K.h.relu[i] = bf16_rne(hgemm_mi355x::gated_mul(gf > 0 ? gf : 0.0f, uf));
      K.h.y[i] = act_fp64(g, K.act) * u;
      K.h.eps[i] = hgemm_mi355x::GATED_ACT_EPS * fabs(g) * fabs(u) + hgemm_mi355x::GATED_MUL_EPS * fabs(K.h.y[i]);
    }
  return 0;
}
static int judge_gated(Check& K) {   // C by judge_act's two rules, then the sentinels behind C
  judge_act(K);
  unsigned char guard[GATED_GUARD];
  HIP_OK(hipMemcpy(guard, (const unsigned char*)K.call.c + K.cn * 2, GATED_GUARD, hipMemcpyDeviceToHost));
  size_t changed = 0;
  for (unsigned char g : guard) changed += g != GATED_SENTINEL;
  if (changed) {
    printf("FAIL %s %d_%d_%d %s s=%d: %zu sentinel bytes behind C changed\n", K.lay.c_str(), K.sh.M, K.sh.N, K.sh.K, K.cname, K.splits & HGEMM_SPLITK_MASK, changed);
    ++K.failures;
  }
  return 0;
}
static void summary_gated(const Check& K) {
  if (K.act == HGEMM_ACT_RELU) printf("check %s: %d runs, %d failures (bit-exact against bf16(relu(g) u) of the exact g and u)\n", K.lay.c_str(), K.runs, K.failures);
  else printf("check %s: %d runs, %d failures (every element within 1/2 ulp_bf16(y*) + 2^-19 |g| |u| + 2^-23 |y*| of the fp64 value of the exact g and u; worst %.3f of it)\n",
              K.lay.c_str(), K.runs, K.failures, K.worst);
}

// ---- The gated aux kind's check (--gated-aux A with --layout tn --bf16; bgemm_mi355x_tn_gated_aux): operands_gated's operands, C judged as
// --gated judges it, g_out and u_out bit for bit against bf16(g) and bf16(u) for every activation; each of the three outputs is followed by
// GATED_GUARD sentinel bytes.
static int judge_gated_aux(Check& K) {
  judge_gated(K);
  const size_t cn = K.cn;
  std::vector<uint16_t> go(cn), uo(cn);
  unsigned char guard[2][GATED_GUARD];
  HIP_OK(hipMemcpy(go.data(), K.call.z, cn * 2, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(uo.data(), K.call.c2, cn * 2, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(guard[0], (const unsigned char*)K.call.z + cn * 2, GATED_GUARD, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(guard[1], (const unsigned char*)K.call.c2 + cn * 2, GATED_GUARD, hipMemcpyDeviceToHost));
  size_t bad = 0, changed = 0;
  for (size_t i = 0; i < cn; ++i) bad += (go[i] != K.h.z[i]) + (uo[i] != K.h.z[cn + i]);
  if (bad) {
    printf("FAIL %s %d_%d_%d %s s=%d%s: %zu elements of g_out / u_out differ from bf16(g) / bf16(u)\n", K.lay.c_str(), K.sh.M, K.sh.N, K.sh.K, K.cname,
           K.splits & HGEMM_SPLITK_MASK, (K.splits & HGEMM_PLAN_NT_STORE) ? "|nt" : "", bad);
    ++K.failures;
  }
  for (const auto& gd : guard) for (unsigned char b : gd) changed += b != GATED_SENTINEL;
  if (changed) {
    printf("FAIL %s %d_%d_%d %s s=%d: %zu sentinel bytes behind g_out or u_out changed\n", K.lay.c_str(), K.sh.M, K.sh.N, K.sh.K, K.cname, K.splits & HGEMM_SPLITK_MASK, changed);
    ++K.failures;
  }
  return 0;
}
static void summary_gated_aux(const Check& K) {
  summary_gated(K);
  printf("check %s: g_out and u_out bit-exact against bf16(g) and bf16(u) in every run\n", K.lay.c_str());
}

// ---- The residual kinds' check (--bias-add with --layout tn --bf16, --nn-add with --layout nn --bf16) ------------------------------------------
// C = bf16((S + bias[n]) + r[m][n]) / bf16(S + r[m][n]), hgemm_residual.hpp's text on the host.  A, B and the bias as in operands_small_int: S
// is exact in fp32 in any order (verified per element); r a seeded matrix of multiples of 1/32 in [-4, 4] (bf16 values, some -0).  Every run
// is judged bit for bit and then made once more IN PLACE -- C refilled with r and passed as r too -- and judged again.
static int operands_add(Check& K) {
  const Shape& sh = K.sh;
  const size_t cn = K.cn;
  int j = 0;
  while ((2 << j) <= sh.K) ++j;   // floor(log2 K)
  const double scale = ldexp(1.0, -std::max(j - 2, 0));
  uint64_t lcg = 0x9E3779B97F4A7C15ull + (uint64_t)sh.M * 1315423911u + (uint64_t)sh.N * 2654435761u + (uint64_t)sh.K;
  auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(lcg >> 33); };
  std::vector<int8_t> ai((size_t)sh.M * sh.K), bi((size_t)sh.K * sh.N);
  for (auto& v : ai) v = (int8_t)((int)(next() % 5) - 2);
  for (auto& v : bi) v = (int8_t)((int)(next() % 5) - 2);
  for (int8_t v : ai) K.h.a.push_back(bf16_rne((float)(v * scale)));
  for (int8_t v : bi) K.h.b.push_back(bf16_rne((float)v));
  std::vector<float> bias(sh.N, 0.0f);
  for (int n = 0; n < sh.N && K.V.out->bias; ++n) {
    bias[n] = (float)(((n * 37 + 11) % 513) - 256) / 256.0f;
    K.h.bias.push_back(bf16_rne(bias[n]));
  }
  K.h.z.resize(cn), K.h.want[0].resize(cn * 2);
  const std::vector<int8_t> bt = K.V.L->b_col_major ? bi : transposed(bi, sh.K, sh.N);   // [N][K]
  for (int m = 0; m < sh.M; ++m)
    for (int n = 0; n < sh.N; ++n) {
      int acc = 0;
      const int8_t *ar = &ai[(size_t)m * sh.K], *br = &bt[(size_t)n * sh.K];
      for (int k = 0; k < sh.K; ++k) acc += ar[k] * br[k];
      const double s = acc * scale;
      if ((double)(float)s != s) { fprintf(stderr, "check %s: S is not exact in fp32 at %d_%d_%d\n", K.lay.c_str(), sh.M, sh.N, sh.K); return 2; }
      const size_t i = (size_t)m * sh.N + n;
      K.h.z[i] = (i % 29 == 7) ? (uint16_t)0x8000 : bf16_rne((float)((int)(next() % 257) - 128) / 32.0f);
      const float r = (float)bf16_value(K.h.z[i]);
      const uint16_t w = bf16_rne(K.V.out->bias ? hgemm_mi355x::bias_residual_add((float)s, bias[n], r) : hgemm_mi355x::residual_add((float)s, r));
      memcpy(&K.h.want[0][i * 2], &w, 2);
    }
  return 0;
}
static int judge_add(Check& K) {
  judge_exact(K);   // the out-of-place run
  const Shape& sh = K.sh;
  const void* r = K.call.z;
  HIP_OK(hipMemcpy(K.call.c, r, K.cn * 2, hipMemcpyDeviceToDevice));
  K.call.z = K.call.c;
  const int st = K.V.launch(K.cfg, K.splits, K.call, sh, K.V.L->lda(sh), K.V.L->ldb(sh));
  K.call.z = const_cast<void*>(r);
  const hipError_t e = hipDeviceSynchronize();
  if (st != HGEMM_OK || e != hipSuccess) {
    printf("FAIL %s %d_%d_%d %s s=%d in place: status %d hip %d\n", K.lay.c_str(), sh.M, sh.N, sh.K, K.cname, K.splits & HGEMM_SPLITK_MASK, st, (int)e);
    ++K.failures;
    return e != hipSuccess ? 3 : 0;
  }
  HIP_OK(hipMemcpy(K.got.data(), K.call.c, K.cn * 2, hipMemcpyDeviceToHost));
  const int before = K.failures;
  judge_exact(K);
  if (K.failures != before) printf("     (the in-place run, r == c)\n");
  return 0;
}
static void summary_add(const Check& K) {
  printf("check %s: %d runs, %d failures (each run out of place and in place, bit-exact against bf16(%s) of the exact S)\n", K.lay.c_str(), K.runs, K.failures,
         K.V.out->bias ? "(S + bias) + r" : "S + r");
}

// ---- The dgated kind's check (--dgated A with --layout nn --bf16; bgemm_mi355x_nn_dgated) ------------------------------------------------------
// dg = bf16(dact_mul(fl32(S u), g)), du = bf16(fl32(act(g) S)): A and B as in operands_small_int, so S is exact in fp32 in any order (verified
// per element); g and u seeded matrices of multiples of 1/32 in [-4, 4] (bf16 values; both signs, zeros, some -0).  The bars: ReLU bit for bit
// against hgemm_dgated.hpp's dgated_store on the exact S; the other three |dg - S u act'*(g)| <= 1/2 ulp_bf16(.) + 2^-19 |S u| and
// |du - act*(g) S| <= 1/2 ulp_bf16(.) + 2^-19 |g| |S| + 2^-23 |.|, fp64 values.  Each output is followed by GATED_GUARD sentinel bytes.
static double dact_fp64_any(double z, int act) {
  if (act != HGEMM_ACT_SILU) return dact_fp64(z, act);
  const double s = 1.0 / (1.0 + exp(-z));
  return s + z * s * (1.0 - s);
}
static int operands_dgated(Check& K) {
  const Shape& sh = K.sh;
  const size_t cn = K.cn;
  int j = 0;
  while ((2 << j) <= sh.K) ++j;   // floor(log2 K)
  const double scale = ldexp(1.0, -std::max(j - 2, 0));
  uint64_t lcg = 0xA0761D6478BD642Full + (uint64_t)sh.M * 1315423911u + (uint64_t)sh.N * 2654435761u + (uint64_t)sh.K;
  auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(lcg >> 33); };
  std::vector<int8_t> ai((size_t)sh.M * sh.K), bi((size_t)sh.K * sh.N);
  for (auto& v : ai) v = (int8_t)((int)(next() % 5) - 2);
  for (auto& v : bi) v = (int8_t)((int)(next() % 5) - 2);
  for (int8_t v : ai) K.h.a.push_back(bf16_rne((float)(v * scale)));
  for (int8_t v : bi) K.h.b.push_back(bf16_rne((float)v));
  std::vector<double> g(cn), u(cn);
  K.h.z.resize(cn), K.h.b2.resize(cn), K.h.relu.resize(2 * cn), K.h.y.resize(2 * cn), K.h.eps.resize(2 * cn);
  for (size_t i = 0; i < cn; ++i) {
    g[i] = (double)((int)(next() % 257) - 128) / 32.0;   // |q| <= 128: at most 8 significant bits, a bf16 value
    u[i] = (double)((int)(next() % 257) - 128) / 32.0;
    K.h.z[i] = (i % 29 == 7) ? (uint16_t)0x8000 : bf16_rne((float)g[i]);   // some -0
    if (i % 29 == 7) g[i] = 0.0;
    K.h.b2[i] = bf16_rne((float)u[i]);
  }
  const std::vector<int8_t> bt = transposed(bi, sh.K, sh.N);   // [N][K]
  for (int m = 0; m < sh.M; ++m)
    for (int n = 0; n < sh.N; ++n) {
      int acc = 0;
      const int8_t *ar = &ai[(size_t)m * sh.K], *br = &bt[(size_t)n * sh.K];
      for (int k = 0; k < sh.K; ++k) acc += ar[k] * br[k];
      const double s = acc * scale;
      if ((double)(float)s != s) { fprintf(stderr, "check %s: S is not exact in fp32 at %d_%d_%d\n", K.lay.c_str(), sh.M, sh.N, sh.K); return 2; }
      const size_t i = (size_t)m * sh.N + n;
      const hgemm_mi355x::DgatedPair r = hgemm_mi355x::dgated_store<HGEMM_ACT_RELU>((float)s, (float)bf16_value(K.h.z[i]), (float)u[i]);
      K.h.relu[i] = bf16_rne(r.dg), K.h.relu[cn + i] = bf16_rne(r.du);
      K.h.y[i] = s * u[i] * dact_fp64_any(g[i], K.act), K.h.eps[i] = ldexp(fabs(s * u[i]), hgemm_mi355x::DGATED_DACT_EPS_LOG2);
      K.h.y[cn + i] = act_fp64(g[i], K.act) * s;
      K.h.eps[cn + i] = ldexp(fabs(g[i]) * fabs(s), hgemm_mi355x::DGATED_ACT_EPS_LOG2) + ldexp(fabs(K.h.y[cn + i]), hgemm_mi355x::DGATED_MUL_EPS_LOG2);
    }
  return 0;
}
static int judge_dgated(Check& K) {   // both outputs by judge_act's two rules, then the sentinels behind each
  const size_t cn = K.cn;
  std::vector<uint16_t> du(cn);
  unsigned char guard[2][GATED_GUARD];
  HIP_OK(hipMemcpy(du.data(), K.call.c2, cn * 2, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(guard[0], (const unsigned char*)K.call.c + cn * 2, GATED_GUARD, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(guard[1], (const unsigned char*)K.call.c2 + cn * 2, GATED_GUARD, hipMemcpyDeviceToHost));
  const uint16_t* dg = (const uint16_t*)K.got.data();
  size_t bad = 0, changed = 0;
  for (size_t i = 0; i < cn; ++i) {
    if (K.act == HGEMM_ACT_RELU) bad += (dg[i] != K.h.relu[i]) || (du[i] != K.h.relu[cn + i]);
    else bad += !within_gelu_bar(dg[i], K.h.y[i], K.h.eps[i], K.worst) || !within_gelu_bar(du[i], K.h.y[cn + i], K.h.eps[cn + i], K.worst);
  }
  K.report(bad);
  for (const auto& gd : guard) for (unsigned char b : gd) changed += b != GATED_SENTINEL;
  if (changed) {
    printf("FAIL %s %d_%d_%d %s s=%d: %zu sentinel bytes behind dg or du changed\n", K.lay.c_str(), K.sh.M, K.sh.N, K.sh.K, K.cname, K.splits & HGEMM_SPLITK_MASK, changed);
    ++K.failures;
  }
  return 0;
}
static void summary_dgated(const Check& K) {
  if (K.act == HGEMM_ACT_RELU) printf("check %s: %d runs, %d failures (both outputs bit-exact against bf16(relu(g) S) and where(g <= 0, +0, bf16(S u)) of the exact S)\n", K.lay.c_str(), K.runs, K.failures);
  else printf("check %s: %d runs, %d failures (every element of dg within 1/2 ulp_bf16 + 2^-19 |S u| and of du within 1/2 ulp_bf16 + 2^-19 |g| |S| + 2^-23 |du*| of the fp64 "
              "values of the exact S; worst %.3f of it)\n", K.lay.c_str(), K.runs, K.failures, K.worst);
}

static int tr_check(const Variant& V, int act, std::vector<Shape> shapes) {
  const TrLayout& L = *V.L;
  const OutKind& O = *V.out;
  if (shapes.empty()) shapes = parse_shapes(L.check_shapes);
  const size_t esz = O.c32 ? 4 : 2;   // bytes per element of C
  Check K = {V, act, V.words("", "-", act)};
  const char* lay = K.lay.c_str();
  const int nc = L.num_configs();
  for (const Shape& sh : shapes) {
    const size_t cn = (size_t)sh.M * sh.N;
    K.sh = sh, K.cn = cn, K.h = {};
    if (const int refused = V.check->operands(K)) return refused;
    DevBufs dev;
    TrCall& call = K.call;
    call = {dev.upload(K.h.a.data(), K.h.a.size() * 2), dev.upload(K.h.b.data(), K.h.b.size() * 2),
            O.bias || O.gated ? dev.upload(K.h.bias.data(), K.h.bias.size() * 2) : nullptr, dev.alloc(cn * esz + (O.gated || O.dgated ? GATED_GUARD : 0)), 0,
            O.z == kZRead || O.dgated || O.add ? dev.upload(K.h.z.data(), cn * 2) : O.z == kZWritten ? dev.alloc(cn * 2) : O.gaux ? dev.alloc(cn * 2 + GATED_GUARD) : nullptr,
            O.db32 ? (float*)dev.alloc((sh.N + DBIAS_GUARD) * sizeof(float)) : nullptr, act};
    if (O.gated) {
      call.b2 = dev.upload(K.h.b2.data(), K.h.b2.size() * 2), call.bias2 = dev.upload(K.h.bias2.data(), K.h.bias2.size() * 2);
      HIP_OK(hipMemset((unsigned char*)call.c + cn * esz, GATED_SENTINEL, GATED_GUARD));
    }
    if (O.gaux) {
      call.c2 = dev.alloc(cn * 2 + GATED_GUARD);
      HIP_OK(hipMemset((unsigned char*)call.z + cn * 2, GATED_SENTINEL, GATED_GUARD));
      HIP_OK(hipMemset((unsigned char*)call.c2 + cn * 2, GATED_SENTINEL, GATED_GUARD));
    }
    if (O.dgated) {
      call.b2 = dev.upload(K.h.b2.data(), cn * 2), call.c2 = dev.alloc(cn * 2 + GATED_GUARD);
      HIP_OK(hipMemset((unsigned char*)call.c + cn * 2, GATED_SENTINEL, GATED_GUARD));
      HIP_OK(hipMemset((unsigned char*)call.c2 + cn * 2, GATED_SENTINEL, GATED_GUARD));
    }
    K.got.resize(cn * esz);
    for (int c = 0; c < nc; ++c) {
      K.cfg = c;
      K.cname = L.config_name(c);
      const int own = V.runs_at(c, sh);
      for (int splits : {1, 1 | HGEMM_PLAN_NT_STORE, 2, 5})
        for (call.accumulate = 0; call.accumulate <= (O.c32 ? 1 : 0); ++call.accumulate) {
          K.splits = splits;
          if (call.accumulate) HIP_OK(hipMemcpy(call.c, K.h.old.data(), cn * esz, hipMemcpyHostToDevice));
          else                 HIP_OK(hipMemset(call.c, 0xff, cn * esz));   // NaN pattern: a store must not read it, unwritten outputs are caught
          if (O.z == kZWritten) HIP_OK(hipMemset(call.z, 0xff, cn * 2));
          if (O.dgated || O.gaux) HIP_OK(hipMemset(call.c2, 0xff, cn * 2));
          if (O.gaux) HIP_OK(hipMemset(call.z, 0xff, cn * 2));
          if (O.db32) HIP_OK(hipMemcpy(call.db32, dbias_prefill(sh.N, false).data(), (sh.N + DBIAS_GUARD) * sizeof(float), hipMemcpyHostToDevice));
          const int st = V.launch(c, splits, call, sh, L.lda(sh), L.ldb(sh));
          const hipError_t e = hipDeviceSynchronize();
          ++K.runs;
          if (st != HGEMM_OK || e != hipSuccess) {
            printf("FAIL %s %d_%d_%d %s s=%d%s: status %d hip %d\n", lay, sh.M, sh.N, sh.K, K.cname, splits & HGEMM_SPLITK_MASK,
                   !O.c32 ? "" : call.accumulate ? " acc=1" : " acc=0", st, (int)e);
            ++K.failures;
            if (e != hipSuccess) return 3;
            continue;
          }
          HIP_OK(hipMemcpy(K.got.data(), call.c, cn * esz, hipMemcpyDeviceToHost));
          if (const int ended = V.check->judge(K)) return ended;
        }
      if (c == 0) printf("checked %s %d_%d_%d (%s)\n", lay, sh.M, sh.N, sh.K, own ? L.kernels : "outside their scope: the reference kernel");
    }
    fflush(stdout);
  }
  if (O.z != kZRead) {   // (the dact kinds' check has never printed the two footers; its output is kept byte for byte)
    printf("check-%s-configs:", lay);
    for (int c = 0; c < nc; ++c) printf(" %s", L.config_name(c));
    printf("\ncheck-%s-forms: 1 1|nt-store 2 5%s\n", lay, O.c32 ? " x store accumulate" : "");
  }
  V.check->summary(K);
  return K.failures ? 1 : 0;
}

// ---- bench --layout ...: the check first, then per shape ONE set of interleaved rounds (time_interleaved) of the variant's contenders --
// what a caller without the fp32-C call runs behind hgemm_mi355x_ta_fp32: main_grad += float(dW16), a plain grid-stride kernel
__global__ void add_f16_into_f32_kernel(float* __restrict__ c32, const f16* __restrict__ c16, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) c32[i] += (float)c16[i];
}
__global__ void f16_to_bf16_kernel(const f16* __restrict__ in, __bf16* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = (__bf16)(float)in[i];
}
__global__ void fill_bias_kernel(__bf16* __restrict__ bias, int n) {   // N(0,1)-sized values, a fixed pattern: timing only
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) bias[i] = (__bf16)((float)((i * 37) % 129 - 64) * (1.0f / 32.0f));
}
__global__ void add_bias_kernel(__bf16* __restrict__ c, const __bf16* __restrict__ bias, size_t total, int n) {   // the unfused second pass
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    c[i] = (__bf16)((float)c[i] + (float)bias[i % n]);
}

// One shape of one bench, as its description sees it: the two operand sets (alloc_set: a [M][K], b [K][N], bt = b_col_major [N][K] of the
// same B, c [M][N]; fp16, N(0,1)), helpers for the further buffers a contender needs -- one per set, freed with this object --, and what
// the description leaves for the driver: contenders, header fields, rounds, verdict.
struct TrBench {
  typedef std::array<void*, 2> PerSet;   // one device pointer per operand set
  const Variant& V;
  const Shape sh;
  const int act;                         // the call's activation (HGEMM_ACT_*), 0 where the kind takes none
  const bool autotune;
  const size_t a_elems, b_elems, cn;
  std::vector<Buffers> sets;
  DevBufs dev;
  int cfg = 0, splits = 1;               // V's plan for sh
  int rounds = 15;
  std::vector<Contender> cs;
  std::string header;                    // the record's fields between "layout" and "rounds"
  const char* verdict_key = nullptr;     // "<key>": cs[va] <= cs[vb] (+ cs[vb]'s slowest round minus its median, recorded as "<vb's key>_spread_us")
  int va = 0, vb = 1;
  bool with_spread = true;
  TrBench(const Variant& v, int activation, const Shape& s, bool at)
      : V(v), sh(s), act(activation), autotune(at), a_elems((size_t)s.M * s.K), b_elems((size_t)s.K * s.N), cn((size_t)s.M * s.N), sets(2) {
    for (size_t i = 0; i < sets.size(); ++i) alloc_set(sets[i], sh, V.bench->seed0 + i, true);
    V.L->plan(sh.M, sh.N, sh.K, &cfg, &splits);
  }
  ~TrBench() { for (Buffers& s : sets) free_set(s); }
  PerSet alloc(size_t bytes, bool zeroed = false) {
    PerSet p;
    for (void*& q : p) {
      q = dev.alloc(bytes);
      if (zeroed) HIP_OK(hipMemset(q, 0, bytes));
    }
    return p;
  }
  PerSet of(f16* Buffers::*member) { return {sets[0].*member, sets[1].*member}; }
  PerSet a_col_major() {   // [K][M] of each set's a
    PerSet p = alloc(a_elems * 2);
    for (size_t i = 0; i < p.size(); ++i) transpose_kernel<<<(unsigned)((a_elems + 255) / 256), 256>>>(sets[i].a, (f16*)p[i], sh.M, sh.K);
    return p;
  }
  PerSet to_bf16(const PerSet& src, size_t n) {
    PerSet p = alloc(n * 2);
    for (size_t i = 0; i < p.size(); ++i) f16_to_bf16_kernel<<<2048, 256>>>((const f16*)src[i], (__bf16*)p[i], n);
    return p;
  }
  // contenders are timed in the order they are added (time_interleaved rotates by index); f(set, the set's index into a PerSet)
  void add(const char* key, std::function<int(Buffers&, size_t)> f) {
    Buffers* first = sets.data();
    cs.push_back({key, [first, f](Buffers& b) { return f(b, (size_t)(&b - first)); }});
  }
  __attribute__((format(printf, 2, 3))) void head(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    header = buf;
  }
  void verdict(const char* key, int a, int b, bool spread) { verdict_key = key; va = a; vb = b; with_spread = spread; }
};

static int tr_bench(const Variant& V, int act, const std::vector<Shape>& shapes, const char* out_path, bool autotune) {
  const int rc = tr_check(V, act, {});   // no timing of a kernel that is wrong
  if (rc != 0) { fprintf(stderr, "bench %s: the check failed, nothing is timed\n", V.words("--layout ", " --").c_str()); return rc; }
  FILE* out = out_path ? fopen(out_path, "w") : stdout;
  if (!out) { fprintf(stderr, "cannot open %s\n", out_path); return 2; }
  V.bench->warm(autotune);
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  for (const Shape& sh : shapes) {
    TrBench B(V, act, sh, autotune);
    V.bench->shape(B);
    HIP_OK(hipDeviceSynchronize());
    time_interleaved(B.cs, B.sets, B.rounds, 0, 0.0, 1.0, e0, e1);
    // one JSON record per shape: the description's header fields (plan, whether the family's kernel runs it), then the contenders' times
    const double flops = 2.0 * sh.M * sh.N * (double)sh.K;
    fprintf(out, "{\"mnk\": \"%d_%d_%d\", \"layout\": \"%s\", %s, \"rounds\": %d, \"protocol\": \"interleaved\"", sh.M, sh.N, sh.K, V.L->label,
            B.header.c_str(), B.rounds);
    for (const Contender& c : B.cs) {
      const double us = c.iso_us();
      fprintf(out, ", \"%s_us\": %.3f, \"%s_tflops\": %.2f", c.key, us, c.key, us > 0 ? flops / us * 1e-6 : -1.0);
    }
    if (B.verdict_key) {
      const Contender &x = B.cs[B.va], &y = B.cs[B.vb];
      const double x_us = x.iso_us(), y_us = y.iso_us();
      double slack = 0.0;
      if (B.with_spread) {
        slack = y.ok && !y.iso.empty() ? *std::max_element(y.iso.begin(), y.iso.end()) - y_us : -1.0;
        fprintf(out, ", \"%s_spread_us\": %.3f", y.key, slack);
      }
      fprintf(out, ", \"%s\": %s", B.verdict_key, x_us > 0 && y_us > 0 && x_us <= y_us + slack ? "true" : "false");
    }
    fprintf(out, "}\n");
    fflush(out);
  }
  HIP_OK(hipEventDestroy(e0));
  HIP_OK(hipEventDestroy(e1));
  if (out != stdout) fclose(out);
  return 0;
}

// nn: the planned NN call, the reference kernel on the same operands (what a b-only call ran before the family), hipBLASLt heuristic /
// autotune _nn, and -- context only -- the shipped TN plan on the pre-built b_col_major.
static void bench_nn(TrBench& B) {
  const Shape sh = B.sh;
  const bool have_at = B.autotune && hgemm_hipblaslt_autotune_find_best_nn(sh.M, sh.N, sh.K, 0) == HGEMM_OK;   // the search before any timing
  B.add("nn", [=](Buffers& b, size_t) { return hgemm_mi355x_nn_fp32(b.a, b.b, b.c, sh.M, sh.N, sh.K, nullptr); });
  B.add("generic", [=](Buffers& b, size_t) { return hgemm_mi355x_launch(HGEMM_CONFIG_GENERIC, 1, 1, b.a, b.b, nullptr, b.c, sh.M, sh.N, sh.K, sh.K, sh.K, sh.N, nullptr); });
  B.add("heur_nn", [=](Buffers& b, size_t) { return hgemm_hipblaslt_heuristic_nn(b.a, b.b, b.c, sh.M, sh.N, sh.K, 0, nullptr); });
  if (have_at) B.add("auto_nn", [=](Buffers& b, size_t) { return hgemm_hipblaslt_autotune_nn(b.a, b.b, b.c, sh.M, sh.N, sh.K, 0, nullptr); });
  B.add("tn_shipped", [=](Buffers& b, size_t) { return hgemm_mi355x_fp32(b.a, nullptr, b.bt, b.c, sh.M, sh.N, sh.K, nullptr); });
  if (2.0 * sh.M * sh.N * (double)sh.K > 1.0e11) B.rounds = 5;   // (the reference kernel takes ~0.1 .. 0.5 s per call on the large shapes)
  B.head("\"nn_config\": \"%s\", \"nn_splits\": %d, \"nn_runs\": %d", B.V.L->config_name(B.cfg), B.splits, B.V.runs_at(B.cfg, sh));
}

// ta: the planned TA call on a_col_major, the planned NN call on the row-major A -- context: what the product costs when the transpose is
// free --, a device-to-device copy of A's bytes followed by that NN call -- no transpose pass can beat a copy, so a lower bound of what a
// caller without the TA entry points pays --, and rocBLAS on the TA operands.
static void bench_ta(TrBench& B) {
  const Shape sh = B.sh;
  const size_t a_bytes = B.a_elems * 2;
  const TrBench::PerSet at = B.a_col_major(), tmp = B.alloc(a_bytes);
  B.add("ta", [=](Buffers& b, size_t i) { return hgemm_mi355x_ta_fp32(at[i], b.b, b.c, sh.M, sh.N, sh.K, nullptr); });
  B.add("nn_pretransposed", [=](Buffers& b, size_t) { return hgemm_mi355x_nn_fp32(b.a, b.b, b.c, sh.M, sh.N, sh.K, nullptr); });
  B.add("copy_nn", [=](Buffers& b, size_t i) {
    if (hipMemcpyAsync(tmp[i], b.a, a_bytes, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) return (int)HGEMM_ERR_HIP;
    return hgemm_mi355x_nn_fp32(tmp[i], b.b, b.c, sh.M, sh.N, sh.K, nullptr);
  });
  B.add("rocblas_ta", [=](Buffers& b, size_t i) { return hgemm_rocblas_ta(at[i], b.b, b.c, sh.M, sh.N, sh.K, 0, nullptr); });
  B.head("\"ta_config\": \"%s\", \"ta_splits\": %d, \"ta_runs\": %d", B.V.L->config_name(B.cfg), B.splits, B.V.runs_at(B.cfg, sh));
}

// ta --c32: the accumulate call, the store call, and the comparator -- hgemm_mi355x_ta_fp32 into an fp16 scratch followed by the
// elementwise add.  "c32_le_two_step" is the first look's condition (accumulate call <= comparator).
static void bench_ta_c32(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const TrBench::PerSet at = B.a_col_major(), c32 = B.alloc(cn * 4, true);
  const unsigned add_grid = (unsigned)std::min<size_t>((cn + 255) / 256, 256 * 8);
  B.add("c32_accumulate", [=](Buffers& b, size_t i) { return hgemm_mi355x_ta_c32(at[i], b.b, (float*)c32[i], sh.M, sh.N, sh.K, 1, nullptr); });
  B.add("c32_store", [=](Buffers& b, size_t i) { return hgemm_mi355x_ta_c32(at[i], b.b, (float*)c32[i], sh.M, sh.N, sh.K, 0, nullptr); });
  B.add("two_step", [=](Buffers& b, size_t i) {
    const int st = hgemm_mi355x_ta_fp32(at[i], b.b, b.c, sh.M, sh.N, sh.K, nullptr);
    if (st != HGEMM_OK) return st;
    add_f16_into_f32_kernel<<<add_grid, 256>>>((float*)c32[i], b.c, cn);
    return hipGetLastError() == hipSuccess ? (int)HGEMM_OK : (int)HGEMM_ERR_HIP;
  });
  B.head("\"output\": \"c32\", \"ta_config\": \"%s\", \"ta_splits\": %d, \"ta_c32_runs\": %d", B.V.L->config_name(B.cfg), B.splits, B.V.runs_at(B.cfg, sh));
  B.verdict("c32_le_two_step", 0, 2, false);
}

// nn|ta [--c32] --bf16: the planned bf16 call, the planned fp16 call -- the same plan on the same shape: the planner does not know the
// element kind -- on the fp16 N(0,1) operands the bf16 ones were rounded from, and, context only, rocBLAS with bf16 in and out (16-bit C
// only).  c32: both calls accumulate.  The two calls move the same bytes and issue the same number of MFMAs, so the one condition is
// bf16 <= fp16 within the fp16 call's own round-to-round spread in this run: "bf16_le_fp16".
static void bench_bf16(TrBench& B) {
  const Shape sh = B.sh;
  const TrLayout* L = B.V.L;
  const bool c32 = B.V.out->c32;
  const Variant *bf = &B.V, *fp = resolve_variant({L->label, false, c32});   // (every bf16 variant of nn and ta has its fp16 twin)
  const TrBench::PerSet a16 = L->a_col_major ? B.a_col_major() : B.of(&Buffers::a);   // A as the layout takes it, fp16
  const TrBench::PerSet ab = B.to_bf16(a16, B.a_elems), bb = B.to_bf16(B.of(&Buffers::b), B.b_elems);
  const TrBench::PerSet cb = c32 ? B.alloc(B.cn * 4, true) : B.alloc(B.cn * 2), ch = c32 ? B.alloc(B.cn * 4, true) : B.of(&Buffers::c);
  B.add("bf16", [=](Buffers&, size_t i) { return bf->planned({ab[i], bb[i], nullptr, cb[i], 1}, sh); });
  B.add("fp16", [=](Buffers& b, size_t i) { return fp->planned({a16[i], b.b, nullptr, ch[i], 1}, sh); });
  if (!c32) B.add("rocblas_bf16", [=](Buffers&, size_t i) { return L->rocblas_bf16(ab[i], bb[i], cb[i], sh.M, sh.N, sh.K, nullptr); });
  B.head("\"output\": \"%s\", \"elem\": \"bf16\", \"config\": \"%s\", \"splits\": %d, \"runs\": %d", c32 ? "c32_accumulate" : "c16", L->config_name(B.cfg), B.splits,
         B.V.runs_at(B.cfg, sh));
  B.verdict("bf16_le_fp16", 0, 1, true);
}

// tn --bf16: the planned bgemm_mi355x_tn call, bgemm_mi355x_launch_nn with the same member (the two tables list the same tiles in the
// same order) and the same splits on the same shape -- the same bytes and MFMAs; ds_read_b128 where family n issues pairs of transposed
// reads --, and, context only, rocBLAS with bf16 in and out on the tn operands.  The one condition: tn <= nn within the nn call's own
// round-to-round spread in this run: "tn_le_nn".
static void bench_tn_bf16(TrBench& B) {
  const Shape sh = B.sh;
  const int cfg = B.cfg, splits = B.splits, nn_lda = kLayoutNN.lda(sh), nn_ldb = kLayoutNN.ldb(sh);
  const TrBench::PerSet ab = B.to_bf16(B.of(&Buffers::a), B.a_elems), bb = B.to_bf16(B.of(&Buffers::b), B.b_elems),
                        btb = B.to_bf16(B.of(&Buffers::bt), B.b_elems), cb = B.alloc(B.cn * 2);
  B.add("tn", [=](Buffers&, size_t i) { return bgemm_mi355x_tn(ab[i], btb[i], cb[i], sh.M, sh.N, sh.K, nullptr); });
  B.add("nn", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_nn(cfg, splits, ab[i], bb[i], cb[i], sh.M, sh.N, sh.K, nn_lda, nn_ldb, sh.N, nullptr); });
  B.add("rocblas_tn", [=](Buffers&, size_t i) { return bgemm_rocblas_tn(ab[i], btb[i], cb[i], sh.M, sh.N, sh.K, nullptr); });
  B.head("\"output\": \"c16\", \"elem\": \"bf16\", \"config\": \"%s\", \"nn_config\": \"%s\", \"splits\": %d, \"runs\": %d, \"nn_runs\": %d", B.V.L->config_name(cfg),
         hgemm_mi355x_nn_config_name(cfg), splits, B.V.runs_at(cfg, sh), bgemm_mi355x_nn_runs(cfg, sh.M, sh.N, sh.K, nn_lda, nn_ldb, sh.N));
  B.verdict("tn_le_nn", 0, 1, true);
}

// What the three tn --bf16 --bias benches share: each set's bf16 A and b_col_major B, a C, the filled bias.
struct TnBiasBufs { TrBench::PerSet ab, btb, cb, bias; };
static TnBiasBufs tn_bias_bufs(TrBench& B) {
  const TnBiasBufs t = {B.to_bf16(B.of(&Buffers::a), B.a_elems), B.to_bf16(B.of(&Buffers::bt), B.b_elems), B.alloc(B.cn * 2), B.alloc((size_t)B.sh.N * 2)};
  for (void* p : t.bias) fill_bias_kernel<<<64, 256>>>((__bf16*)p, B.sh.N);
  return t;
}
static int elementwise_grid(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 8192); }   // blocks of 256 for a grid-stride kernel
// The one place a run-time activation becomes a template argument: f(std::integral_constant<int, ACT>()), for <<<>>> of an <ACT> kernel.
template <class F> static void with_act(int act, F&& f) {
  if (act == HGEMM_ACT_RELU) f(std::integral_constant<int, HGEMM_ACT_RELU>());
  else if (act == HGEMM_ACT_GELU) f(std::integral_constant<int, HGEMM_ACT_GELU>());
  else f(std::integral_constant<int, HGEMM_ACT_GELU_TANH>());
}
template <class F> static void with_gated_act(int act, F&& f) {   // the gated kind's: SiLU too, which the derivative kernels do not have
  if (act == HGEMM_ACT_SILU) f(std::integral_constant<int, HGEMM_ACT_SILU>());
  else with_act(act, f);
}
static void head_act(TrBench& B, const char* output) {   // the header fields of the activation kinds' records
  B.head("\"output\": \"%s\", \"act\": \"%s\", \"elem\": \"bf16\", \"config\": \"%s\", \"splits\": %d, \"runs\": %d", output, kActNames[B.act],
         B.V.L->config_name(B.cfg), B.splits, B.V.runs_at(B.cfg, B.sh));
}

// tn --bf16 --bias: the planned bgemm_mi355x_tn_bias call, bgemm_mi355x_launch_tn with the same member and splits and no bias -- the
// fused kernel adds 2 BN bytes of loads and 4 FM FN adds per lane to a tile --, and, context only, the path the call replaces:
// bgemm_mi355x_tn followed by an element-wise bf16 add (its launch is not checked: the contender answers with the product's status).
// The one condition: fused <= plain within the plain call's own round-to-round spread in this run: "bias_le_plain".
static void bench_tn_bias(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), add_grid = elementwise_grid(cn);
  const TnBiasBufs t = tn_bias_bufs(B);
  const TrBench::PerSet ab = t.ab, btb = t.btb, cb = t.cb, bias = t.bias;
  B.add("bias", [=](Buffers&, size_t i) { return bgemm_mi355x_tn_bias(ab[i], btb[i], bias[i], cb[i], sh.M, sh.N, sh.K, nullptr); });
  B.add("plain", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_tn(cfg, splits, ab[i], btb[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr); });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_tn(ab[i], btb[i], cb[i], sh.M, sh.N, sh.K, nullptr);
    add_bias_kernel<<<add_grid, 256>>>((__bf16*)cb[i], (const __bf16*)bias[i], cn, sh.N);
    return st;
  });
  B.head("\"output\": \"c16_bias\", \"elem\": \"bf16\", \"config\": \"%s\", \"splits\": %d, \"runs\": %d", B.V.L->config_name(cfg), splits, B.V.runs_at(cfg, sh));
  B.verdict("bias_le_plain", 0, 1, true);
}

// the unfused second pass of the contender: an element-wise bf16 activation over all of C, hgemm_act.hpp's text on the value already
// rounded to bf16
template <int ACT>
__global__ void act_bf16_kernel(__bf16* __restrict__ c, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    c[i] = (__bf16)hgemm_mi355x::act_apply<ACT>((float)c[i]);
}

// the unfused second pass of the gated contender: H[m][n] = bf16(act(float(GU[m][n])) x float(GU[m][N + n])) over the bf16 [M][2 N] product
// of the stacked weight, hgemm_act.hpp's text on values already rounded to bf16
template <int ACT>
__global__ void gate_bf16_kernel(const __bf16* __restrict__ gu, __bf16* __restrict__ h, size_t total, int n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / n, c = i % n;
    h[i] = (__bf16)(hgemm_mi355x::act_apply<ACT>((float)gu[m * 2 * n + c]) * (float)gu[m * 2 * n + n + c]);
  }
}
// tn --bf16 --gated A: bgemm_mi355x_launch_tn_gated at the plan of the product of width 2 N against the path it replaces at the SAME member
// and splits -- bgemm_mi355x_launch_tn on the stacked [2 N][K] weight into a bf16 [M][2 N] scratch, then the element-wise kernel above (its
// launch is not checked: the contender answers with the product's status) --, and, context only, that product alone.  Both halves of the
// stacked weight hold the set's B (timing only).  The one condition: fused <= unfused within the unfused path's own round-to-round spread
// in this run: "gated_le_unfused".  (The record's TFLOP/s count 2 M N K with N the output width: half of the product's flops.)
static void bench_tn_gated(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  int cfg = 0, splits = 1;
  bgemm_mi355x_tn_plan(sh.M, 2 * sh.N, sh.K, &cfg, &splits);
  B.cfg = cfg, B.splits = splits;
  const int lda = sh.K, ldb = sh.K, act = B.act, gate_grid = elementwise_grid(cn);
  const TrBench::PerSet ab = B.to_bf16(B.of(&Buffers::a), B.a_elems), half = B.to_bf16(B.of(&Buffers::bt), B.b_elems), w = B.alloc(2 * B.b_elems * 2),
                        gu = B.alloc(2 * cn * 2), cb = B.alloc(cn * 2), bias = B.alloc((size_t)2 * sh.N * 2);
  for (size_t i = 0; i < w.size(); ++i) {
    HIP_OK(hipMemcpy(w[i], half[i], B.b_elems * 2, hipMemcpyDeviceToDevice));
    HIP_OK(hipMemcpy((char*)w[i] + B.b_elems * 2, half[i], B.b_elems * 2, hipMemcpyDeviceToDevice));
    fill_bias_kernel<<<64, 256>>>((__bf16*)bias[i], 2 * sh.N);
  }
  B.add("gated", [=](Buffers&, size_t i) {
    return bgemm_mi355x_launch_tn_gated(cfg, splits, ab[i], w[i], (const char*)w[i] + (size_t)sh.N * sh.K * 2, bias[i], (const char*)bias[i] + (size_t)sh.N * 2, cb[i],
                                        sh.M, sh.N, sh.K, lda, ldb, sh.N, act, nullptr);
  });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_tn(cfg, splits, ab[i], w[i], gu[i], sh.M, 2 * sh.N, sh.K, lda, ldb, 2 * sh.N, nullptr);
    with_gated_act(act, [&](auto A) { gate_bf16_kernel<decltype(A)::value><<<gate_grid, 256>>>((const __bf16*)gu[i], (__bf16*)cb[i], cn, sh.N); });
    return st;
  });
  B.add("product_2n", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_tn(cfg, splits, ab[i], w[i], gu[i], sh.M, 2 * sh.N, sh.K, lda, ldb, 2 * sh.N, nullptr); });
  B.head("\"output\": \"c16_gated\", \"act\": \"%s\", \"elem\": \"bf16\", \"config\": \"%s\", \"splits\": %d, \"runs\": %d", kActNames[act],
         B.V.L->config_name(cfg), splits, B.V.runs_at(cfg, sh));
  B.verdict("gated_le_unfused", 0, 1, true);
}

// tn --bf16 --gated-aux A: bgemm_mi355x_launch_tn_gated_aux (H and a fused [M][2 N] g|u buffer) at the plan of the product of width 2 N against
// the route a training caller has without it, at the SAME member and splits -- bgemm_mi355x_launch_tn_bias on the stacked [2 N][K] weight
// with the stacked bias, which writes g|u, then the element-wise gate kernel above over it (its launch is not checked) --, and, context
// only, bgemm_mi355x_launch_tn_gated alone: the price of the two extra stores.  "gated_aux_le_unfused", within the unfused route's spread.
static void bench_tn_gated_aux(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  int cfg = 0, splits = 1;
  bgemm_mi355x_tn_plan(sh.M, 2 * sh.N, sh.K, &cfg, &splits);
  B.cfg = cfg, B.splits = splits;
  const int lda = sh.K, ldb = sh.K, act = B.act, gate_grid = elementwise_grid(cn);
  const TrBench::PerSet ab = B.to_bf16(B.of(&Buffers::a), B.a_elems), half = B.to_bf16(B.of(&Buffers::bt), B.b_elems), w = B.alloc(2 * B.b_elems * 2),
                        gu = B.alloc(2 * cn * 2), cb = B.alloc(cn * 2), bias = B.alloc((size_t)2 * sh.N * 2);
  for (size_t i = 0; i < w.size(); ++i) {
    HIP_OK(hipMemcpy(w[i], half[i], B.b_elems * 2, hipMemcpyDeviceToDevice));
    HIP_OK(hipMemcpy((char*)w[i] + B.b_elems * 2, half[i], B.b_elems * 2, hipMemcpyDeviceToDevice));
    fill_bias_kernel<<<64, 256>>>((__bf16*)bias[i], 2 * sh.N);
  }
  B.add("gated_aux", [=](Buffers&, size_t i) {
    return bgemm_mi355x_launch_tn_gated_aux(cfg, splits, ab[i], w[i], (const char*)w[i] + (size_t)sh.N * sh.K * 2, bias[i], (const char*)bias[i] + (size_t)sh.N * 2, cb[i],
                                            gu[i], (char*)gu[i] + (size_t)sh.N * 2, sh.M, sh.N, sh.K, lda, ldb, sh.N, 2 * sh.N, act, nullptr);
  });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_tn_bias(cfg, splits, ab[i], w[i], bias[i], gu[i], sh.M, 2 * sh.N, sh.K, lda, ldb, 2 * sh.N, nullptr);
    with_gated_act(act, [&](auto A) { gate_bf16_kernel<decltype(A)::value><<<gate_grid, 256>>>((const __bf16*)gu[i], (__bf16*)cb[i], cn, sh.N); });
    return st;
  });
  B.add("gated", [=](Buffers&, size_t i) {
    return bgemm_mi355x_launch_tn_gated(cfg, splits, ab[i], w[i], (const char*)w[i] + (size_t)sh.N * sh.K * 2, bias[i], (const char*)bias[i] + (size_t)sh.N * 2, cb[i],
                                        sh.M, sh.N, sh.K, lda, ldb, sh.N, act, nullptr);
  });
  B.head("\"output\": \"c16_gated_aux\", \"act\": \"%s\", \"elem\": \"bf16\", \"config\": \"%s\", \"splits\": %d, \"runs\": %d", kActNames[act],
         B.V.L->config_name(cfg), splits, B.V.runs_at(cfg, sh));
  B.verdict("gated_aux_le_unfused", 0, 1, true);
}

// tn --bf16 --bias-add: bgemm_mi355x_launch_tn_bias_add, in place on r, against the route it replaces at the SAME member and splits --
// bgemm_mi355x_launch_tn_bias into a scratch C, then an element-wise x += c over the residual stream (6 M N bytes; its launch is not
// checked) --, and, context only, bgemm_mi355x_launch_tn_bias alone: the price of the loads.  "bias_add_le_unfused", within the unfused
// route's spread.  nn --bf16 --nn-add: the same with bgemm_mi355x_launch_nn_add and bgemm_mi355x_launch_nn, "nn_add_le_unfused".
__global__ void residual_elementwise_kernel(__bf16* __restrict__ x, const __bf16* __restrict__ c, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (__bf16)hgemm_mi355x::residual_add((float)c[i], (float)x[i]);
}
static void bench_tn_bias_add(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), grid = elementwise_grid(cn);
  const TnBiasBufs t = tn_bias_bufs(B);
  const TrBench::PerSet ab = t.ab, btb = t.btb, cb = t.cb, bias = t.bias, xb = B.alloc(cn * 2);
  for (void* p : xb) HIP_OK(hipMemset(p, 0, cn * 2));
  B.add("bias_add", [=](Buffers&, size_t i) {
    return bgemm_mi355x_launch_tn_bias_add(cfg, splits, ab[i], btb[i], bias[i], xb[i], xb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, nullptr);
  });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_tn_bias(cfg, splits, ab[i], btb[i], bias[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
    residual_elementwise_kernel<<<grid, 256>>>((__bf16*)xb[i], (const __bf16*)cb[i], cn);
    return st;
  });
  B.add("bias", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_tn_bias(cfg, splits, ab[i], btb[i], bias[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr); });
  B.head("\"output\": \"c16_bias_add\", \"elem\": \"bf16\", \"config\": \"%s\", \"splits\": %d, \"runs\": %d", B.V.L->config_name(cfg), splits, B.V.runs_at(cfg, sh));
  B.verdict("bias_add_le_unfused", 0, 1, true);
}
static void bench_nn_add(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), grid = elementwise_grid(cn);
  const TrBench::PerSet ab = B.to_bf16(B.of(&Buffers::a), B.a_elems), bb = B.to_bf16(B.of(&Buffers::b), B.b_elems), cb = B.alloc(cn * 2), xb = B.alloc(cn * 2);
  for (void* p : xb) HIP_OK(hipMemset(p, 0, cn * 2));
  B.add("nn_add", [=](Buffers&, size_t i) {
    return bgemm_mi355x_launch_nn_add(cfg, splits, ab[i], bb[i], xb[i], xb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, nullptr);
  });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_nn(cfg, splits, ab[i], bb[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
    residual_elementwise_kernel<<<grid, 256>>>((__bf16*)xb[i], (const __bf16*)cb[i], cn);
    return st;
  });
  B.add("nn", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_nn(cfg, splits, ab[i], bb[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr); });
  B.head("\"output\": \"c16_add\", \"elem\": \"bf16\", \"config\": \"%s\", \"splits\": %d, \"runs\": %d", B.V.L->config_name(cfg), splits, B.V.runs_at(cfg, sh));
  B.verdict("nn_add_le_unfused", 0, 1, true);
}

// tn --bf16 --bias --act A: the planned bgemm_mi355x_tn_bias_act call against the path it replaces -- bgemm_mi355x_launch_tn_bias with the
// same member and splits followed by the element-wise activation kernel above (its launch is not checked: the contender answers with the
// product's status) --, and, context only, the plain bias call.  The one condition: fused <= unfused within the unfused path's own
// round-to-round spread in this run: "act_le_unfused".
static void bench_tn_bias_act(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), act = B.act, act_grid = elementwise_grid(cn);
  const TnBiasBufs t = tn_bias_bufs(B);
  const TrBench::PerSet ab = t.ab, btb = t.btb, cb = t.cb, bias = t.bias;
  B.add("act", [=](Buffers&, size_t i) { return bgemm_mi355x_tn_bias_act(ab[i], btb[i], bias[i], cb[i], sh.M, sh.N, sh.K, act, nullptr); });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_tn_bias(cfg, splits, ab[i], btb[i], bias[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
    with_act(act, [&](auto A) { act_bf16_kernel<decltype(A)::value><<<act_grid, 256>>>((__bf16*)cb[i], cn); });
    return st;
  });
  B.add("bias", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_tn_bias(cfg, splits, ab[i], btb[i], bias[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr); });
  head_act(B, "c16_bias_act");
  B.verdict("act_le_unfused", 0, 1, true);
}

// tn --bf16 --bias --act A --aux: the planned bgemm_mi355x_tn_bias_act_aux call against the sequence it replaces -- bgemm_mi355x_launch_tn_bias
// with the same member and splits writing Z, then an element-wise kernel that reads Z and writes Y = act(Z) (2 M N bytes read, 2 M N
// written) --, and, context only, the fused call without the second output.  "aux_le_unfused", within the unfused path's own spread.
template <int ACT>
__global__ void act_from_z_kernel(__bf16* __restrict__ y, const __bf16* __restrict__ z, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    y[i] = (__bf16)hgemm_mi355x::act_apply<ACT>((float)z[i]);
}
static void bench_tn_aux(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), act = B.act, act_grid = elementwise_grid(cn);
  const TnBiasBufs t = tn_bias_bufs(B);
  const TrBench::PerSet ab = t.ab, btb = t.btb, cb = t.cb, bias = t.bias, zb = B.alloc(cn * 2);
  B.add("aux", [=](Buffers&, size_t i) { return bgemm_mi355x_tn_bias_act_aux(ab[i], btb[i], bias[i], cb[i], zb[i], sh.M, sh.N, sh.K, act, nullptr); });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_tn_bias(cfg, splits, ab[i], btb[i], bias[i], zb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
    with_act(act, [&](auto A) { act_from_z_kernel<decltype(A)::value><<<act_grid, 256>>>((__bf16*)cb[i], (const __bf16*)zb[i], cn); });
    return st;
  });
  B.add("act", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_tn_bias_act(cfg, splits, ab[i], btb[i], bias[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, act, nullptr); });
  head_act(B, "c16_bias_act_aux");
  B.verdict("aux_le_unfused", 0, 1, true);
}

// What the two nn --bf16 --dact benches share: each set's bf16 A and B, a C, a Z filled with a fixed pattern over [-4, 4] (timing only).
__global__ void fill_z_kernel(__bf16* __restrict__ z, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    z[i] = (__bf16)((float)((int)((i * 2654435761u) % 257u) - 128) * (1.0f / 32.0f));
}
struct NnDactBufs { TrBench::PerSet ab, bb, cb, zb; };
static NnDactBufs nn_dact_bufs(TrBench& B) {
  const NnDactBufs t = {B.to_bf16(B.of(&Buffers::a), B.a_elems), B.to_bf16(B.of(&Buffers::b), B.b_elems), B.alloc(B.cn * 2), B.alloc(B.cn * 2)};
  for (void* p : t.zb) fill_z_kernel<<<elementwise_grid(B.cn), 256>>>((__bf16*)p, B.cn);
  return t;
}

// nn --bf16 --dact A: the planned bgemm_mi355x_nn_dact call against the sequence it replaces -- bgemm_mi355x_launch_nn with the same member
// and splits writing a bf16 dH, then an element-wise kernel that reads dH and Z and writes dZ = dH (.) act'(Z) (6 M N bytes) --, and,
// context only, the plain NN call.  "dact_le_unfused", within the unfused path's own spread.
template <int ACT>
__global__ void dact_elementwise_kernel(__bf16* __restrict__ dz, const __bf16* __restrict__ dh, const __bf16* __restrict__ z, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    dz[i] = (__bf16)hgemm_mi355x::dact_mul<ACT>((float)dh[i], (float)z[i]);
}
static void bench_nn_dact(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), act = B.act, grid = elementwise_grid(cn);
  const NnDactBufs t = nn_dact_bufs(B);
  const TrBench::PerSet ab = t.ab, bb = t.bb, cb = t.cb, zb = t.zb, hb = B.alloc(cn * 2);
  B.add("dact", [=](Buffers&, size_t i) { return bgemm_mi355x_nn_dact(ab[i], bb[i], zb[i], cb[i], sh.M, sh.N, sh.K, act, nullptr); });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_nn(cfg, splits, ab[i], bb[i], hb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
    with_act(act, [&](auto A) { dact_elementwise_kernel<decltype(A)::value><<<grid, 256>>>((__bf16*)cb[i], (const __bf16*)hb[i], (const __bf16*)zb[i], cn); });
    return st;
  });
  B.add("nn", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_nn(cfg, splits, ab[i], bb[i], hb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr); });
  head_act(B, "c16_dact");
  B.verdict("dact_le_unfused", 0, 1, true);
}

// nn --bf16 --dgated A: bgemm_mi355x_launch_nn_dgated at the plan against the sequence it replaces at the SAME member and splits --
// bgemm_mi355x_launch_nn writing a bf16 dH, then an element-wise kernel that reads dH, g and u and writes dg and du (10 M N bytes; its launch
// is not checked: the contender answers with the product's status) --, and, context only, the plain NN call.  "dgated_le_unfused", within
// the unfused path's own spread.
template <int ACT>
__global__ void dgated_elementwise_kernel(__bf16* __restrict__ dg, __bf16* __restrict__ du, const __bf16* __restrict__ dh, const __bf16* __restrict__ g,
                                          const __bf16* __restrict__ u, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const hgemm_mi355x::DgatedPair y = hgemm_mi355x::dgated_store<ACT>((float)dh[i], (float)g[i], (float)u[i]);
    dg[i] = (__bf16)y.dg, du[i] = (__bf16)y.du;
  }
}
static void bench_nn_dgated(TrBench& B) {
  const Shape sh = B.sh;
  const size_t cn = B.cn;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), act = B.act, grid = elementwise_grid(cn);
  const NnDactBufs t = nn_dact_bufs(B);
  const TrBench::PerSet ab = t.ab, bb = t.bb, dg = t.cb, gb = t.zb, ub = B.alloc(cn * 2), du = B.alloc(cn * 2), hb = B.alloc(cn * 2);
  for (void* p : ub) fill_z_kernel<<<grid, 256>>>((__bf16*)p, cn);
  B.add("dgated", [=](Buffers&, size_t i) {
    return bgemm_mi355x_launch_nn_dgated(cfg, splits, ab[i], bb[i], gb[i], ub[i], dg[i], du[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, act, nullptr);
  });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_nn(cfg, splits, ab[i], bb[i], hb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr);
    with_gated_act(act, [&](auto A) {
      dgated_elementwise_kernel<decltype(A)::value><<<grid, 256>>>((__bf16*)dg[i], (__bf16*)du[i], (const __bf16*)hb[i], (const __bf16*)gb[i], (const __bf16*)ub[i], cn);
    });
    return st;
  });
  B.add("nn", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_nn(cfg, splits, ab[i], bb[i], hb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, nullptr); });
  head_act(B, "c16_dgated");
  B.verdict("dgated_le_unfused", 0, 1, true);
}

// nn --bf16 --dact A --dbias: bgemm_mi355x_launch_nn_dact_dbias at the plan against the sequence it replaces -- bgemm_mi355x_launch_nn_dact with
// the same member and splits, then bgemm_mi355x_colsum_c32 over the dZ just written (one more launch, 2 M N more bytes read) --, and,
// context only, the dact call alone.  "dbias_le_unfused", within the unfused path's own spread.
static void bench_nn_dact_dbias(TrBench& B) {
  const Shape sh = B.sh;
  const int cfg = B.cfg, splits = B.splits, lda = B.V.L->lda(sh), ldb = B.V.L->ldb(sh), act = B.act;
  const NnDactBufs t = nn_dact_bufs(B);
  const TrBench::PerSet ab = t.ab, bb = t.bb, cb = t.cb, zb = t.zb, db = B.alloc((size_t)sh.N * 4, true);
  B.add("dbias", [=](Buffers&, size_t i) {
    return bgemm_mi355x_launch_nn_dact_dbias(cfg, splits, ab[i], bb[i], zb[i], cb[i], (float*)db[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, act, 0, nullptr);
  });
  B.add("unfused", [=](Buffers&, size_t i) {
    const int st = bgemm_mi355x_launch_nn_dact(cfg, splits, ab[i], bb[i], zb[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, act, nullptr);
    return st != HGEMM_OK ? st : bgemm_mi355x_colsum_c32(cb[i], (float*)db[i], sh.M, sh.N, sh.N, 0, nullptr);
  });
  B.add("dact", [=](Buffers&, size_t i) { return bgemm_mi355x_launch_nn_dact(cfg, splits, ab[i], bb[i], zb[i], cb[i], sh.M, sh.N, sh.K, lda, ldb, sh.N, sh.N, act, nullptr); });
  head_act(B, "c16_dact_dbias");
  B.verdict("dbias_le_unfused", 0, 1, true);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: hgemm_tune check|tune|bench [options]\n");
    return 2;
  }
  std::string mode = argv[1];
  TrFlags tr;   // --layout, --bf16, --c32, --bias, --act, --aux, --dact, --dbias
  std::vector<Shape> shapes;
  const char* out_path = nullptr;
  const char* cfg_name = nullptr;
  double keep = 2.5;
  int max_cand = 12, splits = 1, group = 0, reps = 20;
  bool baselines = false, use_lib = false, sweep_group = false, autotune = false, isolated = false;
  for (int i = 2; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
    if (a == "--shapes" || a == "--shape") { auto v = parse_shapes(next()); shapes.insert(shapes.end(), v.begin(), v.end()); }
    else if (a == "--shape-file") { auto v = read_shape_file(next()); shapes.insert(shapes.end(), v.begin(), v.end()); }
    else if (a == "--out") out_path = next();
    else if (a == "--autotune") autotune = true;
    else if (a == "--layout") {
      tr.layout = next();
      if (tr.layout != "nn" && tr.layout != "tn" && tr.layout != "ta") { fprintf(stderr, "--layout takes nn, ta or tn\n"); return 2; }
    }
    else if (a == "--c32") tr.c32 = true;
    else if (a == "--bf16") tr.bf16 = true;
    else if (a == "--bias") tr.bias = true;
    else if (a == "--aux") tr.aux = true;
    else if (a == "--dbias") tr.dbias = true;
    else if (a == "--act" || a == "--dact") {
      int& which = a == "--act" ? tr.act : tr.dact;
      const std::string nm = next();
      for (int k = 1; k <= 3; ++k) if (nm == kActNames[k]) which = k;
      if (!which) { fprintf(stderr, "%s takes relu, gelu or gelu_tanh\n", a.c_str()); return 2; }
    }
    else if (a == "--gated") {
      const std::string nm = next();
      for (int k = 1; k <= 4; ++k) if (nm == kActNames[k]) tr.gated = k;
      if (!tr.gated) { fprintf(stderr, "--gated takes relu, gelu, gelu_tanh or silu\n"); return 2; }
    }
    else if (a == "--gated-aux") {
      const std::string nm = next();
      for (int k = 1; k <= 4; ++k) if (nm == kActNames[k]) tr.gated_aux = k;
      if (!tr.gated_aux) { fprintf(stderr, "--gated-aux takes relu, gelu, gelu_tanh or silu\n"); return 2; }
    }
    else if (a == "--bias-add") tr.bias_add = tr.bias = true;
    else if (a == "--nn-add") tr.nn_add = true;
    else if (a == "--dgated") {
      const std::string nm = next();
      for (int k = 1; k <= 4; ++k) if (nm == kActNames[k]) tr.dgated = k;
      if (!tr.dgated) { fprintf(stderr, "--dgated takes relu, gelu, gelu_tanh or silu\n"); return 2; }
    }
    else if (a == "--fused") g_fused_too = true;
    else if (a == "--with-shipped") g_with_shipped = true;
    else if (a == "--streamk") g_streamk_too = true;
    else if (a == "--nt") g_try_nt = true;
    else if (a == "--rank") g_rank_both = std::string(next()) == "both";
    else if (a == "--stream") g_stream_report = true;
    else if (a == "--interleave") g_interleave = true;
    else if (a == "--reverse") g_reverse = true;
    else if (a == "--also") {
      std::stringstream ss(next()); std::string t;
      while (std::getline(ss, t, ',')) {
        const size_t x = t.find(':'), y = t.rfind(':');
        if (x == std::string::npos) g_also.push_back({t, 1, 0});
        else g_also.push_back({t.substr(0, x), atoi(t.substr(x + 1).c_str()), y != x ? atoi(t.substr(y + 1).c_str()) : 0});
      }
    }
    else if (a == "--cand-file") { if (!load_cand_file(next())) { fprintf(stderr, "cannot read --cand-file\n"); return 2; } }
    else if (a == "--configs") { std::stringstream ss(next()); std::string t; while (std::getline(ss, t, ',')) if (!t.empty()) g_config_filter.push_back(t); }
    else if (a == "--plan-only") g_plan_only = true;
    else if (a == "--cooldown-ms") g_cooldown_ms = atoi(next());
    else if (a == "--stream-seconds") g_stream_box_s = atof(next());
    else if (a == "--keep") keep = atof(next());
    else if (a == "--max-cand") max_cand = atoi(next());
    else if (a == "--baselines") baselines = true;
    else if (a == "--sweep-group") sweep_group = true;
    else if (a == "--config") cfg_name = next();
    else if (a == "--splits") splits = atoi(next());
    else if (a == "--group") group = atoi(next());
    else if (a == "--reps") reps = atoi(next());
    else if (a == "--lib") use_lib = true;
    else if (a == "--power") g_power = true;
    else if (a == "--timeline") g_timeline = true;
    else if (a == "--isolated") isolated = true;
    else if (a == "--seconds") g_seconds = atof(next());
    else if (a == "--baseline") { g_baseline = next(); g_power = true; }
    else if (a == "--ld") g_ld_override = atoi(next());
    else if (a == "--pad-alloc") g_pad_alloc_mib = (size_t)atol(next());
    else if (a == "--debug") {
      if (!hgemm_mi355x_set_debug) { fprintf(stderr, "--debug needs the ablation build of the library (lib_ablation/)\n"); return 2; }
      hgemm_mi355x_set_debug(atoi(next()));
    }
    else if (a == "--fill") g_zero_fill = (std::string(next()) == "zero");
    // q256x256_w2x2's one-tile-per-workgroup kernel (hgemm_mi355x_set_one_item_kernel): 0 = every launch runs the general kernel,
    // 1 = the launches it takes run it (the library's default; a -DHGEMM_TIMELINE library needs the 1)
    else if (a == "--one-item") hgemm_mi355x_set_one_item_kernel(atoi(next()));
    else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
  }
  // Which of the transposed-read variants, if any, the flags name -- and every refusal that follows from the flags alone, before a
  // device is asked for.  nullptr: the fp16 b_col_major commands below (no --layout, or --layout tn without --bf16).
  if (tr.bias && !(tr.bf16 && tr.layout == "tn")) { fprintf(stderr, "--bias goes with --layout tn --bf16 (bgemm_mi355x_tn_bias)\n"); return 2; }
  if (tr.act && !tr.bias) { fprintf(stderr, "--act goes with --layout tn --bf16 --bias (bgemm_mi355x_tn_bias_act)\n"); return 2; }
  if (tr.c32 && tr.layout != "ta") { fprintf(stderr, "--c32 goes with --layout ta\n"); return 2; }
  if (tr.bf16 && tr.layout.empty()) { fprintf(stderr, "--bf16 goes with --layout nn, ta or tn (the fp16 b_col_major families have no bf16 form)\n"); return 2; }
  if (tr.aux && !tr.act) { fprintf(stderr, "--aux goes with --layout tn --bf16 --bias --act A (bgemm_mi355x_tn_bias_act_aux)\n"); return 2; }
  if (tr.dact && !(tr.bf16 && tr.layout == "nn" && !tr.act)) { fprintf(stderr, "--dact goes with --layout nn --bf16 (bgemm_mi355x_nn_dact)\n"); return 2; }
  if (tr.dbias && !tr.dact) { fprintf(stderr, "--dbias goes with --layout nn --bf16 --dact A (bgemm_mi355x_nn_dact_dbias)\n"); return 2; }
  if (tr.dgated && !(tr.bf16 && tr.layout == "nn" && !tr.act && !tr.dact)) { fprintf(stderr, "--dgated goes with --layout nn --bf16 (bgemm_mi355x_nn_dgated)\n"); return 2; }
  if (tr.gated_aux && !(tr.bf16 && tr.layout == "tn" && !tr.act && !tr.dact && !tr.gated && !tr.dgated)) {
    fprintf(stderr, "--gated-aux goes with --layout tn --bf16 (bgemm_mi355x_tn_gated_aux)\n");
    return 2;
  }
  if (tr.bias_add && !(tr.bf16 && tr.layout == "tn" && !tr.activation() && !tr.aux)) { fprintf(stderr, "--bias-add goes with --layout tn --bf16 (bgemm_mi355x_tn_bias_add)\n"); return 2; }
  if (tr.nn_add && !(tr.bf16 && tr.layout == "nn" && !tr.activation() && !tr.bias)) { fprintf(stderr, "--nn-add goes with --layout nn --bf16 (bgemm_mi355x_nn_add)\n"); return 2; }
  const Variant* variant = resolve_variant(tr);
  if (variant && mode != "check" && mode != "bench") {
    fprintf(stderr, "--layout %s%s goes with check or bench\n", tr.layout.c_str(), variant->L->b_col_major ? " --bf16" : "");
    return 2;
  }
  if (variant && mode == "bench" && shapes.empty()) { fprintf(stderr, "bench needs --shape\n"); return 2; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fprintf(stderr, "hgemm_tune: no HIP device visible\n");
    return 3;
  }
  if (g_pad_alloc_mib) {
    void* pad = nullptr;
    HIP_OK(hipMalloc(&pad, g_pad_alloc_mib << 20));   // (kept until exit)
    HIP_OK(hipMemset(pad, 1, g_pad_alloc_mib << 20));
  }
  if (variant) return mode == "check" ? tr_check(*variant, tr.activation(), shapes) : tr_bench(*variant, tr.activation(), shapes, out_path, autotune);
  if (mode == "check") {
    if (shapes.empty())
      // (the last two: K tails -- 2104 = 32 x 64 + 56 = 8 x 256 + 56, 728 = 11 x 64 + 24 = 5 x 128 + 88 = 2 x 256 + 216: odd and even
      // stage counts, one to seven K = 32 slices of tail, the last one partial.  The item seams of a persistent walk need more
      // items than resident workgroups -- `check --shapes 4352_4352_192,4352_4352_232 --configs <families s, q>`: 289 tiles of
      // 256 x 256, three K-steps per item, with and without a K tail -- and are left out of this list for their size: the every-run
      // net is tests/test_gpu_ladders.py (1 ... 5 K-steps per item, items made by tiles and by splits, bit-exact per member).
      // 1_264_128 / 264_4_128: sliver tiles, one row (whole wave rows out of range) / one 4-column sliver (narrow epilogue))
      shapes = parse_shapes("64_64_64,64_4096_64,128_192_256,200_136_128,256_256_1024,320_448_512,512_1024_2048,1000_520_192,"
                            "1000_520_200,65_30_100,33_17_40,300_260_2048,300_260_2104,520_392_728,"
                            "96_80_4096,"    // (round 6: K / 64 = 64, so that the 37- and 48-way single-launch splits run)
                            "328_456_384,136_200_896,"    // (family u, 128 of K per stage: three and seven stages, ragged M and N)
                            "1_264_128,264_4_128");
    return cmd_check(shapes);
  }
  if (mode == "tune") {
    if (shapes.empty()) { fprintf(stderr, "tune needs --shapes / --shape-file\n"); return 2; }
    return cmd_tune(shapes, out_path, keep, max_cand, baselines, sweep_group, autotune);
  }
  if (mode == "bench") {
    if (shapes.empty()) { fprintf(stderr, "bench needs --shape\n"); return 2; }
    if (isolated) g_power = false;
    int rc = 0;
    for (const Shape& sh : shapes) rc |= cmd_bench(sh, cfg_name, splits, group, reps, use_lib);
    return rc;
  }
  fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
