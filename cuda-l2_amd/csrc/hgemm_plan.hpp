// Planning arithmetic of the host path (hgemm_plan.hip): the tuned index, the two cost models, the two planners, and -- inline, the
// per-call launch resolution of hgemm_api.hip is part of what a harness times -- how a geometry accepts and cuts K.  Internal to the
// library; nothing here calls the HIP runtime.
#pragma once
#include "hgemm_launch.hpp"

#include <algorithm>
#include <cstdint>
#include <mutex>

namespace hgemm_mi355x {
#pragma GCC visibility push(hidden)

// split-K workspace layout (hgemm_api.hip): [kCounterBytes of tile arrival counters][fp32 slabs]
constexpr size_t kCounterBytes = (size_t)256 << 10;             // 65536 tiles
constexpr size_t kMaxFusedTiles = kCounterBytes / sizeof(unsigned);

// ---- tuned plans --------------------------------------------------------------------------------
struct TunedPlan { uint64_t key; int M, N, K; int cfg, splits, group_m; };   // key orders the index; M, N, K decide a hit
extern std::once_flag g_tuned_once;
void build_tuned_index();
const TunedPlan* find_tuned(int M, int N, int K);

// Sort / hash key only: the three fields overlap once a dimension reaches 2^21, so two shapes may share a key --
// every probe compares M, N, K themselves (round 2 compared the key alone: plan(64, 68, 8388864) returned
// the tuned row of (64, 64, 256)).
inline uint64_t shape_key(int M, int N, int K) {
  return ((uint64_t)(uint32_t)M << 42) ^ ((uint64_t)(uint32_t)N << 21) ^ (uint64_t)(uint32_t)K;
}

// ---- analytic plan model --------------------------------------------------------------------------
// MI355X constants (MI355X_MICROARCH.md): 256 CUs, 4 SIMDs/CU, 160 KiB LDS/CU, 512 regs/lane/SIMD.
constexpr int    kCUs          = 256;
constexpr double kLaunchUs     = 2.0;    // host launch + dispatch of one kernel
constexpr double kBoundaryUs   = 3.7;    // dependent kernel boundary + launch of the split-K combine (fitted)
constexpr double kHbmBytesUs   = 4.6e6;  // ~4.6 TB/s sustained for mixed read/write (fitted)
constexpr double kCuFlopUs     = 4069.0 * 2000.0;  // fp16 MFMA flop per CU per us at ~2.0 GHz

// persistent workgroups of a stream-K plan: the plan's low 16 bits, or (0 / 1) one resident wave of them
inline int streamk_grid(const KernelEntry& e, int g_plan) {
  return g_plan > 1 ? std::min(g_plan, 4096) : kCUs * std::max(1, e.sk_wgs_per_cu);
}
// stages closer than this to a tile boundary are not worth a cut (the prologue of a segment is 2-3 stages deep)
inline int streamk_min_steps(const KernelEntry& e) { return e.kgran >= 256 ? 2 : e.kgran >= 128 ? 3 : 4; }

int default_group_m(const KernelEntry& e, int tiles_m, int tiles_n);
double model_us(const KernelEntry& e, int M, int N, int K, int splits);
double model_us_streamk(const KernelEntry& e, int M, int N, int K, int G);

// K the geometry accepts: a multiple of its stage depth, or any multiple of 8 for the families that zero-fill a
// partial last K-step themselves
// ... (classic family: the last LDS-DMA step is padded, so its step count rounds up), or accumulate the remainder from
// fragments loaded straight from global memory behind at least one whole stage (families q and r, "direct" tail: the step
// count rounds down and the remainder rides on the last split)
inline bool direct_tail(const KernelEntry& e) { return e.ktail == KTail::DIRECT; }
inline bool k_ok(const KernelEntry& e, int K) { return K % e.kgran == 0 || (e.ktail != KTail::NONE && K % 8 == 0 && (!direct_tail(e) || K >= e.kgran)); }

// How a geometry cuts K for a split count the caller asked for: `steps` pipeline stages (rounded up for the classic family, whose
// last step may be partial; rounded DOWN for a direct tail, which rides on the last split), at most one split per stage, no empty
// split, chunks of whole stages.  Split s covers [s * k_chunk, min(K, (s + 1) * k_chunk)), the last one of a direct tail up to K.
struct KSplit { int steps, splits, k_chunk; bool tail_direct; };
inline KSplit split_k(const KernelEntry& e, int K, int splits) {
  KSplit r;
  r.tail_direct = direct_tail(e) && K % e.kgran != 0;
  r.steps = r.tail_direct ? K / e.kgran : (K + e.kgran - 1) / e.kgran;
  r.splits = std::max(1, std::min(splits, r.steps));
  const int per = (r.steps + r.splits - 1) / r.splits;
  r.splits = (r.steps + per - 1) / per;
  r.k_chunk = per * e.kgran;
  return r;
}

// Whether a HGEMM_PLAN_STREAMK plan of geometry e REALLY runs as stream-K on (M, N, K), workspace aside -- one predicate for the
// launch, the off-grid planner, hgemm_mi355x_streamk_runs (tuner, candidate generators): the family has the kernel, the tile count fits the
// counter block, the stage sequence fits 30 bits, and K has no direct tail (families q / r: no stream-K kernel with one).
inline bool streamk_really_runs(const KernelEntry& e, int M, int N, int K) {
  if (e.sk_wgs_per_cu <= 0 || !k_ok(e, K)) return false;
  const KSplit ks = split_k(e, K, 1);
  const long tiles = (long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn);
  return !ks.tail_direct && tiles <= (long)kMaxFusedTiles && tiles * ks.steps < (1L << 30);
}

void model_plan(int M, int N, int K, int* cfg, int* splits, int* group_m);
// (round 6) every admissible corner plan with its modelled time, for the first-use selection off the grid: the runners-up of the
// ranking of neighbour_plan are the plans whose order the model is least sure about -- what the box should decide (13272 x 512 x 4440: the
// model ranks q128x256 first, q256x256 at two splits measures 11 % faster)
struct RankedPlan { double us; int cfg, splits, group_m; };
bool neighbour_plan(int M, int N, int K, int* cfg, int* splits, int* group_m, RankedPlan* ranked = nullptr, int* n_ranked = nullptr);

#pragma GCC visibility pop
}  // namespace hgemm_mi355x
