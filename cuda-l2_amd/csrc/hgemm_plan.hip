// Planning arithmetic of the host path: tuned table -> neighbouring tuned plans -> analytic model (no HIP runtime call).
#include "hgemm_plan.hpp"
#include "../../include/hgemm_mi355x.h"

#include <cmath>

namespace hgemm_mi355x {

// ---- tuned plans --------------------------------------------------------------------------------
namespace {
struct TunedRow { int M, N, K; const char* cfg; int splits, group_m; };
const TunedRow g_tuned_rows[] = {
#include "hgemm_tuned_table.inc"
    {0, 0, 0, nullptr, 0, 0}};

TunedPlan* g_tuned = nullptr;
int g_num_tuned = 0;
}  // namespace
std::once_flag g_tuned_once;

void build_tuned_index() {
  const int rows = (int)(sizeof(g_tuned_rows) / sizeof(g_tuned_rows[0])) - 1;
  g_tuned = new TunedPlan[rows > 0 ? rows : 1];
  for (int i = 0; i < rows; ++i) {
    const int id = hgemm_mi355x_config_by_name(g_tuned_rows[i].cfg);
    if (id < 0) continue;  // stale row (geometry removed): fall back to the model
    g_tuned[g_num_tuned++] = {shape_key(g_tuned_rows[i].M, g_tuned_rows[i].N, g_tuned_rows[i].K), g_tuned_rows[i].M,
                              g_tuned_rows[i].N, g_tuned_rows[i].K, id, g_tuned_rows[i].splits, g_tuned_rows[i].group_m};
  }
  std::sort(g_tuned, g_tuned + g_num_tuned,
            [](const TunedPlan& a, const TunedPlan& b) { return a.key < b.key; });
}

// ---- analytic plan model --------------------------------------------------------------------------
// Raster group height.  What matters for L2 reuse is the set of tiles an XCD runs CONCURRENTLY
// (32 CUs x workgroups per CU), not all the tiles it will ever get: consecutive logical ids fill a
// column of `g` tiles, so `c` concurrent tiles touch g A-panels and c/g B-panels; panel bytes are
// g*BM + (c/g)*BN rows, minimal at g = sqrt(c*BN/BM).  (Measured at 8192^3: g=4 1289 TF, g=16 1211.)
int default_group_m(const KernelEntry& e, int tiles_m, int tiles_n) {
  const int nw = e.wm * e.wn;
  const int wg_per_cu = std::max(1, std::min(160 * 1024 / e.lds_bytes, std::max(1, 8 / nw)));
  const long per_xcd_total = std::max<long>(1, ((long)tiles_m * tiles_n + NUM_XCD - 1) / NUM_XCD);
  const double conc = (double)std::min<long>(per_xcd_total, 32L * wg_per_cu);
  const double ideal = std::sqrt(conc * e.bn / e.bm);
  int g = 1;
  while (g * 2 <= ideal * 1.42 && g * 2 <= tiles_m) g *= 2;   // nearest power of two
  return std::max(1, std::min(g, tiles_m));
}

double model_us(const KernelEntry& e, int M, int N, int K, int splits) {
  const int tiles_m = (M + e.bm - 1) / e.bm, tiles_n = (N + e.bn - 1) / e.bn;
  const long wgs = (long)tiles_m * tiles_n * splits;
  const int nw = e.wm * e.wn;
  const int tm = e.bm / e.wm, tn = e.bn / e.wn;
  const int vgprs = tm * tn / 64 + 48 + (tm + tn) / e.mi * 4;
  const int waves_simd = std::max(1, std::min(8, 512 / std::max(vgprs, 64)));
  int conc = std::min(160 * 1024 / e.lds_bytes, std::max(1, waves_simd * 4 / nw));
  conc = (int)std::max<long>(1, std::min<long>(conc, (wgs + kCUs - 1) / kCUs));
  const long rounds = (wgs + (long)kCUs * conc - 1) / ((long)kCUs * conc);
  const int ksteps = (K / splits + BK - 1) / BK;
  // Constants fitted to the measured candidates of the 1000-shape tune (tuning/r01_grid_tune_*.jsonl):
  // geomean regret of the model's pick against the measured best 2.0 % (3.9 % before the fit).
  // MFMA efficiency falls with the wave tile's operand reuse (LDS bytes per flop); the software-
  // pipelined family ('s', one wave per SIMD) sustains ~1.5x the classic schedule's rate.
  // Round 2 (families q, r added; tuning/r02_grid_tune_run{A,B}, r02_skinny_tune_run1): the 128x128 members of
  // family q sustain the classic rate per flop (their gain is the pipelining, modelled by step_lat), and q beats
  // s by a few percent once a work item has >= 16 K-steps, s wins below (one coordinate computation per item).
  // Regret of the model's pick among the measured candidates, ties broken in table order: 5.5 % (6.8 % before).
  if (e.family == Family::W) {
    // family "w" (wave-direct, no LDS staging): a trip of four K = 32 slices is one round trip to memory (~0.9 us cold, less once
    // the rows stream), the "_k4" members walk K with four waves; MFMA and load issue are never what bounds these shapes
    const bool k4 = w_splits_k(e);
    const double trips = std::ceil((double)(K / splits) / 32.0 / (k4 ? 16.0 : 4.0));
    const double main_w = rounds * (0.9 + 0.45 * std::max(0.0, trips - 1.0) + (k4 ? 0.25 : 0.0));
    double bytes_w = 2.0 * ((double)M * K + (double)N * K + (double)M * N), extra_w = 0.0;
    if (splits > 1) {
      bytes_w += 8.0 * (double)M * N * splits;
      extra_w = kBoundaryUs + 4.0 * (double)M * N * (splits + 0.5) / kHbmBytesUs + 0.17 * splits;
    }
    // every wave fetches its own fragments: L2 -> CU traffic is (BM + BN) rows per wave tile, not per workgroup tile
    const double l2_bytes = 2.0 * (double)K * ((double)tiles_m * tiles_n) * (e.wm * e.wn) * (e.bm / e.wm + e.bn / e.wn);
    return kLaunchUs - 0.7 + std::max(main_w, std::max(bytes_w / kHbmBytesUs, l2_bytes / 2.0e7)) + extra_w;
  }
  const bool is_q = e.family == Family::Q, is_q128 = is_q && e.bm == 128 && e.bn == 128;
  const Family family = is_q ? Family::S : e.family;   // 'q' = 's' with the early-A split
  const double reuse = (double)tm * tn / (tm + tn);
  // Round 3 (tuning/r03_late_tune_mi355x.jsonl, 706 candidates): the 8-wave 128x64 / 64x128 members of the classic family run at
  // 0.78 of this model's time where their 4-wave counterparts run at 1.07 -- two waves per SIMD hide the LDS-DMA issue stalls
  // the per-step latency term charges; the 192-wide q members sit on the family's common ratio (1.41 vs 1.39-1.42).
  const bool w8_mid = family == Family::T && nw == 8 && e.bm * e.bn <= 128 * 64 && wgs <= 2L * kCUs;   // (the fitted domain: <= 512 workgroups)
  // a 192-wide q tile costs 0.87 of a 256 x 256 one for 0.75 of its flops (12288 x 1024 x 16384: 396 -> 342 us with as many
  // rounds; 1024 x 12288 x 12288: 256 -> 225): fewer flops per LDS-DMA piece and per fragment read, one of them without the staged
  // epilogue -- without this term the off-grid ranking takes them whenever they save a fraction of a round
  const bool q192 = is_q && (e.bm == 192 || e.bn == 192);
  const double eff = 0.62 * std::min(1.0, reuse / 51.0) * (is_q128 ? 1.0 : family == Family::S ? (q192 ? 1.47 / 1.16 : 1.47) : w8_mid ? 1.4 : 1.0);
  const double step_tp = conc * (2.0 * e.bm * e.bn * BK) / (kCuFlopUs * eff);
  // per-K-step latency floor: barrier + LDS-DMA round trip (double-buffered rings expose all of it)
  const double step_lat = family == Family::S ? 0.40 : (e.nbuf >= 3 ? 0.33 : 0.74);
  double main_us = rounds * (1.0 + ksteps * std::max(step_tp, step_lat));
  // Rows that are not a multiple of 128 bytes apart (K % 64 != 0: only shapes off the grid): every 128-byte row segment of an
  // LDS-DMA piece straddles two cache lines, and the kernels that are bound by piece issue rather than by MFMA time pay for it in
  // proportion to their pieces per MFMA cycle, x = 4 (BM + BN) / (BM BN).  Round 4, first measurements of families q with a K tail
  // (tuning/r04_ktail_candidates_mi355x.jsonl, K = 4440 / 7152 / 520): 128 x 256 tiles 1.40 us per K-step against 0.85 on the
  // grid (+65 %, x = 0.047), 256 x 192 +24 % (x = 0.037), 256 x 256 +7 % (x = 0.031); capped where latency, not issue, bounds the
  // small tiles.  Family r streams 256-512 contiguous bytes per row and is not charged.
  if ((2 * K) % 128 != 0 && e.family != Family::R) {
    const double x = 4.0 * (e.bm + e.bn) / ((double)e.bm * e.bn);
    main_us *= 1.0 + std::min(0.5, std::max(0.0, 25.0 * x - 0.675));
  }
  double bytes = 2.0 * ((double)M * K + (double)N * K + (double)M * N);
  double extra = 0.0;
  if (splits > 1) {
    bytes += 8.0 * (double)M * N * splits;
    extra = kBoundaryUs + 4.0 * (double)M * N * (splits + 0.5) / kHbmBytesUs + 0.17 * splits;
  }
  const double q_bias = (is_q && !is_q128) ? (K / splits >= 1024 ? 0.99 : 1.01) : 1.0;
  return (kLaunchUs + std::max(main_us, bytes / kHbmBytesUs) + extra) * q_bias;
}

// Stream-K plan (EPI_STREAMK) of G persistent workgroups: every workgroup walks ~tiles * stages / G pipeline stages at the
// family's step cost, a cut tile costs one slab round trip (write-through store, arrival, the completer reads the parts).
// Constants are the data-parallel model's; the tuner measures, this only prunes candidates and ranks off-grid corners.
double model_us_streamk(const KernelEntry& e, int M, int N, int K, int G) {
  const long tiles = (long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn);
  const int stages = (K + e.kgran - 1) / e.kgran;
  const long total = tiles * stages;
  G = (int)std::max<long>(1, std::min<long>(G, total));
  const int conc = (int)std::max<long>(1, std::min<long>(e.sk_wgs_per_cu, (G + kCUs - 1) / kCUs));
  const int tm = e.bm / e.wm, tn = e.bn / e.wn;
  const double reuse = (double)tm * tn / (tm + tn);
  const double eff = 0.62 * std::min(1.0, reuse / 51.0) * (e.wm * e.wn == 8 && e.bm * e.bn <= 128 * 64 ? 1.4 : 1.0);
  const double step_tp = conc * (2.0 * e.bm * e.bn * e.kgran) / (kCuFlopUs * eff);
  const double step_lat = (e.family == Family::R ? 0.45 : (e.nbuf >= 3 ? 0.33 : 0.74)) * e.kgran / 64.0 * (e.family == Family::R ? 0.5 : 1.0);
  const double per_wg = (double)((total + G - 1) / G);
  const long rounds = (G + (long)kCUs * conc - 1) / ((long)kCUs * conc);
  const double main_us = rounds * (1.0 + per_wg * std::max(step_tp, step_lat));
  const long cuts = total % G == 0 && (total / G) % stages == 0 ? 0 : std::min<long>(G, tiles * 2);   // partial segments
  const double fix_bytes = 2.0 * cuts * e.bm * e.bn * 4.0;
  const double bytes = 2.0 * ((double)M * K + (double)N * K + (double)M * N) + fix_bytes;
  return kLaunchUs + std::max(main_us, bytes / kHbmBytesUs) + (cuts ? 1.5 : 0.0);
}

void model_plan(int M, int N, int K, int* cfg, int* splits, int* group_m) {
  double best = 1e30;
  int bc = 0, bs = 1;
  const int ksteps = K / BK;
  for (int c = 0; c < g_num_kernels; ++c) {
    const KernelEntry& e = g_kernel_table[c];
    // Do not pick tiles that mostly compute padding.
    if (e.bm > M * 2 && e.bm > 32) continue;
    if (e.bn > N * 2 && e.bn > 32) continue;
    if (!k_ok(e, K)) continue;
    if (e.explicit_only) continue;   // experimental 32x32x16 members of s and q, family u (split inside the workgroup): explicit plans only
    // family "w" inside its domain only: a K of one or two pipeline steps, or a tiny output with a long K
    if (e.family == Family::W && !(K <= 128 || (long)M * N <= 128L * 128L)) continue;
    for (int s = 1; s <= 64; s *= 2) {
      if (s > 1 && ksteps / s < 4) break;
      const double t = model_us(e, M, N, K, s);
      if (t < best) { best = t; bc = c; bs = s; }
    }
  }
  *cfg = bc; *splits = bs;
  const KernelEntry& e = g_kernel_table[bc];
  *group_m = default_group_m(e, (M + e.bm - 1) / e.bm, (N + e.bn - 1) / e.bn);
}

// Off-grid shapes, first choice: the tuned plans of the surrounding grid shapes (the 2 x 2 x 2 lattice corners around
// (M, N, K)), ranked for THIS shape by the analytic model -- the reference's advice for unlisted sizes is "use the
// nearest larger configuration" (README.md:83-86).  Leave-one-out on the round-2 tuning runs (tools/eval_planner_loo.py:
// every grid shape planned from its four nearest neighbours' winners, judged by its own measured candidates;
// tuning/r02_planner_loo.json): geomean regret 3.3 %, 90th percentile 10.7 %, against 3.9 % / 14.7 % for the model
// choosing among all geometries.
const int kLattice[] = {64, 128, 256, 512, 1024, 2048, 4096, 8192, 12288, 16384};
constexpr int kLatticeN = (int)(sizeof(kLattice) / sizeof(kLattice[0]));

const TunedPlan* find_tuned(int M, int N, int K) {
  const uint64_t key = shape_key(M, N, K);
  const TunedPlan* lo = std::lower_bound(g_tuned, g_tuned + g_num_tuned, key,
                                         [](const TunedPlan& p, uint64_t k) { return p.key < k; });
  for (; lo != g_tuned + g_num_tuned && lo->key == key; ++lo)
    if (lo->M == M && lo->N == N && lo->K == K) return lo;
  return nullptr;
}

bool neighbour_plan(int M, int N, int K, int* cfg, int* splits, int* group_m, RankedPlan* ranked, int* n_ranked) {
  double best = 1e30;
  bool found = false;
  // a candidate plan: listed for the first-use selection when `rank`, kept when it is the fastest so far
  auto take = [&](double us, int c, int sp, bool rank) {
    const KernelEntry& e = g_kernel_table[c];
    const int g = default_group_m(e, (M + e.bm - 1) / e.bm, (N + e.bn - 1) / e.bn);
    if (rank && ranked && n_ranked && *n_ranked < 8) ranked[(*n_ranked)++] = RankedPlan{us, c, sp, g};
    if (us < best) { best = us; found = true; *cfg = c; *splits = sp; *group_m = g; }
  };
  int br[3][2];
  const int dims[3] = {M, N, K};
  for (int d = 0; d < 3; ++d) {
    int lo = kLattice[0], hi = kLattice[kLatticeN - 1];
    for (int i = 0; i < kLatticeN; ++i) {
      if (kLattice[i] <= dims[d]) lo = kLattice[i];
      if (kLattice[kLatticeN - 1 - i] >= dims[d]) hi = kLattice[kLatticeN - 1 - i];
    }
    br[d][0] = lo; br[d][1] = hi;
  }
  for (int c = 0; c < 8; ++c) {
    const TunedPlan* p = find_tuned(br[0][c & 1], br[1][(c >> 1) & 1], br[2][(c >> 2) & 1]);
    if (!p || p->cfg < 0) continue;
    const KernelEntry& e = g_kernel_table[p->cfg];
    if (!k_ok(e, K)) continue;
    if ((e.bm > M * 2 && e.bm > 32) || (e.bn > N * 2 && e.bn > 32)) continue;   // mostly padding
    const int ksteps = std::max(1, K / e.kgran);
    // a stream-K corner plan keeps its form (the low bits are its workgroup count, not a split count) and is priced as such
    const bool sk_usable = streamk_really_runs(e, M, N, K);   // (direct K tail, > 65536 tiles: the launch would run data-parallel)
    if ((p->splits & HGEMM_PLAN_STREAMK) && sk_usable) {
      take(model_us_streamk(e, M, N, K, streamk_grid(e, p->splits & HGEMM_SPLITK_MASK)), p->cfg,
           HGEMM_PLAN_STREAMK | (p->splits & HGEMM_SPLITK_MASK), true);
      continue;
    }
    const int s = (p->splits & HGEMM_PLAN_STREAMK) ? 1 : std::max(1, std::min(p->splits & HGEMM_SPLITK_MASK, ksteps));
    const long wgs_here = (long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn) * s;
    // A "_k4" member of family w spends a whole four-wave workgroup on a 32 x 32 (or smaller) tile: it wins where the grid gave it
    // at most one workgroup per CU (256 x 1024 x 1024, 512 x 512 x 512: by 2 % over t32x64) and loses as soon as there are more
    // (512 x 1024 x 512: 7.2 us against 5.7; off the grid 256 x 1600 x 1024 at 400 workgroups 12.2 against 9.0 for t64x64,
    // 640 x 640 x 640 9.2 against 7.4 -- tuning/r04_retune_pass2_mi355x.jsonl, r03_offgrid_tune_mi355x.jsonl, r04 off-grid reports)
    if (w_splits_k(e) && wgs_here > kCUs) continue;
    // Family r is bound by what a CU can stream: its corner plans were tuned with one or two workgroups on EVERY CU.  A count
    // between one and 1.75 rounds of the chip leaves most CUs idle while a few run a second workgroup (64 x 14928 x 10624: 156 tiles
    // of 64 x 96 at two splits = 312 workgroups, 83.4 us, where the 64 x 128 corner plan's 234 take 63.8)
    if (e.family == Family::R && wgs_here > kCUs && wgs_here < kCUs * 7 / 4) continue;
    // the 8-wave mid tiles were tuned (and the model fitted) for at most two workgroups per CU: beyond that the larger tiles of
    // another corner win (1332 x 3108 x 4440: 525 tiles of 64 x 128 measured 101 us against 82 us for the 256 x 256 corner plan)
    if (e.family == Family::T && e.wm * e.wn == 8 && e.bm * e.bn <= 128 * 64 &&
        (long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn) * s > 2L * kCUs) continue;
    int sp = s > 1 ? (s | (p->splits & HGEMM_SPLITK_FUSED)) : 1;
    // family r's load flags travel with the corner plan (they belong to the access pattern of the shape class, not to the shape)
    // -- while the rows stay 128-byte aligned (K % 64 == 0).  With rows that straddle cache lines a non-temporal load drops the
    // half line the next K stage of the same row needs again, and the flags cost instead of paying: 64 x 16384 x 9160 (stride
    // 18320 B) r64x128_k128 split 2 64.0 us plain / 70.6 with both flags, r64x64_k256 66.8 / 70.3, the corner plan itself
    // (r64x128_k128_d, NT loads) 73.6 -> 67.7 without; with aligned rows off the grid they keep paying (16000 x 128 x 16000
    // 0.81 -> 0.79 of hipBLASLt without them, 128 x 16000 x 16000 0.99 -> 0.95, 64 x 14928 x 10624 0.77 -> 0.73:
    // tuning/r04_ktail_candidates_mi355x.jsonl, r04_offgrid_plan_report_call_j3_no_r_flags_mi355x.jsonl)
    if (e.family == Family::R && K % 64 == 0) sp |= p->splits & (HGEMM_PLAN_RS_XCD_STAGGER | HGEMM_PLAN_RS_NT_LOADS);
    // family q's schedule flags (round 5) travel with the corner plan as well: they belong to the shape class (a one-round plan of
    // long rows wants the K stagger, a walk of many short-K items the phase offset), cannot change a result, and fall away by
    // themselves where they do not apply (a K tail takes the ktail variant, a single round has nothing to offset)
    if (e.family == Family::Q) sp |= p->splits & (HGEMM_PLAN_XCD_STAGGER | HGEMM_PLAN_PHASE_OFFSET | HGEMM_PLAN_PHASE_OFFSET4);
    take(model_us(e, M, N, K, s), p->cfg, sp, true);
  }
  // The grid's only multiple of 192 is 12288: a shape with another one (3072, 1536, 6144 ...) finds no corner that uses the 192-wide
  // persistent tiles although they may fit it exactly (3072^2: 144 tiles of 256 x 256 on 256 CUs, 192 of 192 x 256).  They join the
  // ranking with the split count of the best corner and unsplit (the model prices the members of family q on one scale:
  // measured / modelled 1.39-1.42 for all of them, tuning/r03_late_tune_mi355x.jsonl).
  if (found) {
    const int best_s = (*splits & HGEMM_PLAN_STREAMK) ? 1 : std::max(1, *splits & HGEMM_SPLITK_MASK), best_fused = *splits & HGEMM_SPLITK_FUSED;
    const char* extra[2] = {(M % 192 == 0 && N >= 128) ? "q192x256_w2x2" : nullptr,
                            (N % 192 == 0 && M >= 128) ? "q256x192_w2x2" : nullptr};
    for (const char* name : extra) {
      if (!name) continue;
      const int c = hgemm_mi355x_config_by_name(name);
      if (c < 0) continue;
      const KernelEntry& e = g_kernel_table[c];
      // (only where the 192-wide tiles fill at least half the chip: 1968 x 576 has 24 of them and measured 0.72x of its corner plan)
      if ((long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn) < kCUs / 2 || !k_ok(e, K)) continue;
      for (int s : {1, best_s})
        if (s <= std::max(1, K / e.kgran)) take(model_us(e, M, N, K, s), c, s > 1 ? (s | best_fused) : 1, false);
    }
  }
  // A corner plan of family q was tuned on a shape whose tiles fill the resident workgroups; off the grid the same tile may leave
  // much of the last (or only) round empty (1332 x 3108 x 4440: 143 tiles of 128 x 256 on 256 workgroups = 84.7 us, where 204 items
  // of 256 x 192 at two splits take 60.0 and 156 of 256 x 256 at two splits 66.0 -- tuning/r04_ktail_candidates_mi355x.jsonl).
  // When the chosen q plan is a single round that fills less than 80 % of the resident workgroups, its siblings join the ranking
  // at one, two and four splits -- inside the family the model prices on one scale -- provided they do not fill their rounds worse.  (More
  // than one round is the hybrid tail schedule's case, hgemm_mi355x_launch; the 192-wide members keep their own, measured rule
  // above.)
  if (found && !(*splits & HGEMM_PLAN_STREAMK) && g_kernel_table[*cfg].family == Family::Q && g_kernel_table[*cfg].mi == 16) {
    auto fill_of = [&](const KernelEntry& e, int s) {
      const long items = (long)((M + e.bm - 1) / e.bm) * ((N + e.bn - 1) / e.bn) * s, cap = std::max(1, e.persistent_wgs);
      return (double)items / (double)(((items + cap - 1) / cap) * cap);
    };
    const KernelEntry& e0 = g_kernel_table[*cfg];
    const int s0 = std::max(1, *splits & HGEMM_SPLITK_MASK);
    const double fill0 = fill_of(e0, s0);
    // (not for a two-resident corner plan: its 512 slots are two per CU, 256 items of it already occupy every CU)
    if (fill0 < 0.8 && e0.persistent_wgs <= kCUs && (long)((M + e0.bm - 1) / e0.bm) * ((N + e0.bn - 1) / e0.bn) * s0 <= e0.persistent_wgs) {
      const int fused0 = *splits & HGEMM_SPLITK_FUSED;
      for (const char* name : {"q256x256_w2x2", "q256x128_w2x2", "q128x256_w2x2", "q128x128_w2x2_k128"}) {
        const int c = hgemm_mi355x_config_by_name(name);
        if (c < 0) continue;
        const KernelEntry& e = g_kernel_table[c];
        if (!k_ok(e, K) || (e.bm > M * 2 && e.bm > 32) || (e.bn > N * 2 && e.bn > 32)) continue;
        for (int s : {1, 2, 4}) {
          // (round 6: a split of a sibling needs >= 2048 of K per slice -- with 1024 the model took 40 tiles of 256 x 128 at four
          // single-launch splits for 1968 x 576 x 4096 when its corner moved to the K = 128 stages: 39.1 us against 26.9 for the corner plan)
          if (s > 1 && K / s < 2048) break;
          if (fill_of(e, s) >= fill0) take(model_us(e, M, N, K, s), c, s > 1 ? (s | fused0) : 1, false);
        }
      }
    }
  }
  return found;
}

}  // namespace hgemm_mi355x
