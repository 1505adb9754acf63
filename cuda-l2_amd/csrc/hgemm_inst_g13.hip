// The one-tile-per-workgroup kernel of q256x256_w2x2 (hgemm_kernel_sq_one.hpp) and its host side: the selection rule, the process-wide
// switch and the launch counter.  A unit of its own: the kernels of units 0-4 keep their instruction streams and their name set.
#include "hgemm_launch.hpp"
#include "hgemm_kernel_sq_one.hpp"

#include <atomic>

namespace hgemm_mi355x {

template __global__ void hgemm_tn_sq_one_kernel<CfgSQOne>(const GemmArgs);

namespace {
// A measurement build (-DHGEMM_TIMELINE) runs the general kernel unless the switch is turned on explicitly: its records are compared
// with the earlier rounds' by default.
#ifdef HGEMM_TIMELINE
std::atomic<int> g_sq_one_on{0};
#else
std::atomic<int> g_sq_one_on{1};
#endif
std::atomic<unsigned long long> g_sq_one_launches{0};
}  // namespace

int sq_one_set_enabled(int on) { return g_sq_one_on.exchange(on ? 1 : 0); }
unsigned long long sq_one_launch_count() { return g_sq_one_launches.load(); }

// The launches hgemm_tn_sq_one_kernel takes, of those launch_sq<CfgSQOne> is handed (`g` as resolve_launch made it, C set):
bool sq_one_takes(const GemmArgs& g, int grid, int epi) {
  if (!g_sq_one_on.load(std::memory_order_relaxed)) return false;
  if (epi != EPI_C16 || !c_takes_wide_stores(g)) return false;                       // the plain wide fp16 epilogue
  if (g.K % (BK * CfgSQOne::KT) != 0 || g.K / BK < SQ_ONE_MIN_STEPS) return false;   // whole stages, at least the streams' depth
  if (g.splits != 1 || g.tail_tiles != 0 || g.items > grid) return false;            // one whole-K work item per workgroup at most
  if (g.flags & (ARG_XCD_STAGGER | ARG_PHASE_OFFSET | ARG_PHASE_OFFSET4)) return false;
#ifdef HGEMM_ABLATION
  if (g.debug) return false;
#endif
  return true;
}

bool launch_sq_one(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (!sq_one_takes(g, grid, epi)) return false;
  g_sq_one_launches.fetch_add(1, std::memory_order_relaxed);
  HGEMM_LAUNCH((hgemm_tn_sq_one_kernel<CfgSQOne>), grid, CfgSQOne::THREADS, stream, ts, g);
  return true;
}

}  // namespace hgemm_mi355x
