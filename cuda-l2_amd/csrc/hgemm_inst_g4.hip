// Kernel instantiations of family u (hgemm_configs_lu.def): a translation unit of its own, so that the kernels of
// hgemm_inst_g0..g3.hip keep their instruction streams.
#include "hgemm_launch.hpp"

namespace hgemm_mi355x {
#define HGEMM_LU(BM, BN, WM, WN, NIMG, NB) \
  template void launch_lu<CfgLU<BM, BN, WM, WN, NIMG, NB>>(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#include "hgemm_configs_lu.def"
#undef HGEMM_LU
}  // namespace hgemm_mi355x
