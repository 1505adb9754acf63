// Family a's fp32-C kernels (hgemm_kernel_ta.hpp, EPI_C32: the accumulators stored to, or added into, the caller's fp32 C) and their
// launchers.  A unit of its own: unit 6 keeps its eight kernels and their instruction streams, g_ta_table its rows.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

template <class CFG>
void launch_ta_c32(const GemmArgs& g, int grid, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH((CFG::template kernel<EPI_C32>()), grid, CFG::THREADS, stream, ts, g);
}

#define HGEMM_TA_C32_INST(P, CFG, BM, BN, WM, WN, NB) template void launch_ta_c32<CFG<BM, BN, WM, WN, NB>>(const GemmArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_TA_C32_ROW(P, CFG, BM, BN, WM, WN, NB) &launch_ta_c32<CFG<BM, BN, WM, WN, NB>>,

HGEMM_TR_MEMBERS(HGEMM_TA_C32_INST, "a", CfgTA)

#if !defined(__HIP_DEVICE_COMPILE__)
// indexed by TA config id: HGEMM_TR_MEMBERS is the order of g_ta_table's rows (hgemm_inst_g6.hip)
const TaC32Launch g_ta_c32_launch[] = {HGEMM_TR_MEMBERS(HGEMM_TA_C32_ROW, "a", CfgTA)};
const int g_num_ta_c32 = (int)(sizeof(g_ta_c32_launch) / sizeof(g_ta_c32_launch[0]));
#endif

}  // namespace hgemm_mi355x
