// Family a's fp32-C kernels on bfloat16 operands (hgemm_kernel_ta.hpp, CfgTAB with EPI_C32: no convert on the path) and their launchers.
// A unit of its own: units 7 and 9 keep their kernels and instruction streams.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

template <class CFG>
void launch_ta_c32(const GemmArgs& g, int grid, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH((CFG::template kernel<EPI_C32>()), grid, CFG::THREADS, stream, ts, g);
}

#define HGEMM_TA_C32_INST(P, CFG, BM, BN, WM, WN, NB) template void launch_ta_c32<CFG<BM, BN, WM, WN, NB>>(const GemmArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_TA_C32_ROW(P, CFG, BM, BN, WM, WN, NB) &launch_ta_c32<CFG<BM, BN, WM, WN, NB>>,

HGEMM_TR_MEMBERS(HGEMM_TA_C32_INST, "a", CfgTAB)

#if !defined(__HIP_DEVICE_COMPILE__)
// indexed by TA config id, as g_ta_c32_launch is (hgemm_inst_g7.hip)
const TaC32Launch g_ta_bf16_c32_launch[] = {HGEMM_TR_MEMBERS(HGEMM_TA_C32_ROW, "a", CfgTAB)};
const int g_num_ta_bf16_c32 = (int)(sizeof(g_ta_bf16_c32_launch) / sizeof(g_ta_bf16_c32_launch[0]));
#endif

}  // namespace hgemm_mi355x
