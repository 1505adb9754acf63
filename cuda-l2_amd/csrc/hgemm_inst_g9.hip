// Family a's bfloat16 kernels (hgemm_kernel_ta.hpp, CfgTAB: v_mfma_f32_16x16x32_bf16, bf16 C) and their launchers.  A unit of its own:
// unit 6 keeps its eight kernels and their instruction streams, g_ta_table its rows.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, "a", CfgTAB)

#if !defined(__HIP_DEVICE_COMPILE__)
// indexed by TA config id: HGEMM_TR_MEMBERS is the order of g_ta_table's rows (hgemm_inst_g6.hip)
const TrLaunch g_ta_bf16_launch[] = {HGEMM_TR_MEMBERS(HGEMM_TR_LAUNCH_ROW, "a", CfgTAB)};
const int g_num_ta_bf16 = (int)(sizeof(g_ta_bf16_launch) / sizeof(g_ta_bf16_launch[0]));
#endif

}  // namespace hgemm_mi355x
