// Family n's bfloat16 kernels (hgemm_kernel_nn.hpp, CfgNNB: v_mfma_f32_16x16x32_bf16, bf16 C) and their launchers.  A unit of its own:
// unit 5 keeps its eight kernels and their instruction streams, g_nn_table its rows.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, "n", CfgNNB)

#if !defined(__HIP_DEVICE_COMPILE__)
// indexed by NN config id: HGEMM_TR_MEMBERS is the order of g_nn_table's rows (hgemm_inst_g5.hip)
const TrLaunch g_nn_bf16_launch[] = {HGEMM_TR_MEMBERS(HGEMM_TR_LAUNCH_ROW, "n", CfgNNB)};
const int g_num_nn_bf16 = (int)(sizeof(g_nn_bf16_launch) / sizeof(g_nn_bf16_launch[0]));
#endif

}  // namespace hgemm_mi355x
