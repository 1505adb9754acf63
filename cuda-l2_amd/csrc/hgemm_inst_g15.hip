// Family f's fused bias+activation kernels that also write the rounded pre-activation (hgemm_kernel_tn.hpp, CfgTNB with
// EPI_C16_BIAS_AUX + ACT: bgemm_mi355x_tn_bias_act_aux, z_out = bf16(z) and C = bf16(act(z)), z = A B + bias unrounded): four members x
// three activations.  A unit of its own: units 11, 12 and 14 keep exactly their kernels and their instruction streams.
#include "hgemm_kernel_tn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TN_AUX_INST, ACT_RELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_AUX_INST, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_AUX_INST, ACT_GELU_TANH, CfgTNB)

}  // namespace hgemm_mi355x
