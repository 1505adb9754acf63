// Family f's fused bias+activation kernels (hgemm_kernel_tn.hpp, CfgTNB with EPI_C16_BIAS + ACT: bgemm_mi355x_tn_bias_act,
// C = bf16(act(A B + bias)), the activation of hgemm_act.hpp applied to the unrounded fp32 sum and the result rounded once): four members x
// three activations.  A unit of its own: units 11 and 12 keep exactly their kernels and their instruction streams.
#include "hgemm_kernel_tn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TN_ACT_INST, ACT_RELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_ACT_INST, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_ACT_INST, ACT_GELU_TANH, CfgTNB)

}  // namespace hgemm_mi355x
