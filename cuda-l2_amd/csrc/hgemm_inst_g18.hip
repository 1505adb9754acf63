// Family f's gated kernels (hgemm_kernel_tn_gated.hpp: bgemm_mi355x_tn_gated, C = bf16(act(X Wg^T + bg) * (X Wu^T + bu)), bias, activation
// and gate applied once to the finished fp32 sums and the product rounded once): four members x (four activations + the two-pass slab
// form).  A unit of its own: units 0 to 17 keep exactly their kernels and their instruction streams.
#include "hgemm_kernel_tn_gated.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TN_GATED_SLAB_INST, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_INST, ACT_RELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_INST, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_INST, ACT_GELU_TANH, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_INST, ACT_SILU, CfgTNB)

}  // namespace hgemm_mi355x
