// Family f's gated kernels that also write the rounded pre-activations (hgemm_kernel_tn_gated.hpp, hgemm_tn_gated_aux_kernel:
// bgemm_mi355x_tn_gated_aux, g_out = bf16(g), u_out = bf16(u) and C = bf16(act(g) * u), g and u unrounded): four members x four activations.
// The K slices of a two-pass form are unit g18's slab kernels.  A unit of its own: units 0 to 19 keep exactly their kernels and their
// instruction streams.
#include "hgemm_kernel_tn_gated.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_INST, ACT_RELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_INST, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_INST, ACT_GELU_TANH, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_INST, ACT_SILU, CfgTNB)

}  // namespace hgemm_mi355x
