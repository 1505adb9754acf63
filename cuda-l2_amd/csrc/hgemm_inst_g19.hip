// Family n's dgated kernels (hgemm_kernel_nn.hpp, CfgNNB with EPI_C16_DGATED + ACT: bgemm_mi355x_nn_dgated, the gated MLP's input gradient,
// dU = bf16(act(g) x A B) and dG = bf16(A B x u x act'(g)) at the saved bf16 pre-activations, each rounded once): four members x four
// activations.  A unit of its own: units 0 to 18 keep exactly their kernels and their instruction streams.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_INST, ACT_RELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_INST, ACT_GELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_INST, ACT_GELU_TANH, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_INST, ACT_SILU, CfgNNB)

}  // namespace hgemm_mi355x
