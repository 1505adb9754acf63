// Family n's dact kernels (hgemm_kernel_nn.hpp, CfgNNB with EPI_C16_DACT + ACT: bgemm_mi355x_nn_dact, C = bf16(A B x act'(z)), the
// derivative of hgemm_act.hpp at the saved bf16 pre-activation, one fp32 multiply on the finished sum and one rounding): four members x
// three activations.  A unit of its own: unit 8 keeps exactly its kernels and their instruction streams.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_NN_DACT_INST, ACT_RELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DACT_INST, ACT_GELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DACT_INST, ACT_GELU_TANH, CfgNNB)

}  // namespace hgemm_mi355x
