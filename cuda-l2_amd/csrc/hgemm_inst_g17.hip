// Family n's dact + dbias kernels (hgemm_kernel_nn.hpp, CfgNNB with EPI_C16_DACT_DBIAS + ACT: bgemm_mi355x_nn_dact_dbias, the dact C bit
// for bit and the tile's fp32 column sums of the rounded values, hgemm_dbias.hpp): four members x three activations.  A unit of its own:
// unit 16 keeps exactly its kernels and their instruction streams.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_NN_DBIAS_INST, ACT_RELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DBIAS_INST, ACT_GELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DBIAS_INST, ACT_GELU_TANH, CfgNNB)

}  // namespace hgemm_mi355x
