// Family n's residual kernels (hgemm_kernel_nn.hpp, CfgNNB with EPI_C16_ADD: bgemm_mi355x_nn_add, C = bf16(A B + r), one fp32 add on the
// finished sum and one rounding; r may be C): four members.  A unit of its own: units 8 and 16 keep exactly their kernels and their
// instruction streams.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_NN_ADD_INST, CfgNNB)

}  // namespace hgemm_mi355x
