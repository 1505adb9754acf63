// Family f's fused-bias kernels (hgemm_kernel_tn.hpp, CfgTNB with EPI_C16_BIAS: bgemm_mi355x_tn_bias, C = bf16(A B + bias), the bias added
// last in fp32 and the sum rounded once).  A unit of its own: unit 11 keeps exactly its eight kernels and their instruction streams.
#include "hgemm_kernel_tn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TN_BIAS_INST, CfgTNB)

}  // namespace hgemm_mi355x
