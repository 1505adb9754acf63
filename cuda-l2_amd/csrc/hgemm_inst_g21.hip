// Family f's bias + residual kernels (hgemm_kernel_tn.hpp, CfgTNB with EPI_C16_BIAS_ADD: bgemm_mi355x_tn_bias_add, C = bf16((A B + bias) + r),
// two fp32 adds on the finished sum in this order and one rounding; r may be C): four members.  A unit of its own: units 11 and 12 keep
// exactly their kernels and their instruction streams.
#include "hgemm_kernel_tn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TN_ADD_INST, CfgTNB)

}  // namespace hgemm_mi355x
