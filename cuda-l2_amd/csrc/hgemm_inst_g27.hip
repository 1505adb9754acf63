// Family f's grouped gated kernels that also write the rounded pre-activations (hgemm_kernel_tn_grouped_gated.hpp,
// hgemm_tn_grouped_gated_kernel<., ., true>: bgemm_mi355x_tn_grouped_gated with g_out = bf16(g) and u_out = bf16(u), the training form): four
// members x four activations.  A unit of its own: every other unit keeps exactly its kernels and their instruction streams.
#include "hgemm_kernel_tn_grouped_gated.hpp"

namespace hgemm_mi355x {

HGEMM_TN_GROUPED_GATED_ACTS(HGEMM_TN_GROUPED_GATED_INST, true)

}  // namespace hgemm_mi355x
