// Family f's grouped gated kernels (hgemm_kernel_tn_grouped_gated.hpp, hgemm_tn_grouped_gated_kernel<., ., false>: bgemm_mi355x_tn_grouped_gated
// without g_out / u_out, the gated forward of a mixture-of-experts layer in one launch, the tile map read from device offsets): four members x
// four activations.  A unit of its own: every other unit keeps exactly its kernels and their instruction streams.
#include "hgemm_kernel_tn_grouped_gated.hpp"

namespace hgemm_mi355x {

HGEMM_TN_GROUPED_GATED_ACTS(HGEMM_TN_GROUPED_GATED_INST, false)

}  // namespace hgemm_mi355x
