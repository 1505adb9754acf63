// Family f's grouped kernels (hgemm_kernel_tn_grouped.hpp, hgemm_tn_grouped_kernel over CfgTNB: bgemm_mi355x_tn_grouped, the forward product of
// a mixture-of-experts layer in one launch, the tile map read from device offsets): four members.  A unit of its own: every other unit keeps
// exactly its kernels and their instruction streams.
#include "hgemm_kernel_tn_grouped.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TN_GROUPED_INST, CfgTNB)

}  // namespace hgemm_mi355x
