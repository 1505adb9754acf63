// Family a's grouped kernels (hgemm_kernel_ta_grouped.hpp, hgemm_ta_grouped_kernel over CfgTAB with EPI_C32 and EPI_C16: bgemm_mi355x_ta_grouped_c32
// / _ta_grouped, the weight gradient of a mixture-of-experts layer in one launch, each group's K walk read from device offsets): four members,
// two forms.  A unit of its own: every other unit keeps exactly its kernels and their instruction streams.
#include "hgemm_kernel_ta_grouped.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TA_GROUPED_INST, CfgTAB)

}  // namespace hgemm_mi355x
