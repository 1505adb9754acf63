// Family n's grouped kernels (hgemm_kernel_nn_grouped.hpp, hgemm_nn_grouped_kernel over CfgNNB: bgemm_mi355x_nn_grouped, the input gradient of
// a mixture-of-experts layer in one launch, the tile map read from device offsets): four members x {EPI_C16, EPI_C16_ADD}.  A unit of its
// own: every other unit keeps exactly its kernels and their instruction streams.
#include "hgemm_kernel_nn_grouped.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_NN_GROUPED_INST, CfgNNB)

}  // namespace hgemm_mi355x
