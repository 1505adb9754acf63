// Family n's bfloat16 kernels (hgemm_kernel_nn.hpp, CfgNNB: v_mfma_f32_16x16x32_bf16, bf16 C).  A unit of its own: unit 5 keeps its
// eight kernels and their instruction streams.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, CfgNNB, false)

}  // namespace hgemm_mi355x
