// Family a's bfloat16 kernels (hgemm_kernel_ta.hpp, CfgTAB: v_mfma_f32_16x16x32_bf16, bf16 C).  A unit of its own: unit 6 keeps its
// eight kernels and their instruction streams.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, CfgTAB, false)

}  // namespace hgemm_mi355x
