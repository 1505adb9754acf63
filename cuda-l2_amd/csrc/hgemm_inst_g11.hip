// Family f's kernels (hgemm_kernel_tn.hpp, CfgTNB: the bf16 forward product, B given as b_col_major; v_mfma_f32_16x16x32_bf16, bf16 C).
// A unit of its own: units 5 .. 10 keep their kernels and their instruction streams.
#include "hgemm_kernel_tn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, CfgTNB, false)

}  // namespace hgemm_mi355x
