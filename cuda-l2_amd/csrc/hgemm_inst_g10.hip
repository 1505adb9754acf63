// Family a's fp32-C kernels on bfloat16 operands (hgemm_kernel_ta.hpp, CfgTAB with EPI_C32: no convert on the path).  A unit of its
// own: units 7 and 9 keep their kernels and instruction streams.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, CfgTAB, true)

}  // namespace hgemm_mi355x
