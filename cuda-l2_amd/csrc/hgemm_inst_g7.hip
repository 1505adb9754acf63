// Family a's fp32-C kernels (hgemm_kernel_ta.hpp, EPI_C32: the accumulators stored to, or added into, the caller's fp32 C).  A unit
// of its own: unit 6 keeps its eight kernels and their instruction streams.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, CfgTA, true)

}  // namespace hgemm_mi355x
