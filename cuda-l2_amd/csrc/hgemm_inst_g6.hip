// Kernel instantiations of family a (hgemm_kernel_ta.hpp: A given as [K][M], both operands through transposed LDS reads), fp16.  A
// unit of its own: the kernels of units 0-5 keep their instruction streams.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, CfgTA, false)

}  // namespace hgemm_mi355x
