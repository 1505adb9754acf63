// Kernel instantiations of family n (hgemm_kernel_nn.hpp: row-major B through transposed LDS reads), fp16.  A unit of its own: the
// kernels of units 0-4 keep their instruction streams, the geometry table keeps its ids.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, CfgNN, false)

}  // namespace hgemm_mi355x
