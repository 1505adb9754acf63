// Kernel instantiations of family n (hgemm_kernel_nn.hpp: row-major B through transposed LDS reads) and the family's table.
// A unit of its own: the kernels of units 0-4 keep their instruction streams, the geometry table keeps its ids.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, "n", CfgNN)

#if !defined(__HIP_DEVICE_COMPILE__)
// ids of hgemm_mi355x_launch_nn are positions in this table (names: hgemm_mi355x_nn_config_by_name)
const NNEntry g_nn_table[] = {HGEMM_TR_MEMBERS(HGEMM_TR_ROW, "n", CfgNN)};
const int g_num_nn = (int)(sizeof(g_nn_table) / sizeof(g_nn_table[0]));
#endif

}  // namespace hgemm_mi355x
