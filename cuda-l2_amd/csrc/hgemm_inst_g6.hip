// Kernel instantiations of family a (hgemm_kernel_ta.hpp: A given as [K][M], both operands through transposed LDS reads) and the
// family's table.  A unit of its own: the kernels of units 0-5 keep their instruction streams, the geometry and NN tables their ids.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

HGEMM_TR_MEMBERS(HGEMM_TR_INST, "a", CfgTA)

#if !defined(__HIP_DEVICE_COMPILE__)
// ids of hgemm_mi355x_launch_ta are positions in this table (names: hgemm_mi355x_ta_config_by_name)
const NNEntry g_ta_table[] = {HGEMM_TR_MEMBERS(HGEMM_TR_ROW, "a", CfgTA)};
const int g_num_ta = (int)(sizeof(g_ta_table) / sizeof(g_ta_table[0]));
#endif

}  // namespace hgemm_mi355x
