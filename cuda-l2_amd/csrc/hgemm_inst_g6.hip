// Kernel instantiations of family a (hgemm_kernel_ta.hpp: A given as [K][M], both operands through transposed LDS reads) and the
// family's table.  A unit of its own: the kernels of units 0-5 keep their instruction streams, the geometry and NN tables their ids.
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

#define HGEMM_TA_MEMBERS(X) X(64, 64, 2, 2, 4) X(128, 64, 2, 2, 3) X(64, 128, 2, 2, 3) X(128, 128, 2, 2, 3)

#define HGEMM_TA_INST(BM, BN, WM, WN, NB) template void launch_ta<CfgTA<BM, BN, WM, WN, NB>>(const GemmArgs&, int, hipStream_t, int, TimingSlot);
HGEMM_TA_MEMBERS(HGEMM_TA_INST)

#if !defined(__HIP_DEVICE_COMPILE__)
// ids of hgemm_mi355x_launch_ta are positions in this table, smallest tile first (names: hgemm_mi355x_ta_config_by_name)
#define HGEMM_TA_ROW(BM, BN, WM, WN, NB)                                                                                  \
  {"a" #BM "x" #BN "_w" #WM "x" #WN, BM, BN, WM, WN, NB, CfgTA<BM, BN, WM, WN, NB>::THREADS, CfgTA<BM, BN, WM, WN, NB>::LDS_BYTES, \
   &launch_ta<CfgTA<BM, BN, WM, WN, NB>>},
const NNEntry g_ta_table[] = {HGEMM_TA_MEMBERS(HGEMM_TA_ROW)};
const int g_num_ta = (int)(sizeof(g_ta_table) / sizeof(g_ta_table[0]));
#endif

}  // namespace hgemm_mi355x
