// Kernel instantiations of family n (hgemm_kernel_nn.hpp: row-major B through transposed LDS reads) and the family's table.
// A unit of its own: the kernels of units 0-4 keep their instruction streams, the geometry table keeps its ids.
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

#define HGEMM_NN_MEMBERS(X) X(64, 64, 2, 2, 4) X(128, 64, 2, 2, 3) X(64, 128, 2, 2, 3) X(128, 128, 2, 2, 3)

#define HGEMM_NN_INST(BM, BN, WM, WN, NB) template void launch_nn<CfgNN<BM, BN, WM, WN, NB>>(const GemmArgs&, int, hipStream_t, int, TimingSlot);
HGEMM_NN_MEMBERS(HGEMM_NN_INST)

#if !defined(__HIP_DEVICE_COMPILE__)
// ids of hgemm_mi355x_launch_nn are positions in this table, smallest tile first (names: hgemm_mi355x_nn_config_by_name)
#define HGEMM_NN_ROW(BM, BN, WM, WN, NB)                                                                                  \
  {"n" #BM "x" #BN "_w" #WM "x" #WN, BM, BN, WM, WN, NB, CfgNN<BM, BN, WM, WN, NB>::THREADS, CfgNN<BM, BN, WM, WN, NB>::LDS_BYTES, \
   &launch_nn<CfgNN<BM, BN, WM, WN, NB>>},
const NNEntry g_nn_table[] = {HGEMM_NN_MEMBERS(HGEMM_NN_ROW)};
const int g_num_nn = (int)(sizeof(g_nn_table) / sizeof(g_nn_table[0]));
#endif

}  // namespace hgemm_mi355x
