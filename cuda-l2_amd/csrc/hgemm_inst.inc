// Body of the instantiation units hgemm_inst_g<n>.hip (split so that they build in parallel): the explicit instantiations of the
// thunks whose unit is HGEMM_INST_GROUP, in list order.  Unit 4 holds family u alone, so that the kernels of units 0-3 keep their
// instruction streams.
#include "hgemm_launch.hpp"

#define HGEMM_INST_0(...)
#define HGEMM_INST_1(...)
#define HGEMM_INST_2(...)
#define HGEMM_INST_3(...)
#define HGEMM_INST_4(...)
#if HGEMM_INST_GROUP == 0
#undef HGEMM_INST_0
#define HGEMM_INST_0(...) __VA_ARGS__
#elif HGEMM_INST_GROUP == 1
#undef HGEMM_INST_1
#define HGEMM_INST_1(...) __VA_ARGS__
#elif HGEMM_INST_GROUP == 2
#undef HGEMM_INST_2
#define HGEMM_INST_2(...) __VA_ARGS__
#elif HGEMM_INST_GROUP == 3
#undef HGEMM_INST_3
#define HGEMM_INST_3(...) __VA_ARGS__
#elif HGEMM_INST_GROUP == 4
#undef HGEMM_INST_4
#define HGEMM_INST_4(...) __VA_ARGS__
#else
#error "HGEMM_INST_GROUP must be 0..4"
#endif

namespace hgemm_mi355x {
#define HGEMM_THUNK(G, FN, ...) HGEMM_INST_##G(template void FN<__VA_ARGS__>(const GemmArgs&, int, hipStream_t, int, TimingSlot);)
#include "hgemm_thunks.inc"
}  // namespace hgemm_mi355x
