// Every launch thunk of the library, in the order of the two geometry lists: HGEMM_THUNK(unit, thunk, config type) once per entry.
// unit = the translation unit hgemm_inst_g<unit>.hip that compiles the thunk and its kernels (family u: unit 4, a unit of its own).
// Included with HGEMM_THUNK defined (hgemm_inst.inc instantiates, hgemm_registry.hip declares); undefines it.
#define HGEMM_CFG(G, BM, BN, WM, WN, MI, NB) HGEMM_THUNK(G, launch_cfg, Cfg<BM, BN, WM, WN, MI, NB>)
#define HGEMM_SP(G, BM, BN, WM, WN, MI) HGEMM_THUNK(G, launch_sp, CfgSP<BM, BN, WM, WN, MI>)
#define HGEMM_SQ(G, BM, BN, WM, WN, KT, MI) HGEMM_THUNK(G, launch_sq, CfgSQ<BM, BN, WM, WN, KT, MI>)
#define HGEMM_RS(G, BM, BN, BKS, LB) HGEMM_THUNK(G, launch_rs, CfgRS<BM, BN, BKS, LB>)
#define HGEMM_WD(G, FM, FN, KW) HGEMM_THUNK(G, launch_wd, CfgWD<FM, FN, KW>)
#include "hgemm_configs.def"
#define HGEMM_LU(BM, BN, WM, WN, NIMG, NB) HGEMM_THUNK(4, launch_lu, CfgLU<BM, BN, WM, WN, NIMG, NB>)
#include "hgemm_configs_lu.def"
#undef HGEMM_THUNK
