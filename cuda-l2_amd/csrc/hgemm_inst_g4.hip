// Kernel instantiations of family u (hgemm_configs_lu.def).
#define HGEMM_INST_GROUP 4
#include "hgemm_inst.inc"
