// Kernel instantiations, group 3 of hgemm_configs.def.
#define HGEMM_INST_GROUP 3
#include "hgemm_inst.inc"
