// Kernel instantiations, group 2 of hgemm_configs.def.
#define HGEMM_INST_GROUP 2
#include "hgemm_inst.inc"
