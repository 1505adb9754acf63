// Kernel instantiations, group 1 of hgemm_configs.def.
#define HGEMM_INST_GROUP 1
#include "hgemm_inst.inc"
