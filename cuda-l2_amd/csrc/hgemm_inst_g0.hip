// Kernel instantiations, group 0 of hgemm_configs.def.
#define HGEMM_INST_GROUP 0
#include "hgemm_inst.inc"
