// The fused residual add of the bf16 GEMMs (bgemm_mi355x_tn_bias_add, bgemm_mi355x_nn_add): the one text of the add, used by the member
// kernels' epilogues (hgemm_kernel_tn.hpp, hgemm_kernel_nn.hpp), by the combine of the two-pass form and by the reference kernel
// (hgemm_registry.hip: OutBiasAdd, OutAdd).
//   s     the finished fp32 sum: the accumulator of a plain launch, or the slabs of a two-pass plan added in split order
//   bias  float(bias[n]) of the bf16 bias vector; a NULL vector counts as +0.0 and is added like any other
//   r     float(r[m][n]) of the bf16 residual matrix, read before the output element is stored (r may be C itself)
// Plain IEEE fp32 adds in the order written -- the library is built without fast-math, so the compiler neither reassociates nor drops the
// add of a zero --, and the caller rounds the result to bf16 once.  Nothing is ever added to a slab.
#pragma once

namespace hgemm_mi355x {

// C = bf16(residual_add(s, r)): one add on the finished sum
__host__ __device__ __forceinline__ float residual_add(float s, float r) { return s + r; }
// C = bf16(bias_residual_add(s, bias, r)): z = fl32(s + bias) is bgemm_mi355x_tn_bias's value before its rounding, then fl32(z + r)
__host__ __device__ __forceinline__ float bias_residual_add(float s, float bias, float r) { return residual_add(s + bias, r); }

}  // namespace hgemm_mi355x
