// The activations of the fused bias+activation calls (bgemm_mi355x_tn_bias_act): ONE text, used by family f's epilogue
// (hgemm_kernel_tn.hpp), by the split-K combine and by the reference kernel (hgemm_registry.hip), and by a CPU program
// (tests/test_tn_bias_act_host.py builds one with the host compiler).  act_apply<ACT>(z) maps the unrounded fp32 z = S + float(bias[n]) to
// the fp32 value that is then rounded to bf16 once.
//
// Written so that the result does not depend on the caller: contraction is off inside each function, a fused operation is an explicit
// fmaf, and erff / expf are the math library's.  No HIP construct besides the two function attributes, which are empty for a host compiler
// (a host compiler without the pragma below is given -ffp-contract=off instead).
//
//   HGEMM_ACT_RELU      y = z if z > 0 or z is NaN, else +0.0f: -0, -inf and every negative give +0, NaN stays NaN, +inf stays +inf.
//   HGEMM_ACT_GELU      y = (0.5 z) (1 + erf(z / sqrt 2)), the erf form (torch's default).
//   HGEMM_ACT_GELU_TANH y = 0.5 z (1 + tanh(u)), u = sqrt(2 / pi) (z + 0.044715 z^3), evaluated in the algebraically equal sigmoid form
//                       z / (1 + exp(-2u)): one exp and one division, and no cancellation in the negative tail.  A large negative finite z,
//                       where z^3 overflows, gives u = -inf, exp = +inf and y = -0; a large positive z gives exp = 0 and y = z.
//   Both GELUs: NaN gives NaN, +inf gives +inf, -inf gives NaN (0 x inf and inf / inf, as the formulas have it: no select is spent),
//   +-0 gives a zero.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGEMM_ACT_HD __host__ __device__ inline
#else
#define HGEMM_ACT_HD inline
#endif
#if defined(__clang__)
#define HGEMM_ACT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HGEMM_ACT_NO_CONTRACT
#endif

namespace hgemm_mi355x {

// the public constants' values (include/hgemm_mi355x.h: HGEMM_ACT_RELU / _GELU / _GELU_TANH)
constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_GELU_TANH = 3;

template <int ACT>
HGEMM_ACT_HD float act_apply(float z) {
  HGEMM_ACT_NO_CONTRACT
  static_assert(ACT == ACT_RELU || ACT == ACT_GELU || ACT == ACT_GELU_TANH, "relu, gelu (erf), gelu (tanh)");
  if (ACT == ACT_RELU) {
    return (z > 0.0f || z != z) ? z : 0.0f;
  } else if (ACT == ACT_GELU) {
    const float t = 1.0f + erff(z * 0.70710678118654752440f);   // in [0, 2]
    return (0.5f * z) * t;
  } else {
    const float z3 = (z * z) * z;
    const float inner = fmaf(0.044715f, z3, z);                  // z + 0.044715 z^3
    const float e = expf(-1.5957691216057307117f * inner);       // exp(-2u), -2 sqrt(2 / pi)
    return z / (1.0f + e);
  }
}

}  // namespace hgemm_mi355x
