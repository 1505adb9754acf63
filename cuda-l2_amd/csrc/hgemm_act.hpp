// The activations of the fused bias+activation calls (bgemm_mi355x_tn_bias_act): ONE text, used by family f's epilogue
// (hgemm_kernel_tn.hpp), by the split-K combine and by the reference kernel (hgemm_registry.hip), and by a CPU program
// (tests/test_tn_bias_act_host.py builds one with the host compiler).  act_apply<ACT>(z) maps the unrounded fp32 z = S + float(bias[n]) to
// the fp32 value that is then rounded to bf16 once.  Below it the derivatives, dact_apply / dact_mul (bgemm_mi355x_nn_dact; SiLU's for
// bgemm_mi355x_nn_dgated alone).
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
//   HGEMM_ACT_SILU      y = z / (1 + exp(-z)), the gated calls only (bgemm_mi355x_tn_gated, bgemm_mi355x_nn_dgated; every other call refuses the id).  NaN gives NaN,
//                       +inf gives +inf (exp = 0), -inf gives NaN (inf / inf), a large negative finite z gives exp = +inf and y = -0, +-0
//                       gives a zero of its sign.  expf within 1 ulp, one add and one correctly rounded division: within 4 x 2^-24 |y| of
//                       the exact value, so within 2^-22 |z| (|silu(z)| <= |z|).
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
constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_GELU_TANH = 3, ACT_SILU = 4;

template <int ACT>
HGEMM_ACT_HD float act_apply(float z) {
  HGEMM_ACT_NO_CONTRACT
  static_assert(ACT == ACT_RELU || ACT == ACT_GELU || ACT == ACT_GELU_TANH || ACT == ACT_SILU, "relu, gelu (erf), gelu (tanh), silu");
  if (ACT == ACT_RELU) {
    return (z > 0.0f || z != z) ? z : 0.0f;
  } else if (ACT == ACT_GELU) {
    const float t = 1.0f + erff(z * 0.70710678118654752440f);   // in [0, 2]
    return (0.5f * z) * t;
  } else if (ACT == ACT_GELU_TANH) {
    const float z3 = (z * z) * z;
    const float inner = fmaf(0.044715f, z3, z);                  // z + 0.044715 z^3
    const float e = expf(-1.5957691216057307117f * inner);       // exp(-2u), -2 sqrt(2 / pi)
    return z / (1.0f + e);
  } else {
    return z / (1.0f + expf(-z));
  }
}

// ---- the derivatives (bgemm_mi355x_nn_dact: C = bf16(S dact(z)), z the saved bf16 pre-activation) ---------------------------------------
// dact_apply<ACT>(z) is act'(z) in fp32, under the rules above; family n's epilogue, the dact combine and the dact reference kernel
// (hgemm_registry.hip) and a CPU program (tests/test_mlp_backward_host.py) share it.  ReLU is no factor but a select, dact_mul below.
//
//   HGEMM_ACT_RELU      1 if z > 0 or z is NaN, else 0 (-0, -inf and every negative give 0).  dact_mul<ACT_RELU>(S, z) returns S itself or
//                       +0.0f: no multiply, a NaN z passes S (torch's threshold_backward), an inf or NaN S under z <= 0 gives +0.
//   HGEMM_ACT_GELU      g = 1/2 (1 + erf(z / sqrt 2)) + z exp(-z^2 / 2) / sqrt(2 pi).
//   HGEMM_ACT_GELU_TANH g = s + z s (1 - s) 2u', s = 1 / (1 + exp(-2u)), u = sqrt(2 / pi) (z + 0.044715 z^3), u' = sqrt(2 / pi) (1 + 0.134145 z^2):
//                       the derivative of act_apply's own sigmoid form.  Evaluated on a = |z|: e = exp(-2u(a)) <= 1 never overflows,
//                       s(a) = 1 / (1 + e) and s(-a) = 1 - s(a) = e s(a) are both relatively accurate, s (1 - s) = s(a) s(-a) is even in z.
//   Both GELUs clamp z to [-16, 16] first (selects that let a NaN through).  Behind the clamp nothing overflows, so no 0 x inf arises for
//   any finite z; outside it |g - limit| < 2^-180 in exact arithmetic and the text returns the limit: every z >= 16, +inf included,
//   gives exactly 1 and every z <= -16, -inf included, gives +0.  NaN gives NaN.  z = +-0 gives 1/2.
//
// The error of the GELU derivatives, eps = DACT_EPS = 2^-19 (absolute: |g| <= 1.13), from the device math library's documented bounds --
// erff within 16 ulp (the allowance the forward's bar uses), expf within 1 ulp, division correctly rounded -- with h = 2^-24, a product,
// sum or fmaf within h of its value relatively, a constant within h / 2:
//   erf form.  t = 1 + erff(z c): the argument carries 1.5 h relatively, |x erf'(x)| <= 0.49, so 0.73 h; erff 16 ulp of a value in
//     [-1, 1], 16 x 2^-23 = 32 h; the sum 2 h; halved: 17.4 h.  z exp(-z^2 / 2) / sqrt(2 pi), value <= 0.242: the argument carries h
//     relatively, |z^3 / 2 phi(z)| <= 0.232, so 0.23 h; expf 2 h and three roundings 2.5 h of 0.242: 1.1 h.  The last fmaf, |g| < 2:
//     2 h.  The multiply S g: 1.13 h.  Sum 21.9 h < 32 h = 2^-19.
//   tanh form.  x = 2u(a) carries 5 h relatively (a^2, a^3, the fmaf, two constants, the product); e = expf(-x) 5 h x + 2 h relatively.
//     s(a): s(a) s(-a) (5 h x + 2 h) + 2 h s(a) <= 0.224 x 5 h + 0.5 h + 2 h = 3.6 h (t sig(t) sig(-t) <= 0.224); s(-a) = e s(a):
//     sig(-t) t <= 0.279, 0.279 x 5 h + 0.5 x 5 h = 3.9 h.  p = s(a) s(-a) relatively 10 h x + 10 h, 2u' 4 h, the two products 2 h:
//     T = a p 2u' carries (10 x + 16) h relatively, and T (10 x + 16) <= 8.6 over a >= 0 (its maximum, 8.54, lies at a = 1.29), so 8.6 h.  The last sum 2 h, the multiply S g 1.13 h.  Sum 15.6 h < 2^-19.
//   HGEMM_ACT_SILU      g = s + z s (1 - s), s = 1 / (1 + exp(-z)) (the gated backward call only, bgemm_mi355x_nn_dgated; |g| <= 1.0999).
//                       Written as the tanh form is, on a = |z|: e = exp(-a) <= 1, sp = s(a) = 1 / (1 + e), sm = s(-a) = e sp,
//                       t = a (sp sm) >= 0 (even in z), g = z < 0 ? sm - t : sp + t.  a is clamped to DACT_SILU_CLAMP = 128 and not to 16:
//                       at a = 16 the function is still 1.9 x 10^-6 = 32 h from its limit.  exp(-128) = 2.6 x 10^-56 lies 31 binades below
//                       half the least denormal, so expf gives exactly 0 there, sp = 1, sm = t = +0 (a is finite: no 0 x inf): every
//                       z >= 128, +inf included, gives exactly 1, every z <= -128, -inf included, +0 (the function is within 2^-177 of
//                       the limit), NaN gives NaN, +-0 gives 1/2.
//   silu form.  a is exact.  e = expf(-a): 2 h relatively.  sp: e's error enters with weight e / (1 + e) = sm <= 1/2, so h; the sum and the
//     division h each: 3 h relatively, sp <= 1.  sm = e sp: 2 h + 3 h + h = 6 h relatively of a value <= 1/2: 3 h.  p = sp sm: 3 h + 6 h + h =
//     10 h relatively, t = a p 11 h, t <= 0.224 (a sig(a) sig(-a), its maximum at a = 1.54): 2.5 h.  The last sum: sm or sp 3 h, t 2.5 h, its
//     rounding 1.1 h: 6.6 h.  The multiply S g 1.1 h.  Sum 7.7 h < 2^-19.
// The bar of the call: |C - S g*(z)| <= 1/2 ulp_bf16(S g*) + DACT_EPS |S|, g* the derivative in fp64.
// The gated backward call multiplies v = fl32(S u) by g (hgemm_dgated.hpp): v carries h relatively, |g| h more against |S u|, at most 1.13 h:
// 23.0 h (erf), 16.7 h (tanh), 8.8 h (silu), all below 32 h: the same eps against |S u|.
constexpr int DACT_EPS_LOG2 = -19;
constexpr float DACT_EPS = 0x1p-19f;
constexpr float DACT_SILU_CLAMP = 128.0f;

template <int ACT>
HGEMM_ACT_HD float dact_apply(float z) {
  HGEMM_ACT_NO_CONTRACT
  static_assert(ACT == ACT_RELU || ACT == ACT_GELU || ACT == ACT_GELU_TANH || ACT == ACT_SILU, "relu, gelu (erf), gelu (tanh), silu");
  if (ACT == ACT_RELU) {
    return (z <= 0.0f) ? 0.0f : 1.0f;
  } else if (ACT == ACT_GELU) {
    const float zc = z > 16.0f ? 16.0f : (z < -16.0f ? -16.0f : z);   // (a NaN fails both and stays)
    const float t = 1.0f + erff(zc * 0.70710678118654752440f);        // in [0, 2]
    const float e = expf(-0.5f * (zc * zc));                          // 0 from |zc| = 13.3 on
    return fmaf(zc * 0.39894228040143267794f, e, 0.5f * t);           // 1 / sqrt(2 pi)
  } else if (ACT == ACT_SILU) {
    float a = z < 0.0f ? -z : z;
    a = a > DACT_SILU_CLAMP ? DACT_SILU_CLAMP : a;                    // (a NaN fails the test and stays)
    const float e = expf(-a);                                         // in [0, 1], exactly 0 at the clamp
    const float sp = 1.0f / (1.0f + e);                               // s(a) in [1/2, 1]
    const float sm = e * sp;                                          // s(-a) = 1 - s(a)
    const float t = a * (sp * sm);                                    // |z| s (1 - s) >= 0
    return z < 0.0f ? sm - t : sp + t;
  } else {
    float a = z < 0.0f ? -z : z;
    a = a > 16.0f ? 16.0f : a;
    const float a2 = a * a;
    const float inner = fmaf(0.044715f, a2 * a, a);                   // a + 0.044715 a^3
    const float e = expf(-1.5957691216057307117f * inner);            // exp(-2u(a)) in [0, 1]
    const float sp = 1.0f / (1.0f + e);                               // s(a) in [1/2, 1]
    const float sm = e * sp;                                          // s(-a) = 1 - s(a)
    const float du2 = 1.5957691216057307117f * fmaf(0.134145f, a2, 1.0f);   // 2u'
    const float t = (a * (sp * sm)) * du2;                            // |z| s (1 - s) 2u' >= 0
    return z < 0.0f ? sm - t : sp + t;
  }
}

// S x act'(z) as the dact calls round it: one fp32 multiply on the finished sum; ReLU a select (the result is S or +0.0f, bit for bit)
template <int ACT>
HGEMM_ACT_HD float dact_mul(float s, float z) {
  HGEMM_ACT_NO_CONTRACT
  if (ACT == ACT_RELU) return (z <= 0.0f) ? 0.0f : s;
  return s * dact_apply<ACT>(z);
}

}  // namespace hgemm_mi355x
