// The gated MLP's input gradient (bgemm_mi355x_nn_dgated): with S = dY Wd the finished fp32 sum and gf, uf the saved bf16 pre-activations
// of the gate and the up half as floats,
//   du[m][n] = bf16(fl32(act32(gf) S))                       the gradient of the up half
//   dg[m][n] = bf16(dact_mul<act>(fl32(S uf), gf))           the gradient of the gate half: S u act'(g), ReLU a select
// ONE text, dgated_store, for family n's epilogue (hgemm_kernel_nn.hpp), the combine and the reference kernel (hgemm_registry.hip: OutDgated)
// and a CPU program (tests/test_nn_dgated_host.py builds one with the host compiler).  act_apply, dact_apply and dact_mul are hgemm_act.hpp's;
// no HIP construct besides its two function attributes.  Nothing is applied to a slab, each output is rounded once, and no bf16 dH = S exists.
//
// The bars (derived, not measured), fp64 values on the given S, gf, uf, for every element with a finite S; h = 2^-24:
//   du: act32(gf) is within DGATED_ACT_EPS |gf| of act*(gf) (hgemm_gated.hpp's count: both GELUs by erff's 16 ulp allowance, SiLU 2^-22,
//       ReLU exact), the product adds h |y*| and h times that error, which the doubled last term absorbs:
//         |du - act*(gf) S| <= 1/2 ulp_bf16(.) + DGATED_ACT_EPS |gf| |S| + DGATED_MUL_EPS |.|        (the gated forward's bar with u := S)
//   dg: v = fl32(S uf) carries h relatively; hgemm_act.hpp counts act'32 and the second product with it, 23.0 h (erf), 16.7 h (tanh) and
//       8.8 h (silu) of 32 h, absolute against |S uf|:
//         |dg - S uf act'*(gf)| <= 1/2 ulp_bf16(.) + DGATED_DACT_EPS |S uf|
//   ReLU is defined bit for bit for both outputs: du = bf16(fl32(relu(gf) S)), dg = bf16(gf <= 0 ? +0 : fl32(S uf)).
#pragma once

#include "hgemm_act.hpp"

namespace hgemm_mi355x {

constexpr int DGATED_ACT_EPS_LOG2 = -19, DGATED_MUL_EPS_LOG2 = -23, DGATED_DACT_EPS_LOG2 = DACT_EPS_LOG2;
static_assert(DGATED_DACT_EPS_LOG2 == -19, "the dact calls' eps, with the product S u counted in (hgemm_act.hpp)");

struct DgatedPair { float dg, du; };

// the two fp32 values of one element, each rounded to bf16 once by the caller
template <int ACT>
HGEMM_ACT_HD DgatedPair dgated_store(float s, float gf, float uf) {
  HGEMM_ACT_NO_CONTRACT
  DgatedPair o;
  o.du = act_apply<ACT>(gf) * s;
  o.dg = dact_mul<ACT>(s * uf, gf);
  return o;
}

}  // namespace hgemm_mi355x
