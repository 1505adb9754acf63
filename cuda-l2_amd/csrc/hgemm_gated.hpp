// The gated forward product (bgemm_mi355x_tn_gated): C = bf16(act(X Wg^T + bg) * (X Wu^T + bu)).  The index arithmetic of family f's gated
// kernel, the arrangement of its two-pass slabs and the bar of the call, ONE text for the kernel (hgemm_kernel_tn_gated.hpp), the combine
// and the reference kernel (hgemm_registry.hip) and a CPU program (tests/test_tn_gated_host.py builds one with the host compiler and walks
// every lane of every member).  No HIP construct besides the two function attributes, which are empty for a host compiler.
//
// The tile.  A member (BM, BN, WM x WN waves, wave tile TM x TN, FN = TN / 16 column fragments) computes BM rows by BN / 2 OUTPUT columns:
// the B image keeps its BN rows, and inside each wave's TN rows the fragments j < FN / 2 are rows of Wg and the fragments j >= FN / 2 the
// SAME output rows of Wu.  Image row R = wave_n TN + 16 j + r holds
//   gated_is_up(TN, R)        = (R % TN) >= TN / 2                       which weight
//   gated_out_col(TN, R)      = (R / TN) (TN / 2) + (R % TN) % (TN / 2)  which output column of the tile (row n0 + that of the weight)
// A DMA piece is 8 image rows and TN / 2 is 16 or 32, so a piece is wholly gate or wholly up.  tr_mfma leaves lane L with
// acc[i][j][e] = (row dbias_row, image column wave_n TN + 16 j + 4 (L >> 4) + e), so acc[i][jo] and acc[i][jo + FN / 2] of one lane are
// the gate and the up sum of output column gated_lane_col(wave_n, TN, jo, L, e): the gate is an in-register multiply.
//
// The slab of a two-pass plan: [splits][M][2 N] fp32, row m of split s holding its N gate sums and behind them its N up sums --
// gated_slab_index.  That is the slab a plain TN product of width 2 N on the stacked weight [Wg; Wu] writes, so the workspace is that
// product's.  The combine adds the two columns of an output over the splits in split order and applies bias, activation and gate once.
//
// The bar (derived, not measured).  With h = 2^-24, g and u the exactly known fp32 pre-activations and y* = act*(g) u in fp64:
//   act32(g) is within 2^-19 |g| of act*(g): both GELUs by the forward call's allowance (erff within 16 ulp), SiLU by expf within 1 ulp,
//   one add and one correctly rounded division, 4 h |silu(g)| <= 2^-22 |g|; ReLU is exact.  The fp32 product adds h |y*| (and h times
//   the error above, which the doubled last term absorbs), the bf16 rounding 1/2 ulp_bf16:
//     |C - y*| <= 1/2 ulp_bf16(y*) + GATED_ACT_EPS |g| |u| + GATED_MUL_EPS |y*|,   GATED_ACT_EPS = 2^-19, GATED_MUL_EPS = 2^-23.
//   ReLU is held bit for bit against bf16_rne(fl32(relu(g) u)).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGEMM_GATED_HD __host__ __device__ inline
#else
#define HGEMM_GATED_HD inline
#endif
#if defined(__clang__)
#define HGEMM_GATED_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HGEMM_GATED_NO_CONTRACT
#endif

namespace hgemm_mi355x {

constexpr int GATED_ACT_EPS_LOG2 = -19, GATED_MUL_EPS_LOG2 = -23;
constexpr double GATED_ACT_EPS = 0x1p-19, GATED_MUL_EPS = 0x1p-23;

HGEMM_GATED_HD constexpr bool gated_is_up(int tn, int image_row) { return (image_row % tn) >= tn / 2; }
HGEMM_GATED_HD constexpr int gated_out_col(int tn, int image_row) { return (image_row / tn) * (tn / 2) + (image_row % tn) % (tn / 2); }
// The weight row (counted from the tile's first row n0 of ITS weight) that image row `image_row` is loaded from, rows_valid = N - n0 rows of
// each weight lying at or behind n0: clamped to the last valid one PER WEIGHT.  The kernel's DMA source row; without the clamp the gate rows
// of a ragged last tile of a fused [2 N][K] weight would be Wu's first rows, and those of separate weights rows behind Wg's end.
HGEMM_GATED_HD constexpr int gated_source_row(int tn, int image_row, int rows_valid) {
  return gated_out_col(tn, image_row) < rows_valid - 1 ? gated_out_col(tn, image_row) : rows_valid - 1;
}
// output column (inside the tile) of element e of output fragment jo of lane L
HGEMM_GATED_HD constexpr int gated_lane_col(int wave_n, int tn, int jo, int lane, int e) { return wave_n * (tn / 2) + 16 * jo + 4 * (lane >> 4) + e; }
// the image row whose sums that lane holds in acc[.][j][e] (the MFMA's B row of C column 16 j + 4 (L >> 4) + e)
HGEMM_GATED_HD constexpr int gated_lane_image_row(int wave_n, int tn, int j, int lane, int e) { return wave_n * tn + 16 * j + 4 * (lane >> 4) + e; }
// element (m, n) of half `up` (0: gate, 1: up) in the slab of split s
HGEMM_GATED_HD constexpr unsigned long long gated_slab_index(int M, int N, int s, int m, int n, int up) {
  return ((unsigned long long)s * (unsigned long long)M + (unsigned long long)m) * (2ull * (unsigned long long)N) + (unsigned long long)up * (unsigned long long)N +
         (unsigned long long)n;
}

// the one product of the call, on the two finished fp32 values: a = act32(g)
HGEMM_GATED_HD float gated_mul(float a, float u) {
  HGEMM_GATED_NO_CONTRACT
  return a * u;
}


// the view of a member that hgemm_tr_store_c16.inc sees in the gated kernels: the wave tile's OUTPUT columns
template <class MEMBER>
struct GatedOutView {
  static constexpr int TM = MEMBER::TM, TN = MEMBER::TN / 2;
};
// acc[i][J0 + j] under the name acc[i][j]: what that text sees of the up half of the accumulators (V: the lane's quad type; the indices are
// constants after unrolling, so on the device this is a renaming of registers)
template <class V, int FM, int FN_ALL, int J0>
struct GatedFragView {
  V (&a)[FM][FN_ALL];
  HGEMM_GATED_HD const V* operator[](int i) const { return &a[i][J0]; }
};

// bgemm_mi355x_tn_gated_aux: the fp32 pre-activation of one half, the finished sum plus its bias as ONE fp32 add -- the value that g_out /
// u_out round to bf16 (round to nearest even, the conversion to __bf16, once) and that the activation and the gate read UNROUNDED.  The
// text of the kernel's in-place add, of the combine's and the reference kernel's policy and of the CPU programs.
HGEMM_GATED_HD float gated_pre(float sum, float bias) {
  HGEMM_GATED_NO_CONTRACT
  return sum + bias;
}

}  // namespace hgemm_mi355x
