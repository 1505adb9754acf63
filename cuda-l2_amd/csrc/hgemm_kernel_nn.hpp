// Family "n": NN operand form -- C[M,N] = A[M,K] * B[K,N] with B ROW-MAJOR as the caller holds it ([K][ldb], N contiguous), for the
// caller whose B is an activation and not a pre-transposed weight.  Replaces, for a b-only call, the one-output-per-thread
// reference kernel (hgemm_generic_kernel); the vendor baselines have the form as hgemm_rocblas_nn / hgemm_hipblaslt_*_nn
// (reference cublas/fp32/hgemm_cublas.cu:15-41).
//
// The classic family's structure (hgemm_kernel.hpp): NBUF-deep LDS ring of K = 64 stages, ONE barrier per stage, counted vmcnt,
// LDS-DMA fills, v_mfma_f32_16x16x32_f16 with fp32 accumulation, operands swapped so that a lane owns 4 consecutive N of a C row.
//   * A image: unchanged -- [BM rows][128 B], 16-byte chunk c of row r at slot c ^ ((r >> 1) & 7), fragments by ds_read_b128.
//   * B image: [64 k-rows][BN halfs], row-major as B lies in memory.  A k-row of the tile is BN * 2 contiguous bytes, so a 1-KiB
//     DMA piece is 512 / BN whole k-rows and every wave instruction reads whole 128- / 256-byte lines.
//   * The MFMA operand of lane (n = lane & 15, kq = lane >> 4) is k = 8 kq .. 8 kq + 7 of column n: a COLUMN of the image.  It
//     comes from two ds_read_b64_tr_b16, each of which hands a 16-lane group a 4-row x 16-column block transposed: lane 4q + p of
//     the group supplies the address of block row q, columns 4p .. 4p + 3, and lane i receives column i with row q in element q.
//     The two reads take rows 8 kq .. 8 kq + 3 and 8 kq + 4 .. 8 kq + 7 of the K = 32 slice.
//   * Swizzle (nn_swz): a permutation of the 16-byte chunks inside a k-row, applied to the per-lane SOURCE address of the DMA (the
//     destination is lane-linear; inside one row, so coalescing stays) and undone on the read.  A 32-lane half of a transposed read
//     touches 8 rows x 32 bytes (rows 8g + 4h + q, g = two adjacent groups): unswizzled they share banks 8-way (256-byte rows) /
//     4-way (128-byte rows); swizzled they tile the 256-byte bank row exactly (tests/nn_layout_model.py replays both maps).
//     The XOR may swap the two 8-byte halves of a lane pair's 32 bytes, so every lane address is computed from (row, chunk).
//   * Two hardware rules of the transposed read, each giving wrong data without a fault: every lane address is 8-byte aligned
//     (all offsets below are multiples of 8 from a 1024-aligned array), and EXEC is all ones at every read -- there is no
//     lane-dependent branch or early return in front of the K loop; out-of-tile lanes read in-bounds LDS and their products land
//     in accumulators that are never stored.
//   * Edges: M rows clamped on load (classic).  N: a chunk at columns >= N reads whatever follows in memory -- the next row, or
//     zeros behind the end of the matrix, where the B descriptor ends -- and only feeds accumulators of columns >= N; stores are
//     predicated.  Scope (the host sends anything else to the reference kernel): K % 64 == 0, N % 8 == 0, lda / ldb / ldc
//     multiples of 8, 16-byte aligned pointers, operands within 2 GiB of 32-bit offsets.
//   * Epilogues: fp16 C (plain and non-temporal) and the two-pass split-K slab (hgemm_splitk_reduce_kernel combines).
//   * One text for families n, a and f (hgemm_kernel_ta.hpp, hgemm_kernel_tn.hpp): the 16-bit C epilogue (hgemm_tr_store_c16.inc,
//     included by the three kernels) and, for n and a, the accumulator zeroing (tr_zero).  The bar: every kernel's instruction stream,
//     register counts, LDS and scratch as they were.  The preamble, the ring and the operand images did not meet it in
//     any form tried and stay in each kernel, on purpose; an edit to one of them is made in all three.
// This header includes ITSELF: the device text of the family's kernel stands at the end of the file, behind the include guard, under
// HGEMM_NN_KERNEL_TEXT, and each of the two entry points (hgemm_nn_kernel, hgemm_nn_dgated_kernel) includes the file once more with that
// macro set -- the guard skips everything but the text.  Hence a guard and no `#pragma once`.
#ifndef HGEMM_KERNEL_NN_HPP
#define HGEMM_KERNEL_NN_HPP

#include "hgemm_act.hpp"
#include "hgemm_dbias.hpp"
#include "hgemm_dgated.hpp"
#include "hgemm_launch.hpp"
#include "hgemm_residual.hpp"

namespace hgemm_mi355x {

// chunk XOR of k-row `krow` of the B image (see above); BN = 128: the dual-use image of 256-byte rows, BN = 64: two k-rows per
// 256-byte bank row, the pair index takes bit 1 and bit 3 of the row
template <int BN>
__host__ __device__ constexpr int nn_swz(int krow) {
  return BN == 128 ? (((krow & 3) << 2) | ((krow >> 2) & 3)) : ((((krow >> 1) & 1) | (((krow >> 3) & 1) << 1)) << 1);
}

// ---- what the transposed-read families share (family a, hgemm_kernel_ta.hpp, builds on this header) ----------------------------
// The Cfg of both: the wave tiling, the B image and the ring.  A_BYTES is the family's A image of one stage; whatever it looks like, it
// is filled in 1-KiB DMA pieces, A_BYTES / 1024 of them.
template <int BM_, int BN_, int WM_, int WN_, int NBUF_, int A_BYTES_>
struct CfgTR {
  using elem = f16;   // the operands' and the 16-bit C's element; the bf16 Cfgs (CfgNNB below, CfgTAB) name __bf16
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, MI = 16, NBUF = NBUF_;
  static constexpr int NW          = WM * WN;
  static constexpr int THREADS     = NW * 64;
  static constexpr int TM          = BM / WM;
  static constexpr int TN          = BN / WN;
  static constexpr int FM          = TM / 16;
  static constexpr int FN          = TN / 16;
  static constexpr int A_BYTES     = A_BYTES_;
  static constexpr int B_ROW_BYTES = BN * 2;               // one k-row of the B image
  static constexpr int B_BYTES     = BK * B_ROW_BYTES;
  static constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  static constexpr int LDS_BYTES   = STAGE_BYTES * NBUF;
  static constexpr int B_CH        = BN / 8;               // 16-byte chunks per k-row
  static constexpr int B_RPP       = 64 / B_CH;            // k-rows per 1-KiB DMA piece
  static constexpr int NI_A        = A_BYTES / 1024;       // DMA pieces of the A tile (BM / 8) ...
  static constexpr int NI_B        = B_BYTES / 1024;       // ... and of the B tile (BN / 8)
  static constexpr int NJ_A        = NI_A / NW;            // pieces per wave: piece wave + j * NW, the first NJ_A of them are A's
  static constexpr int NJ          = (NI_A + NI_B) / NW;
  static_assert(BN == 64 || BN == 128, "nn_swz is defined for 128- and 256-byte k-rows");
  static_assert(BM % (WM * 16) == 0 && BN % (WN * 16) == 0 && FN % 2 == 0, "wave tile: MFMA-aligned, an even number of column tiles");
  static_assert(NI_A % NW == 0 && NI_B % NW == 0, "every wave owns the same number of A and of B pieces (counted vmcnt)");
  static_assert(NBUF >= 2 && LDS_BYTES <= 160 * 1024, "LDS budget");
};

// the vector a transposed read returns, in LDS
using tr_t = __attribute__((ext_vector_type(4))) short;
typedef __attribute__((address_space(3))) tr_t lds_tr_t;

template <class CFG, int EPI>
__global__ void hgemm_nn_kernel(const GemmArgs g);

// EPI_C16_DACT + ACT_* (hgemm_act.hpp): the bf16 C through the activation's derivative at a saved pre-activation (bgemm_mi355x_nn_dact);
// the CfgNNB members only.
constexpr bool epi_is_dact(int epi) { return epi > EPI_C16_DACT && epi <= EPI_C16_DACT + ACT_GELU_TANH; }
// EPI_C16_DACT_DBIAS + ACT_*: the same C and the tile's column sums (bgemm_mi355x_nn_dact_dbias)
constexpr bool epi_is_dbias(int epi) { return epi > EPI_C16_DACT_DBIAS && epi <= EPI_C16_DACT_DBIAS + ACT_GELU_TANH; }
constexpr int epi_dact(int epi) { return epi_is_dact(epi) ? epi - EPI_C16_DACT : epi_is_dbias(epi) ? epi - EPI_C16_DACT_DBIAS : ACT_NONE; }
// EPI_C16_DGATED + ACT_* (ACT_SILU included): the gated MLP's input gradient, two saved pre-activations in and two bf16 matrices out
// (bgemm_mi355x_nn_dgated, hgemm_dgated.hpp); the CfgNNB members only, through hgemm_nn_dgated_kernel below.
constexpr bool epi_is_dgated(int epi) { return epi > EPI_C16_DGATED && epi <= EPI_C16_DGATED + ACT_SILU; }
constexpr int epi_dgated(int epi) { return epi_is_dgated(epi) ? epi - EPI_C16_DGATED : ACT_NONE; }
// The byte range of the Z descriptor of the tile whose first row is m0: from that row to Z's last valid element (M - 1, N - 1), computed in
// 64 bits and CLAMPED to the descriptor's 32: M is not limited by the host, only a tile's reach is, so a Z of 4 GiB and more is in scope
// and the distance to its end need not fit.  Where the clamp acts, the matrix goes on for more than 4 GiB behind the tile's first row
// while the tile's own offsets stay below (BM ldz + N) 2 + 2 BN < 2^32 (host check: the first term below 2 GiB) -- every row of such a
// tile is a valid row and the range covers all of them; where it does not act, the range ends at the last valid element exactly.
// (hgemm_api.hip shows it to the CPU tests.)
__host__ __device__ constexpr uint32_t dact_z_range_bytes(int M, int N, int ldz, int m0) {
  const unsigned long long bytes = ((unsigned long long)(M - 1 - m0) * (unsigned long long)ldz + (unsigned long long)N) * 2ull;
  return bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bytes;
}
static_assert(dact_z_range_bytes(262144, 8192, 8192, 0) == 0xFFFFFFFFu && dact_z_range_bytes(262144, 8192, 8192, 262016) == (127u * 8192u + 8192u) * 2u &&
              dact_z_range_bytes(1, 8, 8, 0) == 16u, "a range of 2^32 bytes and more is clamped, not wrapped");

// family n: the classic A image, [BM rows][128 B]
template <int BM_, int BN_, int WM_, int WN_, int NBUF_>
struct CfgNN : CfgTR<BM_, BN_, WM_, WN_, NBUF_, BM_ * ROW_BYTES> {
  template <int EPI>
  static constexpr auto kernel() { return &hgemm_nn_kernel<CfgNN, EPI>; }   // the family's entry point (launch_tr)
};

// bfloat16 operands and 16-bit C (bgemm_mi355x_nn, hgemm_inst_g8.hip): the same images, DMA pieces, counts and ring -- elements are 2
// bytes either way and the transposed read does not look into them.  CFG::elem selects, in the kernel text below, the fragment type,
// v_mfma_f32_16x16x32_bf16 and the epilogue's convert (v_cvt_pk_bf16_f32: round to nearest even, once); nothing else asks for it.  A
// Cfg of its own, so that CfgNN's kernels keep their symbols and, as compiled, their instruction streams.
template <int BM_, int BN_, int WM_, int WN_, int NBUF_>
struct CfgNNB : CfgTR<BM_, BN_, WM_, WN_, NBUF_, BM_ * ROW_BYTES> {
  using elem = __bf16;
  template <int EPI>
  static constexpr auto kernel() { return &hgemm_nn_kernel<CfgNNB, EPI>; }
};

// the K = 32 MFMA of the element type: fp32 accumulation, eight-element fragments, the same rate for both
template <class V>
__device__ __forceinline__ f32x4 tr_mfma(V b, V a, f32x4 c) {
  if constexpr (__is_same(V, f16x8)) return __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, c, 0, 0, 0);
  else                               return __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, c, 0, 0, 0);
}

// the sum over the 16 lanes L & 15 in every one of them: hgemm_dbias.hpp's butterfly, four DPP moves and four adds
template <int CTRL>
__device__ __forceinline__ float dbias_dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float dbias_row16_sum(float v) {
  v = dbias_dpp_add<DBIAS_DPP_QUAD_XOR1>(v);
  v = dbias_dpp_add<DBIAS_DPP_QUAD_XOR2>(v);
  v = dbias_dpp_add<DBIAS_DPP_HALF_MIRROR>(v);
  return dbias_dpp_add<DBIAS_DPP_ROW_MIRROR>(v);
}

// accumulators of a wave tile, zeroed (families n and a; family f keeps the loop in place, see there)
template <int FM, int FN>
__device__ __forceinline__ void tr_zero(f32x4 (&acc)[FM][FN]) {
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;
}

// What a dgated kernel is handed: the launch's GemmArgs -- A = dY, Bt = Wd, C = dG, counters = G, tail_first = ldz, as a dact launch carries
// its Z -- and behind it the second input and the second output, the way GatedArgs (below) carries a second weight.  GemmArgs itself keeps its
// size and every kernarg offset.  nn_dgated_u / _du: what the kernel text reads them through; the GemmArgs overloads are never called (the
// text names them under `if constexpr (epi_is_dgated(EPI))` alone) and let the one text compile for both entry points.
struct DgatedArgs : GemmArgs {
  const __bf16* U;
  __bf16* dU;
};
__device__ __forceinline__ const __bf16* nn_dgated_u(const GemmArgs&) { return nullptr; }
__device__ __forceinline__ __bf16* nn_dgated_du(const GemmArgs&) { return nullptr; }
__device__ __forceinline__ const __bf16* nn_dgated_u(const DgatedArgs& g) { return g.U; }
__device__ __forceinline__ __bf16* nn_dgated_du(const DgatedArgs& g) { return g.dU; }

// GemmArgs as the kernel reads it: Bt = the ROW-MAJOR B ([K][ldb]), ldb >= N its row stride; tail_tiles = 0, counters = nullptr.
template <class CFG, int EPI>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_nn_kernel(const GemmArgs g) {
  prefetch_kernargs<sizeof(GemmArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
#define HGEMM_NN_KERNEL_TEXT
#include "hgemm_kernel_nn.hpp"   // the kernel text at the end of this file
#undef HGEMM_NN_KERNEL_TEXT
#endif  // __HIP_DEVICE_COMPILE__
}
// the same text behind a DgatedArgs: the EPI_C16_DGATED + ACT kernels (hgemm_inst_g19.hip)
template <class CFG, int EPI>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_nn_dgated_kernel(const DgatedArgs g) {
  static_assert(epi_is_dgated(EPI), "the dgated epilogues alone");
  prefetch_kernargs<sizeof(DgatedArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
#define HGEMM_NN_KERNEL_TEXT
#include "hgemm_kernel_nn.hpp"   // the kernel text at the end of this file
#undef HGEMM_NN_KERNEL_TEXT
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- host side of both transposed-read families (family a builds on it) -----------------------------------------------------------
// A kernel set is one (element, output) of a layout: CfgNN / CfgNNB / CfgTA / CfgTAB, with a 16-bit C or -- C32 -- the fp32 C.  Each
// set is instantiated in a unit of its own (hgemm_inst_g5.hip .. g10.hip).
//
// The one launcher: member CFG's kernel of epilogue `epi`.  The 16-bit set has the EPI_C16 and EPI_SLAB kernels.  The fp32-C set has
// the EPI_C32 kernel alone: the K slices of its two-pass form are the 16-bit set's EPI_SLAB kernels (slabs are fp32 either way), reached
// through that set's launcher in its own unit -- the extern declarations below keep it from being instantiated a second time.
template <class CFG, bool C32>
void launch_tr(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if constexpr (C32) {
    if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
    HGEMM_LAUNCH((CFG::template kernel<EPI_C32>()), grid, CFG::THREADS, stream, ts, g);
  } else if (epi == EPI_SLAB) {
    HGEMM_LAUNCH((CFG::template kernel<EPI_SLAB>()), grid, CFG::THREADS, stream, ts, g);
  } else {
    HGEMM_LAUNCH((CFG::template kernel<EPI_C16>()), grid, CFG::THREADS, stream, ts, g);
  }
}
using TrLaunch = void (*)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
// What a launcher of the gated sets (hgemm_kernel_tn_gated.hpp) is handed through that signature: the launch's GemmArgs (A = X, Bt = Wg,
// C, partial = the slabs, N = the OUTPUT width, tiles_n = ceil(N / (BN / 2))) and behind it the second weight and the two bias vectors
// (either may be null).  tr_launch (hgemm_api.hip) builds one and passes it as its base; the launcher casts back.  GemmArgs itself keeps
// its size and every kernarg offset.
struct GatedArgs : GemmArgs {
  const __bf16* Bu;
  const __bf16* bias_g;
  const __bf16* bias_u;
};
// The same for the sets that also write the pre-activations (bgemm_mi355x_tn_gated_aux): behind the GatedArgs the two more bf16 outputs
// and their one row stride.  GatedArgs keeps its size and every kernarg offset too; the slab launcher of those sets reads the GatedArgs in it.
struct GatedAuxArgs : GatedArgs {
  __bf16* G;
  __bf16* U;
  int ldz;
};
// What the combine and the reference kernel of those sets are handed as `z` (TrKernels below has no slot for a third output): the address
// of this pair on the HOST, read by the policy's make() in front of the launch; the pointers travel to the device inside the policy.
struct GatedAuxOut {
  void* g_out;
  void* u_out;
};

// The members of both families, smallest tile first, and what is made of them: X(args ..., BM, BN, WM, WN, NBUF) per member.
//   HGEMM_TR_INST(CFG, C32)    a unit's one line: the explicit instantiation of a kernel set's launchers, and with them its kernels
//   HGEMM_TR_EXTERN(CFG, C32)  everyone else's view of the set: no unit but the set's own instantiates a launcher or a kernel
//   HGEMM_TR_ENTRY(P, CFG)     the member's geometry row, named P<BM>x<BN>_w<WM>x<WN>
#define HGEMM_TR_MEMBERS(X, ...) \
  X(__VA_ARGS__, 64, 64, 2, 2, 4) X(__VA_ARGS__, 128, 64, 2, 2, 3) X(__VA_ARGS__, 64, 128, 2, 2, 3) X(__VA_ARGS__, 128, 128, 2, 2, 3)
#define HGEMM_TR_LAUNCHER(CFG, C32, BM, BN, WM, WN, NB) launch_tr<CFG<BM, BN, WM, WN, NB>, C32>
#define HGEMM_TR_INST(...) template void HGEMM_TR_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_TR_EXTERN(...) extern HGEMM_TR_INST(__VA_ARGS__)
#define HGEMM_TR_ENTRY(P, CFG, BM, BN, WM, WN, NB) \
  {P #BM "x" #BN "_w" #WM "x" #WN, BM, BN, WM, WN, NB, CFG<BM, BN, WM, WN, NB>::THREADS, CFG<BM, BN, WM, WN, NB>::LDS_BYTES}

HGEMM_TR_MEMBERS(HGEMM_TR_EXTERN, CfgNN, false)    // hgemm_inst_g5.hip
HGEMM_TR_MEMBERS(HGEMM_TR_EXTERN, CfgNNB, false)   // hgemm_inst_g8.hip

// The dact sets (bgemm_mi355x_nn_dact), one per activation: the member's EPI_C16_DACT + ACT kernel alone; the K slices of a two-pass
// form are the bf16 16-bit set's EPI_SLAB kernels, reached through that set's launcher in its own unit.  g.counters of the dact dispatch
// is Z, g.tail_first its row stride (tr_launch, hgemm_api.hip).
template <class CFG, int ACT>
void launch_nn_dact(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((CFG::template kernel<EPI_C16_DACT + ACT>()), grid, CFG::THREADS, stream, ts, g);
}
#define HGEMM_NN_DACT_LAUNCHER(ACT, CFG, BM, BN, WM, WN, NB) launch_nn_dact<CFG<BM, BN, WM, WN, NB>, ACT>
#define HGEMM_NN_DACT_INST(...) template void HGEMM_NN_DACT_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_NN_DACT_EXTERN(...) extern HGEMM_NN_DACT_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_NN_DACT_EXTERN, ACT_RELU, CfgNNB)        // hgemm_inst_g16.hip
HGEMM_TR_MEMBERS(HGEMM_NN_DACT_EXTERN, ACT_GELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DACT_EXTERN, ACT_GELU_TANH, CfgNNB)

// The dact + dbias sets (bgemm_mi355x_nn_dact_dbias): the member's EPI_C16_DACT_DBIAS + ACT kernel alone -- g.partial of its dispatch is
// P[tiles_m][N] --; a dispatch with the plain dact id (the call without a workspace) and the K slices of a two-pass form go to the dact
// set's launcher in its own unit.
template <class CFG, int ACT>
void launch_nn_dbias(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi != EPI_C16_DACT_DBIAS + ACT) return launch_nn_dact<CFG, ACT>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((CFG::template kernel<EPI_C16_DACT_DBIAS + ACT>()), grid, CFG::THREADS, stream, ts, g);
}
#define HGEMM_NN_DBIAS_LAUNCHER(ACT, CFG, BM, BN, WM, WN, NB) launch_nn_dbias<CFG<BM, BN, WM, WN, NB>, ACT>
#define HGEMM_NN_DBIAS_INST(...) template void HGEMM_NN_DBIAS_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_NN_DBIAS_EXTERN(...) extern HGEMM_NN_DBIAS_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_NN_DBIAS_EXTERN, ACT_RELU, CfgNNB)       // hgemm_inst_g17.hip
HGEMM_TR_MEMBERS(HGEMM_NN_DBIAS_EXTERN, ACT_GELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DBIAS_EXTERN, ACT_GELU_TANH, CfgNNB)

// The dgated sets (bgemm_mi355x_nn_dgated), one per activation: the member's EPI_C16_DGATED + ACT kernel alone, handed a DgatedArgs as its
// GemmArgs base (tr_launch, hgemm_api.hip); the K slices of a two-pass form are the bf16 16-bit set's EPI_SLAB kernels, which read the base.
template <class CFG, int ACT>
void launch_nn_dgated(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((hgemm_nn_dgated_kernel<CFG, EPI_C16_DGATED + ACT>), grid, CFG::THREADS, stream, ts, static_cast<const DgatedArgs&>(g));
}
#define HGEMM_NN_DGATED_LAUNCHER(ACT, CFG, BM, BN, WM, WN, NB) launch_nn_dgated<CFG<BM, BN, WM, WN, NB>, ACT>
#define HGEMM_NN_DGATED_INST(...) template void HGEMM_NN_DGATED_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_NN_DGATED_EXTERN(...) extern HGEMM_NN_DGATED_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_EXTERN, ACT_RELU, CfgNNB)      // hgemm_inst_g19.hip
HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_EXTERN, ACT_GELU, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_EXTERN, ACT_GELU_TANH, CfgNNB)
HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_EXTERN, ACT_SILU, CfgNNB)

// The residual set (bgemm_mi355x_nn_add): the member's EPI_C16_ADD kernel alone; the K slices of a two-pass form are the bf16 16-bit set's
// EPI_SLAB kernels.  g.counters of the dispatch is r, g.tail_first its row stride, as a dact dispatch carries z (tr_launch, hgemm_api.hip).
template <class CFG>
void launch_nn_add(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((CFG::template kernel<EPI_C16_ADD>()), grid, CFG::THREADS, stream, ts, g);
}
#define HGEMM_NN_ADD_LAUNCHER(CFG, BM, BN, WM, WN, NB) launch_nn_add<CFG<BM, BN, WM, WN, NB>>
#define HGEMM_NN_ADD_INST(...) template void HGEMM_NN_ADD_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_NN_ADD_EXTERN(...) extern HGEMM_NN_ADD_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_NN_ADD_EXTERN, CfgNNB)                   // hgemm_inst_g22.hip

// A layout's table (hgemm_registry.hip builds both, each by one expansion of the member list: a config id is a position in `rows`; the
// geometry table of hgemm_configs*.def does not know these families).  A row is the member's geometry and its launcher in every kernel
// set of the layout; TrKernels is what a set has besides: the combine of the two-pass form and the reference kernel (status 0, exact:
// answers whatever is outside the kernels' scope or reach).  All sets share the signatures; a set with a 16-bit C is handed
// accumulate = false and ignores it.  A set the layout does not have (NN with an fp32 C, NN / TA with a fused bias) is empty: null
// launchers, TrKernels{}.
struct TrEntry {
  const char* name;
  int bm, bn, wm, wn, nbuf, threads, lds_bytes;
};
enum TrElem { TR_F16 = 0, TR_BF16 = 1 };   // what the operands and a 16-bit C hold: 2 bytes either way
// The output kinds of a layout: a 16-bit C, an fp32 C (family a), a 16-bit C with a fused bias (family f: bgemm_mi355x_tn_bias).
// TR_C16_BIAS + a (a = 1, 2, 3: hgemm_act.hpp's ACT_RELU / _GELU / _GELU_TANH): the bias followed by that activation (bgemm_mi355x_tn_bias_act).
// TR_C16_BIAS_AUX + a: the same with the rounded pre-activation as a second output (bgemm_mi355x_tn_bias_act_aux).  TR_C16_DACT + a: a
// 16-bit C through that activation's derivative at a saved pre-activation (family n: bgemm_mi355x_nn_dact).
enum TrKind { TR_C16 = 0, TR_C32 = 1, TR_C16_BIAS = 2, TR_C16_BIAS_RELU = 3, TR_C16_BIAS_GELU = 4, TR_C16_BIAS_GELU_TANH = 5,
              TR_C16_BIAS_AUX = 5, TR_C16_DACT = 8, TR_C16_DACT_DBIAS = 11, TR_KINDS = 15,   // TR_C16_DACT_DBIAS + a: dact with the bias gradient
              // TR_C16_GATED + a (a = 1 .. 4, ACT_SILU included): the gated product (family f: bgemm_mi355x_tn_gated).  TR_KINDS keeps counting
              // the kinds with one sum per output; the tables hold TR_KINDS_ALL cells.
              // TR_C16_DGATED + a (a = 1 .. 4): the gated MLP's input gradient (family n: bgemm_mi355x_nn_dgated), one sum, two outputs.
              // TR_C16_GATED_AUX + a (a = 1 .. 4): the gated product with the rounded pre-activations as two more outputs (family f:
              // bgemm_mi355x_tn_gated_aux), two sums, three outputs.
              // TR_C16_BIAS_ADD: the fused bias (may be null) and residual matrix (family f: bgemm_mi355x_tn_bias_add).  TR_C16_ADD: the fused
              // residual matrix (family n: bgemm_mi355x_nn_add).  One sum, one output, no activation; `z` is the read-only r, which may be c.
              TR_C16_GATED = 14, TR_C16_DGATED = 18, TR_C16_GATED_AUX = 22, TR_C16_BIAS_ADD = 27, TR_C16_ADD = 28, TR_KINDS_ALL = 29 };
struct TrRow {
  TrEntry e;
  TrLaunch launch[2][TR_KINDS_ALL];   // [TrElem][TrKind]
};
// `bias`: the bf16 bias vector of the TR_C16_BIAS sets (N elements, added last in fp32, the sum rounded once); every other set is handed
// nullptr and ignores it.  `z` with its row stride ldz: the second matrix -- TR_C16_BIAS_AUX + a: the output z_out, TR_C16_DACT + a: the
// input z --; every other set is handed nullptr / 0 and ignores them, as a set with a 16-bit C ignores `accumulate`.  `b2` and `bias2`: the
// second weight and its bias vector of the TR_C16_GATED sets, whose `b` / `bias` are the gate's (either bias may be null there: +0.0); every
// other set is handed nullptr and ignores them.  The slabs of a gated set are [splits][M][2 N] (hgemm_gated.hpp).  The TR_C16_DGATED sets
// have two inputs and two outputs besides the operands and use the same four: `z` = g and `bias` = u (inputs, both at ldz), `c` = dg and
// `bias2` = du (outputs, both at ldc; the set writes through that one pointer, const in the signature for every other kind's sake).
// The TR_C16_GATED_AUX sets are the gated sets with `z` = the address of a host-side GatedAuxOut (g_out and u_out, both at ldz).
// TR_C16_BIAS_ADD and TR_C16_ADD: `z` = the read-only residual matrix r and ldz = its row stride ldr (non-const in the signature for the
// output kinds' sake); `bias` of TR_C16_BIAS_ADD may be null: +0.0.  r may be c (ldz == ldc): the thread that stores an element read its r first.
struct TrKernels {
  void (*combine)(const float* partial, void* c, const void* bias, const void* bias2, void* z, int M, int N, int ldc, int ldz, int splits,
                  bool accumulate, hipStream_t, TimingSlot);
  void (*reference)(const void* a, const void* b, const void* b2, void* c, const void* bias, const void* bias2, void* z, int M, int N, int K, int lda,
                    int ldb, int ldc, int ldz, bool accumulate, hipStream_t, TimingSlot);
  bool present() const { return reference; }
};
// The column sum of a bf16 matrix in fp32 (hgemm_registry.hip; hgemm_dbias.hpp has the forms): out32[n] (+)= sum over m of float(x[m][n]).
// finish: out32[n] = (accumulate ? out32[n] : 0) + (P[0][n] + P[1][n] + .. + P[rows - 1][n]), the partials of the fused kernels or of
// colsum_blocked, added in that order, then the one add into the old value.
void launch_colsum_direct(const void* x, float* out32, int M, int N, int ldx, bool accumulate, hipStream_t, TimingSlot);
void launch_colsum_blocked(const void* x, float* partial, int M, int N, int ldx, hipStream_t, TimingSlot);
void launch_colsum_finish(const float* partial, float* out32, int rows, int N, bool accumulate, hipStream_t, TimingSlot);
struct TrTable {
  const TrRow* rows;
  int count;
  TrKernels kernels[2][TR_KINDS_ALL];   // [TrElem][TrKind]
};
const TrTable& tr_table_nn();
const TrTable& tr_table_ta();
const TrTable& tr_table_tn();   // family f (hgemm_kernel_tn.hpp): the bf16 forward product, B given as b_col_major; no transposed read

}  // namespace hgemm_mi355x

#endif  // HGEMM_KERNEL_NN_HPP

// ---- the device text of family n's kernel: the statements of hgemm_nn_kernel<CFG, EPI>(const GemmArgs g) and of
// hgemm_nn_dgated_kernel<CFG, EPI>(const DgatedArgs g) behind their kernarg prefetch, included by both (see the head of the file).  A text
// and not a function for hgemm_tr_store_c16.inc's reason: the two entry points differ in the TYPE of g alone -- the dgated kernels find
// their second input and output behind GemmArgs -- and included, every kernel of hgemm_nn_kernel compiles to the stream it had when the
// text stood in its braces.
#ifdef HGEMM_NN_KERNEL_TEXT
  constexpr int BM = CFG::BM, BN = CFG::BN, NBUF = CFG::NBUF;
  constexpr int FM = CFG::FM, FN = CFG::FN, NW = CFG::NW, NJ = CFG::NJ, NJ_A = CFG::NJ_A;
  using elem = typename CFG::elem;   // f16, or __bf16 (the bgemm_ entry points)
  using ex4 = __attribute__((ext_vector_type(4))) elem;
  using ex8 = __attribute__((ext_vector_type(8))) elem;
  static_assert(EPI == EPI_C16 || EPI == EPI_SLAB || ((epi_is_dact(EPI) || epi_is_dbias(EPI) || epi_is_dgated(EPI) || EPI == EPI_C16_ADD) && __is_same(elem, __bf16)),
                "plain, two-pass slab and (bf16) dact / dact + dbias / dgated / residual epilogues");

  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / CFG::WN;
  const int wave_n = wave % CFG::WN;

  const TileCoord tc = map_block(g, BM, BN);

  // ---- LDS-DMA source addressing ---------------------------------------------------------------
  // A: the classic family's (2 GiB descriptor at the tile's first row, the K advance in the scalar offset).
  // B: the descriptor starts at column n0 of row 0 and ENDS WITH THE MATRIX; the whole offset (k-row and chunk) is in the lane's
  // register, which is what the range check sees: a chunk behind the last element reads as zeros.
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)tc.m0 * g.lda), 0, 0x80000000u, 0x00020000);
  const uint32_t b_bytes = (uint32_t)(((size_t)(g.K - 1) * g.ldb + (g.N - tc.n0)) * 2);   // (< 2 GiB: host check)
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)(g.Bt + tc.n0), 0, b_bytes, 0x00020000);
  const uint32_t b_stage = (uint32_t)g.ldb * (uint32_t)(BK * 2);   // bytes between two stages of B

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j < NJ_A) {
      const int il = wave + j * NW;                     // piece of the A tile
      const int r  = il * 8 + (lane >> 3);
      const int rc = min(r, g.M - 1 - tc.m0);
      const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));   // slot (lane & 7) of row r holds chunk slot ^ ((r >> 1) & 7)
      voff[j] = ((uint32_t)rc * (uint32_t)g.lda + (uint32_t)chunk * 8u) * 2u;
    } else {
      const int il = wave + (j - NJ_A) * NW;            // piece of the B tile: k-rows il * B_RPP ..
      const int kr = il * CFG::B_RPP + lane / CFG::B_CH;
      const int chunk = (lane % CFG::B_CH) ^ nn_swz<BN>(kr);
      voff[j] = ((uint32_t)(tc.k_begin + kr) * (uint32_t)g.ldb + (uint32_t)chunk * 8u) * 2u;
    }
  }

  // ---- fragment read offsets (bytes inside a stage) ---------------------------------------------
  int a_off[2];
  {
    const int lr = lane & 15, lq = lane >> 4, sw = (lr >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a_off[ks] = wave_m * CFG::TM * ROW_BYTES + lr * ROW_BYTES + (((ks * 4 + lq) ^ sw) << 4);
  }
  // transposed reads: lane 4q + p of 16-lane group gq addresses k-row 8 gq + 4 h + q (h = 0, 1: the two reads), columns 4p .. 4p + 3
  // of column tile jn -- 16-byte chunk 2 (tile) + (p >> 1), its half p & 1.  (+ ks * 32 rows per K = 32 slice: nn_swz does not see it.)
  int b_off[2][FN];
  {
    const int gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kr = 8 * gq + 4 * h + q;
#pragma unroll
      for (int jn = 0; jn < FN; ++jn) {
        const int chunk = (wave_n * CFG::TN + jn * 16) / 8 + (p >> 1);
        b_off[h][jn] = CFG::A_BYTES + kr * CFG::B_ROW_BYTES + ((chunk ^ nn_swz<BN>(kr)) << 4) + 8 * (p & 1);
      }
    }
  }

  f32x4 acc[FM][FN];
  tr_zero(acc);

  // ---- pipeline ----------------------------------------------------------------------------------
  uint32_t kbyte = (uint32_t)tc.k_begin * 2u;
  auto stage = [&](char* lds_stage) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      lds_void_t* dst = (lds_void_t*)(lds_stage + (wave + j * NW) * 1024);
      if (j < NJ_A) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voff[j], kbyte, 0, 0);
      } else {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, voff[j], 0, 0, 0);
        voff[j] += b_stage;
      }
    }
    kbyte += ROW_BYTES;
  };
  const int nk = tc.nk;
#pragma unroll
  for (int s = 0; s < NBUF - 1; ++s)
    if (s < nk) stage(smem + s * CFG::STAGE_BYTES);

  int rd = 0, wr = NBUF - 1;
  for (int t = 0; t < nk; ++t) {
    if (t + NBUF - 2 < nk)
      wait_vmcnt<NJ*(NBUF - 2)>();
    else
      wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();   // all waves' pieces of stage t landed; stage `wr` is free again

    if (t + NBUF - 1 < nk) stage(smem + wr * CFG::STAGE_BYTES);

    const char* st = smem + rd * CFG::STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      ex8 af[FM], bf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = *(const ex8*)(st + i * 16 * ROW_BYTES + a_off[ks]);
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const char* pb = st + ks * 32 * CFG::B_ROW_BYTES;
        const ex4 lo = __builtin_bit_cast(ex4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_t*)(pb + b_off[0][j])));
        const ex4 hi = __builtin_bit_cast(ex4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_t*)(pb + b_off[1][j])));
        bf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = tr_mfma(bf[j], af[i], acc[i][j]);
    }
    rd = (rd + 1 == NBUF) ? 0 : rd + 1;
    wr = (wr + 1 == NBUF) ? 0 : wr + 1;
  }

  // ---- the activation's derivative (EPI_C16_DACT + ACT, bgemm_mi355x_nn_dact): C = bf16(acc x act'(float(z[m][n]))) ------------------------
  // g.counters is the saved bf16 pre-activation Z ([M][ldz], read-only; the host puts it there for this epilogue alone, ldz in
  // g.tail_first: GemmArgs keeps its layout).  tr_mfma(bf, af, acc) leaves lane (row = lane & 15, q = lane >> 4) with
  // acc[i][j][e] = C[16 i + row][16 j + 4 q + e], so the lane's four z of a fragment are one 8-byte load.  The descriptor starts at the
  // tile's first row and ENDS AT THE LAST VALID ELEMENT, (M - 1, N - 1): a row at or past M is out of range and reads zeros; a column
  // group at or past N (N % 8 == 0: wholly inside or wholly behind) reads pad or the next row, inside the range, or zeros behind its end.
  // Both feed only values the store text never stores.  The offset stays below (BM ldz + N) 2 + 2 BN < 2^32 (host check: below 2 GiB); the
  // range is dact_z_range_bytes above, clamped where Z goes on for 4 GiB and more behind the tile's first row.
  // Issued HERE, behind the K loop, as family f's bias loads are: the loop keeps the EPI_C16 kernel's registers and its counted vmcnt.
  // dact_mul (hgemm_act.hpp) is the combine's and the reference kernel's text: one fp32 multiply on the finished sum, ReLU a select.
  // The sched_barrier per fragment and the parking asm are hgemm_kernel_tn.hpp's register steering.
  // EPI_C16_DACT_DBIAS + ACT (bgemm_mi355x_nn_dact_dbias) is the same text with three additions, steps 1 to 3 of hgemm_dbias.hpp: behind
  // dact_mul the value is rounded to bf16 and converted back -- exact, so the store text below stores the dact kernel's bits -- and added
  // into the lane's column accumulator, a row at or past M counting 0; the butterfly; the wave rows through LDS into P (g.partial).
  if constexpr (epi_is_dact(EPI) || epi_is_dbias(EPI)) {
    constexpr bool DBIAS = epi_is_dbias(EPI);
    float col[DBIAS ? FN : 1][4];
    if constexpr (DBIAS) {
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) col[j][e] = 0.0f;
    }
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    using bx4 = __attribute__((ext_vector_type(4))) __bf16;
    const uint32_t ldz = (uint32_t)g.tail_first;
    const uint32_t z_bytes = dact_z_range_bytes(g.M, g.N, g.tail_first, tc.m0);
    const __amdgpu_buffer_rsrc_t rsZ =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const __bf16*)g.counters + (size_t)tc.m0 * ldz), 0, z_bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const uint32_t row = (uint32_t)dbias_row(wave_m, CFG::TM, i, lane);
      const bool counts = dbias_row_counts(tc.m0, (int)row, g.M);
      bx4 z[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const uint32_t n_z = (uint32_t)(tc.n0 + wave_n * CFG::TN + 16 * j + 4 * (lane >> 4));
        z[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsZ, (row * ldz + n_z) * 2u, 0, 0));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float y = dact_mul<epi_dact(EPI)>(acc[i][j][e], (float)z[j][e]);
          if constexpr (DBIAS) {
            y = (float)(__bf16)y;
            col[j][e] += counts ? y : 0.0f;
          }
          asm volatile("" : "+a"(y));
          acc[i][j][e] = y;
        }
      }
    }
    if constexpr (DBIAS) {
      float* red = (float*)smem;   // [WM][BN]
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) col[j][e] = dbias_row16_sum(col[j][e]);
      __syncthreads();             // every wave has read its last stage: the ring is free
      if ((lane & 15) == 0) {
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) red[wave_m * BN + dbias_col(wave_n, CFG::TN, j, lane, e)] = col[j][e];
      }
      __syncthreads();
      if (tid < BN) {
        float s = red[tid];
#pragma unroll
        for (int w = 1; w < CFG::WM; ++w) s += red[w * BN + tid];
        const int n = tc.n0 + tid;
        if (n < g.N) g.partial[(size_t)(tc.m0 / BM) * (size_t)g.N + (size_t)n] = s;
      }
    }
  }

  // ---- the gated MLP's input gradient (EPI_C16_DGATED + ACT, bgemm_mi355x_nn_dgated): dU = bf16(act(g) x acc), dG = bf16(acc x u x act'(g)) ---
  // The dact epilogue's text with TWO saved bf16 matrices and two outputs: g.counters is G and nn_dgated_u(g) is U (both [M][ldz], read-only,
  // ldz in g.tail_first), g.C is dG and nn_dgated_du(g) is dU (both [M][ldc]).  One 8-byte load per fragment from EACH matrix, each through a
  // descriptor of its own that starts at the tile's first row and ends at ITS matrix's last valid element (dact_z_range_bytes): with a
  // fused [M][2 N] buffer (U = G + N) a column group at or past N of G reads U's data, inside the range, and one of U the next row or zeros
  // behind the end -- values the store text never stores.  Issued behind the K loop, as the dact loads are.  dgated_store (hgemm_dgated.hpp)
  // is the combine's and the reference kernel's text.  Both results are held: dG replaces the sum in acc, dU goes to a second array of
  // FM x FN x 4 registers (the 128 x 128 member: 64 + 64 accumulators); it is stored first, through the shared 16-bit store text entered
  // with `acc` naming it, and the kernel's own store below then writes dG.
  if constexpr (epi_is_dgated(EPI)) {
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    using bx4 = __attribute__((ext_vector_type(4))) __bf16;
    const uint32_t ldz = (uint32_t)g.tail_first;
    const uint32_t z_bytes = dact_z_range_bytes(g.M, g.N, g.tail_first, tc.m0);
    const __amdgpu_buffer_rsrc_t rsG =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const __bf16*)g.counters + (size_t)tc.m0 * ldz), 0, z_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsU = __builtin_amdgcn_make_buffer_rsrc((void*)(nn_dgated_u(g) + (size_t)tc.m0 * ldz), 0, z_bytes, 0x00020000);
    f32x4 du_acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const uint32_t row = (uint32_t)dbias_row(wave_m, CFG::TM, i, lane);
      bx4 zg[FN], zu[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const uint32_t n_z = (uint32_t)(tc.n0 + wave_n * CFG::TN + 16 * j + 4 * (lane >> 4));
        zg[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsG, (row * ldz + n_z) * 2u, 0, 0));
        zu[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsU, (row * ldz + n_z) * 2u, 0, 0));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          DgatedPair y = dgated_store<epi_dgated(EPI)>(acc[i][j][e], (float)zg[j][e], (float)zu[j][e]);
          asm volatile("" : "+a"(y.dg), "+a"(y.du));
          acc[i][j][e] = y.dg;
          du_acc[i][j][e] = y.du;
        }
      }
    }
    {
      f32x4(&acc)[FM][FN] = du_acc;   // the store text reads `acc`
#define HGEMM_TR_STORE_C nn_dgated_du(g)
#define HGEMM_TR_STORE_LD g.ldc
#include "hgemm_tr_store_c16.inc"
#undef HGEMM_TR_STORE_C
#undef HGEMM_TR_STORE_LD
    }
  }

  // ---- the fused residual add (EPI_C16_ADD, bgemm_mi355x_nn_add): C = bf16(acc + float(r[m][n])) ----------------------------------------------
  // The dact epilogue's loads with residual_add (hgemm_residual.hpp: one fp32 add on the finished sum, the combine's and the reference
  // kernel's text) in place of dact_mul: g.counters is the bf16 residual matrix r ([M][ldr], read-only, ldr in g.tail_first), one 8-byte load
  // per fragment through a descriptor from the tile's first row to r's last valid element (dact_z_range_bytes), issued behind the K loop.
  // r may be C itself (ldr == ldc).  Every load of the wave's tile is issued and consumed in this block, in front of the store text below;
  // the element a lane stores there -- its own or, behind the permlane swap, one of another lane of the SAME wave -- is computed from that
  // element's r, so its store depends on its load; wave tiles are disjoint, and what a load reads outside its tile's M x N elements is never
  // stored by this wave.
  if constexpr (EPI == EPI_C16_ADD) {
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    using bx4 = __attribute__((ext_vector_type(4))) __bf16;
    const uint32_t ldr = (uint32_t)g.tail_first;
    const uint32_t r_bytes = dact_z_range_bytes(g.M, g.N, g.tail_first, tc.m0);
    const __amdgpu_buffer_rsrc_t rsR =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const __bf16*)g.counters + (size_t)tc.m0 * ldr), 0, r_bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const uint32_t row = (uint32_t)dbias_row(wave_m, CFG::TM, i, lane);
      bx4 r[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const uint32_t n_r = (uint32_t)(tc.n0 + wave_n * CFG::TN + 16 * j + 4 * (lane >> 4));
        r[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsR, (row * ldr + n_r) * 2u, 0, 0));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] = residual_add(acc[i][j][e], (float)r[j][e]);
    }
  }

  if constexpr (EPI == EPI_SLAB) {
    store_tile<16, FM, FN, CFG::TM, CFG::TN, true>(g, tc, wave_m, wave_n, lane, acc);
  } else {
#include "hgemm_tr_store_c16.inc"   // the 16-bit C epilogue, one text for families n, a and f
  }
#endif  // HGEMM_NN_KERNEL_TEXT
