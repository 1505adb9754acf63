// Family f's gated kernels (bgemm_mi355x_tn_gated): C[M,N] = bf16(act(X Wg^T + bg) * (X Wu^T + bu)), X row-major [M][lda], Wg and Wu each
// b_col_major [N][ldb].  The work of a TN product of width 2 N in one launch: a member's tile is BM rows by BN / 2 OUTPUT columns, its B
// image holds the tile's rows of BOTH weights (hgemm_gated.hpp has the row assignment), and the gate is a multiply of two accumulators of
// the same lane in the epilogue.  A kernel of its own beside hgemm_tn_bf16_kernel and not a branch of it: that kernel's text, and with it
// every instruction stream of units g11, g12, g14 and g15, is untouched.
//   * A image, the ring, the fragment reads, the MFMAs and the counted vmcnt: hgemm_kernel_tn.hpp's, word for word.  MIRRORED TEXT: an edit
//     to hgemm_tn_bf16_kernel's descriptor setup, voff / chunk swizzle, f_off, accumulator zeroing, `stage` lambda, prologue or K loop
//     (wait_vmcnt count, barrier, rd / wr ring) is to be made here too, and the other way round; this kernel differs from it ONLY in the
//     tile width handed to map_block, the second B descriptor with its per-piece choice, gated_source_row in voff, and everything behind
//     the K loop.  tests/test_tn_gated_host.py holds the two K loops to the same MFMA, ds_read_b128, LDS-DMA and barrier counts.
//   * B image: [BN rows][128 B] as there; piece il (image rows 8 il .. 8 il + 7) comes from Wg or from Wu -- wave-uniform -- through that
//     weight's descriptor (2 GiB) at row n0 = tile_n BN / 2, rows clamped to N - 1 - n0 PER WEIGHT: with a fused [2 N][K] weight an
//     unclamped gate row at or past N would read Wu's rows, harmless only because such a column is never stored -- the clamp keeps every
//     read inside the weight the caller named.
//   * Grid: tiles_m x tiles_n with tiles_n = ceil(N / (BN / 2)), through the family's XCD raster map (g.N is the OUTPUT width).
//   * ACT = ACT_RELU .. ACT_SILU: bias loads behind the K loop (two 8-byte loads per output fragment; a NULL bias is a descriptor of
//     length 0 on a valid base, which reads +0.0), y = act_apply<ACT>(acc[i][jo] + bg) * (acc[i][jo + FN / 2] + bu) with the register
//     steering of the bias+activation kernels, then the bf16 store: two output fragments per wave (BN = 128) go through
//     hgemm_tr_store_c16.inc's convert-and-swap and 16-byte stores; one (BN = 64) is stored as the lane's four columns, 8 bytes.
//   * ACT = ACT_NONE: the K slice of a two-pass plan; the fp32 sums go to the slab as gated_slab_index has it, nothing applied.
//   * Scope (the host sends anything else to the reference kernel): family f's, with (BN / 2 ldb + K) 2 bytes below 2 GiB per weight.
// This header includes ITSELF, as hgemm_kernel_nn.hpp does: the device text of the kernel stands at the end of the file, behind the include
// guard, under HGEMM_TN_GATED_KERNEL_TEXT, and each of the two entry points (hgemm_tn_gated_kernel, hgemm_tn_gated_aux_kernel) includes the
// file once more with that macro set.  Hence a guard and no `#pragma once`.
//   * hgemm_tn_gated_aux_kernel (bgemm_mi355x_tn_gated_aux, unit g20): the same text behind a GatedAuxArgs, AUX = true.  Behind the bias
//     loads the biases are added IN PLACE (acc[i][jo] = g, acc[i][jo + OFN] = u, the fp32 adds of the gate pass), g_out = bf16(g) and
//     u_out = bf16(u) are stored from those through hgemm_tn_gated_store.inc (acc only read), then the gate pass runs on the unrounded
//     values and C is stored: three outputs, each rounded once, no register beyond the gated kernel's.
#ifndef HGEMM_KERNEL_TN_GATED_HPP
#define HGEMM_KERNEL_TN_GATED_HPP

#include "hgemm_gated.hpp"
#include "hgemm_kernel_tn.hpp"

namespace hgemm_mi355x {


// What the text reads the aux call's two outputs and their stride through: the GatedArgs overloads are never called (the text names them
// where AUX holds alone) and let the one text compile for both entry points.
__device__ __forceinline__ __bf16* tn_gated_aux_g(const GatedArgs&) { return nullptr; }
__device__ __forceinline__ __bf16* tn_gated_aux_u(const GatedArgs&) { return nullptr; }
__device__ __forceinline__ int tn_gated_aux_ldz(const GatedArgs&) { return 0; }
__device__ __forceinline__ __bf16* tn_gated_aux_g(const GatedAuxArgs& g) { return g.G; }
__device__ __forceinline__ __bf16* tn_gated_aux_u(const GatedAuxArgs& g) { return g.U; }
__device__ __forceinline__ int tn_gated_aux_ldz(const GatedAuxArgs& g) { return g.ldz; }

template <class MEMBER, int ACT>
__global__ void __launch_bounds__(MEMBER::THREADS) hgemm_tn_gated_kernel(const GatedArgs g) {
  prefetch_kernargs<sizeof(GatedArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr bool AUX = false;
#define HGEMM_TN_GATED_KERNEL_TEXT
#include "hgemm_kernel_tn_gated.hpp"   // the kernel text at the end of this file
#undef HGEMM_TN_GATED_KERNEL_TEXT
#endif  // __HIP_DEVICE_COMPILE__
}
// the same text behind a GatedAuxArgs: the kernels that also write g_out and u_out (hgemm_inst_g20.hip)
template <class MEMBER, int ACT>
__global__ void __launch_bounds__(MEMBER::THREADS) hgemm_tn_gated_aux_kernel(const GatedAuxArgs g) {
  static_assert(ACT >= ACT_RELU && ACT <= ACT_SILU, "the four activations; the K slices of a two-pass form are hgemm_tn_gated_kernel<., ACT_NONE>");
  prefetch_kernargs<sizeof(GatedAuxArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr bool AUX = true;
#define HGEMM_TN_GATED_KERNEL_TEXT
#include "hgemm_kernel_tn_gated.hpp"   // the kernel text at the end of this file
#undef HGEMM_TN_GATED_KERNEL_TEXT
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- host side: the gated sets, one per activation.  TrLaunch's signature; `g` is the base of a GatedArgs (see there).  The K slices of a
// two-pass form are the gated slab kernel (ACT_NONE), instantiated with the ReLU set alone and reached from the others through it.
template <class CFG>
void launch_tn_gated_slab(const GemmArgs& g, int grid, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH((hgemm_tn_gated_kernel<CFG, ACT_NONE>), grid, CFG::THREADS, stream, ts, static_cast<const GatedArgs&>(g));
}
template <class CFG, int ACT>
void launch_tn_gated(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tn_gated_slab<CFG>(g, grid, stream, ts);
  HGEMM_LAUNCH((hgemm_tn_gated_kernel<CFG, ACT>), grid, CFG::THREADS, stream, ts, static_cast<const GatedArgs&>(g));
}
#define HGEMM_TN_GATED_SLAB_LAUNCHER(CFG, BM, BN, WM, WN, NB) launch_tn_gated_slab<CFG<BM, BN, WM, WN, NB>>
#define HGEMM_TN_GATED_SLAB_INST(...) template void HGEMM_TN_GATED_SLAB_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_TN_GATED_SLAB_EXTERN(...) extern HGEMM_TN_GATED_SLAB_INST(__VA_ARGS__)
#define HGEMM_TN_GATED_LAUNCHER(ACT, CFG, BM, BN, WM, WN, NB) launch_tn_gated<CFG<BM, BN, WM, WN, NB>, ACT>
#define HGEMM_TN_GATED_INST(...) template void HGEMM_TN_GATED_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_TN_GATED_EXTERN(...) extern HGEMM_TN_GATED_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_SLAB_EXTERN, CfgTNB)             // hgemm_inst_g18.hip
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_EXTERN, ACT_RELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_EXTERN, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_EXTERN, ACT_GELU_TANH, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_EXTERN, ACT_SILU, CfgTNB)

// The sets that also write the pre-activations (bgemm_mi355x_tn_gated_aux), one per activation: `g` is the base of a GatedAuxArgs; the K
// slices of a two-pass form are unit g18's slab kernels, which read the GatedArgs in it.
template <class CFG, int ACT>
void launch_tn_gated_aux(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tn_gated_slab<CFG>(g, grid, stream, ts);
  HGEMM_LAUNCH((hgemm_tn_gated_aux_kernel<CFG, ACT>), grid, CFG::THREADS, stream, ts, static_cast<const GatedAuxArgs&>(g));
}
#define HGEMM_TN_GATED_AUX_LAUNCHER(ACT, CFG, BM, BN, WM, WN, NB) launch_tn_gated_aux<CFG<BM, BN, WM, WN, NB>, ACT>
#define HGEMM_TN_GATED_AUX_INST(...) template void HGEMM_TN_GATED_AUX_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_TN_GATED_AUX_EXTERN(...) extern HGEMM_TN_GATED_AUX_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_EXTERN, ACT_RELU, CfgTNB)    // hgemm_inst_g20.hip
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_EXTERN, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_EXTERN, ACT_GELU_TANH, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_EXTERN, ACT_SILU, CfgTNB)

}  // namespace hgemm_mi355x

#endif  // HGEMM_KERNEL_TN_GATED_HPP

// ---- the device text of family f's gated kernel: the statements of hgemm_tn_gated_kernel<MEMBER, ACT>(const GatedArgs g) and of
// hgemm_tn_gated_aux_kernel<MEMBER, ACT>(const GatedAuxArgs g) behind their kernarg prefetch and their `constexpr bool AUX`, included by
// both (see the head of the file).  A text and not a function for hgemm_tr_store_c16.inc's reason: included, every kernel of
// hgemm_tn_gated_kernel compiles to the stream it had when the text stood in its braces.
#ifdef HGEMM_TN_GATED_KERNEL_TEXT
  constexpr int BM = MEMBER::BM, BN = MEMBER::BN, NBUF = MEMBER::NBUF, TN = MEMBER::TN;
  constexpr int FM = MEMBER::FM, NW = MEMBER::NW, NJ = MEMBER::NJ, NJ_A = MEMBER::NJ_A;
  constexpr int FN_ALL = MEMBER::FN, OFN = FN_ALL / 2;   // column fragments of the image; output fragments of a wave
  using elem = typename MEMBER::elem;   // __bf16
  using ex8 = __attribute__((ext_vector_type(8))) elem;
  static_assert(ACT >= ACT_NONE && ACT <= ACT_SILU, "the slab form (ACT_NONE) and the four activations");
  static_assert((TN / 2) % 8 == 0 && OFN >= 1, "a DMA piece is wholly gate or wholly up");

  __shared__ __attribute__((aligned(1024))) char smem[MEMBER::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / MEMBER::WN;
  const int wave_n = wave % MEMBER::WN;

  const TileCoord tc = map_block(g, BM, BN / 2);   // n0 counts output columns (tc.slab is the plain product's and is not used)

  // ---- LDS-DMA source addressing: hgemm_kernel_tn.hpp's, with a descriptor per weight ------------------------------------------------
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)tc.m0 * g.lda), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsBg = __builtin_amdgcn_make_buffer_rsrc((void*)(g.Bt + (size_t)tc.n0 * g.ldb), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsBu = __builtin_amdgcn_make_buffer_rsrc((void*)(g.Bu + (size_t)tc.n0 * g.ldb), 0, 0x80000000u, 0x00020000);

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const bool isA = j < NJ_A;
    const int il = wave + (isA ? j : j - NJ_A) * NW;    // piece of its operand's image: rows 8 il .. 8 il + 7
    const int r  = il * 8 + (lane >> 3);
    const int rc = isA ? min(r, g.M - 1 - tc.m0) : gated_source_row(TN, r, g.N - tc.n0);   // B: the row of its weight, counted from n0, clamped per weight
    const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));   // slot (lane & 7) of row r holds chunk slot ^ ((r >> 1) & 7)
    voff[j] = ((uint32_t)rc * (uint32_t)(isA ? g.lda : g.ldb) + (uint32_t)chunk * 8u) * 2u;
  }

  // ---- fragment read offsets: hgemm_kernel_tn.hpp's ---------------------------------------------------------------------------------
  int f_off[2];
  {
    const int lr = lane & 15, lq = lane >> 4, sw = (lr >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) f_off[ks] = lr * ROW_BYTES + (((ks * 4 + lq) ^ sw) << 4);
  }
  const int a_row_base = wave_m * MEMBER::TM * ROW_BYTES;
  const int b_row_base = MEMBER::A_BYTES + wave_n * TN * ROW_BYTES;

  f32x4 acc[FM][FN_ALL];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN_ALL; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;

  // ---- pipeline ----------------------------------------------------------------------------------
  uint32_t kbyte = (uint32_t)tc.k_begin * 2u;
  auto stage = [&](char* lds_stage) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      lds_void_t* dst = (lds_void_t*)(lds_stage + (wave + j * NW) * 1024);
      if (j < NJ_A) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voff[j], kbyte, 0, 0);
      } else {
        const int il = wave + (j - NJ_A) * NW;   // wave-uniform: the piece's weight
        if (gated_is_up(TN, il * 8)) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsBu, dst, 16, voff[j], kbyte, 0, 0);
        else                         __builtin_amdgcn_raw_ptr_buffer_load_lds(rsBg, dst, 16, voff[j], kbyte, 0, 0);
      }
    }
    kbyte += ROW_BYTES;
  };
  const int nk = tc.nk;
#pragma unroll
  for (int s = 0; s < NBUF - 1; ++s)
    if (s < nk) stage(smem + s * MEMBER::STAGE_BYTES);

  int rd = 0, wr = NBUF - 1;
  for (int t = 0; t < nk; ++t) {
    if (t + NBUF - 2 < nk)
      wait_vmcnt<NJ*(NBUF - 2)>();
    else
      wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();   // all waves' pieces of stage t landed; stage `wr` is free again

    if (t + NBUF - 1 < nk) stage(smem + wr * MEMBER::STAGE_BYTES);

    const char* st = smem + rd * MEMBER::STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      ex8 af[FM], bf[FN_ALL];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = *(const ex8*)(st + a_row_base + i * 16 * ROW_BYTES + f_off[ks]);
#pragma unroll
      for (int j = 0; j < FN_ALL; ++j) bf[j] = *(const ex8*)(st + b_row_base + j * 16 * ROW_BYTES + f_off[ks]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN_ALL; ++j) acc[i][j] = tr_mfma(bf[j], af[i], acc[i][j]);
    }
    rd = (rd + 1 == NBUF) ? 0 : rd + 1;
    wr = (wr + 1 == NBUF) ? 0 : wr + 1;
  }

  if constexpr (ACT == ACT_NONE) {
    // ---- the K slice of a two-pass plan: the lane's gate quads and up quads to the slab, 16-byte stores (N % 8 == 0) ------------------
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      __builtin_amdgcn_sched_barrier(0);   // one fragment row's accumulator reads at a time (store_tile)
      const int m = tc.m0 + dbias_row(wave_m, MEMBER::TM, i, lane);
#pragma unroll
      for (int j = 0; j < FN_ALL; ++j) {
        const int n = tc.n0 + gated_lane_col(wave_n, TN, j % OFN, lane, 0);
        if (m < g.M && n < g.N) *(f32x4*)(g.partial + gated_slab_index(g.M, g.N, tc.split, m, n, j / OFN)) = acc[i][j];
      }
    }
  } else {
    // ---- bias, activation and gate on the finished sums: y = act(acc_g + bg) * (acc_u + bu), parked where the gate sum was -----------
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    using bx4 = __attribute__((ext_vector_type(4))) __bf16;
    // N % 8 == 0: a lane's group of 4 is inside N or wholly behind it, where the load returns zeros and the values are never stored.  A
    // NULL vector: length 0 on X's base, every load returns +0.0 -- the result of a zero-filled vector, bit for bit.
    const __amdgpu_buffer_rsrc_t rsBiasG = __builtin_amdgcn_make_buffer_rsrc(g.bias_g ? (void*)g.bias_g : (void*)g.A, 0, g.bias_g ? (uint32_t)g.N * 2u : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsBiasU = __builtin_amdgcn_make_buffer_rsrc(g.bias_u ? (void*)g.bias_u : (void*)g.A, 0, g.bias_u ? (uint32_t)g.N * 2u : 0u, 0x00020000);
    bx4 bg[OFN], bu[OFN];
#pragma unroll
    for (int jo = 0; jo < OFN; ++jo) {
      const uint32_t n_b = (uint32_t)(tc.n0 + gated_lane_col(wave_n, TN, jo, lane, 0));
      bg[jo] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBiasG, n_b * 2u, 0, 0));
      bu[jo] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBiasU, n_b * 2u, 0, 0));
    }
    if constexpr (AUX) {
      // ---- the pre-activations as two more outputs (bgemm_mi355x_tn_gated_aux): the gate pass's two fp32 adds made in place, then
      // g_out = bf16(g) from acc[i][jo] and u_out = bf16(u) from acc[i][jo + OFN], each at stride ldz; acc is only read by the stores,
      // so the gate pass below works on the unrounded values
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int jo = 0; jo < OFN; ++jo)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[i][jo][e] = gated_pre(acc[i][jo][e], (float)bg[jo][e]);
            acc[i][jo + OFN][e] = gated_pre(acc[i][jo + OFN][e], (float)bu[jo][e]);
          }
#define HGEMM_GATED_STORE_OUTPUT 0
#include "hgemm_tn_gated_store.inc"
#undef HGEMM_GATED_STORE_OUTPUT
#define HGEMM_GATED_STORE_OUTPUT 1
#include "hgemm_tn_gated_store.inc"
#undef HGEMM_GATED_STORE_OUTPUT
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int jo = 0; jo < OFN; ++jo) {
        __builtin_amdgcn_sched_barrier(0);   // hgemm_kernel_tn.hpp's register steering: a quad's temporaries at a time
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float gv, uv;
          if constexpr (AUX) {
            gv = acc[i][jo][e];
            uv = acc[i][jo + OFN][e];
          } else {
            gv = acc[i][jo][e] + (float)bg[jo][e];
            uv = acc[i][jo + OFN][e] + (float)bu[jo][e];
          }
          float y = gated_mul(act_apply<ACT>(gv), uv);
          asm volatile("" : "+a"(y));   // the finished value waits in an accumulation register for the stores
          acc[i][jo][e] = y;
        }
      }

#include "hgemm_tn_gated_store.inc"   // C: the bf16 store of the gated kernels, one text for the three outputs
  }
#endif  // HGEMM_TN_GATED_KERNEL_TEXT
