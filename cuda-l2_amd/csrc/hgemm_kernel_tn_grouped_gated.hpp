// Family f, grouped and gated (bgemm_mi355x_tn_grouped_gated): the gated forward of a mixture-of-experts layer in ONE launch.  The rows of A and
// of the outputs are sorted by group; group e owns rows [off[e], off[e + 1]), its two weights Wg_e = wg + e group_stride_b and
// Wu_e = wu + e group_stride_b (each [N][ldb]) and its two bias rows:
//   gv = fl32(sum_k A[m][k] Wg_e[n][k] + float(bias_g[e][n])),  uv = fl32(sum_k A[m][k] Wu_e[n][k] + float(bias_u[e][n]))      (gated_pre)
//   C[m][n] = bf16(gated_mul(act_apply<ACT>(gv), uv));   AUX: g_out[m][n] = bf16(gv), u_out[m][n] = bf16(uv), the gate reads them UNROUNDED.
// The join of two kernels the library has, and a kernel of its own beside both: neither text moves, so units g18, g20 and
// g23 keep their instruction streams.
//   * The front is hgemm_grouped_front.inc as it stands (hgemm_kernel_tn_grouped.hpp has the design): `offsets` lives on the device, every
//     wave runs the map redundantly and a workgroup past the real tile count returns in front of its first barrier.  A tile here is BM rows
//     by BN / 2 OUTPUT columns, so the name the front reads as `BN` is the output width and ka.tiles_n = ceil(N / (BN / 2)).
//   * The B image is hgemm_tn_gated_kernel's: inside each wave's TN image rows the fragments j < FN / 2 are rows of Wg and the fragments
//     j >= FN / 2 the same output rows of Wu (hgemm_gated.hpp).  One descriptor per weight, at W?_e + n0 ldb in 64-bit arithmetic; a DMA
//     piece is wholly gate or wholly up (gated_is_up, wave-uniform) and its source rows are gated_source_row, clamped PER WEIGHT to row
//     N - 1 - n0: with a fused per-expert [2 N][K] weight (wu = wg + N ldb) an unclamped gate row of the sliver tile would read Wu's rows,
//     and with stacked experts an unclamped up row would read the NEXT expert's weight.
//   * A's rows are clamped to the GROUP's last row, not to M.  The K loop is family f's ring word for word: LDS-DMA stages, counted vmcnt,
//     one barrier per step, ds_read_b128 fragments, tr_mfma on acc[FM][FN]; acc[i][jo] holds the gate sums, acc[i][jo + FN / 2] the up sums.
//   * Epilogue: the group's two bias rows through descriptors of range N x 2 bytes (0 for a NULL bias: +0.0) at bias + e ldbias; AUX adds
//     them in place and stores g_out and u_out through hgemm_tn_gated_store.inc; the gate pass has the dense kernel's register steering
//     (a sched_barrier per quad, the finished value parked in an accumulation register); then C through the same store text.  That text
//     reads its row bound from `g.M`: it is handed a view whose M is the group's END ROW, so a tile that straddles a group boundary
//     computes the rows behind it from the clamped row and stores none of them, in any of the three outputs.
// With G = 1 and offsets {0, M} every lane runs the dense gated kernel's arithmetic in its order: the same bits (tests/test_gpu_tn_grouped_gated.py).
// Scope (the host sends everything else to the grouped gated reference kernel): K % 64 == 0, N % 8 == 0, every stride a multiple of 8,
// 16-byte aligned pointers, (BM lda + K) 2, (BN / 2 ldb + K) 2 per weight, (BM ldc + N) 2 and (BM ldz + N) 2 bytes below 2 GiB,
// G <= GROUPED_MAX_GROUPS.  No ACT_NONE instance: there is no split-K form and no slab.
#pragma once

#include "hgemm_kernel_tn_gated.hpp"
#include "hgemm_kernel_tn_grouped.hpp"

namespace hgemm_mi355x {

// GroupedArgs (B: the G gate weights, bias: the G gate bias rows) and behind it the up half and the two saved outputs: 128 bytes
struct GroupedGatedArgs : GroupedArgs {
  const __bf16* Bu;       // G up weights [N][ldb], group_stride_b elements apart
  const __bf16* bias_u;   // [G][ldbias] or null (+0.0)
  __bf16* G_out;          // [M][ldz], AUX only
  __bf16* U_out;          // [M][ldz], AUX only
  int ldz;
};

// what the shared store texts read as `g`: M is the GROUP's end row (their predicate, and A's clamp); the three outputs and their strides
struct GroupedGatedView {
  __bf16* C; int ldc, M, N, flags;
  __bf16* G; __bf16* U; int ldz;
};
__device__ __forceinline__ __bf16* tn_gated_aux_g(const GroupedGatedView& g) { return g.G; }
__device__ __forceinline__ __bf16* tn_gated_aux_u(const GroupedGatedView& g) { return g.U; }
__device__ __forceinline__ int tn_gated_aux_ldz(const GroupedGatedView& g) { return g.ldz; }

template <class MEMBER, int ACT, bool AUX>
__global__ void __launch_bounds__(MEMBER::THREADS) hgemm_tn_grouped_gated_kernel(const GroupedGatedArgs ka) {
  static_assert(ACT >= ACT_RELU && ACT <= ACT_SILU, "the four activations: the grouped gated call has no slab form");
  prefetch_kernargs<sizeof(GroupedGatedArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = MEMBER::BM, NBUF = MEMBER::NBUF, TN = MEMBER::TN;
  constexpr int BN = MEMBER::BN / 2;   // the tile's OUTPUT width: what the front's tc.n0 = tn * BN counts
  constexpr int FM = MEMBER::FM, NW = MEMBER::NW, NJ = MEMBER::NJ, NJ_A = MEMBER::NJ_A;
  constexpr int FN_ALL = MEMBER::FN, OFN = FN_ALL / 2;   // column fragments of the image; output fragments of a wave
  constexpr int LG = GROUPED_LANE_GROUPS;
  using elem = typename MEMBER::elem;   // __bf16
  using ex8 = __attribute__((ext_vector_type(8))) elem;
  static_assert((TN / 2) % 8 == 0 && OFN >= 1, "a DMA piece is wholly gate or wholly up");

  __shared__ __attribute__((aligned(1024))) char smem[MEMBER::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / MEMBER::WN;
  const int wave_n = wave % MEMBER::WN;

  // ---- the tile map: offsets -> (group, first row, first OUTPUT column, the group's end row), or no tile ---------------------------------
  struct { int m0, n0; } tc;
  int group, row_end;
#include "hgemm_grouped_front.inc"
  const GroupedGatedView g = {ka.C, ka.ldc, row_end, ka.N, ka.flags, AUX ? ka.G_out : nullptr, AUX ? ka.U_out : nullptr, AUX ? ka.ldz : 0};

  // ---- LDS-DMA source addressing: A from the tile's first row, each weight from row n0 of the GROUP's matrix (64-bit) -------------------
  const long long w_off = (long long)group * ka.group_stride_b + (long long)tc.n0 * ka.ldb;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.A + (size_t)tc.m0 * ka.lda), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsBg = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.B + w_off), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsBu = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.Bu + w_off), 0, 0x80000000u, 0x00020000);

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const bool isA = j < NJ_A;
    const int il = wave + (isA ? j : j - NJ_A) * NW;    // piece of its operand's image: rows 8 il .. 8 il + 7
    const int r  = il * 8 + (lane >> 3);
    // A: the group's last row; B: the row of its weight, counted from n0, clamped per weight inside the group's matrix
    const int rc = isA ? min(r, g.M - 1 - tc.m0) : gated_source_row(TN, r, g.N - tc.n0);
    const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));   // slot (lane & 7) of row r holds chunk slot ^ ((r >> 1) & 7)
    voff[j] = ((uint32_t)rc * (uint32_t)(isA ? ka.lda : ka.ldb) + (uint32_t)chunk * 8u) * 2u;
  }

  // ---- fragment read offsets: hgemm_kernel_tn.hpp's ---------------------------------------------------------------------------------------
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

  // ---- pipeline: family f's ring, the B pieces through the descriptor of their weight -----------------------------------------------------
  uint32_t kbyte = 0;
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
  const int nk = ka.K / BK;
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

  // ---- the group's two bias rows (N % 8 == 0: a lane's four columns are inside N or wholly behind it, where the load returns zeros and
  // nothing is stored; a NULL bias is a descriptor of range 0: +0.0, the bits of a zero-filled row) ----------------------------------------
  using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
  using bx4 = __attribute__((ext_vector_type(4))) __bf16;
  const __amdgpu_buffer_rsrc_t rsBiasG = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.bias ? ka.bias + (size_t)group * ka.ldbias : nullptr), 0,
                                                                           ka.bias ? (uint32_t)g.N * 2u : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsBiasU = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.bias_u ? ka.bias_u + (size_t)group * ka.ldbias : nullptr), 0,
                                                                           ka.bias_u ? (uint32_t)g.N * 2u : 0u, 0x00020000);
  bx4 bg[OFN], bu[OFN];
#pragma unroll
  for (int jo = 0; jo < OFN; ++jo) {
    const uint32_t n_b = (uint32_t)(tc.n0 + gated_lane_col(wave_n, TN, jo, lane, 0));
    bg[jo] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBiasG, n_b * 2u, 0, 0));
    bu[jo] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBiasU, n_b * 2u, 0, 0));
  }
  if constexpr (AUX) {
    // ---- the pre-activations as two more outputs: the two fp32 adds made in place, then g_out = bf16(g) from acc[i][jo] and u_out = bf16(u)
    // from acc[i][jo + OFN], each at stride ldz and each behind the group's row bound; the stores only read acc
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
  // ---- the gate on the unrounded values: y = act(g) * u, parked where the gate sum was ------------------------------------------------------
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int jo = 0; jo < OFN; ++jo) {
      __builtin_amdgcn_sched_barrier(0);   // the dense gated kernel's register steering: a quad's temporaries at a time
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gv, uv;
        if constexpr (AUX) {
          gv = acc[i][jo][e];
          uv = acc[i][jo + OFN][e];
        } else {
          gv = gated_pre(acc[i][jo][e], (float)bg[jo][e]);
          uv = gated_pre(acc[i][jo + OFN][e], (float)bu[jo][e]);
        }
        float y = gated_mul(act_apply<ACT>(gv), uv);
        asm volatile("" : "+a"(y));   // the finished value waits in an accumulation register for the stores
        acc[i][jo][e] = y;
      }
    }

#include "hgemm_tn_gated_store.inc"   // C: g.M is the group's end row
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- host side: a member's launcher per (activation, aux) (hgemm_inst_g26.hip: AUX = false, hgemm_inst_g27.hip: AUX = true), the table and
// the reference kernel (hgemm_registry.hip) -------------------------------------------------------------------------------------------------
template <class CFG, int ACT, bool AUX>
void launch_tn_grouped_gated(const GroupedGatedArgs& g, int grid, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH((hgemm_tn_grouped_gated_kernel<CFG, ACT, AUX>), grid, CFG::THREADS, stream, ts, g);
}
using GroupedGatedLaunch = void (*)(const GroupedGatedArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_TN_GROUPED_GATED_LAUNCHER(ACT, AUX, CFG, BM, BN, WM, WN, NB) launch_tn_grouped_gated<CFG<BM, BN, WM, WN, NB>, ACT, AUX>
#define HGEMM_TN_GROUPED_GATED_INST(...) \
  template void HGEMM_TN_GROUPED_GATED_LAUNCHER(__VA_ARGS__)(const GroupedGatedArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_TN_GROUPED_GATED_EXTERN(...) extern HGEMM_TN_GROUPED_GATED_INST(__VA_ARGS__)
// X(activation, aux, family) per member, over the four activations
#define HGEMM_TN_GROUPED_GATED_ACTS(X, AUX) \
  HGEMM_TR_MEMBERS(X, ACT_RELU, AUX, CfgTNB) HGEMM_TR_MEMBERS(X, ACT_GELU, AUX, CfgTNB) \
  HGEMM_TR_MEMBERS(X, ACT_GELU_TANH, AUX, CfgTNB) HGEMM_TR_MEMBERS(X, ACT_SILU, AUX, CfgTNB)
HGEMM_TN_GROUPED_GATED_ACTS(HGEMM_TN_GROUPED_GATED_EXTERN, false)   // hgemm_inst_g26.hip
HGEMM_TN_GROUPED_GATED_ACTS(HGEMM_TN_GROUPED_GATED_EXTERN, true)    // hgemm_inst_g27.hip

// member `config` of tr_table_tn()'s rows, activation ACT_RELU .. ACT_SILU, with or without the saved pre-activations -> its launcher; the
// reference kernel: a thread per element, the row's group by grouped_find_row, both sums in k order, the same gated_pre / act_apply /
// gated_mul texts (g.G_out non-null: the aux form)
GroupedGatedLaunch tn_grouped_gated_launcher(int config, int act, bool aux);
void launch_tn_grouped_gated_reference(const GroupedGatedArgs& g, int act, hipStream_t stream, TimingSlot ts);

}  // namespace hgemm_mi355x
