// Family n, grouped (bgemm_mi355x_nn_grouped): the input gradient of a mixture-of-experts layer in ONE launch.  The rows of A (= dY), r and C
// (= dX) are sorted by group, group g owns rows [off[g], off[g + 1]) and its own ROW-MAJOR matrix B_g = b + g group_stride_b ([K][ldb], N
// contiguous) -- for the forward Y = X W_g^T with W_g [Nout][Kin] this is the forward call's weight buffer AS IT LIES, K = Nout, N = Kin:
//   S = sum_k A[m][k] B_g[k][n]                     fp32 MFMA accumulation, the dense NN kernel's order
//   EPI_C16:      C[m][n] = bf16(S)
//   EPI_C16_ADD:  C[m][n] = bf16(residual_add(S, float(r[m][n])))      one fp32 add, one rounding; r may be C itself (ldr == ldc)
// Two epilogues and not a NULL r read as +0.0: S = -0.0 stays -0.0 in the plain form, which G = 1 owes to bgemm_mi355x_launch_nn bit for bit.
// `offsets` lives on the DEVICE and the host never reads it.  A kernel of its own, not an epilogue of hgemm_nn_kernel: that kernel's tile is
// a function of the launch, this one's of data, and the dense kernels keep their instruction streams.
//
// The front is the forward kernel's, one text (hgemm_grouped_front.inc): lane-held groups, one round trip of offset loads,
// the DPP wave scan, a ballot and four readlanes, grouped_remap over the real tile count T, grouped_raster -- the row tile runs fastest
// inside a group, so neighbouring workgroups share the K x BN column panel of B_g.  The grid is the host's bound; ids >= T return in front of
// every barrier and operand load.
//
// EXEC at the transposed reads (hgemm_kernel_nn.hpp: ds_read_b64_tr_b16 needs all lanes active, wrong data without a fault otherwise):
//   * The kernel starts with EXEC all ones (THREADS is a multiple of 64) and the front's three exits are taken on values that are kernel
//     arguments, blockIdx or the result of v_readlane: uniform in the wave, scalar branches -- a wave leaves whole or not at all.
//   * The front's one lane-dependent piece, each lane's walk over its own four groups (`if (go)`), is structured control flow closed inside
//     the front's block: the compiler restores EXEC where each `if` ends (as compiled for gfx950: s_and_saveexec regions, every one closed by
//     s_or_b64 exec in front of the readlanes).  The four readlanes behind it already run with every lane active.
//   * From there to the end of the K loop no condition depends on the lane: the prologue's `s < nk`, the vmcnt ladder and the loop's
//     `t + NBUF - 1 < nk` read the kernel argument K alone; clamps and swizzles are arithmetic (min, xor), not branches.  The first
//     lane-dependent predicates of the kernel are the store text's, behind the last LDS read.
//
// Behind the front, family n's text once more (hgemm_kernel_nn.hpp): CfgNNB, the classic A image and the [64 k-rows][BN] B image with
// nn_swz, the LDS-DMA ring with one barrier per stage and counted vmcnt, ds_read_b128 for A and two transposed reads per B fragment,
// tr_mfma, nn_add's residual loads behind the K loop, hgemm_tr_store_c16.inc.  What differs:
//   * A: the descriptor starts at the tile's first row; rows are clamped to the GROUP's last row and the store predicate is row < off[g + 1]
//     -- the shared store text reads both from `g.M`, which here is the group's end row.  A tile that straddles a group boundary computes the
//     rows past it from the clamped row and stores none of them.
//   * B: the descriptor starts at column n0 of row 0 of the GROUP's matrix (the group offset in 64 bits) and ENDS WITH THAT MATRIX, after
//     ((K - 1) ldb + (N - n0)) 2 bytes: a chunk at columns >= N reads pad, the next k-row or zeros behind the group's last element -- never
//     behind the whole buffer -- and only feeds accumulators of columns >= N, which are not stored.
//   * r: the descriptor runs from the tile's first row to r's last valid element OF THE GROUP, dact_z_range_bytes(row_end, N, ldr, m0): a row
//     behind the group boundary reads zeros and touches nothing -- with r == C those rows are another workgroup's to read and write.
// Scope (the host sends everything else to the grouped NN reference kernel): K % 64 == 0, N % 8 == 0, every stride a multiple of 8, 16-byte
// aligned pointers, (BM lda + K) 2, ((K - 1) ldb + N) 2, (BM ldc + N) 2 and (BM ldr + N) 2 bytes below 2 GiB, G <= GROUPED_MAX_GROUPS.
#pragma once

#include "hgemm_grouped.hpp"
#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

// 88 bytes, two kernarg lines
struct NnGroupedArgs {
  const __bf16* A;        // [M][lda]
  const __bf16* B;        // G row-major matrices [K][ldb], group_stride_b elements apart
  const __bf16* R;        // [M][ldr] or null (EPI_C16); may be C
  __bf16* C;              // [M][ldc]
  const int* offsets;     // device, G + 1
  long long group_stride_b;
  int G, M, N, K;
  int lda, ldb, ldr, ldc;
  int tiles_n;
  int flags;              // ARG_NT_STORE
};

template <class CFG, int EPI>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_nn_grouped_kernel(const NnGroupedArgs ka) {
  prefetch_kernargs<sizeof(NnGroupedArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = CFG::BM, BN = CFG::BN, NBUF = CFG::NBUF;
  constexpr int FM = CFG::FM, FN = CFG::FN, NW = CFG::NW, NJ = CFG::NJ, NJ_A = CFG::NJ_A;
  constexpr int LG = GROUPED_LANE_GROUPS;
  using elem = typename CFG::elem;   // __bf16
  using ex4 = __attribute__((ext_vector_type(4))) elem;
  using ex8 = __attribute__((ext_vector_type(8))) elem;
  static_assert((EPI == EPI_C16 || EPI == EPI_C16_ADD) && __is_same(elem, __bf16), "bf16 C, plain or with the residual; there is no split form");

  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / CFG::WN;
  const int wave_n = wave % CFG::WN;

  // ---- the tile map: offsets -> (group, first row, first column, the group's end row), or no tile --------------------------------
  struct { int m0, n0; } tc;
  int group, row_end;
#include "hgemm_grouped_front.inc"   // the tile map, one text with hgemm_tn_grouped_kernel; every lane is active behind it
  // what the shared store text reads as `g`: M is the GROUP's end row (its predicate and A's clamp below)
  const struct { elem* C; int ldc, M, N, flags; } g = {ka.C, ka.ldc, row_end, ka.N, ka.flags};

  // ---- LDS-DMA source addressing: family n's, A from the tile's first row, B from column n0 of the GROUP's matrix to that matrix's end ----
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.A + (size_t)tc.m0 * ka.lda), 0, 0x80000000u, 0x00020000);
  const uint32_t b_bytes = (uint32_t)(((size_t)(ka.K - 1) * ka.ldb + (g.N - tc.n0)) * 2);   // (< 2 GiB: host check)
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void*)(ka.B + (long long)group * ka.group_stride_b + tc.n0), 0, b_bytes, 0x00020000);
  const uint32_t b_stage = (uint32_t)ka.ldb * (uint32_t)(BK * 2);   // bytes between two stages of B

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j < NJ_A) {
      const int il = wave + j * NW;                     // piece of the A tile
      const int r  = il * 8 + (lane >> 3);
      const int rc = min(r, g.M - 1 - tc.m0);           // the group's last row
      const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));   // slot (lane & 7) of row r holds chunk slot ^ ((r >> 1) & 7)
      voff[j] = ((uint32_t)rc * (uint32_t)ka.lda + (uint32_t)chunk * 8u) * 2u;
    } else {
      const int il = wave + (j - NJ_A) * NW;            // piece of the B tile: k-rows il * B_RPP ..
      const int kr = il * CFG::B_RPP + lane / CFG::B_CH;
      const int chunk = (lane % CFG::B_CH) ^ nn_swz<BN>(kr);
      voff[j] = ((uint32_t)kr * (uint32_t)ka.ldb + (uint32_t)chunk * 8u) * 2u;
    }
  }

  // ---- fragment read offsets (bytes inside a stage): family n's ---------------------------------------------------------------------
  int a_off[2];
  {
    const int lr = lane & 15, lq = lane >> 4, sw = (lr >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a_off[ks] = wave_m * CFG::TM * ROW_BYTES + lr * ROW_BYTES + (((ks * 4 + lq) ^ sw) << 4);
  }
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

  // ---- pipeline: family n's ring ------------------------------------------------------------------------------------------------------
  uint32_t kbyte = 0;
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
  const int nk = ka.K / BK;
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

  // ---- the fused residual add (EPI_C16_ADD): nn_add's loads, the descriptor ending with the GROUP's last row of r -----------------------
  // Every load of the wave's tile is issued and consumed in this block, in front of the store text; the element a lane stores there is
  // computed from that element's r, so with r == C its store depends on its load.  Rows at or behind row_end are out of range: zeros.
  if constexpr (EPI == EPI_C16_ADD) {
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    using bx4 = __attribute__((ext_vector_type(4))) __bf16;
    const uint32_t ldr = (uint32_t)ka.ldr;
    const uint32_t r_bytes = dact_z_range_bytes(row_end, g.N, ka.ldr, tc.m0);
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.R + (size_t)tc.m0 * ldr), 0, r_bytes, 0x00020000);
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

#include "hgemm_tr_store_c16.inc"   // the 16-bit C epilogue: g.M is the group's end row
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- host side: the member's launcher of both forms (hgemm_inst_g25.hip), the table and the reference kernel (hgemm_registry.hip) ---------
template <class CFG>
void launch_nn_grouped(const NnGroupedArgs& g, int grid, hipStream_t stream, TimingSlot ts) {
  if (g.R) HGEMM_LAUNCH((hgemm_nn_grouped_kernel<CFG, EPI_C16_ADD>), grid, CFG::THREADS, stream, ts, g);
  else     HGEMM_LAUNCH((hgemm_nn_grouped_kernel<CFG, EPI_C16>), grid, CFG::THREADS, stream, ts, g);
}
using NnGroupedLaunch = void (*)(const NnGroupedArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_NN_GROUPED_LAUNCHER(CFG, BM, BN, WM, WN, NB) launch_nn_grouped<CFG<BM, BN, WM, WN, NB>>
#define HGEMM_NN_GROUPED_INST(...) template void HGEMM_NN_GROUPED_LAUNCHER(__VA_ARGS__)(const NnGroupedArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_NN_GROUPED_EXTERN(...) extern HGEMM_NN_GROUPED_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_NN_GROUPED_EXTERN, CfgNNB)   // hgemm_inst_g25.hip

// member `config` of tr_table_nn()'s rows -> its grouped launcher; the reference kernel: a thread per element, the row's group by binary
// search over the same clamped offsets (grouped_find_row), fmaf over k ascending, the dense kinds' output policies (OutC16 / OutAdd)
NnGroupedLaunch nn_grouped_launcher(int config);
void launch_nn_grouped_reference(const NnGroupedArgs& g, hipStream_t stream, TimingSlot ts);

}  // namespace hgemm_mi355x
