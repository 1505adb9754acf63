// Family f, grouped (bgemm_mi355x_tn_grouped): the forward product of a mixture-of-experts layer in ONE launch.  The rows of A and C are
// sorted by group, group g owns rows [off[g], off[g + 1]) and its own weight W_g = b_col_major + g group_stride_b ([N][ldb]) and bias row:
//   C[m][n] = bf16(sum_k A[m][k] W_g[n][k] + float(bias[g][n]))      fp32 MFMA accumulation, the bias added last, one rounding.
// `offsets` lives on the DEVICE and the host never reads it: the grid is sized from a bound (hgemm_grouped.hpp) and every workgroup finds
// its tile, or that it has none, from the offsets alone.  A kernel of its own, not an epilogue of hgemm_tn_bf16_kernel: that kernel's
// tile is a function of the launch, this one's of data.
//
// The front, which is what is new (its text is hgemm_grouped_front.inc, shared with hgemm_nn_grouped_kernel):
//   * Every wave runs the map redundantly -- no LDS, no barrier, the result is wave-uniform and ends in scalar registers.  Lane l holds
//     the GROUPED_LANE_GROUPS = 4 consecutive groups 4 l .. 4 l + 3: five dword loads of off[4 l .. 4 l + 4] through a descriptor that ends
//     behind off[G] (a load past it returns 0 and touches nothing), all issued at once: ONE round trip, whatever G is, up to 256 groups.
//     Each lane clamps its groups' rows (grouped_rows) and counts their row tiles; one inclusive wave scan of the lane totals (six DPP
//     adds: row_shr 1 / 2 / 4 / 8, row_bcast 15 and 31) gives every lane the tiles in front of it.  T = total x tiles_n.
//   * blockIdx >= T: the workgroup returns, in front of its first barrier and of every operand load.  Otherwise the logical id is the XCD
//     remap over T (grouped_remap), its row-tile index q = id / tiles_n, the owning lane is the first with inclusive sum > q (one ballot),
//     the owning group the first of that lane's four whose running sum passes q, and four v_readlane bring group, prefix and the two
//     offsets to scalar registers.  grouped_raster then gives (row tile, column tile) inside the group.
//   * What the K loop holds of all this: scalars only -- the two descriptors, the tile's first row and column, the group's end row and the
//     group id (for the bias row) -- and the same per-lane offsets as the dense kernel.
// Behind the front, family f's text once more (hgemm_kernel_tn.hpp): CfgTNB, both images and the LDS-DMA ring, ds_read_b128 fragments,
// tr_mfma, the bias loads behind the K loop through a descriptor that ends at N x 2 bytes (range 0 for a NULL bias), the 16-bit C store
// text.  Edges: A's rows are clamped to the GROUP's last row and the store predicate is row < off[g + 1] -- the shared store text reads
// both from `g.M`, which here is the group's end row --, W's rows to row N - 1 of the group's weight.  A tile that straddles a group
// boundary computes rows past the boundary from the clamped row and stores none of them.
// Scope (the host sends everything else to the grouped reference kernel): K % 64 == 0, N % 8 == 0, every stride a multiple of 8, 16-byte
// aligned pointers, (BM lda + K) 2, (BN ldb + K) 2 and (BM ldc + N) 2 bytes below 2 GiB, G <= GROUPED_MAX_GROUPS.
#pragma once

#include "hgemm_grouped.hpp"
#include "hgemm_kernel_tn.hpp"

namespace hgemm_mi355x {

// 88 bytes, two kernarg lines
struct GroupedArgs {
  const __bf16* A;        // [M][lda]
  const __bf16* B;        // G weights [N][ldb], group_stride_b elements apart
  const __bf16* bias;     // [G][ldbias] or null (+0.0)
  __bf16* C;              // [M][ldc]
  const int* offsets;     // device, G + 1
  long long group_stride_b;
  int G, M, N, K;
  int lda, ldb, ldbias, ldc;
  int tiles_n;
  int flags;              // ARG_NT_STORE
};

template <class CFG>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_tn_grouped_kernel(const GroupedArgs ka) {
  prefetch_kernargs<sizeof(GroupedArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = CFG::BM, BN = CFG::BN, NBUF = CFG::NBUF;
  constexpr int FM = CFG::FM, FN = CFG::FN, NW = CFG::NW, NJ = CFG::NJ, NJ_A = CFG::NJ_A;
  constexpr int LG = GROUPED_LANE_GROUPS;
  using elem = typename CFG::elem;   // __bf16
  using ex8 = __attribute__((ext_vector_type(8))) elem;

  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / CFG::WN;
  const int wave_n = wave % CFG::WN;

  // ---- the tile map: offsets -> (group, first row, first column, the group's end row), or no tile --------------------------------
  struct { int m0, n0; } tc;
  int group, row_end;
#include "hgemm_grouped_front.inc"   // the tile map, one text with hgemm_nn_grouped_kernel
  // what the shared store text reads as `g`: M is the GROUP's end row (its predicate and A's clamp below)
  const struct { elem* C; int ldc, M, N, flags; } g = {ka.C, ka.ldc, row_end, ka.N, ka.flags};

  // ---- LDS-DMA source addressing: family f's, A from the tile's first row, W from row n0 of the group's weight (64-bit) -------------
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.A + (size_t)tc.m0 * ka.lda), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(ka.B + (long long)group * ka.group_stride_b + (long long)tc.n0 * ka.ldb), 0, 0x80000000u, 0x00020000);

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const bool isA = j < NJ_A;
    const int il = wave + (isA ? j : j - NJ_A) * NW;    // piece of its operand's tile: rows 8 il .. 8 il + 7
    const int r  = il * 8 + (lane >> 3);
    const int rc = min(r, isA ? g.M - 1 - tc.m0 : g.N - 1 - tc.n0);
    const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));   // slot (lane & 7) of row r holds chunk slot ^ ((r >> 1) & 7)
    voff[j] = ((uint32_t)rc * (uint32_t)(isA ? ka.lda : ka.ldb) + (uint32_t)chunk * 8u) * 2u;
  }

  // ---- fragment read offsets (bytes inside an operand's image): row lane & 15 of a 16-row fragment, chunk 4 ks + (lane >> 4) -------
  int f_off[2];
  {
    const int lr = lane & 15, lq = lane >> 4, sw = (lr >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) f_off[ks] = lr * ROW_BYTES + (((ks * 4 + lq) ^ sw) << 4);
  }
  const int a_row_base = wave_m * CFG::TM * ROW_BYTES;
  const int b_row_base = CFG::A_BYTES + wave_n * CFG::TN * ROW_BYTES;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;

  // ---- pipeline: family f's ring ------------------------------------------------------------------
  uint32_t kbyte = 0;
  auto stage = [&](char* lds_stage) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      lds_void_t* dst = (lds_void_t*)(lds_stage + (wave + j * NW) * 1024);
      if (j < NJ_A) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voff[j], kbyte, 0, 0);
      else          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, voff[j], kbyte, 0, 0);
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
      for (int i = 0; i < FM; ++i) af[i] = *(const ex8*)(st + a_row_base + i * 16 * ROW_BYTES + f_off[ks]);
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[j] = *(const ex8*)(st + b_row_base + j * 16 * ROW_BYTES + f_off[ks]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = tr_mfma(bf[j], af[i], acc[i][j]);
    }
    rd = (rd + 1 == NBUF) ? 0 : rd + 1;
    wr = (wr + 1 == NBUF) ? 0 : wr + 1;
  }

  // ---- the group's bias row, added last in fp32 (the EPI_C16_BIAS text; a NULL bias is a descriptor of range 0: +0.0) ---------------
  {
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    using bx4 = __attribute__((ext_vector_type(4))) __bf16;
    const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.bias ? ka.bias + (size_t)group * ka.ldbias : nullptr), 0,
                                                                            ka.bias ? (uint32_t)g.N * 2u : 0u, 0x00020000);
    bx4 bias[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const uint32_t n_b = (uint32_t)(tc.n0 + wave_n * CFG::TN + 16 * j + 4 * (lane >> 4));
      bias[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBias, n_b * 2u, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] += (float)bias[j][e];
  }

#include "hgemm_tr_store_c16.inc"   // the 16-bit C epilogue: g.M is the group's end row
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- host side: the member's launcher (hgemm_inst_g23.hip), the table and the reference kernel (hgemm_registry.hip) ---------------------
template <class CFG>
void launch_tn_grouped(const GroupedArgs& g, int grid, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH((hgemm_tn_grouped_kernel<CFG>), grid, CFG::THREADS, stream, ts, g);
}
using GroupedLaunch = void (*)(const GroupedArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_TN_GROUPED_LAUNCHER(CFG, BM, BN, WM, WN, NB) launch_tn_grouped<CFG<BM, BN, WM, WN, NB>>
#define HGEMM_TN_GROUPED_INST(...) template void HGEMM_TN_GROUPED_LAUNCHER(__VA_ARGS__)(const GroupedArgs&, int, hipStream_t, TimingSlot);
#define HGEMM_TN_GROUPED_EXTERN(...) extern HGEMM_TN_GROUPED_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TN_GROUPED_EXTERN, CfgTNB)   // hgemm_inst_g23.hip

// member `config` of tr_table_tn()'s rows -> its grouped launcher; the reference kernel: a thread per element, the row's group by binary
// search over the same clamped offsets (grouped_find_row), the sum in k order, the same add and rounding
GroupedLaunch tn_grouped_launcher(int config);
void launch_tn_grouped_reference(const GroupedArgs& g, hipStream_t stream, TimingSlot ts);

}  // namespace hgemm_mi355x
