// Family a, grouped (bgemm_mi355x_ta_grouped / _ta_grouped_c32): the weight gradient of a mixture-of-experts layer in ONE launch.  The rows of
// both operands are sorted by group, group g owns k-rows [s_g, e_g) = grouped_rows(off[g], off[g + 1], K) of a_col_major ([K][lda], = dY) and of
// the row-major b ([K][ldb], = X), and a whole matrix of its own, C_g = c + g group_stride_c ([M][ldc]):
//   S_g[m][n] = sum over t in [s_g, e_g) of a[t][m] b[t][n]      fp32 MFMA accumulation, t ascending in the dense kernel's order
//   EPI_C32: C_g = S_g, or C_g + S_g with ARG_ACCUMULATE (one fp32 add per element); EPI_C16: C_g = bf16(S_g), rounded once.
// `offsets` lives on the DEVICE and the host never reads it.  A kernel of its own, not a flag in hgemm_ta_kernel: there the K walk is a
// function of the launch, here of data, and the dense kernels keep their instruction streams.
//
// What is new against hgemm_kernel_ta.hpp:
//   * The grid is EXACT, G tiles_m tiles_n: the group boundary cuts the K walk and not the rows of C, so no id is without a tile and nothing
//     is scanned (the forward kernel's front, hgemm_kernel_tn_grouped.hpp, does not carry over).  ta_grouped_tile (hgemm_grouped.hpp): the XCD
//     remap over the grid, group = L / (tiles_m tiles_n) -- a group's tiles are one contiguous run of logical ids, so an XCD works on one
//     expert's rows of both operands at a time and every tile of the group re-reads them from L2 --, the family's raster inside the group.
//   * off[g] and off[g + 1] are two wave-uniform dword reads through the constant address space (scalar: the offsets are an input, no
//     kernel of this launch writes them), which compile to ONE scalar two-dword load from offsets + g -- 4-byte aligned only, which a
//     scalar load allows --, issued right behind the kernarg wait: one round trip in front of the first DMA piece.  s, e and
//     nk = ceil((e - s) / 64) stay in scalar registers.
//   * Start of the walk: both descriptors start at k-row s_g of their matrix -- any integer; the base stays 16-byte aligned because lda and
//     ldb are multiples of 8 --, the per-lane offsets and the stage strides are the dense kernel's with k_begin = 0.
//   * END of the walk, the one thing that can go wrong silently: both descriptors END WITH THE GROUP'S LAST ROW, A after
//     ((rows - 1) lda + (M - m0)) 2 bytes and B after ((rows - 1) ldb + (N - n0)) 2.  A k-row >= rows of the last, partial stage starts at
//     rows lda 2 >= that range (lda >= M - m0), so every chunk of it is out of range for every lane, and an out-of-range lane of an LDS-DMA
//     load writes ZEROS into the LDS.  The classic family's K tail rests on the same rule (stage_tile_tail); families n, a and f have never
//     relied on it for values that reach a stored accumulator.  THIS KERNEL DOES, for both operands: the products of the k-rows behind the
//     group are 0 x 0 and never 0 x NaN, whatever the neighbouring group's rows hold.  In front of the group nothing is read at all.
//   * Short walks: nk = 1 and 2 are below NBUF - 1; the prologue's `if (s < nk)` and the vmcnt ladder hold there as in the dense kernel at
//     K = 64 and 128.  rows = 1 is a legal group.
//   * Empty group (nk = 0): with ARG_ACCUMULATE the workgroup returns -- wave- and workgroup-uniform, in front of the first barrier and of
//     every load, so C_g is neither read nor written --; without it the loop does not run and the zeroed accumulators go through the normal
//     epilogue: +0.0.  No lane-dependent branch stands in front of the K loop (the transposed read's EXEC rule).
//   * C: the descriptor base is c + g group_stride_c + m0 ldc in 64-bit arithmetic; the store predicates are the dense kernel's (M, N).
// Unchanged, family a's text once more: CfgTAB, both images and nn_swz, the LDS-DMA ring with one barrier per stage and counted vmcnt, the
// ds_read_b64_tr_b16 fragments and tr_mfma, the EPI_C32 store text and hgemm_tr_store_c16.inc.
// Scope (the host sends everything else to the grouped TA reference kernel): M % 8 == 0, N % 8 == 0, lda / ldb multiples of 8, ldc and
// group_stride_c multiples of 4 (fp32 C) / 8 (bf16 C), 16-byte aligned pointers, family a's reach rules with K rounded up to a stage as the
// bound on a group's rows (the lane offsets of the last, partial stage must not wrap), a grid that fits an int.  K and the offsets are free.
#pragma once

#include "hgemm_grouped.hpp"
#include "hgemm_kernel_ta.hpp"

namespace hgemm_mi355x {

// 80 bytes, two kernarg lines
struct TaGroupedArgs {
  const __bf16* A;        // a_col_major [K][lda]
  const __bf16* B;        // row-major [K][ldb]
  void* C;                // G matrices [M][ldc], group_stride_c elements apart: float (EPI_C32) or bf16 (EPI_C16)
  const int* offsets;     // device, G + 1
  long long group_stride_c;
  int G, M, N, K;
  int lda, ldb, ldc;
  int tiles_m, tiles_n;
  int flags;              // ARG_NT_STORE, ARG_ACCUMULATE
};

template <class CFG, int EPI>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_ta_grouped_kernel(const TaGroupedArgs ka) {
  prefetch_kernargs<sizeof(TaGroupedArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = CFG::BM, BN = CFG::BN, NBUF = CFG::NBUF;
  constexpr int FM = CFG::FM, FN = CFG::FN, NW = CFG::NW, NJ = CFG::NJ, NJ_A = CFG::NJ_A;
  using elem = typename CFG::elem;   // __bf16
  using ex4 = __attribute__((ext_vector_type(4))) elem;
  using ex8 = __attribute__((ext_vector_type(8))) elem;
  using cel = std::conditional_t<EPI == EPI_C32, float, elem>;   // what C holds
  static_assert(EPI == EPI_C16 || EPI == EPI_C32, "bf16 C and fp32 C; there is no split form");

  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / CFG::WN;
  const int wave_n = wave % CFG::WN;

  // ---- the tile and the group's walk: scalars only ------------------------------------------------------------------------------
  const TaGroupedTile tile = ta_grouped_tile(grouped_remap((int)blockIdx.x, (int)gridDim.x), ka.tiles_m, ka.tiles_n);
  const __attribute__((address_space(4))) int* off = (const __attribute__((address_space(4))) int*)ka.offsets + tile.g;
  const GroupRows gr = grouped_rows(off[0], off[1], ka.K);
  const int rows = gr.end - gr.start;
  const int nk = ta_grouped_stages(gr, BK);
  if constexpr (EPI == EPI_C32) {
    if (nk == 0 && (ka.flags & ARG_ACCUMULATE)) return;   // uniform; C_g untouched
  }
  const struct { int m0, n0; } tc = {tile.tile_m * BM, tile.tile_n * BN};
  // what the store texts read as `g`: the group's C, the dense kernel's predicates
  const struct { cel* C; int ldc, M, N, flags; } g = {(cel*)ka.C + (long long)tile.g * ka.group_stride_c, ka.ldc, ka.M, ka.N, ka.flags};

  // ---- LDS-DMA source addressing: from k-row s_g, ending with the group's last row (see the head of the file) ---------------------------
  const int last = rows > 0 ? rows - 1 : 0;
  const uint32_t a_bytes = rows > 0 ? (uint32_t)(((size_t)last * ka.lda + (ka.M - tc.m0)) * 2) : 0u;   // (< 2 GiB: host check)
  const uint32_t b_bytes = rows > 0 ? (uint32_t)(((size_t)last * ka.ldb + (ka.N - tc.n0)) * 2) : 0u;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.A + (size_t)gr.start * ka.lda + tc.m0), 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)(ka.B + (size_t)gr.start * ka.ldb + tc.n0), 0, b_bytes, 0x00020000);
  const uint32_t a_stage = (uint32_t)ka.lda * (uint32_t)(BK * 2);   // bytes between two stages of A ...
  const uint32_t b_stage = (uint32_t)ka.ldb * (uint32_t)(BK * 2);   // ... and of B

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j < NJ_A) {
      const int il = wave + j * NW;                     // piece of the A tile: k-rows il * A_RPP ..
      const int kr = il * CFG::A_RPP + lane / CFG::A_CH;
      const int chunk = (lane % CFG::A_CH) ^ nn_swz<BM>(kr);
      voff[j] = ((uint32_t)kr * (uint32_t)ka.lda + (uint32_t)chunk * 8u) * 2u;
    } else {
      const int il = wave + (j - NJ_A) * NW;            // piece of the B tile: k-rows il * B_RPP ..
      const int kr = il * CFG::B_RPP + lane / CFG::B_CH;
      const int chunk = (lane % CFG::B_CH) ^ nn_swz<BN>(kr);
      voff[j] = ((uint32_t)kr * (uint32_t)ka.ldb + (uint32_t)chunk * 8u) * 2u;
    }
  }

  // ---- fragment read offsets (bytes inside a stage): family a's ------------------------------------------------------------------
  int a_off[2][FM], b_off[2][FN];
  {
    const int gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kr = 8 * gq + 4 * h + q;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int chunk = (wave_m * CFG::TM + i * 16) / 8 + (p >> 1);
        a_off[h][i] = kr * CFG::A_ROW_BYTES + ((chunk ^ nn_swz<BM>(kr)) << 4) + 8 * (p & 1);
      }
#pragma unroll
      for (int jn = 0; jn < FN; ++jn) {
        const int chunk = (wave_n * CFG::TN + jn * 16) / 8 + (p >> 1);
        b_off[h][jn] = CFG::A_BYTES + kr * CFG::B_ROW_BYTES + ((chunk ^ nn_swz<BN>(kr)) << 4) + 8 * (p & 1);
      }
    }
  }

  f32x4 acc[FM][FN];
  tr_zero(acc);

  // ---- pipeline: family a's ring ---------------------------------------------------------------------------------------------------
  auto stage = [&](char* lds_stage) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      lds_void_t* dst = (lds_void_t*)(lds_stage + (wave + j * NW) * 1024);
      if (j < NJ_A) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voff[j], 0, 0, 0);
        voff[j] += a_stage;
      } else {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, voff[j], 0, 0, 0);
        voff[j] += b_stage;
      }
    }
  };
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
      const char* pa = st + ks * 32 * CFG::A_ROW_BYTES;
      const char* pb = st + ks * 32 * CFG::B_ROW_BYTES;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const ex4 lo = __builtin_bit_cast(ex4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_t*)(pa + a_off[0][i])));
        const ex4 hi = __builtin_bit_cast(ex4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_t*)(pa + a_off[1][i])));
        af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
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

  if constexpr (EPI == EPI_C32) {
    // family a's EPI_C32 store text (hgemm_kernel_ta.hpp): 16 consecutive bytes per (i, j), the old value loaded first with ARG_ACCUMULATE
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(g.C + (size_t)tc.m0 * g.ldc), 0, 0xFFFFFFFFu, 0x00020000);
    const int q = lane >> 4;
    const bool accumulate = (g.flags & ARG_ACCUMULATE) != 0;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      __builtin_amdgcn_sched_barrier(0);   // one fragment row's accumulator reads at a time (store_tile)
      const int row = wave_m * CFG::TM + i * 16 + (lane & 15);
      const bool row_ok = tc.m0 + row < g.M;
      f32x4 v[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) v[j] = acc[i][j];
      if (accumulate) {
        f32x4 old[FN];
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int n = tc.n0 + wave_n * CFG::TN + 16 * j + 4 * q;
          const uint32_t off = ((uint32_t)row * (uint32_t)g.ldc + (uint32_t)n) * 4u;
          old[j] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (row_ok && n < g.N) old[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsC, off, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) v[j] = old[j] + v[j];
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = tc.n0 + wave_n * CFG::TN + 16 * j + 4 * q;
        if (row_ok && n < g.N) {
          const u32x4 o = __builtin_bit_cast(u32x4, v[j]);
          const uint32_t off = ((uint32_t)row * (uint32_t)g.ldc + (uint32_t)n) * 4u;
          if (g.flags & ARG_NT_STORE) __builtin_amdgcn_raw_buffer_store_b128(o, rsC, off, 0, 2);
          else                        __builtin_amdgcn_raw_buffer_store_b128(o, rsC, off, 0, 0);
        }
      }
    }
  } else {
#include "hgemm_tr_store_c16.inc"   // the 16-bit C epilogue, one text for families n, a and f
  }
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- host side: the member's launcher of both forms (hgemm_inst_g24.hip), the table and the reference kernel (hgemm_registry.hip) -------
template <class CFG>
void launch_ta_grouped(const TaGroupedArgs& g, int grid, hipStream_t stream, bool c32, TimingSlot ts) {
  if (c32) HGEMM_LAUNCH((hgemm_ta_grouped_kernel<CFG, EPI_C32>), grid, CFG::THREADS, stream, ts, g);
  else     HGEMM_LAUNCH((hgemm_ta_grouped_kernel<CFG, EPI_C16>), grid, CFG::THREADS, stream, ts, g);
}
using TaGroupedLaunch = void (*)(const TaGroupedArgs&, int, hipStream_t, bool, TimingSlot);
#define HGEMM_TA_GROUPED_LAUNCHER(CFG, BM, BN, WM, WN, NB) launch_ta_grouped<CFG<BM, BN, WM, WN, NB>>
#define HGEMM_TA_GROUPED_INST(...) template void HGEMM_TA_GROUPED_LAUNCHER(__VA_ARGS__)(const TaGroupedArgs&, int, hipStream_t, bool, TimingSlot);
#define HGEMM_TA_GROUPED_EXTERN(...) extern HGEMM_TA_GROUPED_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TA_GROUPED_EXTERN, CfgTAB)   // hgemm_inst_g24.hip

// member `config` of tr_table_ta()'s rows -> its grouped launcher; the reference kernel: a thread per element of every C_g, fmaf over the
// group's k-rows ascending, the same grouped_rows and the same empty-group rule, the kinds' Out functors
TaGroupedLaunch ta_grouped_launcher(int config);
void launch_ta_grouped_reference(const TaGroupedArgs& g, bool c32, hipStream_t stream, TimingSlot ts);

}  // namespace hgemm_mi355x
