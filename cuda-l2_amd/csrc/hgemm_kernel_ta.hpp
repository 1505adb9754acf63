// Family "a": TA operand form (transposed A) -- C[M,N] = A[M,K] * B[K,N] with A given as a_col_major ([K][lda], M contiguous) and B
// ROW-MAJOR ([K][ldb], N contiguous): a linear layer's weight gradient dW = X^T dY, whose first operand is the activation as it is
// stored, [tokens][features].  Completes the layer's three products next to the b_col_major families (forward) and family n (input
// gradient).  The vendor baselines call this form "nt"; in this code NT means non-temporal stores throughout, hence "ta".
// Replaces, for such a caller, a transposed copy of A (2 M K bytes read and written) in front of hgemm_mi355x_nn_*; the vendor
// baseline is hgemm_rocblas_ta.
//
// Family n's structure (hgemm_kernel_nn.hpp): NBUF-deep LDS ring of K = 64 stages, ONE barrier per stage, counted vmcnt, LDS-DMA
// fills, v_mfma_f32_16x16x32_f16 with fp32 accumulation, operands swapped so that a lane owns 4 consecutive N of a C row.
//   * B image and its reads: exactly family n's -- [64 k-rows][BN halfs], chunk c of k-row kr at slot c ^ nn_swz<BN>(kr).
//   * A image: [64 k-rows][BM halfs], as A lies in memory -- the shape of family n's B image.  A k-row of the tile is BM * 2
//     contiguous bytes, a 1-KiB DMA piece is 512 / BM whole k-rows, chunk c of k-row kr sits at slot c ^ nn_swz<BM>(kr); the
//     swizzle is applied to the lane's DMA SOURCE address and undone on the read.  Piece counts are the classic ones: BM / 8 for A,
//     BN / 8 for B.
//   * A descriptor: starts at column m0 of k-row 0 and ENDS WITH THE MATRIX, ((K - 1) lda + (M - m0)) * 2 bytes; the whole offset
//     (k-row and chunk) is in the lane's register and advances by 64 lda elements per stage, as B's does.  No scalar K offset.
//   * A fragments: the MFMA operand of lane (m = lane & 15, kq = lane >> 4) is k = 8 kq .. 8 kq + 7 of column m of the image, from
//     two ds_read_b64_tr_b16 per 16-row fragment and K = 32 slice: lane 4q + p of 16-lane group gq addresses k-row
//     32 ks + 8 gq + 4 h + q (h = 0, 1: the two reads), chunk (wave_m TM + 16 i) / 8 + (p >> 1), its half p & 1.  There is no
//     ds_read_b128 in the K loop.
//   * The two hardware rules of the transposed read (each gives wrong data without a fault) hold for every read of both operands:
//     every lane address is a multiple of 8 from a 1024-aligned array, and EXEC is all ones -- no lane-dependent branch or early
//     return in front of the K loop; out-of-tile lanes read in-bounds LDS.
//   * Edges: a chunk at columns >= M (A) / >= N (B) reads whatever follows in memory -- the next k-row, padding, or zeros behind the
//     end of the matrix, where the descriptor ends -- and only feeds accumulators of rows >= M / columns >= N, which are never
//     stored; stores are predicated.  Scope (the host sends anything else to the reference kernel): K % 64 == 0, M % 8 == 0,
//     N % 8 == 0, lda / ldb / ldc multiples of 8, 16-byte aligned pointers; A and B within 2 GiB from row 0 to the end of the matrix,
//     a C tile within 2 GiB from its first row.
//   * Epilogues: family n's: fp16 C (plain and non-temporal) and the two-pass split-K slab (hgemm_splitk_reduce_kernel combines).
//     EPI_C32 (hgemm_inst_g7.hip, hgemm_mi355x_ta_c32): the fp32 accumulators stored to, or added into, the caller's fp32 C -- the
//     weight gradient where a training step consumes it; its two-pass form combines the same slabs with
//     hgemm_splitk_reduce_c32_kernel.
//   * Shared with family n: the Cfg base (CfgTR), launch_tr, the member list and its macros, the table types, nn_swz, tr_zero and the 16-bit C
//     epilogue (hgemm_tr_store_c16.inc).  The preamble, the images and the ring are family n's text once more, on purpose: as shared
//     functions -- the whole body, or an image's addressing and reads alone -- they compiled to a different K loop in every kernel
//     (DESIGN.md 4.22).
//   tests/test_ta_host.py replays the A image with tests/nn_layout_model.py (bn := BM, tn := TM, wave_n := wave_m) and restates the
//   lane address expression of a_off below.
#pragma once

#include "hgemm_kernel_nn.hpp"

namespace hgemm_mi355x {

template <class CFG, int EPI>
__global__ void hgemm_ta_kernel(const GemmArgs g);

// family n's Cfg (CfgTR: wave tiling, B image, ring) with the A image above
template <int BM_, int BN_, int WM_, int WN_, int NBUF_>
struct CfgTA : CfgTR<BM_, BN_, WM_, WN_, NBUF_, BK * BM_ * 2> {
  static constexpr int BM          = BM_;                  // (CfgTR's: a dependent base's names are not found unqualified)
  static constexpr int A_ROW_BYTES = BM * 2;               // one k-row of the A image
  static constexpr int A_CH        = BM / 8;               // 16-byte chunks per k-row
  static constexpr int A_RPP       = 64 / A_CH;            // k-rows per 1-KiB DMA piece
  static_assert(BM == 64 || BM == 128, "nn_swz is defined for 128- and 256-byte k-rows");
  template <int EPI>
  static constexpr auto kernel() { return &hgemm_ta_kernel<CfgTA, EPI>; }   // the family's entry point (launch_tr)
};

// bfloat16 operands and 16-bit C (bgemm_mi355x_ta / _ta_c32, hgemm_inst_g9.hip / g10): CfgNNB's trait on this family's Cfg (hgemm_kernel_nn.hpp)
template <int BM_, int BN_, int WM_, int WN_, int NBUF_>
struct CfgTAB : CfgTA<BM_, BN_, WM_, WN_, NBUF_> {
  using elem = __bf16;
  template <int EPI>
  static constexpr auto kernel() { return &hgemm_ta_kernel<CfgTAB, EPI>; }
};

// GemmArgs as the kernel reads it: A = a_col_major ([K][lda], lda >= M its row stride), Bt = the ROW-MAJOR B ([K][ldb], ldb >= N);
// tail_tiles = 0, counters = nullptr.
template <class CFG, int EPI>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_ta_kernel(const GemmArgs g) {
  prefetch_kernargs<sizeof(GemmArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = CFG::BM, BN = CFG::BN, NBUF = CFG::NBUF;
  constexpr int FM = CFG::FM, FN = CFG::FN, NW = CFG::NW, NJ = CFG::NJ, NJ_A = CFG::NJ_A;
  using elem = typename CFG::elem;   // f16, or __bf16 (the bgemm_ entry points)
  using ex4 = __attribute__((ext_vector_type(4))) elem;
  using ex8 = __attribute__((ext_vector_type(8))) elem;
  static_assert(EPI == EPI_C16 || EPI == EPI_SLAB || EPI == EPI_C32, "plain (fp16 C, fp32 C) and two-pass slab epilogues");

  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / CFG::WN;
  const int wave_n = wave % CFG::WN;

  const TileCoord tc = map_block(g, BM, BN);

  // ---- LDS-DMA source addressing ---------------------------------------------------------------
  // Both descriptors start at the tile's first column of k-row 0 and END WITH THE MATRIX; the whole offset (k-row and chunk) is in
  // the lane's register, which is what the range check sees: a chunk behind the last element reads as zeros.
  const uint32_t a_bytes = (uint32_t)(((size_t)(g.K - 1) * g.lda + (g.M - tc.m0)) * 2);   // (< 2 GiB: host check)
  const uint32_t b_bytes = (uint32_t)(((size_t)(g.K - 1) * g.ldb + (g.N - tc.n0)) * 2);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + tc.m0), 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)(g.Bt + tc.n0), 0, b_bytes, 0x00020000);
  const uint32_t a_stage = (uint32_t)g.lda * (uint32_t)(BK * 2);   // bytes between two stages of A ...
  const uint32_t b_stage = (uint32_t)g.ldb * (uint32_t)(BK * 2);   // ... and of B

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j < NJ_A) {
      const int il = wave + j * NW;                     // piece of the A tile: k-rows il * A_RPP ..
      const int kr = il * CFG::A_RPP + lane / CFG::A_CH;
      const int chunk = (lane % CFG::A_CH) ^ nn_swz<BM>(kr);
      voff[j] = ((uint32_t)(tc.k_begin + kr) * (uint32_t)g.lda + (uint32_t)chunk * 8u) * 2u;
    } else {
      const int il = wave + (j - NJ_A) * NW;            // piece of the B tile: k-rows il * B_RPP ..
      const int kr = il * CFG::B_RPP + lane / CFG::B_CH;
      const int chunk = (lane % CFG::B_CH) ^ nn_swz<BN>(kr);
      voff[j] = ((uint32_t)(tc.k_begin + kr) * (uint32_t)g.ldb + (uint32_t)chunk * 8u) * 2u;
    }
  }

  // ---- fragment read offsets (bytes inside a stage) ---------------------------------------------
  // transposed reads: lane 4q + p of 16-lane group gq addresses k-row 8 gq + 4 h + q (h = 0, 1: the two reads), columns 4p .. 4p + 3
  // of fragment i (A) / column tile jn (B) -- 16-byte chunk 2 (fragment) + (p >> 1), its half p & 1.  (+ ks * 32 rows per K = 32
  // slice: nn_swz does not see it.)  tests/test_ta_host.py: ta_read_address restates a_off.
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

  // ---- pipeline ----------------------------------------------------------------------------------
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

  if constexpr (EPI == EPI_SLAB) {
    store_tile<16, FM, FN, CFG::TM, CFG::TN, true>(g, tc, wave_m, wave_n, lane, acc);
  } else if constexpr (EPI == EPI_C32) {
    // fp32 C (the weight gradient added into an fp32 gradient buffer): g.C holds the float pointer, g.ldc counts fp32 elements.  A lane
    // owns n = 16 j + 4 (lane >> 4) + 0 .. 3 of C row lane & 15 per acc[i][j], 16 consecutive bytes: one buffer store per (i, j), no lane
    // exchange and no conversion.  With ARG_ACCUMULATE (wave-uniform) the old 16 bytes are loaded first -- a fragment row's FN loads in
    // flight together -- and new = old + acc, one fp32 add per element; without it C is never read.  Scope (host): N % 8 == 0 (a lane's
    // four columns are inside or outside together), ldc % 4 == 0, a 16-byte aligned C, (BM ldc + N) 4 bytes below 2 GiB from the
    // tile's first row.  The non-temporal form is an instruction of its own, as below.
    const __amdgpu_buffer_rsrc_t rsC =
        __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<float*>(g.C) + (size_t)tc.m0 * g.ldc), 0, 0xFFFFFFFFu, 0x00020000);
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

// ---- host side: hgemm_kernel_nn.hpp's; the family's four kernel sets -------------------------------------------------------------
HGEMM_TR_MEMBERS(HGEMM_TR_EXTERN, CfgTA, false)    // hgemm_inst_g6.hip
HGEMM_TR_MEMBERS(HGEMM_TR_EXTERN, CfgTA, true)     // hgemm_inst_g7.hip
HGEMM_TR_MEMBERS(HGEMM_TR_EXTERN, CfgTAB, false)   // hgemm_inst_g9.hip
HGEMM_TR_MEMBERS(HGEMM_TR_EXTERN, CfgTAB, true)    // hgemm_inst_g10.hip

}  // namespace hgemm_mi355x
