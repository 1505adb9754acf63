// Family "u" (local split-U): the K walk of ONE output tile is split INSIDE the workgroup and reduced through LDS.
//
// Every other way this library has of putting more than one wave-set on the K walk of one tile goes through HBM (two-pass
// split-K, single-launch split-K, stream-K: fp32 slabs, and for the one-launch forms arrival counters).  Here a workgroup is
// WM x WN x KS waves, KS = 4 K-groups: sixteen waves (1024 threads, four per SIMD) for a 2 x 2 wave grid.
//
//   * One pipeline stage holds NIMG images of [BM + BN rows][128 B] = 64 of K each, in the classic family's layout (16-byte
//     chunk c of row r at slot c ^ ((r >> 1) & 7), applied to the per-lane SOURCE address of the LDS-DMA and to the fragment
//     read: hgemm_kernel.hpp).  All sixteen waves issue the stage's 1-KiB LDS-DMA pieces, NI / 16 each.
//   * A stage is 4 * BKG of K, BKG = 16 * NIMG per group: K-group g runs its KSG = NIMG / 2 MFMA slices (K = 32 each), slice
//     g * KSG + s of the stage -- image (g * KSG + s) / 2, half (g * KSG + s) % 2 of its rows.  The WM x WN waves of a group
//     share the slice; four waves per SIMD have four stages' worth of independent MFMA chains and fragment reads to overlap.
//   * NBUF-deep ring, one barrier per stage, counted vmcnt: NBUF - 2 stages stay in flight across the barrier.
//   * After the walk: a barrier, then in R rounds (R = 1 when four copies of the tile fit the ring's LDS) EVERY group writes
//     the round's accumulators to its own fp32 image (rows padded by 16 B: the sixteen rows a ds_write_b128 lane group touches
//     fall on sixteen different 16-byte slots), a barrier, and the 1024 threads each take quads of the round's rows: four
//     ds_read_b128, added in group order ((g0 + g1) + g2) + g3 -- a fixed order, the result does not depend on timing -- one
//     RNE rounding to fp16 and an 8-byte store (or the fp32 quad to the two-pass slab).  Add and store are spread over all
//     sixteen waves; a row of the tile is stored by consecutive lanes.
//   * No K tail (K is a multiple of the stage depth: the host sends anything else to the any-shape kernel), no single-launch
//     split-K and no stream-K variant (the plan resolver degrades those plan words to the two-pass form / to splits = 1).
//     An external split count composes: the slab is written after the LDS reduce, the existing combine kernel adds the slabs.
#pragma once

#include "hgemm_kernel.hpp"

namespace hgemm_mi355x {

constexpr int LU_KS = 4;   // K-groups of a workgroup

template <int BM_, int BN_, int WM_, int WN_, int NIMG_, int NBUF_>
struct CfgLU {
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, NIMG = NIMG_, NBUF = NBUF_, MI = 16, KS = LU_KS;
  static constexpr int NWG         = WM * WN;             // waves of one K-group
  static constexpr int NW          = NWG * KS;            // waves per workgroup
  static constexpr int THREADS     = NW * 64;
  static constexpr int TM          = BM / WM;             // wave tile
  static constexpr int TN          = BN / WN;
  static constexpr int FM          = TM / 16;             // MFMA fragments per wave tile
  static constexpr int FN          = TN / 16;
  static constexpr int KSG         = NIMG / 2;            // K = 32 MFMA slices per group per stage
  static constexpr int STAGE_K     = NIMG * BK;           // K per stage, all groups together
  static constexpr int IMG_BYTES   = (BM + BN) * ROW_BYTES;
  static constexpr int STAGE_BYTES = IMG_BYTES * NIMG;
  static constexpr int RING_BYTES  = STAGE_BYTES * NBUF;
  static constexpr int PPI         = (BM + BN) / 8;       // 1-KiB DMA pieces per image
  static constexpr int NI_A        = BM / 8;              // ... of its A rows
  static constexpr int NI          = PPI * NIMG;          // ... per stage
  static constexpr int NJ          = NI / NW;             // pieces per wave per stage
  // the reduce: KS fp32 images of the round's rows, row stride BN * 4 + 16 bytes
  static constexpr int RED_ROW     = BN * 4 + 16;
  static constexpr int ROUNDS      = (KS * BM * RED_ROW <= RING_BYTES) ? 1 : (KS * BM * RED_ROW <= 2 * RING_BYTES) ? 2 : FM;
  static constexpr int FMR         = FM / ROUNDS;         // fragment rows per wave per round
  static constexpr int RROWS       = WM * FMR * 16;       // tile rows per round
  static constexpr int RED_IMG     = RROWS * RED_ROW;     // bytes of one group's image
  static constexpr int NQ          = RROWS * (BN / 4) / THREADS;   // quads per thread per round
  static constexpr int LDS_BYTES   = RING_BYTES;
  static_assert(NIMG == 2 || NIMG == 4, "a stage is 128 or 256 of K: every group gets whole K = 32 slices");
  static_assert(BM % (WM * 16) == 0 && BN % (WN * 16) == 0, "wave tile must be MFMA-aligned");
  static_assert(NI % NW == 0, "counted vmcnt needs every wave to own the same number of DMA pieces per stage");
  static_assert(NBUF >= 2, "need at least double buffering");
  static_assert(FM % ROUNDS == 0 && KS * RED_IMG <= RING_BYTES, "the reduce images reuse the ring");
  static_assert(RROWS * (BN / 4) % THREADS == 0, "every thread owns the same number of quads per round");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  static_assert(THREADS <= 1024, "workgroup size");
};

// EPI: EPI_C16 (fp16 C) or EPI_SLAB (fp32 partial of an external split, combined by hgemm_splitk_reduce_kernel)
template <class CFG, int EPI>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_tn_lu_kernel(const GemmArgs g) {
  prefetch_kernargs<sizeof(GemmArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = CFG::BM, BN = CFG::BN, NBUF = CFG::NBUF, NW = CFG::NW, NJ = CFG::NJ;
  constexpr int FM = CFG::FM, FN = CFG::FN, KSG = CFG::KSG;
  static_assert(EPI == EPI_C16 || EPI == EPI_SLAB, "family u: plain and two-pass slab epilogues");

  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES];   // the ring; the reduce images reuse it

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp  = wave / CFG::NWG;            // K-group
  const int wq   = wave % CFG::NWG;
  const int wave_m = wq / CFG::WN;
  const int wave_n = wq % CFG::WN;

  const TileCoord tc = map_block(g, BM, BN);
  const int nk = (min(g.K, tc.k_begin + g.k_chunk) - tc.k_begin) / CFG::STAGE_K;   // whole stages: the host guarantees it

  // ---- LDS-DMA source addressing (hgemm_kernel.hpp: classic_mainloop), one descriptor per operand based at the tile's first
  // row; rows past the matrix edge are clamped to the last valid row (their products are never stored).  Range 4 GiB: every
  // real offset is below it (host check), nothing is marked out of range (no K tail).
  const __amdgpu_buffer_rsrc_t rsA =
      __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)tc.m0 * g.lda), 0, 0xFFFFFFFFu, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void*)(g.Bt + (size_t)tc.n0 * g.ldb), 0, 0xFFFFFFFFu, 0x00020000);
  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p    = wave + j * NW;                // piece of the stage (wave-uniform)
    const int img  = p / CFG::PPI, i = p % CFG::PPI;
    const bool isA = i < CFG::NI_A;
    const int il   = isA ? i : i - CFG::NI_A;      // piece index inside its operand's rows
    const int r    = il * 8 + (lane >> 3);         // tile row written by this lane
    const int rmax = isA ? (g.M - 1 - tc.m0) : (g.N - 1 - tc.n0);
    const int rc   = min(r, rmax);
    const int ld   = isA ? g.lda : g.ldb;
    // LDS slot (lane & 7) of row r holds source chunk slot ^ ((r >> 1) & 7); r & 15 = (il & 1) * 8 + (lane >> 3)
    const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));
    voff[j] = ((uint32_t)rc * (uint32_t)ld + (uint32_t)(img * BK + chunk * 8)) * 2u;
  }
  auto stage = [&](char* lds_stage, uint32_t kbyte) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int p = wave + j * NW;
      lds_void_t* dst = (lds_void_t*)(lds_stage + p * 1024);   // image-major, rows in piece order: p * 1 KiB
      if (p % CFG::PPI < CFG::NI_A)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voff[j], kbyte, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, voff[j], kbyte, 0, 0);
    }
  };

  // ---- fragment read offsets of this K-group's slices (bytes inside a stage, without the wave tile's row base)
  int frag_off[KSG];
  {
    const int lr = lane & 15, lq = lane >> 4, sw = (lr >> 1) & 7;
#pragma unroll
    for (int s = 0; s < KSG; ++s) {
      const int slice = grp * KSG + s;             // K = 32 slice of the stage
      const int c = (slice & 1) * 4 + lq;
      frag_off[s] = (slice >> 1) * CFG::IMG_BYTES + lr * ROW_BYTES + ((c ^ sw) << 4);
    }
  }
  const int a_row_base = wave_m * CFG::TM * ROW_BYTES;
  const int b_row_base = BM * ROW_BYTES + wave_n * CFG::TN * ROW_BYTES;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;

  // ---- pipeline ----------------------------------------------------------------------------------
  uint32_t kbyte = (uint32_t)tc.k_begin * 2u;
#pragma unroll
  for (int s = 0; s < NBUF - 1; ++s) {
    if (s < nk) {
      stage(smem + s * CFG::STAGE_BYTES, kbyte);
      kbyte += CFG::STAGE_K * 2;
    }
  }
  int rd = 0;             // stage being consumed
  int wr = NBUF - 1;      // stage being refilled
  for (int t = 0; t < nk; ++t) {
    // Stage t must have landed: allow the NBUF-2 younger stages to stay in flight.
    if (t + NBUF - 2 < nk)
      wait_vmcnt<NJ*(NBUF - 2)>();
    else
      wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();   // all waves' pieces of stage t landed; stage `wr` is free again

    if (t + NBUF - 1 < nk && !HGEMM_DBG(g, 1)) {
      stage(smem + wr * CFG::STAGE_BYTES, kbyte);
      kbyte += CFG::STAGE_K * 2;
    }

    const char* st = smem + rd * CFG::STAGE_BYTES;
#pragma unroll
    for (int s = 0; s < KSG; ++s) {
      f16x8 af[FM], bf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = *(const f16x8*)(st + a_row_base + i * 16 * ROW_BYTES + frag_off[s]);
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[j] = *(const f16x8*)(st + b_row_base + j * 16 * ROW_BYTES + frag_off[s]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
    }
    rd = (rd + 1 == NBUF) ? 0 : rd + 1;
    wr = (wr + 1 == NBUF) ? 0 : wr + 1;
  }

  // ---- reduce over the K-groups through LDS, store ---------------------------------------------------
  if (HGEMM_DBG(g, 2)) return;
  constexpr int RED_ROW = CFG::RED_ROW, FMR = CFG::FMR, QPR = BN / 4;
  using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
  // C from the tile's first row on (column offsets are absolute)
  const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(g.C + (size_t)tc.m0 * g.ldc), 0, 0xFFFFFFFFu, 0x00020000);
  const int lm = lane & 15, ln = (lane >> 4) * 4;
#pragma unroll
  for (int r = 0; r < CFG::ROUNDS; ++r) {
    __syncthreads();   // the last stage's fragment reads (round 0) / the previous round's image reads are done in every wave
    char* mine = smem + grp * CFG::RED_IMG;
#pragma unroll
    for (int ii = 0; ii < FMR; ++ii)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        *(f32x4*)(mine + ((wave_m * FMR + ii) * 16 + lm) * RED_ROW + (wave_n * CFG::TN + j * 16 + ln) * 4) = acc[r * FMR + ii][j];
    __syncthreads();
#pragma unroll
    for (int x = 0; x < CFG::NQ; ++x) {
      const int q = x * CFG::THREADS + tid;
      const int lr = q / QPR, col = (q % QPR) * 4;                          // row of the round's image, first column of the quad
      const int row = (lr / (FMR * 16)) * CFG::TM + r * FMR * 16 + lr % (FMR * 16);   // its row of the tile
      const char* src = smem + lr * RED_ROW + col * 4;
      f32x4 s = *(const f32x4*)src;                                          // group order 0, 1, 2, 3
#pragma unroll
      for (int k = 1; k < CFG::KS; ++k) s += *(const f32x4*)(src + k * CFG::RED_IMG);
      const int m = tc.m0 + row, n = tc.n0 + col;
      if (m < g.M && n < g.N) {   // (N % 4 == 0 on this path: a quad is inside or outside the matrix as a whole)
        if constexpr (EPI == EPI_SLAB) {
          *(f32x4*)(tc.slab + (size_t)row * tc.slab_ld + col) = s;
        } else {
          // buffer stores: the non-temporal form is an instruction of its own (two plain C++ stores that differ only in the
          // hint are merged by the optimiser and the hint is lost); the tile's bytes are below 2 GiB from its first row (host check)
          const f16x4 o = {(f16)s[0], (f16)s[1], (f16)s[2], (f16)s[3]};
          const uint32_t off = ((uint32_t)row * (uint32_t)g.ldc + (uint32_t)n) * 2u;
          if (g.flags & ARG_NT_STORE) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), rsC, off, 0, 2);
          else                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), rsC, off, 0, 0);
        }
      }
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

}  // namespace hgemm_mi355x
