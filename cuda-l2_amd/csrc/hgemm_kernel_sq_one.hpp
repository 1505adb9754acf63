// Family "q", one tile per workgroup: hgemm_tn_sq_one_kernel, a sibling of hgemm_tn_sq_kernel (hgemm_kernel_sq.hpp) for the launches
// in which every workgroup computes EXACTLY ONE work item -- 4096^3 on q256x256_w2x2 is 256 tiles on 256 workgroups.
//
// hgemm_tn_sq_kernel is the general persistent kernel: its two LDS-DMA streams cross work-item seams (cursors, SQ_LOAD_ITEM), its
// accumulators are re-zeroed per item, and past the last K-step of the last item its branch-free DMA keeps issuing pieces of a tile
// nobody consumes.  With one item per workgroup none of that is needed.  This kernel keeps the steady-state K-step (the interval
// plan SqPlan / SqSlots, the fragment sets, the sync points) and changes what surrounds it.  The interval is the general kernel's
// text: sq_interval (hgemm_kernel_sq.hpp), whose parts -- late pieces, early pieces, the sync point's vmcnt count, "a next tile
// exists" -- are compile-time switches that default to the steady state; their meaning and the "younger pieces" rule for the vmcnt
// count are described there, the HGEMM_SQ_ABL ablations reach this kernel through it, and the HGEMM_TIMELINE record is the shared
// sq_timeline_record.  What this header holds is its own: the K-step macro that names the switches, the peeled-tail schedule, the
// kernel's control flow.  (The lane offsets, the descriptors, the prologue and the first fragment reads are the same statements as
// in hgemm_tn_sq_kernel and still written out in both: as shared functions they moved instructions in this kernel or in the general
// ones -- DESIGN.md section 4.27.)
//
//
//   1. No item walk.  The tile coordinates and the two descriptors are computed once; a stream position is one scalar byte offset.
//   2. Peeled tail.  The A stream runs three tiles ahead of the MFMAs and the B stream two, so the last three K-steps are written
//      out with only the pieces of tiles that exist (nk = K-steps of the item, tiles 0 .. nk-1):
//        step nk-3   interval A: late A(nk-1), early B(nk-1); interval B: late B(nk-1), NO early A (it would be tile nk)
//        step nk-2   no piece at all
//        step nk-1   no piece, no sync point, no read of a next tile (only the leading reads of its own slice-1 B fragments)
//      The stream order is A(t+1), B(t+1), A(t+2), B(t+2), ...; a sync point waits with vmcnt(number of YOUNGER pieces):
//        step nk-3   P: A(nk-2) landed, younger B(nk-2) + A(nk-1) = NJB + NJA; Q: B(nk-2), younger A(nk-1) + B(nk-1) = NJA + NJB
//        step nk-2   P: A(nk-1) landed, younger B(nk-1) = NJB;                 Q: B(nk-1), younger none = 0
//        step nk-1   nothing in flight
//      Five dead half-tiles (A(nk), B(nk), A(nk+1), B(nk+1), the early part of A(nk+2)) are not requested, no LDS-DMA is in flight
//      when the epilogue's stores are issued, and the workgroup ends without draining vmcnt.
//   Not built here: the peeled head (first K-step with a zero C operand, B(1) behind the first MFMAs) and
//   the epilogue inside the last K-step.
//
// The summation order of every C element is hgemm_tn_sq_kernel's (K-steps in order, slice 0 before slice 1), and the epilogue is
// the same sp_epilogue_staged: C is bit-identical to the general kernel's.
//
// K-step count: the prologue issues tiles 0 and 1 and the early pieces of A(2); the three peeled steps follow.  With an even count
// one full step runs in front (it issues A(3): 4 <= nk holds for every even nk >= 3).  So the kernel takes nk >= SQ_ONE_MIN_STEPS = 3
// (= the depth of the A stream), whole stages only (K % 64 == 0).
#pragma once

#include "hgemm_kernel_sq.hpp"

namespace hgemm_mi355x {

constexpr int SQ_ONE_MIN_STEPS = 3;   // K-steps (K = 64 each) the kernel needs: the A stream's depth (see above)

// Fragment source of interval h (K = 32 half h of the stage image), this lane's row and swizzled chunk (KT = 1, MI = 16)
#define SQ1_FRAG(STAGE, OPOFF, H) ((STAGE) + (OPOFF) + foff[H])
// One K-step on stage (step & 1), as SQ_K_STEP: LA / EB / LB / EA = the late A, early B (interval A), late B, early A (interval B)
// pieces are issued; VMP / VMQ = vmcnt counts of the two sync points; NEXT = tile step + 1 exists.  The A stream's offset moves on
// between the intervals (interval B issues the early pieces of the tile behind the one whose late pieces interval A issued).
#define SQ1_K_STEP(YS, ZS, LA, EB, LB, EA, VMP, VMQ, NEXT)                                                              \
  do {                                                                                                                  \
    char* st  = smem + (step & 1) * CFG::STAGE_BYTES;                                                                   \
    char* nst = smem + ((step + 1) & 1) * CFG::STAGE_BYTES;                                                             \
    sq_interval<CFG, 0, LA, EB, VMP, NEXT>(fX, fU, fV, SQ1_FRAG(st, b_base_off, 1), SQ1_FRAG(st, b_base_off, 1),        \
                                           ZS, SQ1_FRAG(nst, a_base_off, 1), SQ1_FRAG(nst, a_base_off, 1), wave, voffA, voffB, \
                                           rsA, st, kbA, rsB, st, kbB);                                                 \
    kbA += ROW_BYTES;                                                                                                   \
    sq_interval<CFG, 1, LB, EA, VMQ, NEXT>(YS, fV, fX, SQ1_FRAG(nst, a_base_off, 0), SQ1_FRAG(nst, a_base_off, 0),      \
                                           fU, SQ1_FRAG(nst, b_base_off, 0), SQ1_FRAG(nst, b_base_off, 0), wave, voffA, voffB, \
                                           rsB, st, kbB, rsA, nst, kbA);                                                \
    kbB += ROW_BYTES;                                                                                                   \
    ++step;                                                                                                             \
  } while (0)
#define SQ1_FULL_STEP(YS, ZS) SQ1_K_STEP(YS, ZS, true, true, true, true, CFG::NJA + CFG::NJB, CFG::NJA + CFG::NJB, true)

// Plain wide fp16 epilogue (SP_EPI_WIDE, LDS-staged), whole stages of K, one work item per workgroup: the host sends nothing else
// (sq_one_takes, hgemm_inst_g13.hip).  NT stores follow the plan flag (ARG_NT_STORE) inside sp_epilogue_staged, as in the general kernel.
template <class CFG>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_tn_sq_one_kernel(const GemmArgs g) {
  prefetch_kernargs<sizeof(GemmArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(CFG::MI == 16 && CFG::KT == 1 && CFG::WGS == 1, "the 16x16x32, K = 64 per stage, one-workgroup-per-CU member");
  static_assert(sp_staged_ok<CFG>(CFG::LDS_BYTES), "the LDS-staged wide epilogue");
  constexpr int BM = CFG::BM, BN = CFG::BN, FM = CFG::FM, FN = CFG::FN, MI = CFG::MI;
  constexpr int NFA = CFG::NFA, NFB = CFG::NFB;
#ifdef HGEMM_TIMELINE
  constexpr int TL_EXTRA = 64;
#else
  constexpr int TL_EXTRA = 0;
#endif
  constexpr int STAGED_BYTES = CFG::NW * SP_STAGED_BYTES_PER_WAVE;
  // ONE LDS object, laid out as hgemm_tn_sq_kernel's: the two stages, 64 scratch bytes, the epilogue's 4 KiB per wave
  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES + 64 + STAGED_BYTES + TL_EXTRA];

  const int tid  = threadIdx.x;
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES, 0, tid);
  HGEMM_TL_REALTIME(smem + CFG::LDS_BYTES, 1, tid);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / CFG::WN;
  const int wave_n = wave % CFG::WN;

  // the one work item of this workgroup (the host launches no more items than workgroups; a workgroup without one leaves)
  const ItemWalk walk = persistent_walk(g.items);
  if (walk.count == 0) return;
  const TileCoord tc = map_logical(g, walk.base + walk.first, BM, BN);
  const int m0 = __builtin_amdgcn_readfirstlane(tc.m0), n0 = __builtin_amdgcn_readfirstlane(tc.n0);
  const int nk = __builtin_amdgcn_readfirstlane(tc.nk);

  const int lr = lane & (MI - 1), lq = lane / MI, sw = (lr >> 1) & 7;
  int foff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) foff[h] = lr * ROW_BYTES + (((h * 4 + lq) ^ sw) << 4);
  const int a_base_off = wave_m * CFG::TM * ROW_BYTES;
  const int b_base_off = BM * ROW_BYTES + wave_n * CFG::TN * ROW_BYTES;

  sp_reserve_agprs<CFG::AGPRS>();

  // ---- the two LDS-DMA streams: descriptors of the tile's rows (provably uniform; they end with the operand's last row, so rows
  //      past the M / N edge arrive as zeros) and one byte offset along K per stream ------------------------------------------------
  static_assert(CFG::NW % 2 == 0, "the swizzle key of a wave's row blocks must not depend on the piece");
  const uint32_t chunk0 = (uint32_t)((lane & 7) ^ (((wave & 1) << 2) | (lane >> 4)));
  uint32_t voffA[CFG::PA], voffB[CFG::PB];
#pragma unroll
  for (int q = 0; q < CFG::PA; ++q) voffA[q] = ((uint32_t)((wave + q * CFG::NW) * 8 + (lane >> 3)) * (uint32_t)g.lda + chunk0 * 8u) * 2u;
#pragma unroll
  for (int q = 0; q < CFG::PB; ++q) voffB[q] = ((uint32_t)((wave + q * CFG::NW) * 8 + (lane >> 3)) * (uint32_t)g.ldb + chunk0 * 8u) * 2u;
  auto tile_rsrc = [](const f16* base, int row0, int rows, int ld) __attribute__((always_inline)) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(base + (size_t)row0 * ld);
    const uintptr_t uni = ((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(addr >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)addr);
    const unsigned long long rem = (unsigned long long)(rows - row0) * (unsigned long long)ld * 2ull;
    const unsigned range = (unsigned)__builtin_amdgcn_readfirstlane((int)(rem > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)rem));
    return __builtin_amdgcn_make_buffer_rsrc((void*)uni, 0, (int)range, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rsA = tile_rsrc(g.A, m0, g.M, g.lda), rsB = tile_rsrc(g.Bt, n0, g.N, g.ldb);
  const uint32_t kb0 = (uint32_t)__builtin_amdgcn_readfirstlane(tc.k_begin * 2);
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES + 64 + STAGED_BYTES, 0, tid);   // arguments read, coordinates and offsets computed
  // prologue: A(0), B(0) -> stage 0, A(1), B(1) -> stage 1, the accumulators cleared between the pieces (the VALU work fits into
  // the issue stalls of the cold pieces, as in the general kernel)
  constexpr int NZ = FM * FN, NPIECE = 2 * (CFG::NJA + CFG::NJB);
  int zi = 0, pi = 0;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int p = 0; p < CFG::NJA; ++p) {
      sq_issue_piece<CFG, 0>(rsA, voffA, smem + s * CFG::STAGE_BYTES, wave, p, kb0 + s * ROW_BYTES);
      for (++pi; zi < (pi * NZ) / NPIECE; ++zi) sp_zero_acc(zi);
    }
#pragma unroll
    for (int p = 0; p < CFG::NJB; ++p) {
      sq_issue_piece<CFG, 1>(rsB, voffB, smem + s * CFG::STAGE_BYTES, wave, p, kb0 + s * ROW_BYTES);
      for (++pi; zi < (pi * NZ) / NPIECE; ++zi) sp_zero_acc(zi);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (; zi < NZ; ++zi) sp_zero_acc(zi);
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES + 64 + STAGED_BYTES, 1, tid);   // both tiles issued, accumulators cleared
  wait_vmcnt<CFG::NJA + CFG::NJB>();   // tile 0 landed (tile 1 may fly)
  __builtin_amdgcn_s_barrier();
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES + 64 + STAGED_BYTES, 2, tid);   // tile 0 landed for every wave

  // fragment sets: X = A first half, Y / Z = A second half (alternating), U = B first half, V = B second half
  f16x8 fX[NFA], fY[NFA], fZ[NFA], fU[NFB], fV[NFB];
#pragma unroll
  for (int r = 0; r < NFA; ++r) {
    fX[r] = *(const f16x8*)(SQ1_FRAG(smem, a_base_off, 0) + r * MI * ROW_BYTES);
    fY[r] = *(const f16x8*)(SQ1_FRAG(smem, a_base_off, 1) + r * MI * ROW_BYTES);
  }
#pragma unroll
  for (int r = 0; r < NFB; ++r) fU[r] = *(const f16x8*)(SQ1_FRAG(smem, b_base_off, 0) + r * MI * ROW_BYTES);
  // the A region of stage 0 is consumed: the early pieces of A(2) go there; its late pieces follow in interval A of the first K-step
  uint32_t kbA = kb0 + 2 * ROW_BYTES, kbB = kb0 + 2 * ROW_BYTES;   // stream positions: tile 2
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
  sp_sync();
#pragma unroll
  for (int p = 0; p < CFG::DA; ++p) sq_issue_piece<CFG, 0>(rsA, voffA, smem, wave, p, kbA);

  int step = 0;
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES, 2, tid);
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES, 3, tid);
  // The steps in front of the peeled tail are taken two at a time (the slice-1 A sets Y and Z swap roles every step); an even step
  // count runs one full step first and puts the next tile's slice-1 fragments back into Y.  Both the copy and the merge in front of
  // the loop are places where hipcc may move fragment registers with VALU instructions right in front of an asm MFMA it does not
  // see: sq_settle pins the sets and spends the wait states (hgemm_kernel_sq.hpp, the odd K-step of the general kernel).
  if ((nk & 1) == 0) {
    sq_settle(fX, fY, fU);
    SQ1_FULL_STEP(fY, fZ);
#pragma unroll
    for (int r = 0; r < NFA; ++r) fY[r] = fZ[r];
  }
  sq_settle(fX, fY, fU);
#pragma clang loop unroll(disable)
  for (int t = step; t + 4 < nk; t += 2) {
    SQ1_FULL_STEP(fY, fZ);
    SQ1_FULL_STEP(fZ, fY);
  }
  sq_settle(fX, fY, fU);
  // ---- peeled tail: steps nk-3, nk-2, nk-1 (see the header comment for the pieces and the vmcnt counts) --------------------------
  SQ1_K_STEP(fY, fZ, true, true, true, false, CFG::NJA + CFG::NJB, CFG::NJA + CFG::NJB, true);
  SQ1_K_STEP(fZ, fY, false, false, false, false, CFG::NJB, 0, true);
  SQ1_K_STEP(fY, fZ, false, false, false, false, -1, -1, false);

  // ---- epilogue: the general kernel's LDS-staged one, nothing to re-zero ---------------------------------------------------------
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES, 4, tid);
  sp_mfma_drain();
  const int m_wave = m0 + wave_m * CFG::TM, n_wave = n0 + wave_n * CFG::TN;
  __builtin_amdgcn_sched_barrier(0);
  sp_epilogue_staged<CFG>(g, m_wave, n_wave, false, smem + CFG::LDS_BYTES + 64 + wave * SP_STAGED_BYTES_PER_WAVE);
  __builtin_amdgcn_sched_barrier(0);
  // (no LDS-DMA piece is in flight here: the workgroup may end with its stores outstanding)
#ifdef HGEMM_TIMELINE
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES, 5, tid);
  wait_vmcnt<0>();
  HGEMM_TL_STAMP(smem + CFG::LDS_BYTES, 6, tid);
  HGEMM_TL_REALTIME(smem + CFG::LDS_BYTES, 7, tid);
  sq_timeline_record(g, smem + CFG::LDS_BYTES, smem + CFG::LDS_BYTES + 64 + STAGED_BYTES, step, 1, tid);
#endif
#endif  // __HIP_DEVICE_COMPILE__
}

#undef SQ1_FULL_STEP
#undef SQ1_K_STEP
#undef SQ1_FRAG

// hgemm_inst_g13.hip holds the kernel and its host side
extern template __global__ void hgemm_tn_sq_one_kernel<CfgSQOne>(const GemmArgs);

}  // namespace hgemm_mi355x
