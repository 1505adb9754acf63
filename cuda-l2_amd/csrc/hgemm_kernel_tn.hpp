// Family "f": the forward product of a linear layer in bfloat16 -- C[M,N] = A[M,K] * B[K,N] with A ROW-MAJOR ([M][lda], K contiguous)
// and B given as b_col_major ([N][ldb], K contiguous): Y = X W^T with W stored [out][in].  The third of the layer's three products next
// to family n (input gradient) and family a (weight gradient); the operand form of hgemm_mi355x_fp32's b_col_major and of
// hgemm_rocblas_tn.  Replaces, for a bf16 caller, a cast of X and W to fp16 in front of hgemm_mi355x_fp32 or a rocblas_gemm_ex call with
// bf16 types; the vendor baseline is bgemm_rocblas_tn.  bf16 only: the fp16 forward families (hgemm_kernel.hpp and the rest) are
// untouched and there is no fp16 kernel here.
//
// Family n's structure (hgemm_kernel_nn.hpp): NBUF-deep LDS ring of K = 64 stages, ONE barrier per stage, counted vmcnt, LDS-DMA
// fills in 1-KiB pieces, v_mfma_f32_16x16x32_bf16 (tr_mfma) with fp32 accumulation, operands swapped so that a lane owns 4 consecutive
// N of a C row.
//   * A image, its DMA and its reads: family n's text -- [BM rows][128 B], 16-byte chunk c of row r at slot c ^ ((r >> 1) & 7),
//     descriptor (2 GiB) at the tile's first row, the K advance in the scalar offset, rows clamped to M - 1 - m0, ds_read_b128.
//   * B image: THE SAME image over the tile's BN rows of b_col_major, [BN rows][128 B] = BN * 128 bytes -- as many as family n's
//     [64 k-rows][BN halfs], so CfgTR's B_BYTES, piece counts, ring depths and LDS bytes are the n members'.  Piece il of B holds rows
//     8 il .. 8 il + 7; descriptor (2 GiB) at row n0, the K advance in the scalar offset, rows clamped to N - 1 - n0 on load: a row
//     at or past N reads row N - 1 again and only feeds accumulators of columns >= N, which are never stored.
//   * B fragments: the MFMA operand of lane (n = lane & 15, kq = lane >> 4) is k = 8 kq .. 8 kq + 7 of ROW n of the image: 16
//     contiguous bytes, one ds_read_b128 at row n, slot (4 ks + kq) ^ ((n >> 1) & 7).  There is no transposed read in this family, so
//     neither of that instruction's rules (8-byte lane addresses by construction, EXEC all ones) is needed here.
//   * Scope (the host sends anything else to the reference kernel): K % 64 == 0, N % 8 == 0 (C's 16-byte stores; M is free),
//     lda / ldb / ldc multiples of 8, 16-byte aligned pointers, (BM lda + K) 2, (BN ldb + K) 2 and (BM ldc + N) 2 bytes below 2 GiB.
//   * Epilogues: family n's: bf16 C (each accumulator rounded once by v_cvt_pk_bf16_f32, v_permlane16_swap, 16-byte buffer stores, the
//     plain and the non-temporal store an instruction each) and the two-pass split-K slab (hgemm_splitk_reduce_kernel<OutC16<__bf16>> combines).
//   * Shared with family n: CfgTR, tr_mfma, launch_tr, the member list and its macros, the table types and the 16-bit C epilogue
//     (hgemm_tr_store_c16.inc).  The preamble, the images and the ring are family n's text a third time, on purpose (a
//     repeated text over a changed loop); families n and a keep their symbols and, as compiled, their instruction streams.
#pragma once

#include "hgemm_act.hpp"
#include "hgemm_kernel_nn.hpp"
#include "hgemm_residual.hpp"

namespace hgemm_mi355x {

// The epilogues with a bias vector: EPI_C16_BIAS and, with an activation behind the add, EPI_C16_BIAS + ACT_* (hgemm_act.hpp).
// EPI_C16_BIAS_AUX + ACT_*: the activation forms that also write the rounded pre-activation (bgemm_mi355x_tn_bias_act_aux).
constexpr bool epi_has_aux(int epi) { return epi > EPI_C16_BIAS_AUX && epi <= EPI_C16_BIAS_AUX + ACT_GELU_TANH; }
// EPI_C16_BIAS_ADD: the bias (which may be null: +0.0) and then a residual matrix r, two fp32 adds and one rounding (bgemm_mi355x_tn_bias_add).
constexpr bool epi_has_bias(int epi) { return (epi >= EPI_C16_BIAS && epi <= EPI_C16_BIAS_GELU_TANH) || epi_has_aux(epi) || epi == EPI_C16_BIAS_ADD; }
constexpr int epi_act(int epi) { return epi_has_aux(epi) ? epi - EPI_C16_BIAS_AUX : epi == EPI_C16_BIAS_ADD ? ACT_NONE : epi_has_bias(epi) ? epi - EPI_C16_BIAS : ACT_NONE; }
static_assert(epi_has_bias(EPI_C16_BIAS_ADD) && epi_act(EPI_C16_BIAS_ADD) == ACT_NONE && !epi_has_aux(EPI_C16_BIAS_ADD) && !epi_has_bias(EPI_C16_ADD),
              "the residual form has a bias and no activation; family n's add id is not family f's");
static_assert(epi_act(EPI_C16_BIAS_AUX + ACT_RELU) == ACT_RELU && epi_act(EPI_C16_BIAS_AUX + ACT_GELU_TANH) == ACT_GELU_TANH &&
              !epi_has_aux(EPI_C16_BIAS_GELU_TANH) && !epi_has_bias(EPI_C16_DACT + ACT_RELU), "the aux ids follow the activation ids");
static_assert(epi_act(EPI_C16_BIAS_RELU) == ACT_RELU && epi_act(EPI_C16_BIAS_GELU) == ACT_GELU && epi_act(EPI_C16_BIAS_GELU_TANH) == ACT_GELU_TANH &&
              epi_act(EPI_C16_BIAS) == ACT_NONE, "an activation's epilogue id is EPI_C16_BIAS + its ACT_ id");

template <class CFG, int EPI>
__global__ void hgemm_tn_bf16_kernel(const GemmArgs g);

// family f: both operand images are the classic one; elements are bfloat16
template <int BM_, int BN_, int WM_, int WN_, int NBUF_>
struct CfgTNB : CfgTR<BM_, BN_, WM_, WN_, NBUF_, BM_ * ROW_BYTES> {
  using elem = __bf16;
  static_assert(BN_ * ROW_BYTES == CfgTR<BM_, BN_, WM_, WN_, NBUF_, BM_ * ROW_BYTES>::B_BYTES, "[BN rows][128 B] fills CfgTR's B image");
  template <int EPI>
  static constexpr auto kernel() { return &hgemm_tn_bf16_kernel<CfgTNB, EPI>; }   // the family's entry point (launch_tr)
};

// GemmArgs as the kernel reads it: A = [M][lda], Bt = b_col_major ([N][ldb], ldb >= K its row stride); tail_tiles = 0, counters = nullptr
// -- except EPI_C16_BIAS and its activation forms, where counters is the bias vector (const __bf16*, N elements, 16-byte aligned), reinterpreted below as the fp32-C
// kernels reinterpret g.C.  EPI_C16_BIAS_ADD: counters is the bias vector or null, partial the residual matrix r and tail_first its row stride.
template <class CFG, int EPI>
__global__ void __launch_bounds__(CFG::THREADS) hgemm_tn_bf16_kernel(const GemmArgs g) {
  prefetch_kernargs<sizeof(GemmArgs)>();
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = CFG::BM, BN = CFG::BN, NBUF = CFG::NBUF;
  constexpr int FM = CFG::FM, FN = CFG::FN, NW = CFG::NW, NJ = CFG::NJ, NJ_A = CFG::NJ_A;
  using elem = typename CFG::elem;   // __bf16
  using ex8 = __attribute__((ext_vector_type(8))) elem;
  static_assert(EPI == EPI_C16 || EPI == EPI_SLAB || epi_has_bias(EPI), "plain, two-pass slab, fused-bias, fused-bias-activation, pre-activation-output and bias + residual epilogues");

  __shared__ __attribute__((aligned(1024))) char smem[CFG::LDS_BYTES];

  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / CFG::WN;
  const int wave_n = wave % CFG::WN;

  const TileCoord tc = map_block(g, BM, BN);

  // ---- LDS-DMA source addressing ---------------------------------------------------------------
  // Both operands as the classic family has them: a 2 GiB descriptor at the tile's first row, rows past the matrix edge clamped to the
  // last valid row, the K advance in the scalar offset (every real offset is below 2 GiB: host check).
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)tc.m0 * g.lda), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)(g.Bt + (size_t)tc.n0 * g.ldb), 0, 0x80000000u, 0x00020000);

  uint32_t voff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const bool isA = j < NJ_A;
    const int il = wave + (isA ? j : j - NJ_A) * NW;    // piece of its operand's tile: rows 8 il .. 8 il + 7
    const int r  = il * 8 + (lane >> 3);
    const int rc = min(r, isA ? g.M - 1 - tc.m0 : g.N - 1 - tc.n0);
    const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));   // slot (lane & 7) of row r holds chunk slot ^ ((r >> 1) & 7)
    voff[j] = ((uint32_t)rc * (uint32_t)(isA ? g.lda : g.ldb) + (uint32_t)chunk * 8u) * 2u;
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
  // (not tr_zero, hgemm_kernel_nn.hpp: through the function, the four EPI_C16 kernels here number their scalar registers differently)
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;

  // ---- pipeline ----------------------------------------------------------------------------------
  uint32_t kbyte = (uint32_t)tc.k_begin * 2u;
  auto stage = [&](char* lds_stage) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      lds_void_t* dst = (lds_void_t*)(lds_stage + (wave + j * NW) * 1024);
      if (j < NJ_A) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voff[j], kbyte, 0, 0);
      else          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, voff[j], kbyte, 0, 0);
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

  // ---- fused bias (EPI_C16_BIAS, bgemm_mi355x_tn_bias): C = bf16(acc + float(bias[n])), added LAST and rounded ONCE ----------------------
  // g.counters is the bf16 bias vector of N elements (the host puts it there for this epilogue alone: GemmArgs keeps its layout), read
  // through a descriptor that ENDS at N * 2 bytes.  tr_mfma(bf, af, acc) leaves lane (row = lane & 15, q = lane >> 4) with
  // acc[i][j][e] = C[16 i + row][16 j + 4 q + e]: the operands are swapped, the MFMA's lane owns 4 consecutive N of a C row.  So the lane
  // adds bias[n_b + e], n_b = n0 + wave_n TN + 16 j + 4 q, one 8-byte load per column tile; N % 8 == 0, so a group of 4 is inside N or
  // wholly behind it, where the load returns zeros and the values are never stored.  The add stands in front of the convert and the
  // swap of the shared epilogue, which moves finished bf16 values only.
  // The loads are issued HERE, behind the K loop: the loop keeps the EPI_C16 kernel's registers and its counted vmcnt; the price is
  // one L2 round trip per tile in front of the stores.
  if constexpr (epi_has_bias(EPI)) {
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    using bx4 = __attribute__((ext_vector_type(4))) __bf16;
    const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc((void*)g.counters, 0, (uint32_t)g.N * 2u, 0x00020000);
    bx4 bias[FN];
    if constexpr (EPI == EPI_C16_BIAS_ADD) {
      // This epilogue alone takes a NULL bias: the same loads through a descriptor whose range is then 0 bytes, so every load is out of range
      // and returns zeros without touching memory -- four bf16 +0.0, the bits of a zero-filled vector --, added below like any other bias.
      // One kernel set, one scalar select.
      const __amdgpu_buffer_rsrc_t rsBiasOrNone = __builtin_amdgcn_make_buffer_rsrc((void*)g.counters, 0, g.counters ? (uint32_t)g.N * 2u : 0u, 0x00020000);
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const uint32_t n_b = (uint32_t)(tc.n0 + wave_n * CFG::TN + 16 * j + 4 * (lane >> 4));
        bias[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBiasOrNone, n_b * 2u, 0, 0));
      }
    } else {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n_b = tc.n0 + wave_n * CFG::TN + 16 * j + 4 * (lane >> 4);
      bias[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBias, (uint32_t)n_b * 2u, 0, 0));
    }
    }
    if constexpr (EPI != EPI_C16_BIAS_ADD) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] += (float)bias[j][e];
    } else {
      // ---- fused bias and residual (EPI_C16_BIAS_ADD, bgemm_mi355x_tn_bias_add): C = bf16((acc + float(bias[n])) + float(r[m][n])) ------------
      // g.partial is the bf16 residual matrix r ([M][ldr], read-only, reinterpreted; ldr in g.tail_first -- the fields the aux kernels' z_out
      // travels in).  The loads are family n's dact loads (hgemm_kernel_nn.hpp): the lane's four r of a fragment are one 8-byte load through a
      // descriptor that starts at the tile's first row and ENDS AT r's LAST VALID ELEMENT (dact_z_range_bytes): a row at or past M reads zeros,
      // a column group at or past N pad, the next row or zeros -- values the store text never stores.  Issued here, behind the K loop and the
      // bias loads.  bias_residual_add (hgemm_residual.hpp) is the combine's and the reference kernel's text: two fp32 adds in this order.
      // r may be C itself (ldr == ldc).  Every load of the wave's tile is issued and consumed in this block, in front of the store text below;
      // the element a lane stores there -- its own or, behind the permlane swap, one of another lane of the SAME wave -- is computed from that
      // element's r, so its store depends on its load; wave tiles are disjoint, and what a load reads outside its tile's M x N elements is
      // never stored by this wave.
      const uint32_t ldr = (uint32_t)g.tail_first;
      const uint32_t r_bytes = dact_z_range_bytes(g.M, g.N, g.tail_first, tc.m0);
      const __amdgpu_buffer_rsrc_t rsR =
          __builtin_amdgcn_make_buffer_rsrc((void*)((const __bf16*)g.partial + (size_t)tc.m0 * ldr), 0, r_bytes, 0x00020000);
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
          for (int e = 0; e < 4; ++e) acc[i][j][e] = bias_residual_add(acc[i][j][e], (float)bias[j][e], (float)r[j][e]);
      }
    }
  }

  // ---- the rounded pre-activation as a second output (EPI_C16_BIAS_AUX + ACT, bgemm_mi355x_tn_bias_act_aux): z_out = bf16(z) ----------------
  // The finished z values go through the shared 16-bit C store text, entered here with z_out (g.partial, reinterpreted) and its row
  // stride ldz (g.tail_first) in place of C and ldc: the same convert, swap, predicate and 16-byte buffer stores, the NT form included.
  // acc is only read; the activation below then works on the unrounded z, as in the kernels without this output.
  if constexpr (epi_has_aux(EPI)) {
#define HGEMM_TR_STORE_C ((f16*)g.partial)
#define HGEMM_TR_STORE_LD g.tail_first
#include "hgemm_tr_store_c16.inc"
#undef HGEMM_TR_STORE_C
#undef HGEMM_TR_STORE_LD
  }

  // ---- fused activation (EPI_C16_BIAS + ACT, bgemm_mi355x_tn_bias_act): C = bf16(act(z)), z the unrounded fp32 value above -------------------
  // act_apply (hgemm_act.hpp) is the text the combine and the reference kernel use; it works on the lane's own pre-swap values, so the
  // ownership is the bias code's.  A compile-time property of the kernel: no runtime branch, and the kernels without one compile as before.
  // Register steering, not semantics: the sched_barrier per quad keeps the transcendental's temporaries those of four values, and the empty
  // asm parks each finished value in an accumulation register.  Without the asm the inlined erf's per-value branch made the compiler hold
  // all 64 finished values of f128x128_w2x2 in architectural VGPRs: next_free_vgpr 264 against the EPI_C16_BIAS twin's 257 (accum_offset
  // 200 against 84).  With it every kernel has its twin's figure.  Nothing but tests/test_tn_bias_act_host.py's audit of unit g14 guards
  // that: after a compiler change the audit fails, and the steering is to be looked at again.
  if constexpr (epi_act(EPI) != ACT_NONE) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float y = act_apply<epi_act(EPI)>(acc[i][j][e]);
          asm volatile("" : "+a"(y));   // the finished value waits in an accumulation register for the stores, where the sum was
          acc[i][j][e] = y;
        }
      }
  }

  if constexpr (EPI == EPI_SLAB) {
    store_tile<16, FM, FN, CFG::TM, CFG::TN, true>(g, tc, wave_m, wave_n, lane, acc);
  } else {
#include "hgemm_tr_store_c16.inc"   // the 16-bit C epilogue, one text for families n, a and f
  }
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- host side: hgemm_kernel_nn.hpp's (tr_table_tn is declared there); the family's kernel sets ----------------------------------------
HGEMM_TR_MEMBERS(HGEMM_TR_EXTERN, CfgTNB, false)   // hgemm_inst_g11.hip

// The fused-bias set (bgemm_mi355x_tn_bias): the member's EPI_C16_BIAS kernel alone.  The K slices of its two-pass form are the 16-bit
// set's EPI_SLAB kernels, reached through that set's launcher in its own unit (as launch_tr's fp32-C set reaches them): no slab kernel is
// instantiated twice.  TrLaunch's signature; g.counters of an EPI_C16_BIAS dispatch is the bias pointer (tr_launch, hgemm_api.hip).
template <class CFG>
void launch_tn_bias(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((CFG::template kernel<EPI_C16_BIAS>()), grid, CFG::THREADS, stream, ts, g);
}
#define HGEMM_TN_BIAS_LAUNCHER(CFG, BM, BN, WM, WN, NB) launch_tn_bias<CFG<BM, BN, WM, WN, NB>>
#define HGEMM_TN_BIAS_INST(...) template void HGEMM_TN_BIAS_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_TN_BIAS_EXTERN(...) extern HGEMM_TN_BIAS_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TN_BIAS_EXTERN, CfgTNB)     // hgemm_inst_g12.hip

// The fused bias+activation sets (bgemm_mi355x_tn_bias_act), one per activation: the member's EPI_C16_BIAS + ACT kernel alone; the K slices
// of a two-pass form are again the 16-bit set's EPI_SLAB kernels.
template <class CFG, int ACT>
void launch_tn_bias_act(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((CFG::template kernel<EPI_C16_BIAS + ACT>()), grid, CFG::THREADS, stream, ts, g);
}
#define HGEMM_TN_ACT_LAUNCHER(ACT, CFG, BM, BN, WM, WN, NB) launch_tn_bias_act<CFG<BM, BN, WM, WN, NB>, ACT>
#define HGEMM_TN_ACT_INST(...) template void HGEMM_TN_ACT_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_TN_ACT_EXTERN(...) extern HGEMM_TN_ACT_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TN_ACT_EXTERN, ACT_RELU, CfgTNB)        // hgemm_inst_g14.hip
HGEMM_TR_MEMBERS(HGEMM_TN_ACT_EXTERN, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_ACT_EXTERN, ACT_GELU_TANH, CfgTNB)

// The sets that also write the pre-activation (bgemm_mi355x_tn_bias_act_aux), one per activation: the member's EPI_C16_BIAS_AUX + ACT
// kernel alone, the K slices again the 16-bit set's EPI_SLAB kernels.
template <class CFG, int ACT>
void launch_tn_bias_act_aux(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((CFG::template kernel<EPI_C16_BIAS_AUX + ACT>()), grid, CFG::THREADS, stream, ts, g);
}
#define HGEMM_TN_AUX_LAUNCHER(ACT, CFG, BM, BN, WM, WN, NB) launch_tn_bias_act_aux<CFG<BM, BN, WM, WN, NB>, ACT>
#define HGEMM_TN_AUX_INST(...) template void HGEMM_TN_AUX_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_TN_AUX_EXTERN(...) extern HGEMM_TN_AUX_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TN_AUX_EXTERN, ACT_RELU, CfgTNB)        // hgemm_inst_g15.hip
HGEMM_TR_MEMBERS(HGEMM_TN_AUX_EXTERN, ACT_GELU, CfgTNB)
HGEMM_TR_MEMBERS(HGEMM_TN_AUX_EXTERN, ACT_GELU_TANH, CfgTNB)

// The fused bias + residual set (bgemm_mi355x_tn_bias_add): the member's EPI_C16_BIAS_ADD kernel alone, the K slices again the 16-bit
// set's EPI_SLAB kernels.  g.counters of the dispatch is the bias pointer or null, g.partial r, g.tail_first ldr (tr_launch, hgemm_api.hip).
template <class CFG>
void launch_tn_bias_add(const GemmArgs& g, int grid, hipStream_t stream, int epi, TimingSlot ts) {
  if (epi == EPI_SLAB) return launch_tr<CFG, false>(g, grid, stream, epi, ts);
  HGEMM_LAUNCH((CFG::template kernel<EPI_C16_BIAS_ADD>()), grid, CFG::THREADS, stream, ts, g);
}
#define HGEMM_TN_ADD_LAUNCHER(CFG, BM, BN, WM, WN, NB) launch_tn_bias_add<CFG<BM, BN, WM, WN, NB>>
#define HGEMM_TN_ADD_INST(...) template void HGEMM_TN_ADD_LAUNCHER(__VA_ARGS__)(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#define HGEMM_TN_ADD_EXTERN(...) extern HGEMM_TN_ADD_INST(__VA_ARGS__)
HGEMM_TR_MEMBERS(HGEMM_TN_ADD_EXTERN, CfgTNB)      // hgemm_inst_g21.hip

}  // namespace hgemm_mi355x
