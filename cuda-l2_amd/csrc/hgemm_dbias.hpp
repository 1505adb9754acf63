// The bias gradient's column sum (bgemm_mi355x_nn_dact_dbias, bgemm_mi355x_colsum_c32): the index arithmetic of the fused epilogue and the
// bar of the sum, ONE text for family n's kernel (hgemm_kernel_nn.hpp), the column-sum kernels (hgemm_registry.hip) and a CPU program
// (tests/test_dbias_host.py builds one with the host compiler and walks every lane of every member).  No HIP construct besides the two
// function attributes, which are empty for a host compiler.
//
// The fused epilogue.  tr_mfma leaves lane L of wave (wave_m, wave_n) with acc[i][j][e] = C[dbias_row][dbias_col] of the tile:
//   dbias_row(wave_m, TM, i, L)    = wave_m TM + 16 i + (L & 15)
//   dbias_col(wave_n, TN, j, L, e) = wave_n TN + 16 j + 4 (L >> 4) + e
//   1. per lane, col[j][e] = sum over i = 0 .. FM - 1, in that order, of the ROUNDED value float(bf16(y)), a row at or past M counting 0
//      (dbias_row_counts: family n clamps A's rows, so the S of such a row is the last valid row's S and with a GELU, g(0) = 1/2, not 0);
//   2. over the 16 lanes L & 15 -- the 16 rows of a fragment -- a fixed xor butterfly of four DPP moves, stage s adding the value of lane
//      dbias_bfly_src(s, L): xor 1 and xor 2 as quad permutes, then row_half_mirror and row_mirror, which behind the first two stages (all
//      four lanes of a quad equal, then all eight of a half row) deliver what xor 4 and xor 8 would.  Every lane ends with the same bits;
//   3. lanes L & 15 == 0 write their FN x 4 sums to LDS [wave_m][BN] behind a barrier (the ring is free behind the K loop), and behind a
//      second barrier thread t < BN adds the WM wave rows in the order wave_m = 0 .. WM - 1 and stores P[tile_m][n0 + t], n0 + t < N.
// The finish kernel adds P over tile_m = 0 .. tiles_m - 1 in that order.  The order of every add is fixed by (member, M, N): two identical
// calls give identical bits.
//
// The bar of an M-term fp32 sum in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4)): with u = 2^-24 the
// unit roundoff of fp32,  |fl(sum x_m) - sum x_m| <= gamma_{M-1} sum |x_m|,  gamma_k = k u / (1 - k u).  Derived, not measured; the GPU
// tests read u from here.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGEMM_DBIAS_HD __host__ __device__ inline
#else
#define HGEMM_DBIAS_HD inline
#endif

namespace hgemm_mi355x {

constexpr int COLSUM_U_LOG2 = -24;
constexpr double colsum_gamma(int terms) { return (terms - 1) * 0x1p-24 / (1.0 - (terms - 1) * 0x1p-24); }

HGEMM_DBIAS_HD constexpr int dbias_row(int wave_m, int tm, int i, int lane) { return wave_m * tm + 16 * i + (lane & 15); }
HGEMM_DBIAS_HD constexpr int dbias_col(int wave_n, int tn, int j, int lane, int e) { return wave_n * tn + 16 * j + 4 * (lane >> 4) + e; }
HGEMM_DBIAS_HD constexpr bool dbias_row_counts(int m0, int row, int M) { return m0 + row < M; }

// the DPP controls of the four butterfly stages and the lane each makes lane L read
constexpr int DBIAS_BFLY_STAGES = 4;
constexpr int DBIAS_DPP_QUAD_XOR1 = 0xB1;    // quad_perm:[1,0,3,2]
constexpr int DBIAS_DPP_QUAD_XOR2 = 0x4E;    // quad_perm:[2,3,0,1]
constexpr int DBIAS_DPP_HALF_MIRROR = 0x141; // row_half_mirror: lane i of each 8 reads lane 7 - i
constexpr int DBIAS_DPP_ROW_MIRROR = 0x140;  // row_mirror: lane i of each 16 reads lane 15 - i
HGEMM_DBIAS_HD constexpr int dbias_bfly_src(int stage, int lane) {
  return stage == 0 ? (lane ^ 1) : stage == 1 ? (lane ^ 2) : stage == 2 ? ((lane & ~7) | (7 - (lane & 7))) : ((lane & ~15) | (15 - (lane & 15)));
}

// ---- the stand-alone column sum (bgemm_mi355x_colsum_c32) and part 2 of the fused call's other forms ---------------------------------------
// direct: one thread per column walks the M rows in order, no workspace -- M <= COLSUM_DIRECT_ROWS, or a call that gets no workspace.
// blocked: row blocks of COLSUM_BLOCK_ROWS rows to fp32 partials P[block][N], then the finish kernel.  A block of the grid is
// COLSUM_ROW_LANES row lanes x COLSUM_COL_GROUPS column groups of VEC columns (VEC = 8: 16-byte loads, ldx % 8 == 0 and x 16-byte aligned, a
// ragged last group of N % 8 columns by element loads; VEC = 1 otherwise); row lane r adds rows r, r + COLSUM_ROW_LANES, .. of the block in that order, then thread (0, c) adds the row lanes
// in the order 0 .. COLSUM_ROW_LANES - 1 through LDS.
constexpr int COLSUM_DIRECT_ROWS = 256, COLSUM_BLOCK_ROWS = 256, COLSUM_ROW_LANES = 8, COLSUM_COL_GROUPS = 32;
constexpr int colsum_blocks(int M) { return (M + COLSUM_BLOCK_ROWS - 1) / COLSUM_BLOCK_ROWS; }

}  // namespace hgemm_mi355x
