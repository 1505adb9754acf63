// The tile map of the grouped forward product (bgemm_mi355x_tn_grouped: group g owns rows [off[g], off[g + 1]) of A and C and its own weight),
// as arithmetic: what the member kernels (hgemm_kernel_tn_grouped.hpp), the grouped reference kernel (hgemm_registry.hip) and a CPU program
// (tests/test_grouped_map_host.py) all compute with.  Plain C++ with no device header: a host compiler reads it as it is.
//
//   * A group's rows: each of its two offsets is clamped to [0, M] and an end below the start makes the group empty (grouped_rows), so no
//     offset vector, however malformed, yields a row outside [0, M).
//   * A group of r rows has ceil(r / BM) row tiles, each over all tiles_n column tiles.  The tiles of group g stand in the logical order at
//     [P_g tiles_n, P_{g+1} tiles_n), P the prefix sum of the groups' row-tile counts; T = P_G tiles_n is the REAL tile count, which only
//     the device knows.  The host sizes the grid from the bound grouped_tiles_m_max alone (valid for non-decreasing offsets: the groups'
//     rows then sum to at most M and every group rounds up by less than one tile).
//   * Workgroup id -> logical id: the family's XCD remap (map_block, hgemm_kernel.hpp) with T in the place of the grid size.  Ids at or
//     above T have no tile; ids below it are dealt round-robin to the XCDs by the dispatcher, so each XCD gets T / 8 real tiles -- with
//     the grid size in that place the empty ids would all fall on the last XCDs.
//   * Inside a group (grouped_raster): bands of GROUPED_BAND row tiles; inside a band the row tile runs fastest, then the column tile.
// grouped_find_tile walks all of it serially; the kernels do the prefix sum and the search across a wave's lanes and use the rest as it is.
// The grouped input gradient (bgemm_mi355x_nn_grouped, hgemm_kernel_nn_grouped.hpp) cuts the rows of ITS A and C by the same offsets, so the
// whole map is its map too: the two kernels share the front's text (hgemm_grouped_front.inc, with grouped_wave_scan below), the two reference
// kernels grouped_find_row, the two host sides grouped_tiles_m_max.  Only the device pass sees grouped_wave_scan; everything else in this
// file stays plain C++.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGEMM_HD __host__ __device__
#else
#define HGEMM_HD
#endif

namespace hgemm_mi355x {

constexpr int GROUPED_LANE_GROUPS = 4;                        // consecutive groups one lane of the kernel's map holds
constexpr int GROUPED_MAX_GROUPS  = 64 * GROUPED_LANE_GROUPS; // HGEMM_GROUPED_MAX_GROUPS: one pass of a wave
constexpr int GROUPED_BAND        = 8;                        // row tiles of a raster band
constexpr int GROUPED_XCDS        = 8;

struct GroupRows { int start, end; };   // rows [start, end), 0 <= start <= end <= M

HGEMM_HD inline int grouped_clamp(int v, int M) { return v < 0 ? 0 : (v > M ? M : v); }
HGEMM_HD inline GroupRows grouped_rows(int off_g, int off_g1, int M) {
  const int s = grouped_clamp(off_g, M), e = grouped_clamp(off_g1, M);
  return GroupRows{s, e < s ? s : e};
}
HGEMM_HD inline int grouped_tiles_m(GroupRows r, int BM) { return (r.end - r.start + BM - 1) / BM; }

// the host's grid bound in row tiles
HGEMM_HD inline long long grouped_tiles_m_max(int M, int G, int BM) { return ((long long)M + (long long)G * (BM - 1)) / BM; }

// workgroup id bid < T -> logical id: XCD x (bid % 8) owns one contiguous run of the T logical ids
HGEMM_HD inline int grouped_remap(int bid, int T) {
  const int xcd = bid % GROUPED_XCDS, idx = bid / GROUPED_XCDS;
  const int q = T / GROUPED_XCDS, r = T % GROUPED_XCDS;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// local id l in [0, tiles_g tiles_n) of a group with tiles_g row tiles -> (row tile, column tile)
HGEMM_HD inline void grouped_raster(int l, int tiles_g, int tiles_n, int& tile_m, int& tile_n) {
  const int band = GROUPED_BAND * tiles_n;
  const int first = (l / band) * GROUPED_BAND;
  const int h = tiles_g - first < GROUPED_BAND ? tiles_g - first : GROUPED_BAND;
  const int r = l % band;
  tile_n = r / h;
  tile_m = first + r % h;
}

struct GroupedTile { int g, m0, n0, end; };   // rows [m0, min(m0 + BM, end)) of group g, columns from n0; g < 0: no tile

// The whole map, serially (the kernels' result for the same arguments).  T must fit an int: the host checks its bound.
HGEMM_HD inline GroupedTile grouped_find_tile(const int* off, int G, int M, int BM, int BN, int tiles_n, int bid) {
  int total = 0;
  for (int g = 0; g < G; ++g) total += grouped_tiles_m(grouped_rows(off[g], off[g + 1], M), BM);
  const int T = total * tiles_n;
  if (bid < 0 || bid >= T) return GroupedTile{-1, 0, 0, 0};
  const int L = grouped_remap(bid, T), q = L / tiles_n;
  int before = 0;
  for (int g = 0; g < G; ++g) {
    const GroupRows r = grouped_rows(off[g], off[g + 1], M);
    const int tg = grouped_tiles_m(r, BM);
    if (q < before + tg) {
      int tm, tn;
      grouped_raster(L - before * tiles_n, tg, tiles_n, tm, tn);
      return GroupedTile{g, r.start + tm * BM, tn * BN, r.end};
    }
    before += tg;
  }
  return GroupedTile{-1, 0, 0, 0};
}

// The group that owns row m (the reference kernel's search): the first group whose clamped end lies behind m, if m is not in front of its
// start; -1 for a row no group owns (a dropped token).  A binary search: exact for non-decreasing offsets, in bounds for any.
HGEMM_HD inline int grouped_find_row(const int* off, int G, int M, int m) {
  int lo = 0, hi = G;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (grouped_clamp(off[mid + 1], M) <= m) lo = mid + 1; else hi = mid;
  }
  if (lo >= G) return -1;
  const GroupRows r = grouped_rows(off[lo], off[lo + 1], M);
  return (m >= r.start && m < r.end) ? lo : -1;
}

#if defined(__HIP_DEVICE_COMPILE__)
// (the device pass alone: what hgemm_grouped_front.inc, the front of the two kernels that search the map, sums the lanes' tile counts with)
// inclusive sum over the 64 lanes (EXEC all ones): Hillis-Steele inside each row of 16 by DPP row shifts -- a lane whose source lies outside
// its row adds the `old` operand, 0 --, then lane 15 of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3
__device__ inline __attribute__((always_inline)) int grouped_wave_scan(int v) {   // (no HIP header in front of this file: __forceinline__ spelled out)
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
  return v;
}
#endif

// ---- the grouped weight gradient (bgemm_mi355x_ta_grouped, hgemm_kernel_ta_grouped.hpp): group g owns k-rows [off[g], off[g + 1]) of BOTH
// operands and a whole M x N matrix C_g.  The group boundary cuts the K walk, not the rows of C, so the tile count does not depend on the
// offsets: the grid is EXACT and host-known, G tiles_m tiles_n, every id has a tile and nothing is searched.
//   * Workgroup id -> logical id L: grouped_remap over the grid (the family's XCD remap).
//   * Group g's tiles are one contiguous run of logical ids, g = L / (tiles_m tiles_n): the ids an XCD owns walk one expert's rows of dY and
//     X at a time.  Inside the group: grouped_raster, which with GROUPED_BAND = 8 is the dense family's raster (group_m = min(tiles_m, 8)).
//   * A group's k-rows are grouped_rows with K as the bound; its walk has ceil(rows / 64) stages, the last one partial.
struct TaGroupedTile { int g, tile_m, tile_n; };
HGEMM_HD inline long long ta_grouped_grid(int G, int tiles_m, int tiles_n) { return (long long)G * tiles_m * tiles_n; }
HGEMM_HD inline TaGroupedTile ta_grouped_tile(int L, int tiles_m, int tiles_n) {
  const int per = tiles_m * tiles_n;
  TaGroupedTile t;
  t.g = L / per;
  grouped_raster(L - t.g * per, tiles_m, tiles_n, t.tile_m, t.tile_n);
  return t;
}
HGEMM_HD inline int ta_grouped_stages(GroupRows r, int BK) { return (r.end - r.start + BK - 1) / BK; }

}  // namespace hgemm_mi355x
