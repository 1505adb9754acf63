// The contract of the grouped tile map (cuda-l2_amd/csrc/hgemm_grouped.hpp), restated against a plain loop over rows; built with the host
// compiler and its address and undefined-behaviour sanitizers by tests/test_grouped_map_host.py.  No GPU, nothing but the header.
#include "hgemm_grouped.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace hgemm_mi355x;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d): BM %d M %d vector %d\n", #cond, __LINE__, BM, M, v); return 1; } } while (0)

int main() {
  unsigned seed = 12345u;
  auto next = [&seed](int lo, int hi) { seed = seed * 1664525u + 1013904223u; return lo + (int)((seed >> 8) % (unsigned)(hi - lo + 1)); };
  long checked = 0;
  for (int BM : {64, 128})
    for (int v = 0; v < 400; ++v) {
      const int G = next(1, 9), M = next(1, 700), tiles_n = next(1, 3), BN = 64;
      // v % 4: 0 sorted inside [0, M]; 1 sorted but reaching below 0 and above M; 2, 3 anything, decreasing entries included
      std::vector<int> off(G + 1);
      for (int& o : off) o = v % 4 == 0 ? next(0, M) : next(-M / 2 - 2, M + M / 2 + 2);
      if (v % 4 < 2) for (int i = 1; i <= G; ++i) if (off[i] < off[i - 1]) off[i] = off[i - 1];
      if (v % 8 == 0) for (int& o : off) o = off[0];                           // all groups empty
      const bool sorted = v % 4 < 2;
      int real = 0;
      for (int g = 0; g < G; ++g) real += grouped_tiles_m(grouped_rows(off[g], off[g + 1], M), BM) * tiles_n;
      if (sorted) REQUIRE(real <= grouped_tiles_m_max(M, G, BM) * tiles_n);
      // cover[g][m][tile_n]: how many (workgroup, row) pairs hold row m of group g in that column tile
      std::vector<std::vector<int>> cover(G, std::vector<int>((size_t)M * tiles_n, 0));
      for (int bid = 0; bid < real + 2 * tiles_n + 3; ++bid) {
        const GroupedTile t = grouped_find_tile(off.data(), G, M, BM, BN, tiles_n, bid);
        REQUIRE((t.g >= 0) == (bid < real));
        if (t.g < 0) continue;
        const GroupRows r = grouped_rows(off[t.g], off[t.g + 1], M);
        REQUIRE(t.g < G && t.end == r.end && t.m0 >= r.start && t.m0 < r.end && (t.m0 - r.start) % BM == 0);
        REQUIRE(t.n0 % BN == 0 && t.n0 / BN < tiles_n);
        for (int m = t.m0; m < t.m0 + BM && m < t.end; ++m) {
          REQUIRE(m >= 0 && m < M);
          ++cover[t.g][(size_t)m * tiles_n + t.n0 / BN];
        }
      }
      for (int g = 0; g < G; ++g) {
        const GroupRows r = grouped_rows(off[g], off[g + 1], M);
        REQUIRE(r.start >= 0 && r.start <= r.end && r.end <= M);
        for (int m = 0; m < M; ++m)
          for (int n = 0; n < tiles_n; ++n) REQUIRE(cover[g][(size_t)m * tiles_n + n] == (m >= r.start && m < r.end ? 1 : 0));
      }
      // the reference kernel's search: for sorted offsets the one group that holds the row; for any, a group that does or none
      for (int m = 0; m < M; ++m) {
        const int g = grouped_find_row(off.data(), G, M, m);
        REQUIRE(g >= -1 && g < G);
        int owner = -1;
        for (int h = 0; h < G; ++h) { const GroupRows r = grouped_rows(off[h], off[h + 1], M); if (m >= r.start && m < r.end) owner = h; if (h == g) REQUIRE(owner == g); }
        if (sorted) REQUIRE(g == owner);
      }
      ++checked;
    }
  std::printf("grouped map: %ld offset vectors checked\n", checked);
  return 0;
}
