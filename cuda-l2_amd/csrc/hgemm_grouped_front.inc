// The front of the two grouped kernels whose group boundary cuts the ROWS of C (hgemm_tn_grouped_kernel, hgemm_nn_grouped_kernel): device
// offsets -> (group, the tile's first row and column, the group's end row), or no tile.  DESIGN.md 4.37 has the design; the arithmetic is
// hgemm_grouped.hpp's.  A text and not a function for hgemm_tr_store_c16.inc's reason: included, hgemm_tn_grouped_kernel compiles to the
// stream it had when the text stood in its braces (DESIGN.md 4.39).
// The including kernel provides `ka` (offsets, G, M, tiles_n), lane, BM, BN and LG = GROUPED_LANE_GROUPS, and declares
//   struct { int m0, n0; } tc;  int group, row_end;
// in front of the include.  Every `return` below is taken on values that came through v_readlane or are kernel arguments: wave-uniform
// scalar branches, in front of the first barrier and of every operand load.  The one lane-dependent piece, each lane's walk over its own
// four groups, is closed inside this block: behind it every lane is active again.
  {
    const __amdgpu_buffer_rsrc_t rsOff = __builtin_amdgcn_make_buffer_rsrc((void*)ka.offsets, 0, ((uint32_t)ka.G + 1u) * 4u, 0x00020000);
    int o[LG + 1];
#pragma unroll
    for (int j = 0; j <= LG; ++j) o[j] = (int)__builtin_amdgcn_raw_buffer_load_b32(rsOff, (uint32_t)(LG * lane + j) * 4u, 0, 0);
    int t[LG], mine = 0;
#pragma unroll
    for (int j = 0; j < LG; ++j) {
      t[j] = LG * lane + j < ka.G ? grouped_tiles_m(grouped_rows(o[j], o[j + 1], ka.M), BM) : 0;
      mine += t[j];
    }
    const int incl = grouped_wave_scan(mine);
    const int T = __builtin_amdgcn_readlane(incl, 63) * ka.tiles_n;
    const int bid = blockIdx.x;
    if (bid >= T) return;   // beyond the real tile count: nothing loaded but the offsets, no barrier met
    const int L = grouped_remap(bid, T), q = L / ka.tiles_n;
    const int owner = __builtin_ctzll(__builtin_amdgcn_ballot_w64(incl > q));   // q < total: some lane's sum passes it
    // every lane walks its own four groups; the owner's walk stops inside them
    int before = incl - mine, js = 0, os = o[0], oe = o[1];
    bool go = true;
#pragma unroll
    for (int j = 0; j + 1 < LG; ++j) {
      go = go && q >= before + t[j];
      if (go) { before += t[j]; js = j + 1; os = o[j + 1]; oe = o[j + 2]; }
    }
    group = LG * owner + __builtin_amdgcn_readlane(js, owner);
    const int tiles_before = __builtin_amdgcn_readlane(before, owner);
    const GroupRows gr = grouped_rows(__builtin_amdgcn_readlane(os, owner), __builtin_amdgcn_readlane(oe, owner), ka.M);
    const int tg = grouped_tiles_m(gr, BM);
    int tm, tn;
    grouped_raster(L - tiles_before * ka.tiles_n, tg, ka.tiles_n, tm, tn);
    // (never taken for offsets the host's bound covers; for others it keeps every row inside the group, whatever the sums wrapped to)
    if ((unsigned)tm >= (unsigned)tg || (unsigned)tn >= (unsigned)ka.tiles_n || group >= ka.G) return;
    tc.m0 = gr.start + tm * BM;
    tc.n0 = tn * BN;
    row_end = gr.end;
  }
