"""CPU tests of the bias gradient -- bgemm_mi355x_nn_dact_dbias (family n's EPI_C16_DACT_DBIAS + ACT kernels, hgemm_inst_g17.hip, and the
column-sum kernels of hgemm_registry.hip) and bgemm_mi355x_colsum_c32: the names, the header block and the refusals; the self-check hook
over tests/test_tn_bias_host.py's sweep -- the dact call's plan, dispatch for dispatch, with the new id in the plain dispatch and the
column sum behind it, in the split, reference and no-workspace forms as well --; the workspace query against the hook; the row mask and
the butterfly of csrc/hgemm_dbias.hpp built with the host compiler into a program of its own that walks every lane of every member; and
a scratch and register audit of unit g17 against its twins of unit g16, by counting."""
import ctypes
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_mlp_backward_host import ACTS, DACT_HOOK, GELU, NN_KERNEL, RELU, device_isa, k_loop, kernel_of, mnemonics, reg
from test_mlp_backward_host import hook_answer as dact_answer
from test_nn_host import MEMBERS as NN_MEMBERS, nn_info
from test_ta_host import CSRC, HIPCC, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import (EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, THUNK_ENTRY, THUNK_GENERIC, THUNK_SPLITK_REDUCE, TILES, WORDS)
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the tn prototypes)
from test_tn_bias_host import SHAPES

EPI_C16_DACT, EPI_DBIAS = 11, 32
THUNK_COLSUM_BLOCKED, THUNK_COLSUM_FINISH, THUNK_COLSUM_DIRECT = 5, 6, 7
COUNTER_BYTES = 256 << 10
DIRECT_ROWS = BLOCK_ROWS = 256
NO_SPLIT, NO_WORKSPACE = 1 << FORM_SPLITK, (1 << FORM_SPLITK) | (1 << FORM_PLAIN)
PUBLIC = ("bgemm_mi355x_nn_dact_dbias", "bgemm_mi355x_launch_nn_dact_dbias", "bgemm_mi355x_nn_dact_dbias_runs",
          "bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes", "bgemm_mi355x_nn_dact_dbias_reserve_workspace", "bgemm_mi355x_colsum_c32")
HOOK = "bgemm_mi355x_selfcheck_launch_nn_dact_dbias"


def answer(lib, act, cid, word, aligned, m, n, k, lda, ldb, ldc, ldz, ruled_out=0):
    """[status, form, dispatches, slab bytes, counters, (thunk, grid, epi, splits, k_chunk, items) ...]"""
    out = (ctypes.c_longlong * 44)()
    st = getattr(lib, HOOK)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ldz, ruled_out, act, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:10 + 8 * i]) for i in range(out[1])]


def test_the_header_declares_the_names_and_states_the_semantics(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None
    assert getattr(lib, HOOK) is not None and HOOK not in header
    flat = lambda a, b: re.sub(r"\s*\n \*\s*", " ", header[header.index(a):header.index(b)])   # noqa: E731
    dact = flat("Input gradient through the activation", "The same with the bias gradient")
    assert "no bias gradient" in dact and "bgemm_mi355x_nn_dact_dbias below" in dact
    block = flat("The same with the bias gradient", "hgemm_mi355x_strerror")
    for phrase in ("C[m][n] is the C of bgemm_mi355x_launch_nn_dact for the same arguments and plan, bit for bit",
                   "s[n] = sum over m < M of float( C[m][n] )", "the sum of the ROUNDED bf16 values the call stores", "taken in fp32",
                   "two identical calls give identical bits", "HGEMM_PLAN_NT_STORE does not change the bits", "A row at or past M counts 0",
                   "accumulate == 0: db32[n] = s[n]; the old contents are never read and may be NaN",
                   "accumulate == 1: db32[n] = fl32( old + s[n] ), one fp32 add", "Any other value: HGEMM_ERR_BAD_ARG",
                   "db32 == NULL: HGEMM_ERR_BAD_ARG", "4-byte alignment is enough", "nothing behind db32[N-1] is written",
                   "gamma_k = k u / (1 - k u), u = 2^-24", "derived, not measured", "tile_m = 0 .. tiles_m - 1 in that order",
                   "still HGEMM_OK and a correct db", "Nothing is allocated during capture", "ldx >= N (less: HGEMM_ERR_BAD_ARG)",
                   "one thread per column walks the M rows in order"):
        assert phrase in block, phrase
    for nm in ("hgemm_mi355x_nn_dact_dbias", "bgemm_mi355x_ta_dact_dbias", "bgemm_mi355x_tn_dact_dbias", "bgemm_mi355x_nn_dbias",
               "bgemm_mi355x_nn_dact_dbias_plan", "bgemm_mi355x_nn_dact_dbias_num_configs", "hgemm_mi355x_colsum_c32", "bgemm_mi355x_colsum_c16"):
        assert not hasattr(lib, nm), nm
    text = (CSRC / "hgemm_dbias.hpp").read_text()
    assert "constexpr int COLSUM_U_LOG2 = -24;" in text and "gamma_k = k u / (1 - k u)" in text
    assert '#include "hgemm_dbias.hpp"' in (CSRC / "hgemm_kernel_nn.hpp").read_text()


def test_the_unit_the_ids_and_the_kinds(lib):
    assert "hgemm_inst_g17.hip" in (PKG / "build.py").read_text()
    g17 = (CSRC / "hgemm_inst_g17.hip").read_text()
    for act in ("ACT_RELU", "ACT_GELU", "ACT_GELU_TANH"):
        assert f"HGEMM_TR_MEMBERS(HGEMM_NN_DBIAS_INST, {act}, CfgNNB)" in g17
    assert "HGEMM_NN_DBIAS" not in (CSRC / "hgemm_inst_g16.hip").read_text() and "HGEMM_NN_DBIAS" not in (CSRC / "hgemm_inst_g8.hip").read_text()
    kernel_hpp = (CSRC / "hgemm_kernel.hpp").read_text()
    assert "constexpr int EPI_C16_DACT_DBIAS = 32;" in kernel_hpp and "constexpr int EPI_C16_DACT = 11;" in kernel_hpp
    assert "constexpr int EPI_KTAIL = 8;" in kernel_hpp and "constexpr int EPI_KSTAGGER = 16;" in kernel_hpp
    assert all((EPI_DBIAS + act) & (8 | 16) == 0 for act in ACTS), "a dbias id reads as a kernel-template flag"
    assert "TR_C16_DACT_DBIAS = 11, TR_KINDS = 15" in (CSRC / "hgemm_kernel_nn.hpp").read_text()
    assert lib.hgemm_mi355x_nn_num_configs() == 4


def expected(dact, act, m, n, bm, ruled_out):
    """The dbias call's answer from the dact call's answer (same arguments, same ruled_out & NO_SPLIT)."""
    if dact == [-1]:
        return dact
    form, disp = dact[1], [tuple(d) + (None,) for d in dact[5:]]
    slab = dact[3]
    sum_row = lambda thunk, rows: (thunk, 0, EPI_DBIAS, None, None, rows)                 # noqa: E731
    if form == FORM_PLAIN and ruled_out != NO_WORKSPACE:
        tiles_m = -(-m // bm)
        disp = [(disp[0][0], disp[0][1], EPI_DBIAS + act) + disp[0][3:]] + [sum_row(THUNK_COLSUM_FINISH, tiles_m)]
        slab = tiles_m * n * 4
    elif form == FORM_SPLITK and m > DIRECT_ROWS:
        blocks = -(-m // BLOCK_ROWS)
        disp += [sum_row(THUNK_COLSUM_BLOCKED, blocks), sum_row(THUNK_COLSUM_FINISH, blocks)]
        slab += blocks * n * 4
    else:
        disp += [sum_row(THUNK_COLSUM_DIRECT, 0)]
    return [0, form, len(disp), slab, dact[4]] + disp


def same(got, want):
    if got[:5] != want[:5] or len(got) != len(want):
        return False
    return all(all(w is None or gv == w for gv, w in zip(gd, wd)) for gd, wd in zip(got[5:], want[5:]))


def test_the_hook_answers_as_the_dact_call_with_the_column_sum_behind_it_over_the_sweep(lib):
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES + [(1000, 64, 64), (520, 72, 192)], WORDS):
        bm = TILES[cid][0]
        for lds in ((k, n, n), (k + 8, n + 16, n + 8), (k, n + 4, n), (k, n, n + 4), (k + 4, n, n)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, NO_SPLIT), (True, NO_WORKSPACE)):
                for act, ldz in itertools.product(ACTS, (n, n + 24)):
                    dact = dact_answer(lib, DACT_HOOK, act, cid, word, aligned, m, n, k, *lds, ldz, ruled_out & NO_SPLIT)
                    got = answer(lib, act, cid, word, aligned, m, n, k, *lds, ldz, ruled_out)
                    want = expected(dact, act, m, n, bm, ruled_out)
                    assert same(got, want), (cid, (m, n, k), hex(word), lds, ldz, aligned, ruled_out, act, got, want)
                    # in every dispatch the two calls share, the plan is the dact call's: thunk, grid, splits, k_chunk (and the id, but for the plain one)
                    for gd, dd in zip(got[5:], dact[5:]):
                        assert (gd[0], gd[1], gd[3], gd[4]) == (dd[0], dd[1], dd[3], dd[4]) and (gd[2] == dd[2] or gd[2] == EPI_DBIAS + act)
                    if ruled_out == NO_WORKSPACE:
                        assert got[3] == 0 and got[5:][-1][0] == THUNK_COLSUM_DIRECT and EPI_DBIAS + act not in [d[2] for d in got[5:]]
                    seen.add((got[1], tuple(d[0] for d in got[5:])))
                got = answer(lib, GELU, cid, word, aligned, m, n, k, *lds, n + 4, ruled_out)
                assert got[:3] == [0, FORM_REFERENCE, 2] and [(d[0], d[2]) for d in got[5:]] == [(THUNK_GENERIC, EPI_C16_DACT + GELU), (THUNK_COLSUM_DIRECT, EPI_DBIAS)]
                assert answer(lib, GELU, cid, word, aligned, m, n, k, *lds, n - 8, ruled_out) == [-1]
            for ldz in (n, n + 8, n + 4, n - 8):
                assert lib.bgemm_mi355x_nn_dact_dbias_runs(cid, m, n, k, *lds, ldz) == lib.bgemm_mi355x_nn_dact_runs(cid, m, n, k, *lds, ldz)
    assert seen == {(FORM_REFERENCE, (THUNK_GENERIC, THUNK_COLSUM_DIRECT)), (FORM_PLAIN, (THUNK_ENTRY, THUNK_COLSUM_FINISH)),
                    (FORM_PLAIN, (THUNK_ENTRY, THUNK_COLSUM_DIRECT)), (FORM_SPLITK, (THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_COLSUM_DIRECT)),
                    (FORM_SPLITK, (THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_COLSUM_BLOCKED, THUNK_COLSUM_FINISH))}


def test_the_workspace_query_is_what_the_hook_reports(lib):
    lib.bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes.restype = ctypes.c_size_t
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES + [(1000, 64, 64)], WORDS):
        got = answer(lib, RELU, cid, word, True, m, n, k, k, n, n, n)
        want = COUNTER_BYTES + got[3] if got[0] == 0 and got[3] else 0
        assert lib.bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes(cid, word, m, n, k) == want, (cid, (m, n, k), hex(word))
        if got[0] == 0 and got[1] == FORM_PLAIN:
            assert want == COUNTER_BYTES + -(-m // TILES[cid][0]) * n * 4
    assert lib.bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes(0, 1, 0, 64, 64) == 0


def test_bad_arguments_are_refused_before_any_device_call(lib):
    m, n, k = 200, 136, 128
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_nn_dact_dbias.argtypes = [ci] * 2 + [vp] * 5 + [ci] * 9 + [vp]
    lib.bgemm_mi355x_nn_dact_dbias.argtypes = [vp] * 5 + [ci] * 5 + [vp]
    lib.bgemm_mi355x_colsum_c32.argtypes = [vp] * 2 + [ci] * 4 + [vp]
    lib.bgemm_mi355x_nn_dact_dbias_reserve_workspace.argtypes = [ci] * 3 + [vp]
    null, some, other, db = vp(0), vp(4096), vp(8192), vp(16384)
    for act in (0, 4, -1):
        assert lib.bgemm_mi355x_launch_nn_dact_dbias(0, 1, some, some, other, some, db, m, n, k, k, n, n, n, act, 0, null) == -1
        assert lib.bgemm_mi355x_nn_dact_dbias(some, some, other, some, db, m, n, k, act, 0, null) == -1
        assert answer(lib, act, 0, 1, True, m, n, k, k, n, n, n) == [-1]
    for act in ACTS:
        for accumulate in (2, -1, 256):
            assert lib.bgemm_mi355x_launch_nn_dact_dbias(0, 1, some, some, other, some, db, m, n, k, k, n, n, n, act, accumulate, null) == -1
            assert lib.bgemm_mi355x_nn_dact_dbias(some, some, other, some, db, m, n, k, act, accumulate, null) == -1
        assert lib.bgemm_mi355x_launch_nn_dact_dbias(0, 1, some, some, other, some, null, m, n, k, k, n, n, n, act, 0, null) == -1   # db32 == NULL
        assert lib.bgemm_mi355x_nn_dact_dbias(some, some, other, some, null, m, n, k, act, 1, null) == -1
        for z in (null, some):                                                                                                 # z NULL, z == c
            assert lib.bgemm_mi355x_launch_nn_dact_dbias(0, 1, some, some, z, some, db, m, n, k, k, n, n, n, act, 0, null) == -1
        for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
            assert lib.bgemm_mi355x_nn_dact_dbias(null, null, null, null, null, *shape, act, 0, null) == -1
            assert lib.bgemm_mi355x_nn_dact_dbias_runs(0, *shape, k, n, n, n) == 0
            assert lib.bgemm_mi355x_nn_dact_dbias_reserve_workspace(*shape, null) == -1
        for cid in (-1, 4):
            assert answer(lib, act, cid, 1, True, m, n, k, k, n, n, n) == [-1]
    for args in ((null, db, 4, 16, 16, 0), (some, null, 4, 16, 16, 0), (some, db, 4, 16, 8, 0), (some, db, 0, 16, 16, 0), (some, db, 4, 0, 16, 0),
                 (some, db, 4, 16, 16, 2), (some, db, 4, 16, 16, -1)):
        assert lib.bgemm_mi355x_colsum_c32(*args, null) == -1, args[2:]
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    assert not re.search(r"bgemm_mi355x_(launch_)?(ta|tn)\w*dbias", header), "another layout declares a dbias call"


# ---- the row mask and the butterfly on the CPU ---------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "hgemm_dbias.hpp"
using namespace hgemm_mi355x;
// One tile of member (BM, BN, WM, WN) whose first row is m0 of an M-row matrix: every lane's column accumulators as COUNTS per tile row
// (so that a row summed twice or never shows), through the kernel's steps 1 to 3 with hgemm_dbias.hpp's own index functions.
static int tile(int BM, int BN, int WM, int WN, int m0, int M) {
  const int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16, NW = WM * WN;
  typedef std::vector<int> Rows;                                     // count per tile row
  std::vector<Rows> col((size_t)NW * 64 * FN * 4, Rows(BM, 0));
  auto at = [&](int wave, int lane, int j, int e) -> Rows& { return col[(((size_t)wave * 64 + lane) * FN + j) * 4 + e]; };
  std::vector<int> owner((size_t)BM * BN, 0);                        // how many accumulators hold element (row, column)
  for (int wave = 0; wave < NW; ++wave)
    for (int lane = 0; lane < 64; ++lane)
      for (int i = 0; i < FM; ++i)
        for (int j = 0; j < FN; ++j)
          for (int e = 0; e < 4; ++e) {
            const int row = dbias_row(wave / WN, TM, i, lane), c = dbias_col(wave % WN, TN, j, lane, e);
            if (row < 0 || row >= BM || c < 0 || c >= BN) return 1;
            ++owner[(size_t)row * BN + c];
            if (dbias_row_counts(m0, row, M)) ++at(wave, lane, j, e)[row];
          }
  for (int v : owner) if (v != 1) return 2;                          // the lanes' accumulators tile the tile exactly once
  for (int s = 0; s < DBIAS_BFLY_STAGES; ++s) {                      // the butterfly: every lane adds the value of its source lane
    std::vector<Rows> next = col;
    for (int wave = 0; wave < NW; ++wave)
      for (int lane = 0; lane < 64; ++lane) {
        const int src = dbias_bfly_src(s, lane);
        if (src < 0 || src >= 64 || (src >> 4) != (lane >> 4) || dbias_bfly_src(s, src) != lane) return 3;   // inside the row of 16, an involution
        for (int j = 0; j < FN; ++j)
          for (int e = 0; e < 4; ++e)
            for (int r = 0; r < BM; ++r) next[(((size_t)wave * 64 + lane) * FN + j) * 4 + e][r] += at(wave, src, j, e)[r];
      }
    col.swap(next);
  }
  for (int wave = 0; wave < NW; ++wave)                              // every lane of a row of 16 ends with the same counts
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < FN; ++j)
        for (int e = 0; e < 4; ++e)
          if (at(wave, lane, j, e) != at(wave, lane & ~15, j, e)) return 4;
  std::vector<Rows> red((size_t)WM * BN, Rows(BM, 0));
  std::vector<int> written((size_t)WM * BN, 0);
  for (int wave = 0; wave < NW; ++wave)
    for (int lane = 0; lane < 64; lane += 16)
      for (int j = 0; j < FN; ++j)
        for (int e = 0; e < 4; ++e) {
          const size_t slot = (size_t)(wave / WN) * BN + dbias_col(wave % WN, TN, j, lane, e);
          red[slot] = at(wave, lane, j, e);
          ++written[slot];
        }
  for (int v : written) if (v != 1) return 5;                        // every LDS slot written by exactly one lane
  for (int t = 0; t < BN; ++t)
    for (int r = 0; r < BM; ++r) {
      int count = 0;
      for (int w = 0; w < WM; ++w) count += red[(size_t)w * BN + t][r];
      if (count != (m0 + r < M ? 1 : 0)) return 6;                   // each (row, column) of the tile exactly once, a row at or past M never
    }
  return 0;
}
int main() {
  static_assert(COLSUM_U_LOG2 == -24 && DBIAS_DPP_QUAD_XOR1 == 0xB1 && DBIAS_DPP_QUAD_XOR2 == 0x4E && DBIAS_DPP_HALF_MIRROR == 0x141 &&
                DBIAS_DPP_ROW_MIRROR == 0x140, "the controls the model's source lanes stand for");
  const int members[4][4] = {{64, 64, 2, 2}, {128, 64, 2, 2}, {64, 128, 2, 2}, {128, 128, 2, 2}};
  int tiles = 0;
  for (const auto& mb : members)
    for (int M : {1, 8, 63, 64, 65, 136, 152, 264, 1000})
      for (int m0 = 0; m0 < M; m0 += mb[0], ++tiles) {
        const int rc = tile(mb[0], mb[1], mb[2], mb[3], m0, M);
        if (rc) { printf("FAIL %d: member %dx%d M %d m0 %d\n", rc, mb[0], mb[1], M, m0); return 1; }
      }
  printf("OK %d tiles\n", tiles);
  return 0;
}
"""


def test_the_row_mask_and_the_butterfly_count_every_element_of_a_tile_exactly_once(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the index arithmetic cannot be built for the CPU")
    (tmp_path / "dbias_main.cpp").write_text(PROGRAM)
    done = subprocess.run([cxx, "-O2", "-std=c++17", f"-I{CSRC}", str(tmp_path / "dbias_main.cpp"), "-o", str(tmp_path / "dbias_main")],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([str(tmp_path / "dbias_main")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("OK "), run.stdout[-500:]
    # the kernel uses the functions the program walked, and the four controls in the program's order
    kernel = (CSRC / "hgemm_kernel_nn.hpp").read_text()
    for text in ("dbias_row(wave_m, CFG::TM, i, lane)", "dbias_row_counts(tc.m0, (int)row, g.M)", "dbias_col(wave_n, CFG::TN, j, lane, e)",
                 "col[j][e] += counts ? y : 0.0f;", "y = (float)(__bf16)y;"):
        assert text in kernel, text
    order = [kernel.index(f"dbias_dpp_add<{c}>(v)") for c in ("DBIAS_DPP_QUAD_XOR1", "DBIAS_DPP_QUAD_XOR2", "DBIAS_DPP_HALF_MIRROR", "DBIAS_DPP_ROW_MIRROR")]
    assert order == sorted(order)


# ---- scratch and register audit of unit g17 against its twins of unit g16, by counting ----------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_dbias")
    return {u: device_isa(tmp, u, NN_KERNEL) for u in ("g17", "g16")}


def test_unit_g17_holds_twelve_kernels_without_scratch_and_records_its_registers_beside_g16s(lib, isa):
    """No private segment, the member's LDS (the wave rows cross inside the ring's bytes), the K loop of the g16 twin by mnemonic and count.
    next_free_vgpr is printed beside the twin's and must stay within the twin's occupancy step (a few registers are no failure, a spill is)."""
    (text, funcs, meta), (_, tfuncs, tmeta) = isa["g17"], isa["g16"]
    assert set(funcs) == set(meta) and len(funcs) == 12
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family, element type or epilogue"
    assert not re.search(r"^\s*scratch_", text, re.M)
    print("member act accum_offset next_free_vgpr next_free_sgpr | g16 twin")
    for cid, act in itertools.product(range(4), ACTS):
        name, twin = kernel_of(funcs, "CfgNNB", cid, EPI_DBIAS + act), kernel_of(tfuncs, "CfgNNB", cid, EPI_C16_DACT + act)
        md, tmd = meta[name], tmeta[twin]
        print(NN_MEMBERS[cid], act, *(reg(md, k) for k in ("accum_offset", "next_free_vgpr", "next_free_sgpr")), "|",
              *(reg(tmd, k) for k in ("accum_offset", "next_free_vgpr", "next_free_sgpr")))
        assert reg(md, "private_segment_fixed_size") == 0, (name, "private segment: the epilogue spills")
        assert reg(md, "group_segment_fixed_size") == nn_info(lib, cid)[7] == reg(tmd, "group_segment_fixed_size"), (name, "LDS bytes")
        waves = lambda v: 512 // (-(-v // 8) * 8)                                      # noqa: E731  (waves per SIMD the unified file allows)
        assert waves(reg(md, "next_free_vgpr")) == waves(reg(tmd, "next_free_vgpr")), (name, "occupancy: next_free_vgpr left the twin's step")
        # what the epilogue adds to the registers in front of the accumulators: col[FN][4] per lane, FN = BN / WN / 16, and at most 8 more
        # for the row mask, the row index and the rounded values of a fragment in flight -- more than that is a regression to look at
        info = nn_info(lib, cid)
        fn = info[1] // info[3] // 16
        assert reg(md, "accum_offset") - reg(tmd, "accum_offset") <= 4 * fn + 8, (name, "accum_offset grew past the column accumulators")
        (lo, hi), (tlo, thi) = k_loop(name, funcs[name]), k_loop(twin, tfuncs[twin])
        body, tbody = funcs[name][lo:hi + 1], tfuncs[twin][tlo:thi + 1]
        assert mnemonics(body) == mnemonics(tbody), (name, "the K loop differs from the twin's")
        assert [c for c in body if "vmcnt" in c] == [c for c in tbody if "vmcnt" in c], (name, "the counted vmcnt of the loop")
