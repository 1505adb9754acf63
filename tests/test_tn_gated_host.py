"""CPU tests of the gated forward product, bgemm_mi355x_tn_gated (H = act(X Wg^T + bg) (.) (X Wu^T + bu): family f's gated kernels in
hgemm_inst_g18.hip, the kinds TR_C16_GATED + act on the transposed-read host path): the names and constants; the self-check hook over
tests/test_tn_bias_host.py's sweep against the plain call at width 2 N; refusals and fallbacks; the workspace; act_apply<ACT_SILU> of
hgemm_act.hpp built with the host compiler and held to its special values and to 2^-22 |z| against fp64; the index text of hgemm_gated.hpp
walked over every lane of every member; and an ISA audit of unit g18 by counting, against the EPI_C16 twins of unit g11 and the
EPI_C16_BIAS + ACT twins of unit g14."""
import ctypes
import itertools
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_ta_host import CSRC, HIPCC, NBUF, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import (EPI_C16, EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, MEMBERS, THUNK_ENTRY, THUNK_GENERIC, THUNK_SPLITK_REDUCE,
                               TILES, WORDS, answer, tn_info)
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the tn prototypes)
from test_tn_bias_act_host import act_answer, device_isa, k_loop, reg
from test_tn_bias_host import SHAPES

EPI_C16_GATED, EPI_C16_BIAS = 64, 5
RELU, GELU, GELU_TANH, SILU = 1, 2, 3, 4
ACTS = (RELU, GELU, GELU_TANH, SILU)
PUBLIC = ("bgemm_mi355x_tn_gated", "bgemm_mi355x_launch_tn_gated", "bgemm_mi355x_tn_gated_runs")
HOOK = "bgemm_mi355x_selfcheck_launch_tn_gated"
COUNTER_BYTES = 256 << 10


def gated_answer(lib, act, cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out=0, hook=HOOK):
    return act_answer(lib, act, cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out, hook=hook)


def with_gated_epi(plain, act):
    """The answer of the plain bgemm_mi355x_launch_tn call of width 2 N with EPI_C16 replaced by EPI_C16_GATED + act in the plain dispatch
    and in the combine dispatch (which carries EPI_SLAB there); nothing else touched."""
    if plain == [-1]:
        return plain
    out = list(plain[:5])
    for thunk, grid, epi, splits, k_chunk in plain[5:]:
        if thunk == THUNK_SPLITK_REDUCE or (thunk in (THUNK_ENTRY, THUNK_GENERIC) and epi == EPI_C16):
            epi = EPI_C16_GATED + act
        out.append((thunk, grid, epi, splits, k_chunk))
    return out


def test_the_names_the_constants_and_the_unit(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None
    assert getattr(lib, HOOK) is not None and "selfcheck_launch_tn_gated" not in header
    assert re.search(r"#define HGEMM_ACT_SILU 4\b", header)
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("Gated forward product"):header.index("Training forward that also saves")])
    for words in ("wu = wg + N ldb", "never to a slab", "One bf16 rounding", "-inf gives NaN (inf / inf)", "gives -0", "vector of +0.0",
                  "1/2 ulp_bf16(y*) + 2^-19 |g| |u| + 2^-23 |y*|", "bgemm_mi355x_tn_plan(M, 2N, K)", "(BN / 2 ldb + K) 2"):
        assert words in block, words
    assert "no SiLU or gated form" not in header
    for nm in ("hgemm_mi355x_tn_gated", "bgemm_mi355x_nn_gated", "bgemm_mi355x_ta_gated", "bgemm_mi355x_tn_gated_plan", "bgemm_mi355x_tn_gated_reserve_workspace"):
        assert not hasattr(lib, nm), nm                                       # no fp16 form, no other layout, no second plan or workspace call
    assert "ACT_GELU_TANH = 3, ACT_SILU = 4" in (CSRC / "hgemm_act.hpp").read_text()
    assert "hgemm_inst_g18.hip" in (PKG / "build.py").read_text()
    g18 = (CSRC / "hgemm_inst_g18.hip").read_text()
    for act in ("ACT_RELU", "ACT_GELU", "ACT_GELU_TANH", "ACT_SILU"):
        assert f"HGEMM_TR_MEMBERS(HGEMM_TN_GATED_INST, {act}, CfgTNB)" in g18
    assert "constexpr int EPI_C16_GATED = 64;" in (CSRC / "hgemm_kernel.hpp").read_text()
    for src in ("hgemm_kernel_tn_gated.hpp", "hgemm_registry.hip"):
        text = (CSRC / src).read_text()
        assert "act_apply<" in text and "gated_mul(" in text, f"{src} does not use the one activation text and the one product"


def test_the_hook_answers_as_the_plain_call_of_width_2n_over_the_sweep(lib):
    """Every (member, shape, plan word, stride set, aligned / misaligned / no workspace) of tests/test_tn_bias_host.py's sweep, for each
    activation: form, thunks, grids, splits, k_chunk and slab bytes are those of bgemm_mi355x_selfcheck_launch_tn at (M, 2 N, K) with the
    gated epi id in the plain dispatch and in the combine dispatch; the grid is ceil(M / BM) ceil(N / (BN / 2)).  One exception, which the
    call's own scope makes: N % 8 != 0 with 2 N % 8 == 0 (N = 100) -- the plain call of width 200 runs the kernels, the gated call's rows of
    C and bias quads do not align, and it is answered by the reference kernel."""
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, WORDS):
        bm, bn = TILES[cid]
        for lds in ((k, k, n), (k + 8, k + 16, n + 8), (k, k + 4, n), (k, k, n + 4), (k + 4, k, n)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                plain = answer(lib, cid, word, aligned, m, 2 * n, k, lds[0], lds[1], lds[2] + n, ruled_out)
                for act in ACTS:
                    got = gated_answer(lib, act, cid, word, aligned, m, n, k, *lds, ruled_out)
                    if n % 8:
                        assert got[:3] == [0, FORM_REFERENCE, 1] and got[5][0] == THUNK_GENERIC and got[5][2] == EPI_C16_GATED + act, (MEMBERS[cid], (m, n, k))
                        continue
                    assert got == with_gated_epi(plain, act), (MEMBERS[cid], (m, n, k), hex(word), lds, aligned, ruled_out, act)
                    epis = [d[2] for d in got[5:]]
                    assert got[0] == 0 and EPI_C16 not in epis and epis.count(EPI_C16_GATED + act) == 1
                    if got[1] != FORM_REFERENCE:
                        assert got[5][1] == -(-m // bm) * -(-n // (bn // 2)) * got[5][3], (MEMBERS[cid], (m, n, k), "grid")
                    seen.add((act, got[1], tuple(epis)))
            assert lib.bgemm_mi355x_tn_gated_runs(cid, m, n, k, *lds) == (lib.bgemm_mi355x_tn_runs(cid, m, 2 * n, k, lds[0], lds[1], lds[2] + n) if n % 8 == 0 else 0)
            assert lib.bgemm_mi355x_tn_gated_runs(cid, m, n, k, *lds) == (1 if gated_answer(lib, SILU, cid, 1, True, m, n, k, *lds)[1] != FORM_REFERENCE else 0)
    assert seen == {(act, form, epis) for act in ACTS for form, epis in ((FORM_REFERENCE, (EPI_C16_GATED + act,)), (FORM_PLAIN, (EPI_C16_GATED + act,)),
                                                                        (FORM_SPLITK, (EPI_SLAB, EPI_C16_GATED + act)))}


def test_the_workspace_is_the_plain_products_of_width_2n(lib):
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, (1, 2, 5, 32)):
        if n % 8:
            continue
        got = gated_answer(lib, SILU, cid, word, True, m, n, k, k, k, n)
        ws = lib.bgemm_mi355x_tn_plan_workspace_bytes(cid, word, m, 2 * n, k)
        assert (COUNTER_BYTES + got[3] if got[3] else 0) == ws, (MEMBERS[cid], (m, n, k), word)
        if got[1] == FORM_SPLITK:
            assert got[3] == got[5][3] * m * 2 * n * 4


def test_the_reach_of_a_weight_is_half_the_tile(lib):
    """(BN / 2 ldb + K) 2 bytes below 2 GiB for each weight: the largest ldb that runs is the rule's; from the edge on the reference kernel."""
    for cid, (bm, bn) in enumerate(TILES):
        m, n, k = bm + 8, bn + 8, 128
        edge = ((1 << 31) - 2 * k) // (2 * (bn // 2))                             # the first ldb with (BN / 2 ldb + K) 2 >= 2 GiB ...
        edge = -(-edge // 8) * 8
        while (bn // 2 * edge + k) * 2 < (1 << 31):
            edge += 8
        assert gated_answer(lib, RELU, cid, 1, True, m, n, k, k, edge - 8, n)[1] == FORM_PLAIN and lib.bgemm_mi355x_tn_gated_runs(cid, m, n, k, k, edge - 8, n) == 1
        assert gated_answer(lib, RELU, cid, 1, True, m, n, k, k, edge, n)[:2] == [0, FORM_REFERENCE] and lib.bgemm_mi355x_tn_gated_runs(cid, m, n, k, k, edge, n) == 0


def test_the_nn_and_ta_layouts_refuse_the_gated_kinds(lib):
    for hook, lds in (("bgemm_mi355x_selfcheck_launch_nn_gated", lambda m, n, k: (k, n, n)), ("bgemm_mi355x_selfcheck_launch_ta_gated", lambda m, n, k: (m, n, n))):
        for cid, (m, n, k), word, act in itertools.product(range(4), SHAPES[:4], (1, 2), ACTS):
            for aligned in (True, False):
                assert gated_answer(lib, act, cid, word, aligned, m, n, k, *lds(m, n, k), hook=hook) == [-1], (hook, cid, (m, n, k), word, act)


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    m, n, k = 200, 136, 128
    out = (ctypes.c_longlong * 20)()
    for lds in ((k - 8, k, n), (k, k - 8, n), (k, k, n - 8), (0, k, n), (k, 0, n), (k, k, 0), (-k, k, n)):
        for aligned, act in itertools.product((True, False), ACTS):
            assert gated_answer(lib, act, 0, 1, aligned, m, n, k, *lds) == [-1], lds
        assert lib.bgemm_mi355x_tn_gated_runs(0, m, n, k, *lds) == 0
    for cid in (-1, 4):
        assert gated_answer(lib, SILU, cid, 1, True, m, n, k, k, k, n) == [-1] and lib.bgemm_mi355x_tn_gated_runs(cid, m, n, k, k, k, n) == 0
    assert gated_answer(lib, SILU, 0, 1, True, 8, 1 << 30, 64, 64, 64, 1 << 30) == [-1]                        # 2 N does not fit an int
    assert gated_answer(lib, SILU, 0, 1, True, 8, (1 << 30) - 8, 64, 64, 64, (1 << 30) - 8)[0] == 0
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_tn_gated.argtypes = [ci] * 2 + [vp] * 6 + [ci] * 7 + [vp]
    lib.bgemm_mi355x_tn_gated.argtypes = [vp] * 6 + [ci] * 4 + [vp]
    null, some = vp(0), vp(4096)
    for act in (0, 5, -1):                                                    # with every pointer given
        assert lib.bgemm_mi355x_launch_tn_gated(0, 1, some, some, some, some, some, some, m, n, k, k, k, n, act, null) == -1
        assert lib.bgemm_mi355x_tn_gated(some, some, some, some, some, some, m, n, k, act, null) == -1
        assert gated_answer(lib, act, 0, 1, True, m, n, k, k, k, n) == [-1]
    for act in ACTS:
        for ptrs in ((null, some, some, some), (some, null, some, some), (some, some, null, some), (some, some, some, null)):   # a, wg, wu, c
            a, wg, wu, c = ptrs
            for bg, bu in ((some, some), (null, null)):
                assert lib.bgemm_mi355x_launch_tn_gated(0, 1, a, wg, wu, bg, bu, c, m, n, k, k, k, n, act, null) == -1
                assert lib.bgemm_mi355x_tn_gated(a, wg, wu, bg, bu, c, m, n, k, act, null) == -1
        for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
            assert lib.bgemm_mi355x_tn_gated(null, null, null, null, null, null, *shape, act, null) == -1
            assert getattr(lib, HOOK)(0, 1, 4, *shape, k, k, n, 0, act, out) == -1 and lib.bgemm_mi355x_tn_gated_runs(0, *shape, k, k, n) == 0
        assert getattr(lib, HOOK)(0, 1, 4, m, n, k, k, k, n, 0, act, None) == -1
    # SiLU stays refused by every other call (tests/test_tn_bias_act_host.py and tests/test_dbias_host.py hold the rest)
    assert act_answer(lib, SILU, 0, 1, True, m, n, k, k, k, n) == [-1]


# ---- act_apply<ACT_SILU> and the index text on the CPU -------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <set>
#include <utility>
#include "hgemm_act.hpp"
#include "hgemm_dbias.hpp"
#include "hgemm_gated.hpp"
using namespace hgemm_mi355x;
static void show(float z) {
  const float y = act_apply<ACT_SILU>(z);
  uint32_t u[2];
  memcpy(&u[0], &z, 4);
  memcpy(&u[1], &y, 4);
  printf("%08x %08x\n", u[0], u[1]);
}
// every lane of every wave of a member: each (row, output column) once, gate and up from image rows of the same output column
static int walk(int bm, int bn) {
  const int tm = bm / 2, tn = bn / 2, fm = tm / 16, fn = tn / 16, ofn = fn / 2;
  std::set<std::pair<int, int>> seen;
  for (int wave = 0; wave < 4; ++wave)
    for (int lane = 0; lane < 64; ++lane)
      for (int i = 0; i < fm; ++i)
        for (int jo = 0; jo < ofn; ++jo)
          for (int e = 0; e < 4; ++e) {
            const int wave_m = wave / 2, wave_n = wave % 2;
            const int row = dbias_row(wave_m, tm, i, lane), col = gated_lane_col(wave_n, tn, jo, lane, e);
            const int rg = gated_lane_image_row(wave_n, tn, jo, lane, e), ru = gated_lane_image_row(wave_n, tn, jo + ofn, lane, e);
            if (gated_is_up(tn, rg) || !gated_is_up(tn, ru)) return 1;
            if (gated_out_col(tn, rg) != col || gated_out_col(tn, ru) != col) return 2;
            if (row < 0 || row >= bm || col < 0 || col >= bn / 2) return 3;
            if (!seen.insert({row, col}).second) return 4;
          }
  if ((int)seen.size() != bm * (bn / 2)) return 5;
  // every image row belongs to one weight and one output column; a DMA piece of 8 rows is wholly gate or wholly up
  for (int half = 0; half < 2; ++half) {
    std::set<int> cols;
    for (int r = 0; r < bn; ++r)
      if ((int)gated_is_up(tn, r) == half && !cols.insert(gated_out_col(tn, r)).second) return 6;
    if ((int)cols.size() != bn / 2 || *cols.begin() != 0 || *cols.rbegin() != bn / 2 - 1) return 7;
  }
  for (int r = 0; r < bn; r += 8)
    for (int d = 1; d < 8; ++d)
      if (gated_is_up(tn, r + d) != gated_is_up(tn, r) || gated_out_col(tn, r + d) != gated_out_col(tn, r) + d) return 8;
  return 0;
}
// The kernel's DMA source rows at a ragged N: for every tile n0 of every N, each image row of the B image is loaded from row
// n0 + gated_source_row(tn, R, N - n0) of ITS weight -- inside [n0, N - 1], so a gate row never reaches row N (with a fused [2 N][K] weight:
// Wu's first row; with separate weights: behind Wg's end) and an up row never reaches behind Wu's end; a row whose output column lies inside
// N is loaded from exactly that column's row.
static int clamp_walk(int bn) {
  const int tn = bn / 2, half = bn / 2;
  for (int N = 8; N <= 3 * half + 8; N += 8)
    for (int n0 = 0; n0 < N; n0 += half) {
      const int valid = N - n0;
      int past = 0;
      for (int R = 0; R < bn; ++R) {
        const int col = gated_out_col(tn, R), src = gated_source_row(tn, R, valid);
        if (src < 0 || n0 + src > N - 1) return 1;                 // outside the weight the caller named
        if (col < valid && src != col) return 2;                  // a stored column's row is its own
        if (col >= valid) { ++past; if (src != valid - 1) return 3; }
      }
      if (valid < half && past != 2 * (half - valid)) return 4;   // the ragged tile has such rows, in both weights
    }
  return 0;
}
int main() {
  for (int q = -5120; q <= 5120; ++q) show((float)q / 256.0f);
  const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x7f7fffffu, 0xff7fffffu, 0x42c80000u, 0xc2c80000u};
  for (uint32_t s : special) { float z; memcpy(&z, &s, 4); show(z); }
  const int tiles[4][2] = {{64, 64}, {128, 64}, {64, 128}, {128, 128}};
  for (auto& t : tiles) printf("walk %d %d %d\n", t[0], t[1], walk(t[0], t[1]));
  // the slab: [splits][M][2 N], gate sums then up sums in a row -- the index of the plain product of width 2 N on the stacked weight
  int bad = 0;
  const int M = 5, N = 24;
  for (int s = 0; s < 3; ++s) for (int m = 0; m < M; ++m) for (int n = 0; n < N; ++n) for (int up = 0; up < 2; ++up)
    bad += gated_slab_index(M, N, s, m, n, up) != ((unsigned long long)(s * M + m) * (2 * N) + up * N + n);
  printf("slab %d\n", bad);
  printf("clamp %d %d\n", clamp_walk(64), clamp_walk(128));
  printf("eps %d %d %a\n", GATED_ACT_EPS_LOG2, GATED_MUL_EPS_LOG2, (double)gated_mul(3.0f, 0.5f));
  return 0;
}
"""
GRID = 10241


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the activation and index texts cannot be built for the CPU")
    d = tmp_path_factory.mktemp("gated_cpu")
    (d / "gated_main.cpp").write_text(PROGRAM)
    done = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", str(d / "gated_main.cpp"), "-o", str(d / "gated_main"), "-lm"],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([str(d / "gated_main")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0
    lines = run.stdout.splitlines()
    rows = np.array([[int(x, 16) for x in ln.split()] for ln in lines[:GRID + 9]], dtype=np.uint32)
    return rows, lines[GRID + 9:]


def test_silu_special_values_and_the_bound_against_fp64(program):
    rows, _ = program
    f = rows.view(np.float32)
    z, y = f[:GRID, 0].astype(np.float64), f[:GRID, 1].astype(np.float64)
    assert z[0] == -20 and z[-1] == 20
    want = z / (1.0 + np.exp(-z))
    err = np.abs(y - want)
    print(f"silu: worst fp32 error {np.max(err[z != 0] / (2.0 ** -24 * np.abs(z[z != 0]))):.2f} x 2^-24 |z|")
    assert (err <= 2.0 ** -22 * np.abs(z)).all(), int((err > 2.0 ** -22 * np.abs(z)).sum())
    sp = {int(a): int(b) for a, b in rows[GRID:]}
    assert sp[0x00000000] in (0, 0x80000000) and sp[0x80000000] in (0, 0x80000000)           # +-0 gives a zero
    assert sp[0x7f800000] == 0x7f800000                                                      # +inf gives +inf
    nan = lambda b: (b & 0x7f800000) == 0x7f800000 and (b & 0x007fffff) != 0                 # noqa: E731
    assert nan(sp[0xff800000]) and nan(sp[0x7fc00000])                                       # -inf gives NaN (inf / inf), NaN gives NaN
    assert sp[0xff7fffff] == 0x80000000 and sp[0x7f7fffff] == 0x7f7fffff                     # a large negative finite z gives -0
    assert sp[0x42c80000] == 0x42c80000 and abs(np.uint32(sp[0xc2c80000]).view(np.float32)) <= 2.0 ** -19 * 100


def test_the_index_text_pairs_gate_and_up_of_one_output_column_in_every_lane(program):
    _, lines = program
    assert lines[:4] == [f"walk {bm} {bn} 0" for bm, bn in TILES], lines[:4]
    assert lines[4] == "slab 0" and lines[6] == "eps -19 -23 0x1.8p+0"
    assert lines[5] == "clamp 0 0", "a DMA source row of a ragged tile leaves its weight: the per-weight clamp"
    kernel = (CSRC / "hgemm_kernel_tn_gated.hpp").read_text()
    registry = (CSRC / "hgemm_registry.hip").read_text()
    for text, uses in ((kernel, ("gated_source_row(TN, r, g.N - tc.n0)", "gated_is_up(TN, il * 8)", "gated_lane_col(wave_n, TN,", "gated_slab_index(g.M, g.N, tc.split, m, n, j / OFN)",
                                 "isA ? min(r, g.M - 1 - tc.m0) :")),
                       (registry, ("gated_slab_index(M, N, k, m, n, 0)", "gated_slab_index(M, N, k, m, n, 1)"))):
        for u in uses:
            assert u in text, u


# ---- ISA audit of unit g18 -------------------------------------------------------------------------------------------------------------------
GATED_KERNEL = r"_ZN12hgemm_mi355x21hgemm_tn_gated_kernel\w+"


def gated_isa(tmp):
    out = tmp / "g18.s"
    done = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S", "--cuda-device-only",
                           str(CSRC / "hgemm_inst_g18.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-2000:]
    text = out.read_text()
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({GATED_KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    funcs = {}
    for m in re.finditer(rf"^({GATED_KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        funcs[m.group(1)] = [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c and (c.endswith(":") or not c.startswith("."))]
    return text, funcs, meta


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_tn_gated")
    return gated_isa(tmp), device_isa(tmp, "g11"), device_isa(tmp, "g14")


def member_kernel(funcs, cid, tag):
    bm, bn = TILES[cid]
    mine = [f for f in funcs if f"6CfgTNBILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}EEELi{tag}E" in f]
    assert len(mine) == 1, (MEMBERS[cid], tag)
    return mine[0]


def test_unit_g18_holds_the_twenty_kernels_without_a_private_segment(lib, isa):
    (text, funcs, meta), _, _ = isa
    assert set(funcs) == set(meta) and len(funcs) == 20
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family in the unit"
    for cid, act in itertools.product(range(4), (0,) + ACTS):
        md = meta[member_kernel(funcs, cid, act)]
        assert reg(md, "private_segment_fixed_size") == 0, (MEMBERS[cid], act, "private segment")
        assert reg(md, "group_segment_fixed_size") == tn_info(lib, cid)[7], (MEMBERS[cid], act, "LDS bytes")
    assert not re.search(r"^\s*scratch_", text, re.M)


def test_the_k_loop_is_the_plain_twins_and_the_registers_are_within_the_activation_twins(isa):
    """Per stage the MFMA and ds_read_b128 counts (and the LDS-DMA and barrier counts) of the member's EPI_C16 kernel of unit g11;
    next_free_vgpr of each gated kernel at most that of the member's EPI_C16_BIAS + ACT kernel of unit g14 (SiLU: the GELU_TANH one; the
    slab form: the ReLU one).  Prints the register table."""
    (_, funcs, meta), (_, funcs11, _), (_, funcs14, meta14) = isa
    print("member act accum_offset next_free_vgpr next_free_sgpr twin_next_free_vgpr")
    for cid in range(4):
        twin = member_kernel(funcs11, cid, EPI_C16)
        tlo, thi = k_loop(twin, funcs11[twin])
        tbody = funcs11[twin][tlo:thi + 1]
        bm, bn = TILES[cid]
        fm, fn = bm // 32, bn // 32
        for act in (0,) + ACTS:
            name = member_kernel(funcs, cid, act)
            codes = funcs[name]
            lo, hi = k_loop(name, codes)
            body = codes[lo:hi + 1]
            for prefix in ("v_mfma_f32_16x16x32_bf16", "ds_read_b128", "buffer_load_dwordx4", "s_barrier"):
                mine, his = (sum(1 for c in seq if c.startswith(prefix)) for seq in (body, tbody))
                assert mine == his, (name, prefix, mine, his)
            assert sum(1 for c in body if c.startswith("v_mfma")) == 2 * fm * fn and sum(1 for c in body if c.startswith("ds_read_b128")) == 2 * (fm + fn)
            assert not any(c.startswith(("v_mfma", "ds_read")) for c in codes[:lo] + codes[hi + 1:]), name
            act_twin = member_kernel(funcs14, cid, EPI_C16_BIAS + {0: RELU, SILU: GELU_TANH}.get(act, act))
            print(MEMBERS[cid], {0: "slab", 1: "relu", 2: "gelu", 3: "gelu_tanh", 4: "silu"}[act], reg(meta[name], "accum_offset"), reg(meta[name], "next_free_vgpr"),
                  reg(meta[name], "next_free_sgpr"), reg(meta14[act_twin], "next_free_vgpr"))
            assert reg(meta[name], "next_free_vgpr") <= reg(meta14[act_twin], "next_free_vgpr"), (name, "next_free_vgpr above the activation twin's")
            if act:
                tail = codes[hi + 1:]
                assert sum(1 for c in tail if c.startswith("buffer_load_dwordx2")) == fn and not any(c.startswith("buffer_load_dwordx2") for c in codes[:hi + 1]), name
                assert sum(1 for c in tail if c.startswith("v_cvt_pk_bf16_f32")) == fm * fn, name       # 2 per quad, FM FN / 2 output quads
                stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
                want = "buffer_store_dwordx4" if bn == 128 else "buffer_store_dwordx2"
                assert stores and all(c.startswith(want) for c in stores), (name, "the C stores")
