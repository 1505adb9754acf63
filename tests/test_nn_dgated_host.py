"""CPU tests of the gated MLP's input gradient, bgemm_mi355x_nn_dgated (dU = act(G) (.) dH, dG = dH (.) U (.) act'(G), dH = dY Wd: family n's
dgated kernels in hgemm_inst_g19.hip, the kinds TR_C16_DGATED + act): the names and constants; the self-check hook against the dact call of
the same arguments; refusals; dact_apply<ACT_SILU> of hgemm_act.hpp and dgated_store of hgemm_dgated.hpp built with the host compiler and
held against fp64 and a numpy fp32 restatement; and an audit of unit g19 by counting, against the EPI_C16 twins of unit g8."""
import concurrent.futures as cf
import ctypes
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_mlp_backward_host import DACT_HOOK, NN_KERNEL, device_isa, hook_answer, k_loop, kernel_of, mnemonics, reg
from test_nn_host import MEMBERS as NN_MEMBERS, nn_info
from test_ta_host import CSRC, HIPCC, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import EPI_C16, EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, TILES, WORDS
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the prototypes)
from test_tn_bias_host import SHAPES

RELU, GELU, GELU_TANH, SILU = 1, 2, 3, 4
ACTS = (RELU, GELU, GELU_TANH, SILU)
EPI_C16_DACT, EPI_C16_DGATED = 11, 96
PUBLIC = ("bgemm_mi355x_nn_dgated", "bgemm_mi355x_launch_nn_dgated", "bgemm_mi355x_nn_dgated_runs")
HOOK = "bgemm_mi355x_selfcheck_launch_nn_dgated"
DGATED_KERNEL = r"_ZN12hgemm_mi355x22hgemm_nn_dgated_kernel\w+"


def constants():
    """The constants of the bars, read from the one place that states them: csrc/hgemm_dgated.hpp and csrc/hgemm_act.hpp."""
    text = (CSRC / "hgemm_dgated.hpp").read_text()
    m = re.search(r"constexpr int DGATED_ACT_EPS_LOG2 = (-\d+), DGATED_MUL_EPS_LOG2 = (-\d+), DGATED_DACT_EPS_LOG2 = DACT_EPS_LOG2;", text)
    assert m, "hgemm_dgated.hpp does not state the constants of the bars"
    d = re.search(r"constexpr int DACT_EPS_LOG2 = (-\d+);", (CSRC / "hgemm_act.hpp").read_text())
    c = re.search(r"constexpr float DACT_SILU_CLAMP = (\d+)\.0f;", (CSRC / "hgemm_act.hpp").read_text())
    return 2.0 ** int(m.group(1)), 2.0 ** int(m.group(2)), 2.0 ** int(d.group(1)), float(c.group(1))


ACT_EPS, MUL_EPS, DACT_EPS, SILU_CLAMP = constants()


def dgated_answer(lib, act, cid, word, aligned, m, n, k, lda, ldb, ldz, ldc, ruled_out=0):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, HOOK)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldz, ldc, ruled_out, act, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def test_the_names_the_constants_and_the_unit(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None
    assert getattr(lib, HOOK) is not None and "selfcheck_launch_nn_dgated" not in header
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("Input gradient of the gated MLP"):header.index("int bgemm_mi355x_nn_dgated(")])
    for words in ("u = g + N with ldz >= 2N", "du = dg + N with ldc >= 2N", "bgemm_mi355x_colsum_c32 over the [M][2N] result", "Nothing is applied to a slab",
                  "no bf16 dH exists", "du[m][n] = bf16_rne( fl32( act32(gf) x S ) )", "dg[m][n] = bf16_rne( dact_mul<act>( fl32( S x uf ), gf ) )",
                  "1/2 ulp_bf16(.) + 2^-19 |gf| |S| + 2^-23 |.|", "1/2 ulp_bf16(.) + 2^-19 |S uf|", "hgemm_mi355x_nn_plan(M, N, K)", "dg == du"):
        assert words in block, words
    for nm in ("hgemm_mi355x_nn_dgated", "bgemm_mi355x_ta_dgated", "bgemm_mi355x_tn_dgated", "bgemm_mi355x_nn_dgated_plan", "bgemm_mi355x_nn_dgated_reserve_workspace"):
        assert not hasattr(lib, nm), nm                                       # no fp16 form, no other layout, no second plan or workspace call
    assert (ACT_EPS, MUL_EPS, DACT_EPS, SILU_CLAMP) == (2.0 ** -19, 2.0 ** -23, 2.0 ** -19, 128.0)
    assert "hgemm_inst_g19.hip" in (PKG / "build.py").read_text()
    g19 = (CSRC / "hgemm_inst_g19.hip").read_text()
    for act in ("ACT_RELU", "ACT_GELU", "ACT_GELU_TANH", "ACT_SILU"):
        assert f"HGEMM_TR_MEMBERS(HGEMM_NN_DGATED_INST, {act}, CfgNNB)" in g19
    assert "constexpr int EPI_C16_DGATED = 96;" in (CSRC / "hgemm_kernel.hpp").read_text()
    for src in ("hgemm_kernel_nn.hpp", "hgemm_registry.hip"):
        assert "dgated_store<" in (CSRC / src).read_text(), f"{src} does not use the one text of the two products"
    # both outputs lie at ldc, both inputs at ldz: the second output's store text is entered with g.ldc, the policy's two stores share one index
    assert "#define HGEMM_TR_STORE_C nn_dgated_du(g)\n#define HGEMM_TR_STORE_LD g.ldc\n" in (CSRC / "hgemm_kernel_nn.hpp").read_text()
    registry = (CSRC / "hgemm_registry.hip").read_text()
    for text in ("const size_t at_c = (size_t)at.m() * ldc + at.n();", "out_store<V>(dU + at_c, du);", "out_store<V>(dG + at_c, s);",
                 "const size_t at_z = (size_t)at.m() * ldz + at.n();", "out_load<__bf16, V>(G + at_z), out_load<__bf16, V>(U + at_z)"):
        assert text in registry, text


def test_the_hook_answers_as_the_dact_call_of_the_same_arguments_over_the_sweep(lib):
    """Every (member, shape, plan word, stride set, aligned / misaligned / no workspace): the dact call's answer (z = g) with EPI_C16_DACT + a
    replaced by EPI_C16_DGATED + act; _runs equals bgemm_mi355x_nn_dact_runs."""
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, WORDS):
        for lda, ldb, ldz, ldc in ((k, n, n, n), (k + 8, n + 16, 2 * n + 8, 2 * n), (k, n, n + 4, n), (k, n, n, n + 4), (k, n + 4, n, n), (k + 4, n, n, n)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                for act in ACTS:
                    twin = hook_answer(lib, DACT_HOOK, min(act, GELU_TANH), cid, word, aligned, m, n, k, lda, ldb, ldc, ldz, ruled_out)
                    want = twin[:5] + [(t, g, EPI_C16_DGATED + act if e == EPI_C16_DACT + min(act, GELU_TANH) else e, s, kc) for t, g, e, s, kc in twin[5:]]
                    got = dgated_answer(lib, act, cid, word, aligned, m, n, k, lda, ldb, ldz, ldc, ruled_out)
                    assert got == want, (NN_MEMBERS[cid], (m, n, k), hex(word), (lda, ldb, ldz, ldc), aligned, ruled_out, act)
                    epis = tuple(d[2] for d in got[5:])
                    assert epis.count(EPI_C16_DGATED + act) == 1 and EPI_C16 not in epis
                    seen.add((act, got[1], epis))
            runs = lib.bgemm_mi355x_nn_dgated_runs(cid, m, n, k, lda, ldb, ldz, ldc)
            assert runs == lib.bgemm_mi355x_nn_dact_runs(cid, m, n, k, lda, ldb, ldc, ldz)
            assert runs == (1 if dgated_answer(lib, SILU, cid, 1, True, m, n, k, lda, ldb, ldz, ldc)[1] != FORM_REFERENCE else 0)
    assert seen == {(act, form, epis) for act in ACTS for form, epis in ((FORM_REFERENCE, (EPI_C16_DGATED + act,)), (FORM_PLAIN, (EPI_C16_DGATED + act,)),
                                                                        (FORM_SPLITK, (EPI_SLAB, EPI_C16_DGATED + act)))}


def test_runs_answers_0_for_each_out_of_scope_case(lib):
    m, n, k = 200, 136, 128
    assert lib.bgemm_mi355x_nn_dgated_runs(0, m, n, k, k, n, n, n) == 1
    for shape, lds in (((m, n + 4, k), (k, n + 8, n + 8, n + 8)),      # N % 8 == 4
                       ((m, n, k + 8), (k + 8, n, n, n)),             # K % 64 != 0
                       ((m, n, k), (k + 4, n, n, n)), ((m, n, k), (k, n + 4, n, n)), ((m, n, k), (k, n, n + 4, n)), ((m, n, k), (k, n, n, n + 4)),   # a stride % 8 == 4
                       ((m, n, k), (k, n, n - 8, n)), ((m, n, k), (k, n, n, n - 8)),     # refused by the launch: 0 here
                       ((m, n, k), (k, n, 1 << 24, n)), ((m, n, k), (k, n, n, 1 << 24))):   # (BM ld + N) 2 >= 2 GiB at BM = 64
        assert lib.bgemm_mi355x_nn_dgated_runs(0, *shape, *lds) == 0, (shape, lds)
    assert lib.bgemm_mi355x_nn_dgated_runs(0, m, n, k, k, n, (1 << 24) - 8, n) == 1 and lib.bgemm_mi355x_nn_dgated_runs(0, m, n, k, k, n, n, (1 << 24) - 8) == 1
    assert lib.bgemm_mi355x_nn_dgated_runs(3, m, n, k, k, n, 1 << 23, n) == 0 and lib.bgemm_mi355x_nn_dgated_runs(0, m, n, k, k, n, 1 << 23, n) == 1   # BM = 128 against 64
    for cid in (-1, 4):
        assert lib.bgemm_mi355x_nn_dgated_runs(cid, m, n, k, k, n, n, n) == 0


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    m, n, k = 200, 136, 128
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_nn_dgated.argtypes = [ci] * 2 + [vp] * 6 + [ci] * 8 + [vp]
    lib.bgemm_mi355x_nn_dgated.argtypes = [vp] * 6 + [ci] * 4 + [vp]
    lib.bgemm_mi355x_launch_nn_dact.argtypes = [ci] * 2 + [vp] * 4 + [ci] * 8 + [vp]
    lib.bgemm_mi355x_nn_dact.argtypes = [vp] * 4 + [ci] * 4 + [vp]
    null = vp(0)
    a, b, g, u, dg, du = (vp(4096 * (i + 1)) for i in range(6))
    launch = lambda ptrs, lds=(k, n, n, n), act=SILU, cid=0: lib.bgemm_mi355x_launch_nn_dgated(cid, 1, *ptrs, m, n, k, *lds, act, null)   # noqa: E731
    for act in (0, 5, -1):
        assert launch((a, b, g, u, dg, du), act=act) == -1 and lib.bgemm_mi355x_nn_dgated(a, b, g, u, dg, du, m, n, k, act, null) == -1
        assert dgated_answer(lib, act, 0, 1, True, m, n, k, k, n, n, n) == [-1]
    for act in ACTS:
        for i in range(6):                                                    # any NULL of the six pointers
            ptrs = [a, b, g, u, dg, du]
            ptrs[i] = null
            assert launch(ptrs, act=act) == -1 and lib.bgemm_mi355x_nn_dgated(*ptrs, m, n, k, act, null) == -1, i
        assert launch((a, b, g, u, dg, dg), act=act) == -1                    # dg == du
        for pair in ((g, du), (u, du), (dg, g), (dg, u)):                     # an output equal to g or u: no in-place form
            assert launch((a, b, g, u) + pair, act=act) == -1, pair
        assert launch((a, b, g, g, dg, g), act=act) == -1
        assert launch((a, b, g, u, dg, du), (k, n, n - 8, n), act) == -1 and launch((a, b, g, u, dg, du), (k, n, n, n - 8), act) == -1   # ldz < N, ldc < N
        assert launch((a, b, g, u, dg, du), (k - 8, n, n, n), act) == -1 and launch((a, b, g, u, dg, du), (k, n - 8, n, n), act) == -1
        for cid in (-1, 4):                                                   # a bad id
            assert launch((a, b, g, u, dg, du), act=act, cid=cid) == -1 and dgated_answer(lib, act, cid, 1, True, m, n, k, k, n, n, n) == [-1]
        for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
            assert lib.bgemm_mi355x_nn_dgated(a, b, g, u, dg, du, *shape, act, null) == -1
            assert lib.bgemm_mi355x_nn_dgated_runs(0, *shape, k, n, n, n) == 0
    # SiLU stays refused by the dact calls
    assert lib.bgemm_mi355x_launch_nn_dact(0, 1, a, b, g, dg, m, n, k, k, n, n, n, SILU, null) == -1
    assert lib.bgemm_mi355x_nn_dact(a, b, g, dg, m, n, k, SILU, null) == -1
    assert hook_answer(lib, DACT_HOOK, SILU, 0, 1, True, m, n, k, k, n, n, n) == [-1]
    assert hook_answer(lib, "bgemm_mi355x_selfcheck_launch_nn_dact_dbias", SILU, 0, 1, True, m, n, k, k, n, n, n) == [-1]


# ---- dact_apply<ACT_SILU> and dgated_store on the CPU -----------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include "hgemm_dgated.hpp"
using namespace hgemm_mi355x;
static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float val(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
static void show(float z) { printf("%08x %08x %08x\n", bits(z), bits(dact_apply<ACT_SILU>(z)), bits(dact_mul<ACT_SILU>(3.0f, z))); }
template <int ACT>
static void pairs() {
  // a fixed walk over (s, g, u): bf16-valued g and u, any fp32 s
  uint32_t x = 12345u;
  for (int i = 0; i < 4096; ++i) {
    x = x * 1664525u + 1013904223u; const float s = ((int)(x >> 8) - (1 << 23)) * 0x1p-18f;
    x = x * 1664525u + 1013904223u; const float g = ((int)((x >> 16) & 0xffu) - 128) * 0x1p-5f;   // [-4, 4) in steps of 1/32: bf16 values
    x = x * 1664525u + 1013904223u; const float u = ((int)((x >> 16) & 0xffu) - 128) * 0x1p-6f;
    const DgatedPair y = dgated_store<ACT>(s, g, u);
    printf("%d %08x %08x %08x %08x %08x\n", ACT, bits(s), bits(g), bits(u), bits(y.dg), bits(y.du));
  }
  const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x3f800000u, 0xbf800000u};
  for (uint32_t gs : special)
    for (uint32_t ss : {0x40400000u, 0x7f800000u, 0xff800000u}) {
      const DgatedPair y = dgated_store<ACT>(val(ss), val(gs), 2.0f);
      printf("%d %08x %08x %08x %08x %08x\n", ACT, ss, gs, bits(2.0f), bits(y.dg), bits(y.du));
    }
}
int main() {
  for (int q = -5120; q <= 5120; ++q) show((float)q / 256.0f);
  const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x7f7fffffu, 0xff7fffffu,
                              0x43000000u, 0xc3000000u, 0x42ffffffu, 0xc2ffffffu, 0x43000001u, 0xc3000001u, 0x41800000u, 0xc1800000u};
  for (uint32_t s : special) show(val(s));
  pairs<ACT_RELU>(); pairs<ACT_GELU>(); pairs<ACT_GELU_TANH>(); pairs<ACT_SILU>();
  static_assert(DACT_SILU_CLAMP == 128.0f && DGATED_ACT_EPS_LOG2 == -19 && DGATED_MUL_EPS_LOG2 == -23 && DGATED_DACT_EPS_LOG2 == -19, "constants");
  return 0;
}
"""
GRID, SPECIAL, PAIRS = 10241, 15, 4096 + 21


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the shared text cannot be built for the CPU")
    d = tmp_path_factory.mktemp("dgated_cpu")
    (d / "dgated_main.cpp").write_text(PROGRAM)
    done = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", str(d / "dgated_main.cpp"), "-o", str(d / "dgated_main"), "-lm"],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([str(d / "dgated_main")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0
    lines = run.stdout.splitlines()
    assert len(lines) == GRID + SPECIAL + 4 * PAIRS
    silu = np.array([[int(x, 16) for x in ln.split()] for ln in lines[:GRID + SPECIAL]], dtype=np.uint32)
    pairs = np.array([[int(ln.split()[0])] + [int(x, 16) for x in ln.split()[1:]] for ln in lines[GRID + SPECIAL:]], dtype=np.uint32)
    return silu, pairs


def dsilu64(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(z))
    sp = 1.0 / (1.0 + e)
    sm = e * sp
    t = np.abs(z) * sp * sm
    return np.where(z < 0, sm - t, sp + t)


def test_the_silu_derivative_is_within_the_derived_count_of_fp64(program):
    """hgemm_act.hpp derives 6.6 x 2^-24 for the derivative alone and 8.8 x 2^-24 with both products, of the 32 x 2^-24 = DACT_EPS the bar
    allows; the measured worst error (printed) only confirms the derivation."""
    silu, _ = program
    f = silu.view(np.float32)
    z, y, p = (f[:GRID, i].astype(np.float64) for i in range(3))
    assert z[0] == -20 and z[-1] == 20
    ref = dsilu64(z)
    err = np.abs(y - ref)
    print(f"silu': worst |g - g*| = {err.max() / 2.0 ** -24:.2f} x 2^-24 (derived 6.6, eps {DACT_EPS / 2.0 ** -24:.0f})")
    assert (err <= 6.6 * 2.0 ** -24).all(), int((err > 6.6 * 2.0 ** -24).sum())
    assert (np.abs(p - 3.0 * ref) <= 3.0 * 7.7 * 2.0 ** -24).all() and 7.7 * 2.0 ** -24 < DACT_EPS
    forward = z / (1.0 + np.exp(-z))
    # (silu - silu' tends to -e^z for z -> -inf, inside eps = 2^-19 below z = -13.17: 1749 points of the grid, and a few at the two crossings)
    assert int((np.abs(forward - ref) > DACT_EPS).sum()) >= 8400, "the forward activation in place of the derivative is outside eps"
    assert y.min() < -0.09 and y.max() > 1.09                                   # negative near -2.4, above 1 near 2.4


def test_the_silu_derivative_limits_are_exact(program):
    silu, _ = program
    sp = {int(a): int(b) for a, b, _ in silu[GRID:]}
    one, half = 0x3f800000, 0x3f000000
    nan = lambda b: (b & 0x7f800000) == 0x7f800000 and (b & 0x007fffff) != 0    # noqa: E731
    assert sp[0x00000000] == half and sp[0x80000000] == half, "+-0 gives 1/2"
    assert sp[0x7f800000] == one and sp[0xff800000] == 0, "+inf gives exactly 1, -inf gives +0: no 0 x inf"
    assert nan(sp[0x7fc00000]), "NaN gives NaN"
    assert sp[0x7f7fffff] == one and sp[0xff7fffff] == 0, "the largest finite values"
    assert sp[0x43000000] == one and sp[0xc3000000] == 0 and sp[0x43000001] == one and sp[0xc3000001] == 0, "at and behind the clamp"
    below = np.array([sp[0x42ffffff], sp[0xc2ffffff]], dtype=np.uint32).view(np.float32)       # the clamp's other side: within 2^-149 of the limit
    assert abs(float(below[0]) - 1.0) <= 2.0 ** -23 and abs(float(below[1])) <= 2.0 ** -100
    at16 = np.array([sp[0x41800000], sp[0xc1800000]], dtype=np.uint32).view(np.float32).astype(np.float64)
    assert at16[0] > 1.0 + 1e-6 and at16[1] < -1e-6, "at |z| = 16 the function is still 2e-6 from its limit: a clamp of 16 is too early"
    assert np.abs(at16 - dsilu64([16.0, -16.0])).max() <= 6.6 * 2.0 ** -24
    assert "constexpr float DACT_SILU_CLAMP = 128.0f;" in (CSRC / "hgemm_act.hpp").read_text()


def test_dgated_store_is_the_numpy_fp32_restatement_bit_for_bit_for_relu(program):
    _, pairs = program
    rows = pairs[pairs[:, 0] == RELU]
    assert len(rows) == PAIRS
    s, g, u = (rows[:, i].copy().view(np.float32) for i in (1, 2, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        relu = np.where((g > 0) | np.isnan(g), g, np.float32(0.0)).astype(np.float32)
        du = (relu * s).astype(np.float32)
        dg = np.where(g <= 0, np.float32(0.0), (s * u).astype(np.float32)).astype(np.float32)
    for col, want in ((4, dg), (5, du)):                                       # bit for bit; a NaN for a NaN (0 x inf)
        got, nan = rows[:, col].copy(), np.isnan(want)
        assert np.array_equal(got[~nan], want.view(np.uint32)[~nan]) and np.isnan(got.view(np.float32)[nan]).all(), col
    sp = {(int(r[1]), int(r[2])): (int(r[4]), int(r[5])) for r in rows[4096:]}
    inf, three = 0x7f800000, 0x40400000
    assert sp[(inf, 0x80000000)][0] == 0 and sp[(inf, 0xff800000)][0] == 0 and sp[(inf, 0xbf800000)][0] == 0, "S = inf under g <= 0: dg = +0 (a select)"
    assert sp[(three, 0x3f800000)] == (0x40c00000, three) and sp[(three, 0xbf800000)] == (0, 0)
    assert sp[(three, 0x7fc00000)][0] == 0x40c00000, "a NaN g passes S u (torch's threshold_backward)"


@pytest.mark.parametrize("act", [GELU, GELU_TANH, SILU], ids=["gelu", "gelu_tanh", "silu"])
def test_dgated_store_is_inside_the_bars_before_the_bf16_rounding(program, act):
    from test_mlp_backward_host import dact64, gelu64
    _, pairs = program
    rows = pairs[pairs[:, 0] == act][:4096]
    s, g, u, dg, du = (rows[:, i].copy().view(np.float32).astype(np.float64) for i in (1, 2, 3, 4, 5))
    a64 = g / (1.0 + np.exp(-g)) if act == SILU else gelu64(g, act)
    d64 = dsilu64(g) if act == SILU else dact64(g, act)
    assert (np.abs(du - a64 * s) <= ACT_EPS * np.abs(g) * np.abs(s) + MUL_EPS * np.abs(a64 * s)).all()
    assert (np.abs(dg - s * u * d64) <= DACT_EPS * np.abs(s * u)).all()
    assert (np.abs(du - d64 * s) > ACT_EPS * np.abs(g) * np.abs(s) + MUL_EPS * np.abs(d64 * s)).mean() > 0.5, "act' in place of act is outside"


# ---- audit of unit g19 against the EPI_C16 twins of unit g8, by counting -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_nn_dgated")
    with cf.ThreadPoolExecutor(max_workers=3) as ex:
        jobs = {u: ex.submit(device_isa, tmp, u, k) for u, k in (("g19", DGATED_KERNEL), ("g16", NN_KERNEL), ("g8", NN_KERNEL))}
        return {u: j.result() for u, j in jobs.items()}


def test_unit_g19_holds_sixteen_kernels_without_a_private_segment_and_with_the_twins_k_loop(lib, isa):
    """No private segment, the member's LDS, and a K loop with the EPI_C16 twin's instructions by mnemonic and count (MFMA, LDS reads, barriers
    and LDS-DMA among them): the loads of g and u are behind it.  next_free_vgpr at most 512 and the dact twin's of unit g16 printed beside it
    (SiLU's twin is the GELU_TANH kernel)."""
    (text, funcs, meta), (_, dfuncs, dmeta), (_, tfuncs, _) = isa["g19"], isa["g16"], isa["g8"]
    assert set(funcs) == set(meta) and len(funcs) == 16
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family, element type or epilogue in the unit"
    assert not re.search(r"^\s*scratch_", text, re.M)
    print("member act accum_offset next_free_vgpr next_free_sgpr | dact twin")
    for cid, act in itertools.product(range(4), ACTS):
        name = kernel_of(funcs, "CfgNNB", cid, EPI_C16_DGATED + act)
        twin = kernel_of(tfuncs, "CfgNNB", cid, EPI_C16)
        dtwin = kernel_of(dfuncs, "CfgNNB", cid, EPI_C16_DACT + min(act, GELU_TANH))
        md = meta[name]
        print(NN_MEMBERS[cid], act, *(reg(md, k) for k in ("accum_offset", "next_free_vgpr", "next_free_sgpr")), "|",
              *(reg(dmeta[dtwin], k) for k in ("accum_offset", "next_free_vgpr", "next_free_sgpr")))
        assert reg(md, "private_segment_fixed_size") == 0, (name, "private segment: the epilogue spills")
        assert reg(md, "group_segment_fixed_size") == nn_info(lib, cid)[7], (name, "LDS bytes")
        assert reg(md, "next_free_vgpr") <= 512
        codes, tcodes = funcs[name], tfuncs[twin]
        (lo, hi), (tlo, thi) = k_loop(name, codes), k_loop(twin, tcodes)
        body, tbody = codes[lo:hi + 1], tcodes[tlo:thi + 1]
        assert mnemonics(body) == mnemonics(tbody), (name, "the K loop differs from the twin's")
        bm, bn = TILES[cid]
        fm, fn = bm // 32, bn // 32
        assert sum(1 for c in body if c.startswith("v_mfma")) == 2 * fm * fn and sum(1 for c in body if c.startswith("s_barrier")) == 1
        assert [c for c in body if c.startswith("s_waitcnt vmcnt")] == [c for c in tbody if c.startswith("s_waitcnt vmcnt")], (name, "the counted vmcnt")
        tail = codes[hi + 1:]
        assert sum(1 for c in tail if c.startswith("buffer_load_dwordx2")) == 2 * fm * fn and not any(c.startswith("buffer_load_dwordx2") for c in codes[:hi + 1]), name
        assert sum(1 for c in tail if c.startswith("v_cvt_pk_bf16_f32")) == 2 * 2 * fm * fn, name          # two outputs, 2 per quad
        stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
        assert stores and all(c.startswith("buffer_store_dwordx4") for c in stores), (name, "the 16-byte stores of both outputs")
        assert not any(c.startswith(("v_mfma", "ds_read")) for c in tail), name
