"""CPU tests of the fused MLP backward pair -- bgemm_mi355x_tn_bias_act_aux (the forward that also writes the rounded pre-activation;
family f's EPI_C16_BIAS_AUX + ACT kernels, hgemm_inst_g15.hip) and bgemm_mi355x_nn_dact (dZ = (dY W) (.) act'(Z); family n's
EPI_C16_DACT + ACT kernels, hgemm_inst_g16.hip): the names, the header blocks and the refusals; the self-check hooks over
tests/test_tn_bias_host.py's sweep -- the plain call's plan with only the epilogue id replaced in the plain dispatch and in the combine
dispatch --; the derivative text of hgemm_act.hpp built with the host compiler into a program of its own and run over all 65 280 finite
bf16 z (ReLU bit for bit, both GELUs finite and within the derived eps of fp64, the other form and the forward activation outside it);
and a register and scratch audit of the two new units by counting, against their twins of units g14 and g8."""
import concurrent.futures as cf
import ctypes
import itertools
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_nn_host import MEMBERS as NN_MEMBERS, nn_info
from test_ta_host import CSRC, HIPCC, NBUF, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import (EPI_C16, EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, MEMBERS, THUNK_ENTRY, THUNK_GENERIC, THUNK_SPLITK_REDUCE,
                               TILES, WORDS, answer, tables_unchanged, tn_info)
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the tn prototypes)
from test_tn_bias_host import SHAPES

RELU, GELU, GELU_TANH = 1, 2, 3
ACTS = (RELU, GELU, GELU_TANH)
EPI_C16_BIAS, EPI_C16_BIAS_AUX, EPI_C16_DACT = 5, 8, 11
PUBLIC = ("bgemm_mi355x_tn_bias_act_aux", "bgemm_mi355x_launch_tn_bias_act_aux", "bgemm_mi355x_tn_bias_act_aux_runs",
          "bgemm_mi355x_nn_dact", "bgemm_mi355x_launch_nn_dact", "bgemm_mi355x_nn_dact_runs")
AUX_HOOK, DACT_HOOK = "bgemm_mi355x_selfcheck_launch_tn_bias_act_aux", "bgemm_mi355x_selfcheck_launch_nn_dact"


def _eps():
    """The derived eps of the GELU bar, read from the one place that states it: csrc/hgemm_act.hpp."""
    text = (CSRC / "hgemm_act.hpp").read_text()
    m = re.search(r"constexpr int DACT_EPS_LOG2 = (-\d+);\nconstexpr float DACT_EPS = 0x1p(-\d+)f;", text)
    assert m and m.group(1) == m.group(2), "hgemm_act.hpp does not state DACT_EPS"
    return 2.0 ** int(m.group(1))


DACT_EPS = _eps()


def hook_answer(lib, hook, act, cid, word, aligned, m, n, k, lda, ldb, ldc, ldz, ruled_out=0):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, hook)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ldz, ruled_out, act, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def nn_answer(lib, cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out=0):
    out = (ctypes.c_longlong * 20)()
    st = lib.bgemm_mi355x_selfcheck_launch_nn(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ruled_out, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def with_epi(plain, epi_new):
    """The plain call's answer with EPI_C16 replaced by `epi_new` in the plain dispatch and in the combine dispatch; nothing else touched."""
    if plain == [-1]:
        return plain
    out = list(plain[:5])
    for thunk, grid, epi, splits, k_chunk in plain[5:]:
        if thunk == THUNK_SPLITK_REDUCE or (thunk in (THUNK_ENTRY, THUNK_GENERIC) and epi == EPI_C16):
            epi = epi_new
        out.append((thunk, grid, epi, splits, k_chunk))
    return out


def test_the_header_declares_the_names_and_states_the_semantics(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None
    for hook in (AUX_HOOK, DACT_HOOK):
        assert getattr(lib, hook) is not None and hook not in header
    flat = lambda a, b: re.sub(r"\s*\n \*\s*", " ", header[header.index(a):header.index(b)])   # noqa: E731
    aux = flat("Training forward that also saves the pre-activation", "Input gradient through the activation")
    assert "z_out[m][n] = bf16_rne( z[m][n] )" in aux and "C[m][n]     = bf16_rne( act32( z[m][n] ) )" in aux
    assert "applied to the UNROUNDED z" in aux and "both outputs are rounded once" in aux
    assert "C is the C of bgemm_mi355x_launch_tn_bias_act" in aux and "z_out is the C of bgemm_mi355x_launch_tn_bias" in aux
    assert "HGEMM_PLAN_NT_STORE applies to both outputs" in aux and "no slab is touched" in aux
    assert "z_out == NULL and z_out == c: HGEMM_ERR_BAD_ARG" in aux and "ldz >= N (less: HGEMM_ERR_BAD_ARG)" in aux
    dact = flat("Input gradient through the activation", "hgemm_mi355x_strerror")
    assert "eplaces bgemm_mi355x_nn followed by an element-wise kernel" in dact and "a second rounding" in dact
    assert "C[m][n] = bf16_rne( fl32( S[m][n] x dact32(zf) ) )" in dact and "ONE fp32 multiply on the finished sum, never on a slab" in dact
    assert "a select, not a multiply" in dact and "a NaN z passes S" in dact and "-0 and -inf give +0" in dact
    assert "g is finite for every finite z" in dact and "+inf included, gives exactly 1" in dact and "-inf included, gives +0" in dact
    assert "A NaN z gives NaN" in dact
    assert "|C - S g*(zf)| <= 1/2 ulp_bf16(S g*) + 2^-19 |S|" in dact and "derived, not measured" in dact and DACT_EPS == 2.0 ** -19
    assert "z == NULL, z == c and any act outside 1..3: HGEMM_ERR_BAD_ARG" in dact
    assert "no fp16 form" in dact and "no TA / TN form" in dact and "no bias gradient" in dact
    for nm in ("hgemm_mi355x_nn_dact", "bgemm_mi355x_ta_dact", "bgemm_mi355x_tn_dact", "bgemm_mi355x_nn_bias", "bgemm_mi355x_nn_bias_act",
               "bgemm_mi355x_tn_act", "bgemm_mi355x_nn_dact_plan", "bgemm_mi355x_tn_bias_act_aux_plan", "bgemm_mi355x_nn_dact_num_configs",
               "bgemm_mi355x_tn_bias_act_aux_num_configs", "bgemm_mi355x_nn_dact_reserve_workspace", "bgemm_mi355x_tn_bias_act_aux_reserve_workspace"):
        assert not hasattr(lib, nm), nm
    for src in ("hgemm_kernel_nn.hpp", "hgemm_registry.hip"):
        assert "dact_mul<" in (CSRC / src).read_text(), f"{src} does not use the one derivative text"


def test_the_tables_the_units_and_the_epilogue_ids(lib):
    assert lib.hgemm_mi355x_nn_num_configs() == 4 and [lib.hgemm_mi355x_nn_config_name(i).decode() for i in range(4)] == list(NN_MEMBERS)
    assert lib.bgemm_mi355x_tn_num_configs() == 4 and [lib.bgemm_mi355x_tn_config_name(i).decode() for i in range(4)] == list(MEMBERS)
    assert lib.hgemm_mi355x_ta_num_configs() == 4
    tables_unchanged(lib)                                                       # the geometry table's count and name hash
    build_py = (PKG / "build.py").read_text()
    for unit, inst in (("g15", "HGEMM_TN_AUX_INST"), ("g16", "HGEMM_NN_DACT_INST")):
        assert f"hgemm_inst_{unit}.hip" in build_py
        text = (CSRC / f"hgemm_inst_{unit}.hip").read_text()
        for act in ("ACT_RELU", "ACT_GELU", "ACT_GELU_TANH"):
            assert f"HGEMM_TR_MEMBERS({inst}, {act}, Cfg{'TNB' if unit == 'g15' else 'NNB'})" in text
    for unit in ("g8", "g11", "g12", "g14"):
        text = (CSRC / f"hgemm_inst_{unit}.hip").read_text()
        assert "HGEMM_TN_AUX" not in text and "HGEMM_NN_DACT" not in text
    kernel_hpp = (CSRC / "hgemm_kernel.hpp").read_text()
    assert "constexpr int EPI_C16_BIAS_AUX = 8;" in kernel_hpp and "constexpr int EPI_C16_DACT = 11;" in kernel_hpp and "EPI_KSTAGGER = 16" in kernel_hpp


def test_the_hooks_answer_as_the_plain_calls_with_only_the_epilogue_id_replaced_over_the_sweep(lib):
    """Every (member, shape, plan word, stride set, aligned / misaligned / no workspace) of tests/test_tn_bias_host.py's sweep, each
    activation, ldz = N and a padded ldz: the plain call's answer with the new id.  ldz % 8 != 0: the reference form, and _runs 0."""
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, WORDS):
        for family, hook, base, plain_of, runs, plain_runs, lds_of in (
                ("f", AUX_HOOK, EPI_C16_BIAS_AUX, answer, lib.bgemm_mi355x_tn_bias_act_aux_runs, lib.bgemm_mi355x_tn_runs,
                 ((k, k, n), (k + 8, k + 16, n + 8), (k, k + 4, n), (k, k, n + 4), (k + 4, k, n))),
                ("n", DACT_HOOK, EPI_C16_DACT, nn_answer, lib.bgemm_mi355x_nn_dact_runs, lib.bgemm_mi355x_nn_runs,
                 ((k, n, n), (k + 8, n + 16, n + 8), (k, n + 4, n), (k, n, n + 4), (k + 4, n, n)))):
            for lds in lds_of:
                for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                    plain = plain_of(lib, cid, word, aligned, m, n, k, *lds, ruled_out)
                    for act, ldz in itertools.product(ACTS, (n, n + 24)):
                        got = hook_answer(lib, hook, act, cid, word, aligned, m, n, k, *lds, ldz, ruled_out)
                        assert got == with_epi(plain, base + act), (family, cid, (m, n, k), hex(word), lds, ldz, aligned, ruled_out, act)
                        epis = [d[2] for d in got[5:]]
                        assert got[0] == 0 and EPI_C16 not in epis and epis.count(base + act) == 1
                        seen.add((family, act, got[1], tuple(epis)))
                    got = hook_answer(lib, hook, GELU, cid, word, aligned, m, n, k, *lds, n + 4, ruled_out)
                    assert got[:3] == [0, FORM_REFERENCE, 1] and got[5][0] == THUNK_GENERIC and got[5][2] == base + GELU, (family, lds)
                    assert hook_answer(lib, hook, GELU, cid, word, aligned, m, n, k, *lds, n - 8, ruled_out) == [-1]
                for ldz in (n, n + 8, n + 24):
                    assert runs(cid, m, n, k, *lds, ldz) == plain_runs(cid, m, n, k, *lds), (family, lds, ldz)
                assert runs(cid, m, n, k, *lds, n + 4) == 0 and runs(cid, m, n, k, *lds, n - 8) == 0
    assert seen == {(fam, act, form, epis) for fam, base in (("f", EPI_C16_BIAS_AUX), ("n", EPI_C16_DACT)) for act in ACTS
                    for form, epis in ((FORM_REFERENCE, (base + act,)), (FORM_PLAIN, (base + act,)), (FORM_SPLITK, (EPI_SLAB, base + act)))}


def test_z_beyond_reach_goes_to_the_reference_kernel(lib):
    m, n, k = 256, 128, 64
    for hook, lds in ((AUX_HOOK, (k, k, n)), (DACT_HOOK, (k, n, n))):
        for cid, (bm, _) in enumerate(TILES):
            edge = ((1 << 31) // 2 - n) // bm                                   # (bm ldz + n) 2 < 2^31 <=> ldz <= edge, up to the rounding below
            ok, over = edge // 8 * 8 - 8, (edge + 8) // 8 * 8
            assert (bm * ok + n) * 2 < 1 << 31 <= (bm * over + n) * 2
            assert hook_answer(lib, hook, RELU, cid, 1, True, m, n, k, *lds, ok)[1] == FORM_PLAIN
            assert hook_answer(lib, hook, RELU, cid, 1, True, m, n, k, *lds, over)[1] == FORM_REFERENCE


def test_the_z_range_of_a_z_of_4_gib_and_more_is_clamped_and_covers_every_tile(lib):
    """M is not limited, only a tile's reach: M = 262144, N = ldz = 8192 is in scope (the hook says plain) and the distance from the first
    tile's first row to Z's end is exactly 2^32 bytes.  For every tile of every member the range the kernels use is at most the true
    distance to the last valid element, covers the tile's own valid rows, and equals the true distance wherever that fits 32 bits."""
    lib.bgemm_mi355x_selfcheck_dact_z_range.restype = ctypes.c_uint
    for (m, n, ldz) in ((262144, 8192, 8192), (262144 + 72, 8192, 8192 + 8), (600000, 4096, 4104), (300, 136, 152)):
        for cid, (bm, _) in enumerate(TILES):
            assert hook_answer(lib, DACT_HOOK, GELU, cid, 1, True, m, n, 64, 64, n, n, ldz)[1] == FORM_PLAIN, (m, n, ldz)
            for m0 in range(0, m, bm):
                true = ((m - 1 - m0) * ldz + n) * 2
                own = ((min(bm, m - m0) - 1) * ldz + n) * 2                     # up to the end of the tile's last valid row
                got = lib.bgemm_mi355x_selfcheck_dact_z_range(m, n, ldz, m0)
                assert own <= got <= true and (got == true or (true > 0xFFFFFFFF and got == 0xFFFFFFFF)), (m, n, ldz, cid, m0, got, true)
    assert lib.bgemm_mi355x_selfcheck_dact_z_range(262144, 8192, 8192, 0) == 0xFFFFFFFF
    assert "bgemm_mi355x_selfcheck_dact_z_range" not in (REPO / "include" / "hgemm_mi355x.h").read_text()


def test_bad_arguments_are_refused(lib):
    m, n, k = 200, 136, 128
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_tn_bias_act_aux.argtypes = [ci] * 2 + [vp] * 5 + [ci] * 8 + [vp]
    lib.bgemm_mi355x_tn_bias_act_aux.argtypes = [vp] * 5 + [ci] * 4 + [vp]
    lib.bgemm_mi355x_launch_nn_dact.argtypes = [ci] * 2 + [vp] * 4 + [ci] * 8 + [vp]
    lib.bgemm_mi355x_nn_dact.argtypes = [vp] * 4 + [ci] * 4 + [vp]
    null, some, other = vp(0), vp(4096), vp(8192)
    # act outside 1..3: refused with every pointer given -- before any HIP call
    for act in (0, 4, -1):
        assert lib.bgemm_mi355x_launch_tn_bias_act_aux(0, 1, some, some, some, some, other, m, n, k, k, k, n, n, act, null) == -1
        assert lib.bgemm_mi355x_tn_bias_act_aux(some, some, some, some, other, m, n, k, act, null) == -1
        assert lib.bgemm_mi355x_launch_nn_dact(0, 1, some, some, other, some, m, n, k, k, n, n, n, act, null) == -1
        assert lib.bgemm_mi355x_nn_dact(some, some, other, some, m, n, k, act, null) == -1
        assert hook_answer(lib, AUX_HOOK, act, 0, 1, True, m, n, k, k, k, n, n) == [-1]
        assert hook_answer(lib, DACT_HOOK, act, 0, 1, True, m, n, k, k, n, n, n) == [-1]
    for act in ACTS:
        # the second matrix: NULL, equal to c, ldz < N
        for z in (null, some):
            assert lib.bgemm_mi355x_launch_tn_bias_act_aux(0, 1, some, some, some, some, z, m, n, k, k, k, n, n, act, null) == -1
            assert lib.bgemm_mi355x_tn_bias_act_aux(some, some, some, some, z, m, n, k, act, null) == -1
            assert lib.bgemm_mi355x_launch_nn_dact(0, 1, some, some, z, some, m, n, k, k, n, n, n, act, null) == -1
            assert lib.bgemm_mi355x_nn_dact(some, some, z, some, m, n, k, act, null) == -1
        assert lib.bgemm_mi355x_launch_tn_bias_act_aux(0, 1, some, some, null, some, other, m, n, k, k, k, n, n, act, null) == -1   # null bias
        for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
            assert lib.bgemm_mi355x_tn_bias_act_aux(null, null, null, null, null, *shape, act, null) == -1
            assert lib.bgemm_mi355x_nn_dact(null, null, null, null, *shape, act, null) == -1
            assert lib.bgemm_mi355x_tn_bias_act_aux_runs(0, *shape, k, k, n, n) == 0 and lib.bgemm_mi355x_nn_dact_runs(0, *shape, k, n, n, n) == 0
        for cid in (-1, 4):
            assert hook_answer(lib, AUX_HOOK, act, cid, 1, True, m, n, k, k, k, n, n) == [-1]
            assert hook_answer(lib, DACT_HOOK, act, cid, 1, True, m, n, k, k, n, n, n) == [-1]


# ---- the derivative text on the CPU ------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "hgemm_act.hpp"
using namespace hgemm_mi355x;
static void show(uint32_t bits) {
  float z;
  memcpy(&z, &bits, 4);
  const float s = 3.0f;
  const float y[6] = {dact_apply<ACT_RELU>(z), dact_apply<ACT_GELU>(z), dact_apply<ACT_GELU_TANH>(z),
                      dact_mul<ACT_RELU>(s, z), dact_mul<ACT_GELU>(s, z), dact_mul<ACT_GELU_TANH>(s, z)};
  uint32_t u[6];
  memcpy(u, y, 24);
  printf("%08x %08x %08x %08x %08x %08x %08x\n", bits, u[0], u[1], u[2], u[3], u[4], u[5]);
}
int main() {
  for (uint32_t h = 0; h < 0x10000u; ++h) show(h << 16);   // every bf16 value, the non-finite ones included
  static_assert(DACT_EPS == 0x1p-19f && DACT_EPS_LOG2 == -19, "eps");
  return 0;
}
"""


@pytest.fixture(scope="module")
def dact_values(tmp_path_factory):
    """Rows (z, relu', gelu', gelu_tanh', 3 x each through dact_mul) for all 65 536 bf16 patterns, from a stand-alone program built with the
    host compiler from hgemm_act.hpp alone."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the derivative text cannot be built for the CPU")
    d = tmp_path_factory.mktemp("dact_cpu")
    (d / "dact_main.cpp").write_text(PROGRAM)
    done = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", str(d / "dact_main.cpp"), "-o", str(d / "dact_main"), "-lm"],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([str(d / "dact_main")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0
    rows = np.array([[int(x, 16) for x in ln.split()] for ln in run.stdout.splitlines()], dtype=np.uint32)
    assert rows.shape == (65536, 7)
    return rows.view(np.float32), rows


def dact64(z, act):
    z = z.astype(np.float64)
    if act == GELU:
        return np.array([0.5 * math.erfc(-v / math.sqrt(2.0)) + v * math.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi) for v in z])
    c = math.sqrt(2.0 / math.pi)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.clip(2.0 * c * (z + 0.044715 * z ** 3), -700, 700)
        s = 1.0 / (1.0 + np.exp(-x))
        t = np.where(np.abs(z) > 40, 0.0, z * s * (1.0 - s) * 2.0 * c * (1.0 + 3 * 0.044715 * z * z))   # (below 1e-300 there; no inf x 0 in the reference either)
    return s + t


def gelu64(z, act):
    z = z.astype(np.float64)
    if act == GELU:
        return np.array([0.5 * v * math.erfc(-v / math.sqrt(2.0)) for v in z])
    with np.errstate(over="ignore"):
        return z / (1.0 + np.exp(-np.clip(2.0 * math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3), -700, 700)))


def test_relu_is_a_select_bit_for_bit(dact_values):
    f, u = dact_values
    z = f[:, 0]
    nan = np.isnan(z)
    assert int((~nan & ~np.isinf(z)).sum()) == 65280
    want = np.where(z <= 0, np.float32(0.0), np.float32(1.0))                   # a NaN z fails the compare: 1
    assert np.array_equal(u[:, 1], want.view(np.uint32))
    passed = np.where(z <= 0, np.float32(0.0), np.float32(3.0))
    assert np.array_equal(u[:, 4], passed.view(np.uint32))                      # S itself or +0: -0 and -inf give +0 (bits 0), NaN passes S
    assert u[0x8000, 4] == 0 and u[0xff80, 4] == 0 and u[0x7fc0, 4] == 0x40400000 and u[0x7f80, 4] == 0x40400000 and u[0x0000, 4] == 0


@pytest.mark.parametrize("act", [GELU, GELU_TANH], ids=["gelu", "gelu_tanh"])
def test_the_gelu_derivatives_are_finite_and_within_eps_of_fp64_on_every_finite_bf16(dact_values, act):
    """With the host math library (the device library is the GPU tests' business).  The other form's derivative and the forward activation in
    place of the derivative are outside eps at no fewer z than stated, counted from the fp64 references alone."""
    f, _ = dact_values
    z = f[:, 0]
    fin = np.isfinite(z)
    zf, gf = z[fin], f[fin, act]
    assert len(zf) == 65280 and np.isfinite(gf).all(), "a finite z with a non-finite derivative"
    ref = dact64(zf, act)
    err = np.abs(gf.astype(np.float64) - ref)
    print(f"act {act}: worst |g - g*| = {err.max() / 2.0 ** -24:.2f} x 2^-24 (eps = {DACT_EPS / 2.0 ** -24:.0f} x 2^-24)")
    assert (err <= DACT_EPS).all(), int((err > DACT_EPS).sum())
    prod = f[fin, 3 + act].astype(np.float64)                                   # dact_mul(3, z): one fp32 multiply behind the derivative
    assert (np.abs(prod - 3.0 * ref) <= 3.0 * DACT_EPS).all()
    other = int((np.abs(dact64(zf, GELU + GELU_TANH - act) - ref) > DACT_EPS).sum())
    forward = int((np.abs(gelu64(zf, act) - ref) > DACT_EPS).sum())
    print(f"act {act}: outside eps: the other form {other}, the forward activation {forward} of 65280")
    assert other >= 1000 and forward >= 30000


@pytest.mark.parametrize("act", [GELU, GELU_TANH], ids=["gelu", "gelu_tanh"])
def test_the_gelu_derivatives_special_values(dact_values, act):
    f, u = dact_values
    g = lambda h: int(u[h, act])                                                # noqa: E731
    one, half = 0x3f800000, 0x3f000000
    assert g(0x7f80) == one and g(0xff80) == 0, "+inf gives exactly 1, -inf gives +0"
    assert math.isnan(f[0x7fc0, act]) and math.isnan(f[0xffc0, act]), "NaN gives NaN"
    assert g(0x0000) == half and g(0x8000) == half, "+-0 gives 1/2"
    z = f[:, 0]
    with np.errstate(invalid="ignore"):
        assert (u[z >= 16, act] == one).all() and (u[z <= -16, act] == 0).all(), "beyond the clamp the limit itself, the largest finite z included"
    assert g(0x7f7f) == one and g(0xff7f) == 0
    assert f[:, act][np.isfinite(z)].min() < -0.1                               # the derivative is negative somewhere (z near -1.5)


# ---- register and scratch audit of units g15 and g16 against their twins, by counting ------------------------------------------------------
def device_isa(tmp, unit, kernel):
    out = tmp / f"{unit}.s"
    done = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S", "--cuda-device-only",
                           str(CSRC / f"hgemm_inst_{unit}.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-2000:]
    text = out.read_text()
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({kernel})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    funcs = {}
    for m in re.finditer(rf"^({kernel}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        funcs[m.group(1)] = [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c and (c.endswith(":") or not c.startswith("."))]
    return text, funcs, meta


TN_KERNEL, NN_KERNEL = r"_ZN12hgemm_mi355x20hgemm_tn_bf16_kernel\w+", r"_ZN12hgemm_mi355x15hgemm_nn_kernel\w+"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_mlp_backward")
    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        jobs = {u: ex.submit(device_isa, tmp, u, k) for u, k in (("g15", TN_KERNEL), ("g14", TN_KERNEL), ("g16", NN_KERNEL), ("g8", NN_KERNEL))}
        return {u: j.result() for u, j in jobs.items()}


def kernel_of(funcs, cfg, cid, epi):
    bm, bn = TILES[cid]
    mine = [f for f in funcs if f"{len(cfg)}{cfg}ILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}EEELi{epi}E" in f]
    assert len(mine) == 1, (cfg, cid, epi)
    return mine[0]


def k_loop(name, codes):
    labels = {c[:-1]: i for i, c in enumerate(codes) if c.endswith(":")}
    loops = []
    for i, c in enumerate(codes):
        m = re.match(r"s_c?branch\w* (\S+)", c)
        if m and m.group(1) in labels and labels[m.group(1)] < i and any(x.startswith("v_mfma") for x in codes[labels[m.group(1)]:i + 1]):
            loops.append((labels[m.group(1)], i))
    assert loops, f"{name}: no K loop found"
    return min(a for a, _ in loops), max(b for _, b in loops)


def reg(md, key):
    return int(re.search(rf"\.amdhsa_{key} (\d+)", md).group(1))


def mnemonics(seq):
    out = {}
    for c in seq:
        if not c.endswith(":") and not c.startswith(("s_waitcnt", "s_nop")):
            out[c.split()[0]] = out.get(c.split()[0], 0) + 1
    return out


@pytest.mark.parametrize("unit", ["g15", "g16"])
def test_the_new_units_hold_twelve_kernels_without_scratch_and_with_their_twins_registers_and_k_loop(lib, isa, unit):
    """g15 against the EPI_C16_BIAS + ACT twins of g14, g16 against the EPI_C16 twins of g8, by counting: no private segment, the member's
    LDS, the twin's next_free_vgpr (occupancy unchanged), and a K loop with the twin's instructions by mnemonic and count -- no particular
    instruction is looked for.  Prints the register table."""
    twin_unit, cfg, base, twin_base, info = ("g14", "CfgTNB", EPI_C16_BIAS_AUX, EPI_C16_BIAS, tn_info) if unit == "g15" else ("g8", "CfgNNB", EPI_C16_DACT, None, nn_info)
    (text, funcs, meta), (_, tfuncs, tmeta) = isa[unit], isa[twin_unit]
    assert set(funcs) == set(meta) and len(funcs) == 12
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family, element type or epilogue (a slab kernel twice)"
    assert not re.search(r"^\s*scratch_", text, re.M)
    print("unit member act accum_offset next_free_vgpr next_free_sgpr | twin")
    for cid, act in itertools.product(range(4), ACTS):
        name = kernel_of(funcs, cfg, cid, base + act)
        twin = kernel_of(tfuncs, cfg, cid, twin_base + act if twin_base is not None else EPI_C16)
        md, tmd = meta[name], tmeta[twin]
        print(unit, (MEMBERS if unit == "g15" else NN_MEMBERS)[cid], act, *(reg(md, k) for k in ("accum_offset", "next_free_vgpr", "next_free_sgpr")), "|",
              *(reg(tmd, k) for k in ("accum_offset", "next_free_vgpr", "next_free_sgpr")))
        assert reg(md, "private_segment_fixed_size") == 0, (name, "private segment: the epilogue spills")
        assert reg(md, "group_segment_fixed_size") == info(lib, cid)[7] == reg(tmd, "group_segment_fixed_size"), (name, "LDS bytes")
        assert reg(md, "next_free_vgpr") == reg(tmd, "next_free_vgpr"), (name, "occupancy: next_free_vgpr is not the twin's")
        codes, tcodes = funcs[name], tfuncs[twin]
        (lo, hi), (tlo, thi) = k_loop(name, codes), k_loop(twin, tcodes)
        body, tbody = codes[lo:hi + 1], tcodes[tlo:thi + 1]
        # the K loop is the twin's: the same instructions by mnemonic and count, whichever the compiler selected (wait and nop counts are the
        # scheduler's), and the same counted vmcnt waits in the same order; nothing of the epilogue's memory traffic was hoisted into it
        assert mnemonics(body) == mnemonics(tbody), (name, "the K loop differs from the twin's")
        assert [c for c in body if "vmcnt" in c] == [c for c in tbody if "vmcnt" in c], (name, "the counted vmcnt of the loop")
