"""CPU tests of the forward product with a fused bias and activation, bgemm_mi355x_tn_bias_act (Y = act(X W^T + b): family f's
EPI_C16_BIAS + ACT kernels in hgemm_inst_g14.hip, one more output kind per activation on the transposed-read host path): the names, the
header block and the refusals; the self-check hook over tests/test_tn_bf16_host.py's sweep for each activation -- the plain call's plan with
the activation's epi id in the plain dispatch and in the combine dispatch and nothing else --; the activation text of hgemm_act.hpp built
with the host compiler into a program of its own and held to the bars (ReLU bit for bit, both GELUs inside
1/2 ulp_bf16(y*) + 2^-19 |z| against fp64, the other GELU form outside it); and an ISA audit of unit g14 by counting, against the
EPI_C16_BIAS twins of unit g12."""
import ctypes
import itertools
import math
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_nn_host import MEMBERS as NN_MEMBERS
from test_ta_host import CSRC, HIPCC, MEMBERS as TA_MEMBERS, NBUF, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import (EPI_C16, EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, MEMBERS, THUNK_ENTRY, THUNK_GENERIC, THUNK_SPLITK_REDUCE,
                               TILES, WORDS, answer, tables_unchanged, tn_info)
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the tn prototypes)
from test_tn_bias_host import SHAPES

EPI_C16_BIAS = 5
RELU, GELU, GELU_TANH = 1, 2, 3
ACTS = (RELU, GELU, GELU_TANH)
PUBLIC = ("bgemm_mi355x_tn_bias_act", "bgemm_mi355x_launch_tn_bias_act", "bgemm_mi355x_tn_bias_act_runs")
HOOK = "bgemm_mi355x_selfcheck_launch_tn_bias_act"


def act_answer(lib, act, cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out=0, hook=HOOK):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, hook)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ruled_out, act, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def with_act_epi(plain, act):
    """The answer of the plain bgemm_mi355x_launch_tn call with EPI_C16 replaced by EPI_C16_BIAS + act in the plain dispatch and in the
    combine dispatch (which carries EPI_SLAB there); nothing else touched."""
    if plain == [-1]:
        return plain
    out = list(plain[:5])
    for thunk, grid, epi, splits, k_chunk in plain[5:]:
        if thunk == THUNK_SPLITK_REDUCE or (thunk in (THUNK_ENTRY, THUNK_GENERIC) and epi == EPI_C16):
            epi = EPI_C16_BIAS + act
        out.append((thunk, grid, epi, splits, k_chunk))
    return out


def test_the_header_declares_the_names_and_states_the_semantics(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None                                   # (ctypes raises AttributeError for a missing symbol)
    assert getattr(lib, HOOK) is not None and "selfcheck_launch_tn_bias_act" not in header
    for nm, v in (("HGEMM_ACT_RELU", 1), ("HGEMM_ACT_GELU", 2), ("HGEMM_ACT_GELU_TANH", 3)):
        assert re.search(rf"#define {nm} {v}\b", header), nm
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("Forward product with a fused bias AND activation"):header.index("hgemm_mi355x_strerror")])
    assert "eplaces bgemm_mi355x_tn_bias followed by an element-wise activation kernel" in block and "already rounded to bf16" in block
    assert "applied to the unrounded sum" in block and "never applied to a slab" in block and "rounded once" in block
    assert "-0, -inf and every negative give +0" in block and "NaN stays NaN" in block and "+inf stays +inf" in block
    assert "NaN gives NaN, +inf gives +inf, -inf gives NaN" in block and "gives a zero" in block
    assert "1/2 ulp_bf16(y*) + 2^-19 |z|" in block
    assert "bias == NULL: HGEMM_ERR_BAD_ARG" in block and "zero vector" in block and "act == 0 or any other value: HGEMM_ERR_BAD_ARG" in block
    for nm in ("hgemm_mi355x_tn_bias_act", "bgemm_mi355x_nn_bias_act", "bgemm_mi355x_ta_bias_act", "bgemm_mi355x_tn_act", "bgemm_mi355x_tn_bias_act_plan",
               "bgemm_mi355x_tn_bias_act_num_configs", "bgemm_mi355x_tn_bias_act_reserve_workspace"):
        assert not hasattr(lib, nm), nm                                       # no fp16 form, no other layout, no call without a bias, no second table
    text = (CSRC / "hgemm_act.hpp").read_text()
    assert "ACT_RELU = 1, ACT_GELU = 2, ACT_GELU_TANH = 3" in text
    for src in ("hgemm_kernel_tn.hpp", "hgemm_registry.hip"):
        assert "act_apply<" in (CSRC / src).read_text(), f"{src} does not use the one activation text"


def test_the_tables_the_units_and_the_epilogue_ids(lib):
    assert lib.hgemm_mi355x_ta_num_configs() == 4 and [lib.hgemm_mi355x_ta_config_name(i).decode() for i in range(4)] == list(TA_MEMBERS)
    assert lib.hgemm_mi355x_nn_num_configs() == 4 and [lib.hgemm_mi355x_nn_config_name(i).decode() for i in range(4)] == list(NN_MEMBERS)
    assert lib.bgemm_mi355x_tn_num_configs() == 4 and [lib.bgemm_mi355x_tn_config_name(i).decode() for i in range(4)] == list(MEMBERS)
    tables_unchanged(lib)                                                       # the geometry table's count and name hash
    build_py = (PKG / "build.py").read_text()
    for unit in ("g11", "g12", "g14"):
        assert f"hgemm_inst_{unit}.hip" in build_py
    for unit in ("g11", "g12"):
        assert "HGEMM_TN_ACT" not in (CSRC / f"hgemm_inst_{unit}.hip").read_text()
    g14 = (CSRC / "hgemm_inst_g14.hip").read_text()
    for act in ("ACT_RELU", "ACT_GELU", "ACT_GELU_TANH"):
        assert f"HGEMM_TR_MEMBERS(HGEMM_TN_ACT_INST, {act}, CfgTNB)" in g14
    kernel_hpp = (CSRC / "hgemm_kernel.hpp").read_text()
    assert "EPI_C16_BIAS_RELU = 6, EPI_C16_BIAS_GELU = 7, EPI_C16_BIAS_GELU_TANH = 8" in kernel_hpp


def test_the_hook_answers_as_the_plain_call_with_the_activations_epilogue_over_the_sweep(lib):
    """Every (member, shape, plan word, stride set, aligned / misaligned / no workspace) of tests/test_tn_bf16_host.py's sweep, for each
    activation: tiles, cuts, slabs, the splits clamp, grids and forms are the plain call's; _tn_bias_act_runs equals _tn_runs."""
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, WORDS):
        for lds in ((k, k, n), (k + 8, k + 16, n + 8), (k, k + 4, n), (k, k, n + 4), (k + 4, k, n)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                plain = answer(lib, cid, word, aligned, m, n, k, *lds, ruled_out)
                for act in ACTS:
                    got = act_answer(lib, act, cid, word, aligned, m, n, k, *lds, ruled_out)
                    assert got == with_act_epi(plain, act), (MEMBERS[cid], (m, n, k), hex(word), lds, aligned, ruled_out, act)
                    epis = [d[2] for d in got[5:]]
                    assert got[0] == 0 and EPI_C16 not in epis and EPI_C16_BIAS not in epis and epis.count(EPI_C16_BIAS + act) == 1
                    seen.add((act, got[1], tuple(epis)))
            assert lib.bgemm_mi355x_tn_bias_act_runs(cid, m, n, k, *lds) == lib.bgemm_mi355x_tn_runs(cid, m, n, k, *lds)
    assert seen == {(act, form, epis) for act in ACTS for form, epis in ((FORM_REFERENCE, (EPI_C16_BIAS + act,)), (FORM_PLAIN, (EPI_C16_BIAS + act,)),
                                                                        (FORM_SPLITK, (EPI_SLAB, EPI_C16_BIAS + act)))}


def test_the_nn_and_ta_layouts_refuse_the_activation_kinds(lib):
    for hook, lds in (("bgemm_mi355x_selfcheck_launch_nn_bias_act", lambda m, n, k: (k, n, n)), ("bgemm_mi355x_selfcheck_launch_ta_bias_act", lambda m, n, k: (m, n, n))):
        for cid, (m, n, k), word, act in itertools.product(range(4), SHAPES[:4], (1, 2, 5), ACTS):
            for aligned in (True, False):
                assert act_answer(lib, act, cid, word, aligned, m, n, k, *lds(m, n, k), hook=hook) == [-1], (hook, cid, (m, n, k), word, act)


def test_bad_arguments_are_refused(lib):
    m, n, k = 200, 136, 128
    out = (ctypes.c_longlong * 20)()
    for lds in ((k - 8, k, n), (k, k - 8, n), (k, k, n - 8), (0, k, n), (k, 0, n), (k, k, 0), (-k, k, n), (k, -k, n), (k, k, -n)):
        for aligned, act in itertools.product((True, False), ACTS):
            assert act_answer(lib, act, 0, 1, aligned, m, n, k, *lds) == [-1], lds
        assert lib.bgemm_mi355x_tn_bias_act_runs(0, m, n, k, *lds) == 0
    for cid in (-1, 4):
        assert act_answer(lib, GELU, cid, 1, True, m, n, k, k, k, n) == [-1] and lib.bgemm_mi355x_tn_bias_act_runs(cid, m, n, k, k, k, n) == 0
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_tn_bias_act.argtypes = [ci] * 2 + [vp] * 4 + [ci] * 7 + [vp]
    lib.bgemm_mi355x_tn_bias_act.argtypes = [vp] * 4 + [ci] * 4 + [vp]
    null, some = vp(0), vp(4096)
    # act 0, 4 and -1: refused by the calls and by the hook, with every pointer given -- before any HIP call
    for act in (0, 4, -1):
        assert lib.bgemm_mi355x_launch_tn_bias_act(0, 1, some, some, some, some, m, n, k, k, k, n, act, null) == -1
        assert lib.bgemm_mi355x_tn_bias_act(some, some, some, some, m, n, k, act, null) == -1
        assert act_answer(lib, act, 0, 1, True, m, n, k, k, k, n) == [-1]
    for act in ACTS:
        # a null bias (a layer without one passes a zero vector), null operands, empty shapes
        assert lib.bgemm_mi355x_launch_tn_bias_act(0, 1, some, some, null, some, m, n, k, k, k, n, act, null) == -1
        assert lib.bgemm_mi355x_tn_bias_act(some, some, null, some, m, n, k, act, null) == -1
        for ptrs in ((null, some, some, some), (some, null, some, some), (some, some, some, null), (null, null, null, null)):
            assert lib.bgemm_mi355x_launch_tn_bias_act(0, 1, *ptrs, m, n, k, k, k, n, act, null) == -1
        for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
            assert lib.bgemm_mi355x_tn_bias_act(null, null, null, null, *shape, act, null) == -1
            assert lib.bgemm_mi355x_launch_tn_bias_act(0, 1, null, null, null, null, *shape, k, k, n, act, null) == -1
            assert getattr(lib, HOOK)(0, 1, 4, *shape, k, k, n, 0, act, out) == -1 and lib.bgemm_mi355x_tn_bias_act_runs(0, *shape, k, k, n) == 0
        assert getattr(lib, HOOK)(0, 1, 4, m, n, k, k, k, n, 0, act, None) == -1


# ---- the activation text on the CPU ----------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "hgemm_act.hpp"
using namespace hgemm_mi355x;
static void show(float z) {
  const float y[3] = {act_apply<ACT_RELU>(z), act_apply<ACT_GELU>(z), act_apply<ACT_GELU_TANH>(z)};
  uint32_t u[4];
  memcpy(&u[0], &z, 4);
  memcpy(&u[1], y, 12);
  printf("%08x %08x %08x %08x\n", u[0], u[1], u[2], u[3]);
}
int main() {
  for (int q = -4096; q <= 4096; ++q) show((float)q / 256.0f);
  const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x7f7fffffu, 0xff7fffffu, 0x552bcc77u, 0xd52bcc77u,
                              0x42c80000u, 0xc2c80000u, 0x00000001u, 0x80000001u, 0x5e000000u, 0xde000000u};
  for (uint32_t s : special) { float z; memcpy(&z, &s, 4); show(z); }
  return 0;
}
"""
GRID = 8193


@pytest.fixture(scope="module")
def act_values(tmp_path_factory):
    """(z, relu, gelu, gelu_tanh) as float32 arrays, from a stand-alone program built with the host compiler from hgemm_act.hpp alone."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the activation text cannot be built for the CPU")
    d = tmp_path_factory.mktemp("act_cpu")
    (d / "act_main.cpp").write_text(PROGRAM)
    done = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", str(d / "act_main.cpp"), "-o", str(d / "act_main"), "-lm"],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([str(d / "act_main")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0
    rows = np.array([[int(x, 16) for x in ln.split()] for ln in run.stdout.splitlines()], dtype=np.uint32)
    assert rows.shape == (GRID + 15, 4)
    return rows.view(np.float32), rows


def bf16_rne(x32):
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16
    return r.astype(np.uint32).view(np.float32)


def gelu64(z, act):
    z = z.astype(np.float64)
    if act == GELU:
        return np.array([0.5 * v * math.erfc(-v / math.sqrt(2.0)) for v in z])
    u = math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)
    with np.errstate(over="ignore"):
        return z / (1.0 + np.exp(-2.0 * u))


def bar(y, z):
    ay = np.abs(y)
    half = np.where(ay > 0, 2.0 ** (np.floor(np.log2(np.where(ay > 0, ay, 1.0))) - 8), 0.0)
    return half + 2.0 ** -19 * np.abs(z)


def test_relu_is_exact_on_the_grid_and_on_the_special_values(act_values):
    f, u = act_values
    z, y = f[:, 0], f[:, 1]
    want = np.where(z > 0, z, np.float32(0.0))
    finite = ~np.isnan(z)
    assert np.array_equal(y[finite].view(np.uint32), want[finite].view(np.uint32))          # -0, -inf and every negative give +0 (bits 0)
    sp = {int(a): int(b) for a, b in zip(u[GRID:, 0], u[GRID:, 1])}
    assert sp[0x80000000] == 0 and sp[0xff800000] == 0 and sp[0x7f800000] == 0x7f800000 and sp[0x7fc00000] == 0x7fc00000 and sp[0x80000001] == 0
    assert sp[0x00000001] == 1 and sp[0xff7fffff] == 0 and sp[0x7f7fffff] == 0x7f7fffff


@pytest.mark.parametrize("act", [GELU, GELU_TANH], ids=["gelu", "gelu_tanh"])
def test_the_gelus_are_inside_the_bar_and_the_other_form_is_outside(act_values, act):
    """k / 256 over [-16, 16]: bf16_rne of the text's fp32 value against the fp64 activation; the worst ratio and the worst fp32 error in
    units of 2^-24 |z| are printed.  The OTHER form's values are outside this form's bar at no fewer than 500 points of [-8, 8]."""
    f, _ = act_values
    z, mine, other = f[:GRID, 0], f[:GRID, act], f[:GRID, GELU + GELU_TANH - act]
    y = gelu64(z, act)
    b = bar(y, z)
    err = np.abs(bf16_rne(mine).astype(np.float64) - y)
    nz = z != 0
    print(f"act {act}: worst error / bar {np.max(err[nz] / b[nz]):.3f}; worst fp32 error {np.max(np.abs(mine.astype(np.float64) - y)[nz] / (2.0 ** -24 * np.abs(z[nz]))):.2f} x 2^-24 |z|")
    assert (err <= b).all(), int((err > b).sum())
    assert err[~nz].max() == 0
    part = np.abs(z) <= 8
    off = int((np.abs(bf16_rne(other).astype(np.float64) - y) > b)[part].sum())
    print(f"act {act}: the other form is outside the bar at {off} of {int(part.sum())} points of [-8, 8]")
    assert int(part.sum()) == 4097 and off >= 500


@pytest.mark.parametrize("act", [GELU, GELU_TANH], ids=["gelu", "gelu_tanh"])
def test_the_gelus_special_values(act_values, act):
    f, u = act_values
    sp = {int(a): (float(b), int(c)) for a, b, c in zip(u[GRID:, 0], f[GRID:, act], u[GRID:, act])}
    assert sp[0x00000000][1] == 0 and sp[0x80000000][1] in (0, 0x80000000)                  # +-0 gives a zero
    assert sp[0x7f800000][0] == math.inf and math.isnan(sp[0xff800000][0]) and math.isnan(sp[0x7fc00000][0])
    # large finite z, where z^3 overflows (3.4e38, 1.18e13, 2.3e18): z for the positive one, -0 or a value inside the bound for the negative
    for bits in (0x7f7fffff, 0x552bcc77, 0x5e000000, 0x42c80000):
        zf = struct.unpack("f", struct.pack("I", bits))[0]
        assert sp[bits][0] == zf, hex(bits)
        neg = sp[bits | 0x80000000][0]
        assert abs(neg) <= 2.0 ** -19 * zf and not math.isnan(neg), hex(bits)
    assert sp[0xff7fffff][1] == 0x80000000 and sp[0xd52bcc77][1] == 0x80000000            # -0 where the cube overflowed
    assert sp[0x00000001][0] >= 0 and abs(sp[0x80000001][0]) <= 1e-44                     # a denormal z gives half of it or a zero


# ---- ISA audit of unit g14 against the EPI_C16_BIAS twins of unit g12 ------------------------------------------------------------------------
KERNEL = r"_ZN12hgemm_mi355x20hgemm_tn_bf16_kernel\w+"
CFG = "CfgTNB"


def device_isa(tmp, unit):
    out = tmp / f"{unit}.s"
    done = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S", "--cuda-device-only",
                           str(CSRC / f"hgemm_inst_{unit}.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-2000:]
    text = out.read_text()
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    funcs = {}
    for m in re.finditer(rf"^({KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):   # (as tests/test_tn_bias_host.py cuts them: up to the first s_endpgm)
        funcs[m.group(1)] = [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c and (c.endswith(":") or not c.startswith("."))]
    return text, funcs, meta


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_tn_bias_act")
    return device_isa(tmp, "g14"), device_isa(tmp, "g12")


def kernel_of(funcs, cid, epi):
    bm, bn = TILES[cid]
    mine = [f for f in funcs if f"{len(CFG)}{CFG}ILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}EEELi{epi}E" in f]
    assert len(mine) == 1, (MEMBERS[cid], epi)
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


def test_the_unit_holds_the_twelve_kernels_and_nothing_else(lib, isa):
    (text, funcs, meta), _ = isa
    assert set(funcs) == set(meta) and len(funcs) == 12
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family, element type or epilogue (a slab kernel twice)"
    for cid, act in itertools.product(range(4), ACTS):
        md = meta[kernel_of(funcs, cid, EPI_C16_BIAS + act)]
        assert reg(md, "private_segment_fixed_size") == 0, (MEMBERS[cid], act, "private segment: the activation spills")
        assert reg(md, "group_segment_fixed_size") == tn_info(lib, cid)[7], (MEMBERS[cid], act, "LDS bytes")
    assert not re.search(r"^\s*scratch_", text, re.M)


def test_the_k_loop_is_the_twins_and_the_registers_are_the_twins(isa):
    """Per stage the MFMA, ds_read_b128, LDS-DMA, barrier and wait counts of the EPI_C16_BIAS twin; FN 8-byte bias loads behind the loop
    and none in it; 2 FM FN conversions to bf16, all behind the loop and every one behind the activation's arithmetic (its signature
    instruction: the compare of ReLU, the v_exp_f32 of the GELUs), which stands behind the first bias add; no scratch, no load through a
    raw pointer; 4 FM FN finished values parked in accumulation registers, one per accumulator, in front of the converts; next_free_vgpr is
    the twin's, so occupancy is unchanged.  Prints the register table."""
    (_, funcs, meta), (_, funcs12, meta12) = isa
    print("member act arch_vgpr next_free_vgpr next_free_sgpr")
    for cid in range(4):
        twin = kernel_of(funcs12, cid, EPI_C16_BIAS)
        tlo, thi = k_loop(twin, funcs12[twin])
        tbody = funcs12[twin][tlo:thi + 1]
        print(MEMBERS[cid], "bias", reg(meta12[twin], "accum_offset"), reg(meta12[twin], "next_free_vgpr"), reg(meta12[twin], "next_free_sgpr"))
        bm, bn = TILES[cid]
        fm, fn = bm // 32, bn // 32
        for act in ACTS:
            name = kernel_of(funcs, cid, EPI_C16_BIAS + act)
            codes = funcs[name]
            lo, hi = k_loop(name, codes)
            body, tail = codes[lo:hi + 1], codes[hi + 1:]
            print(MEMBERS[cid], {1: "relu", 2: "gelu", 3: "gelu_tanh"}[act], reg(meta[name], "accum_offset"), reg(meta[name], "next_free_vgpr"),
                  reg(meta[name], "next_free_sgpr"))
            for prefix in ("v_mfma_f32_16x16x32_bf16", "ds_read_b128", "buffer_load_dwordx4", "s_barrier", "s_waitcnt"):
                mine, his = (sum(1 for c in seq if c.startswith(prefix)) for seq in (body, tbody))
                assert mine == his, (name, prefix, mine, his)
            assert sum(1 for c in body if c.startswith("v_mfma")) == 2 * fm * fn and sum(1 for c in body if c.startswith("ds_read_b128")) == 2 * (fm + fn)
            assert not any(c.startswith(("v_mfma", "ds_read")) for c in codes[:lo] + tail), name
            assert sum(1 for c in tail if c.startswith("buffer_load_dwordx2")) == fn and not any(c.startswith("buffer_load_dwordx2") for c in codes[:hi + 1]), name
            assert not [c for c in codes if c.startswith(("global_load", "flat_load", "scratch_"))], name
            cvt = [i for i, c in enumerate(tail) if c.startswith("v_cvt_pk_bf16_f32")]
            assert len(cvt) == 2 * fm * fn and not any(c.startswith("v_cvt_pk_bf16_f32") for c in codes[:hi + 1]), (name, len(cvt))
            # the activation's arithmetic, by its signature instruction: 4 FM FN of them, every one in front of the first convert
            sig = {RELU: r"v_cmp_\w+_f32|v_max_f32|v_cmp_class_f32", GELU: r"v_exp_f32", GELU_TANH: r"v_exp_f32"}[act]
            marks = [i for i, c in enumerate(tail) if re.match(sig, c)]
            assert len(marks) >= (4 * fm * fn if act != GELU else 1), (name, len(marks))
            assert marks[-1] < cvt[0], f"{name}: a conversion to bf16 in front of the activation's arithmetic"
            # the per-value marker: each finished value is written to an accumulation register once, behind its activation and in front
            # of every convert -- 4 FM FN of them, so no accumulator is left without its activation
            parked = [i for i, c in enumerate(tail) if c.startswith("v_accvgpr_write")]
            assert len(parked) == 4 * fm * fn and marks[0] < parked[0] and parked[-1] < cvt[0], (name, len(parked))
            adds = [i for i, c in enumerate(tail) if re.match(r"v_(pk_)?add_f32", c)]
            assert adds and adds[0] < marks[0], f"{name}: the activation in front of the bias add"
            assert not [c for c in codes if re.match(r"v_cvt_(pk_?)?(rtz_)?f16_|v_cvt_pkrtz_f16", c)], f"{name}: a conversion to fp16"
            stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
            assert all(c.startswith("buffer_store_dwordx4") for c in stores) and len(stores) == fm * fn, name
            assert reg(meta[name], "next_free_vgpr") == reg(meta12[twin], "next_free_vgpr"), (name, "occupancy: next_free_vgpr is not the twin's")
