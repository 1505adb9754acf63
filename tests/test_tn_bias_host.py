"""CPU tests of the forward product with a fused bias, bgemm_mi355x_tn_bias (Y = X W^T + b: family f's EPI_C16_BIAS kernels in
hgemm_inst_g12.hip, the third output kind of the transposed-read host path): the names and the header block, the tables the feature must
leave alone, the self-check hook against bgemm_mi355x_selfcheck_launch_tn over tests/test_tn_bf16_host.py's sweep -- the same plan with
EPI_C16_BIAS in the plain dispatch and the combine dispatch and nothing else --, the refusals, a replay of the epilogue's ownership (the
column whose bias a lane adds is the column the value is stored to, and no bias index at or past N is read), and an ISA audit of unit g12 by
the method of that file's audit of g11."""
import ctypes
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from kernel_layout_model import mfma
from test_nn_host import MEMBERS as NN_MEMBERS
from test_ta_host import CSRC, HIPCC, MEMBERS as TA_MEMBERS, NBUF, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import (EPI_C16, EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, MEMBERS, THUNK_ENTRY, THUNK_GENERIC, THUNK_SPLITK_REDUCE,
                               TILES, WORDS, answer, tables_unchanged, tn_info)
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the tn prototypes)

EPI_C16_BIAS = 5
PUBLIC = ("bgemm_mi355x_tn_bias", "bgemm_mi355x_launch_tn_bias", "bgemm_mi355x_tn_bias_runs")
HOOK = "bgemm_mi355x_selfcheck_launch_tn_bias"
SHAPES = [(64, 64, 64), (136, 72, 128), (152, 152, 320), (264, 264, 512), (100, 136, 128), (200, 136, 72), (200, 100, 128), (328, 456, 2048)]


def bias_answer(lib, cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out=0, hook=HOOK):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, hook)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ruled_out, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def with_bias_epi(plain):
    """The answer of the plain bgemm_mi355x_launch_tn call with EPI_C16 replaced by EPI_C16_BIAS in the plain dispatch and in the combine
    dispatch (which carries EPI_SLAB there): (thunk, grid, epi, splits, k_chunk) per dispatch, nothing else touched."""
    if plain == [-1]:
        return plain
    out = list(plain[:5])
    for thunk, grid, epi, splits, k_chunk in plain[5:]:
        if thunk == THUNK_SPLITK_REDUCE or (thunk in (THUNK_ENTRY, THUNK_GENERIC) and epi == EPI_C16):
            epi = EPI_C16_BIAS
        out.append((thunk, grid, epi, splits, k_chunk))
    return out


def test_the_header_declares_the_names_and_the_library_exports_them(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None                                   # (ctypes raises AttributeError for a missing symbol)
    assert getattr(lib, HOOK) is not None and "selfcheck_launch_tn_bias" not in header
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("Forward product with a fused bias"):header.index("hgemm_mi355x_strerror")])
    assert "eplaces bgemm_mi355x_tn followed by an element-wise add" in block and "rounds to bf16 a second time" in block   # what it replaces
    assert "vendor GEMM with a bias epilogue" in block
    assert "added last" in block and "rounded once" in block and "nearest even" in block
    assert "not the accumulators' initial value" in block and "not added into a slab" in block
    assert "bias == NULL: HGEMM_ERR_BAD_ARG" in block and "16-byte aligned" in block and "reference kernel" in block
    for nm in ("hgemm_mi355x_tn", "hgemm_mi355x_launch_tn", "hgemm_mi355x_tn_bias", "bgemm_mi355x_tn_c32", "bgemm_mi355x_nn_bias", "bgemm_mi355x_ta_bias",
               "bgemm_mi355x_tn_bias_plan", "bgemm_mi355x_tn_bias_num_configs"):
        assert not hasattr(lib, nm), nm                                       # no fp16 form, no other layout, no second table


def test_the_tables_and_their_name_hashes_are_unchanged(lib):
    assert lib.hgemm_mi355x_ta_num_configs() == 4 and [lib.hgemm_mi355x_ta_config_name(i).decode() for i in range(4)] == list(TA_MEMBERS)
    assert lib.hgemm_mi355x_nn_num_configs() == 4 and [lib.hgemm_mi355x_nn_config_name(i).decode() for i in range(4)] == list(NN_MEMBERS)
    assert lib.bgemm_mi355x_tn_num_configs() == 4 and [lib.bgemm_mi355x_tn_config_name(i).decode() for i in range(4)] == list(MEMBERS)
    tables_unchanged(lib)                                                       # the geometry table's count and name hash
    build_py = (PKG / "build.py").read_text()
    for unit in ("g11", "g12"):
        assert f"hgemm_inst_{unit}.hip" in build_py
    g11 = (CSRC / "hgemm_inst_g11.hip").read_text()
    assert "HGEMM_TN_BIAS" not in g11 and "HGEMM_TR_MEMBERS(HGEMM_TN_BIAS_INST, CfgTNB)" in (CSRC / "hgemm_inst_g12.hip").read_text()


def test_the_hook_answers_as_the_plain_call_with_the_bias_epilogue_over_the_sweep(lib):
    """Every (member, shape, plan word, stride set, aligned / misaligned / no workspace) of tests/test_tn_bf16_host.py's sweep: tiles,
    cuts, slabs, the splits clamp, grids and forms are the plain call's; bgemm_mi355x_tn_bias_runs equals bgemm_mi355x_tn_runs."""
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, WORDS):
        for lds in ((k, k, n), (k + 8, k + 16, n + 8), (k, k + 4, n), (k, k, n + 4), (k + 4, k, n)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                plain = answer(lib, cid, word, aligned, m, n, k, *lds, ruled_out)
                got = bias_answer(lib, cid, word, aligned, m, n, k, *lds, ruled_out)
                assert got == with_bias_epi(plain), (MEMBERS[cid], (m, n, k), hex(word), lds, aligned, ruled_out)
                assert got[0] == 0 and EPI_C16 not in [d[2] for d in got[5:]] and [d[2] for d in got[5:]].count(EPI_C16_BIAS) == 1
                seen.add((got[1], tuple(d[2] for d in got[5:])))
            assert lib.bgemm_mi355x_tn_bias_runs(cid, m, n, k, *lds) == lib.bgemm_mi355x_tn_runs(cid, m, n, k, *lds)
    assert seen == {(FORM_REFERENCE, (EPI_C16_BIAS,)), (FORM_PLAIN, (EPI_C16_BIAS,)), (FORM_SPLITK, (EPI_SLAB, EPI_C16_BIAS))}
    # the plan words, spelled out on one shape: NT store honoured (same plan), FUSED runs two-pass, STREAMK runs plain, no workspace -> unsplit
    m, n, k = 264, 264, 512
    assert bias_answer(lib, 0, 2 | 0x10000, True, m, n, k, k, k, n)[1] == FORM_SPLITK and bias_answer(lib, 0, 0x40000 | 37, True, m, n, k, k, k, n)[1] == FORM_PLAIN
    assert bias_answer(lib, 0, 5, True, m, n, k, k, k, n, 1 << FORM_SPLITK)[:3] == [0, FORM_PLAIN, 1]
    assert bias_answer(lib, 0, 1 | 0x20000, True, m, n, k, k, k, n) == bias_answer(lib, 0, 1, True, m, n, k, k, k, n)


def test_the_nn_and_ta_layouts_refuse_the_bias_kind(lib):
    for hook, lds in (("bgemm_mi355x_selfcheck_launch_nn_bias", lambda m, n, k: (k, n, n)), ("bgemm_mi355x_selfcheck_launch_ta_bias", lambda m, n, k: (m, n, n))):
        for cid, (m, n, k), word in itertools.product(range(4), SHAPES[:4], (1, 2, 5)):
            for aligned in (True, False):
                assert bias_answer(lib, cid, word, aligned, m, n, k, *lds(m, n, k), hook=hook) == [-1], (hook, cid, (m, n, k), word)


def test_bad_arguments_are_refused(lib):
    m, n, k = 200, 136, 128
    out = (ctypes.c_longlong * 20)()
    for lds in ((k - 8, k, n), (k, k - 8, n), (k, k, n - 8), (0, k, n), (k, 0, n), (k, k, 0), (-k, k, n), (k, -k, n), (k, k, -n)):
        for aligned in (True, False):
            assert bias_answer(lib, 0, 1, aligned, m, n, k, *lds) == [-1], lds
        assert lib.bgemm_mi355x_tn_bias_runs(0, m, n, k, *lds) == 0
    for cid in (-1, 4):
        assert bias_answer(lib, cid, 1, True, m, n, k, k, k, n) == [-1] and lib.bgemm_mi355x_tn_bias_runs(cid, m, n, k, k, k, n) == 0
    # null pointers -- the bias among them -- and empty shapes return before any HIP call
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [ci] * 2 + [vp] * 4 + [ci] * 6 + [vp]
    lib.bgemm_mi355x_tn_bias.argtypes = [vp] * 4 + [ci] * 3 + [vp]
    null, some = vp(0), vp(4096)
    assert lib.bgemm_mi355x_launch_tn_bias(0, 1, some, some, null, some, m, n, k, k, k, n, null) == -1       # a caller without a bias has bgemm_mi355x_tn
    assert lib.bgemm_mi355x_tn_bias(some, some, null, some, m, n, k, null) == -1
    assert lib.bgemm_mi355x_launch_tn_bias(0, 1, null, null, null, null, m, n, k, k, k, n, null) == -1
    for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
        assert lib.bgemm_mi355x_tn_bias(null, null, null, null, *shape, null) == -1
        assert lib.bgemm_mi355x_launch_tn_bias(0, 1, null, null, null, null, *shape, k, k, n, null) == -1
        assert getattr(lib, HOOK)(0, 1, 4, *shape, k, k, n, 0, out) == -1 and lib.bgemm_mi355x_tn_bias_runs(0, *shape, k, k, n) == 0
    assert getattr(lib, HOOK)(0, 1, 4, m, n, k, k, k, n, 0, None) == -1


# ---- the epilogue's ownership, replayed ------------------------------------------------------------------------------------------------
KERNEL_LINES = ("acc[i][j] = tr_mfma(bf[j], af[i], acc[i][j]);",                       # operands swapped: the B fragment is the MFMA's first
                "const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc((void*)g.counters, 0, (uint32_t)g.N * 2u, 0x00020000);",
                "const int n_b = tc.n0 + wave_n * CFG::TN + 16 * j + 4 * (lane >> 4);",
                "bias[j] = __builtin_bit_cast(bx4, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsBias, (uint32_t)n_b * 2u, 0, 0));",
                "for (int e = 0; e < 4; ++e) acc[i][j][e] += (float)bias[j][e];")
EPILOGUE_LINES = ("const int row = wave_m * CFG::TM + i * 16 + (lane & 15);",
                  "const h2 a01 = {(elem)acc[i][j][0], (elem)acc[i][j][1]}, a23 = {(elem)acc[i][j][2], (elem)acc[i][j][3]};",
                  "const h2 b01 = {(elem)acc[i][j + 1][0], (elem)acc[i][j + 1][1]}, b23 = {(elem)acc[i][j + 1][2], (elem)acc[i][j + 1][3]};",
                  "const auto r0 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a01), __builtin_bit_cast(unsigned, b01), false, false);",
                  "const auto r1 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a23), __builtin_bit_cast(unsigned, b23), false, false);",
                  "const int n = tc.n0 + wave_n * CFG::TN + 16 * (j + (q & 1)) + 8 * (q >> 1);",
                  "const u32x4 o = {r0[0], r1[0], r0[1], r1[1]};")


def test_the_replay_helpers_are_the_kernels_expressions():
    text = (CSRC / "hgemm_kernel_tn.hpp").read_text()
    for line in KERNEL_LINES:
        assert line in text, line
    # the bias block stands behind the K loop and in front of the shared epilogue, which is included as it is
    assert text.index("rd = (rd + 1 == NBUF) ? 0 : rd + 1;") < text.index(KERNEL_LINES[1]) < text.index('#include "hgemm_tr_store_c16.inc"')
    inc = (CSRC / "hgemm_tr_store_c16.inc").read_text()
    for line in EPILOGUE_LINES:
        assert line in inc, line


def mfma_owner():
    """{(lane, e): (n, m)} inside a 16 x 16 fragment, from the documented v_mfma_f32_16x16x32 layout (kernel_layout_model.mfma) with the
    kernel's operand order: first operand the B fragment (lane & 15 = n), second the A fragment (lane & 15 = m)."""
    index, ones = np.zeros((64, 8)), np.zeros((64, 8))
    for lane in range(16):                                            # k = 0 alone: D[n][m] = first[n] * second[m]
        index[lane, 0], ones[lane, 0] = 1 + lane, 1
    n_of, m_of = mfma(16, index, ones), mfma(16, ones, index)
    return {(lane, e): (int(n_of[lane, e]) - 1, int(m_of[lane, e]) - 1) for lane in range(64) for e in range(4)}


def permlane16_swap(vdst, src):
    """v_permlane16_swap over {lane: value}: the odd 16-lane rows of vdst are exchanged with the even rows of src."""
    v, s = dict(vdst), dict(src)
    for lane in range(64):
        if (lane >> 4) & 1:
            v[lane], s[lane - 16] = src[lane - 16], vdst[lane]
    return v, s


@pytest.mark.parametrize("cid", range(4), ids=MEMBERS)
def test_every_lane_adds_the_bias_of_the_column_its_value_is_stored_to(cid):
    """Every accumulator element carries two tags through the epilogue of hgemm_tr_store_c16.inc: the column whose bias the kernel's
    expression adds (n_b + e) and the (row, column) of C the MFMA layout says it holds.  After the two swaps and the store's column
    expression both tags equal the column stored to, for every wave, lane, i, j and e -- and every C element of the tile is stored once."""
    bm, bn = TILES[cid]
    tm, tn = bm // 2, bn // 2
    fm, fn = tm // 16, tn // 16
    own = mfma_owner()
    for lane in range(64):
        for e in range(4):
            assert own[(lane, e)] == (4 * (lane >> 4) + e, lane & 15)            # what the kernel's comment states
    stored = {}
    for wave in range(4):
        wave_m, wave_n = wave // 2, wave % 2
        for i in range(fm):
            for j in range(0, fn, 2):
                def tagged(jj, e):
                    return {lane: (wave_n * tn + 16 * jj + 4 * (lane >> 4) + e,                                     # the bias column (n_b + e, n0 = 0)
                                   (wave_m * tm + 16 * i + own[(lane, e)][1], wave_n * tn + 16 * jj + own[(lane, e)][0])) for lane in range(64)}
                a, b = [tagged(j, e) for e in range(4)], [tagged(j + 1, e) for e in range(4)]
                r0 = [permlane16_swap(a[e], b[e]) for e in (0, 1)]               # the two halves of a01 / b01 move together
                r1 = [permlane16_swap(a[e], b[e]) for e in (2, 3)]
                for lane in range(64):
                    q = lane >> 4
                    n = wave_n * tn + 16 * (j + (q & 1)) + 8 * (q >> 1)
                    row = wave_m * tm + i * 16 + (lane & 15)
                    o = [r0[0][0][lane], r0[1][0][lane], r1[0][0][lane], r1[1][0][lane], r0[0][1][lane], r0[1][1][lane], r1[0][1][lane], r1[1][1][lane]]
                    for x, (bias_col, (c_row, c_col)) in enumerate(o):
                        assert (row, n + x) == (c_row, c_col), (MEMBERS[cid], wave, i, j, lane, x)
                        assert bias_col == n + x, (MEMBERS[cid], wave, i, j, lane, x, "the bias of another column")
                        assert (row, n + x) not in stored
                        stored[(row, n + x)] = bias_col
    assert len(stored) == bm * bn
    # a wrong owner is told apart: the post-swap column, or the next column tile
    assert any(16 * (0 + ((lane >> 4) & 1)) + 8 * (lane >> 5) + e != 4 * (lane >> 4) + e for lane in range(64) for e in range(4))


@pytest.mark.parametrize("n_total", [72, 136])
def test_no_bias_index_at_or_past_n_is_read(n_total):
    """The bias descriptor ends at N x 2 bytes and a lane's load is 8 bytes at n_b x 2: the hardware answers a load whose bytes are not
    all inside with zeros and reads nothing.  With N % 8 == 0 a lane's group of four is inside N or wholly at or past it -- never
    straddling, so no in-range load is cut short and every column < N gets its own bias."""
    for cid, (bm, bn) in enumerate(TILES):
        tn, fn = bn // 2, bn // 32
        read, cols = set(), set()
        for n0 in range(0, n_total, bn):
            for wave_n, j, lane in itertools.product(range(2), range(fn), range(64)):
                n_b = n0 + wave_n * tn + 16 * j + 4 * (lane >> 4)
                offset, records = n_b * 2, n_total * 2
                inside = offset + 8 <= records                      # the range check of a raw buffer load of 8 bytes
                assert inside or offset >= records, (MEMBERS[cid], n0, wave_n, j, lane, "a group of four straddles N")
                if inside:
                    read.update(range(n_b, n_b + 4))
                cols.update(c for c in range(n_b, n_b + 4) if c < n_total)
        assert read == set(range(n_total)) == cols and max(read) == n_total - 1, MEMBERS[cid]


# ---- ISA audit of unit g12 -------------------------------------------------------------------------------------------------------------
KERNEL = r"_ZN12hgemm_mi355x20hgemm_tn_bf16_kernel\w+"
CFG = "CfgTNB"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    out = tmp_path_factory.mktemp("audit_tn_bias") / "g12.s"
    done = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S", "--cuda-device-only",
                           str(CSRC / "hgemm_inst_g12.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-2000:]
    text = out.read_text()
    funcs = {m.group(1): [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c]
             for m in re.finditer(rf"^({KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    return text, funcs, meta


def test_the_unit_holds_the_four_bias_kernels_and_nothing_else(lib, isa):
    text, funcs, meta = isa
    assert set(funcs) == set(meta) and len(funcs) == 4
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family, element type or epilogue (a slab kernel twice)"
    for cid, (bm, bn) in enumerate(TILES):
        mine = [f for f in funcs if f"{len(CFG)}{CFG}ILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}EEELi{EPI_C16_BIAS}E" in f]
        assert len(mine) == 1, MEMBERS[cid]
        md = meta[mine[0]]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", md), f"{mine[0]}: private segment"
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", md).group(1)) == tn_info(lib, cid)[7], f"{mine[0]}: LDS bytes"


def test_the_k_loop_is_the_plain_kernels_and_the_bias_is_added_between_the_loop_and_the_converts(isa):
    """Per K stage 2 FM FN v_mfma_f32_16x16x32_bf16 on 2 (FM + FN) ds_read_b128 -- the figures test_tn_bf16_host.py audits of the g11
    EPI_C16 twins --; behind the loop FN 8-byte bias loads, 4 FM FN fp32 adds (v_add_f32, v_pk_add_f32 counting two) and no add anywhere
    else, every one of them in front of the last convert; 2 FM FN v_cvt_pk_bf16_f32 behind the loop only (each sum rounded once); no
    scratch; the plain and the non-temporal 16-byte stores an instruction each."""
    _, funcs, _ = isa
    for name, codes in funcs.items():
        labels = {c[:-1]: i for i, c in enumerate(codes) if c.endswith(":")}
        loops = []
        for i, c in enumerate(codes):
            m = re.match(r"s_c?branch\w* (\S+)", c)
            if m and m.group(1) in labels and labels[m.group(1)] < i and any(x.startswith("v_mfma") for x in codes[labels[m.group(1)]:i + 1]):
                loops.append((labels[m.group(1)], i))
        assert loops, f"{name}: no K loop found"
        lo, hi = min(a for a, _ in loops), max(b for _, b in loops)
        body, tail = codes[lo:hi + 1], codes[hi + 1:]
        fm, fn = (int(x) // 32 for x in re.search(rf"{CFG}ILi(\d+)ELi(\d+)E", name).groups())
        mfma_ = [c for c in body if c.startswith("v_mfma")]
        assert len(mfma_) == 2 * fm * fn and all(c.startswith("v_mfma_f32_16x16x32_bf16") for c in mfma_), name
        assert not [c for c in codes if c.startswith("v_mfma") and not c.startswith("v_mfma_f32_16x16x32_bf16")], f"{name}: another MFMA"
        assert sum(1 for c in body if c.startswith("ds_read_b128")) == 2 * (fm + fn), name
        assert not any(c.startswith(("v_mfma", "ds_read")) for c in codes[:lo] + tail), name

        def adds(seq):
            return sum(2 if c.startswith("v_pk_add_f32") else 1 for c in seq if re.match(r"v_(pk_)?add_f32", c))
        cvt = [i for i, c in enumerate(tail) if c.startswith("v_cvt_pk_bf16_f32")]
        assert len(cvt) == 2 * fm * fn and not any(c.startswith("v_cvt_pk_bf16_f32") for c in codes[:hi + 1]), (name, len(cvt))
        assert adds(codes[:hi + 1]) == 0 and adds(tail[:cvt[-1]]) == 4 * fm * fn == adds(tail), (name, adds(tail))
        assert adds(tail[:cvt[0]]) > 0, f"{name}: a convert in front of the first bias add"
        assert not [c for c in codes if c.startswith(("global_load", "flat_load"))], f"{name}: a load through a raw pointer"
        assert sum(1 for c in tail if c.startswith("buffer_load_dwordx2")) == fn and not any(c.startswith("buffer_load_dwordx2") for c in codes[:hi + 1]), name
        assert not [c for c in codes if re.match(r"v_cvt_(pk_?)?(rtz_)?f16_|v_cvt_pkrtz_f16|v_cvt_\w*_bf8|v_cvt_\w*_fp8", c)], f"{name}: a conversion to fp16"
        assert not [c for c in codes if c.startswith("scratch_")], f"{name}: scratch"
        stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
        assert all(c.startswith("buffer_store_dwordx4") for c in stores), name
        assert sum(1 for c in stores if c.endswith(" nt")) == fm * fn // 2 == sum(1 for c in stores if not c.endswith(" nt")), (name, len(stores))
