"""CPU tests of the bfloat16 forward product, bgemm_mi355x_tn (Y = X W^T, B given as b_col_major [N][ldb]; family f in
hgemm_kernel_tn.hpp, instantiated in hgemm_inst_g11.hip; kLayoutTN, the third layout of the transposed-read host path): the names, the
tables the layout must leave alone, its own table, what the self-check hook answers against the rules restated here in Python -- plan
words, scope, reach, strides, ids --, bad arguments, and an ISA audit of unit g11 by the method of test_tr_bf16_host.py's audit of g8."""
import ctypes
import itertools
import re
import subprocess
from pathlib import Path

import pytest

from test_nn_host import MEMBERS as NN_MEMBERS
from test_ta_host import COUNTER_BYTES, CSRC, GIB, HIPCC, MEMBERS as TA_MEMBERS, NBUF, PKG, REPO, reach_limit
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_ta_host import test_the_geometry_table_and_the_nn_table_are_unchanged_by_the_family as tables_unchanged

MEMBERS = ("f64x64_w2x2", "f128x64_w2x2", "f64x128_w2x2", "f128x128_w2x2")
TILES = ((64, 64), (128, 64), (64, 128), (128, 128))
EPI_C16, EPI_SLAB = 0, 1
THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_GENERIC = 0, 1, 4           # hgemm_api.hip: enum Thunk
FORM_REFERENCE, FORM_SPLITK, FORM_PLAIN = 0, 3, 6                   # hgemm_api.hip: enum Form
FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000                # include/hgemm_mi355x.h: the words of a splits argument
PUBLIC = ("bgemm_mi355x_tn", "bgemm_mi355x_launch_tn", "bgemm_mi355x_tn_runs", "bgemm_mi355x_tn_num_configs", "bgemm_mi355x_tn_config_name",
          "bgemm_mi355x_tn_config_by_name", "bgemm_mi355x_tn_config_info", "bgemm_mi355x_tn_plan", "bgemm_mi355x_tn_plan_workspace_bytes",
          "bgemm_mi355x_tn_reserve_workspace", "bgemm_rocblas_tn")
HOOK = "bgemm_mi355x_selfcheck_launch_tn"


@pytest.fixture(scope="module")
def lib(ta_lib):
    L = ta_lib
    L.bgemm_mi355x_tn_config_name.restype = ctypes.c_char_p
    L.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    L.bgemm_mi355x_tn_plan_workspace_bytes.restype = ctypes.c_size_t
    L.bgemm_mi355x_tn_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    return L


def tn_info(lib, cid):
    out = (ctypes.c_int * 8)()
    assert lib.bgemm_mi355x_tn_config_info(cid, out) == 0
    return list(out)


def test_the_header_declares_the_names_and_the_library_exports_them(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None                                   # (ctypes raises AttributeError for a missing symbol)
    assert getattr(lib, HOOK) is not None and HOOK not in header
    block = header[header.index("bfloat16 forward product"):header.index("hgemm_mi355x_strerror")]
    assert "eplace" in block and "hgemm_mi355x_fp32" in block and "rocblas_gemm_ex" in block        # what the block replaces
    assert "b_col_major" in block and "nearest even" in block and "reference kernel" in block
    assert "unchanged" in block and 'no fp16 "tn" call' in re.sub(r"\s*\n \* ", " ", block)          # the fp16 forward calls; no fp16 tn here
    for nm in ("hgemm_mi355x_tn", "hgemm_mi355x_launch_tn", "hgemm_mi355x_tn_fp32", "bgemm_mi355x_tn_c32"):
        assert not hasattr(lib, nm)
    # the old block's sentence is kept and corrected where it stands
    old = header[header.index("bfloat16 on the NN and TA layouts"):header.index("bfloat16 forward product")]
    assert "NO bf16 form" in old and "bgemm_mi355x_tn" in old


def test_the_other_tables_and_their_name_hashes_are_unchanged(lib):
    assert lib.hgemm_mi355x_ta_num_configs() == 4 and [lib.hgemm_mi355x_ta_config_name(i).decode() for i in range(4)] == list(TA_MEMBERS)
    assert lib.hgemm_mi355x_nn_num_configs() == 4 and [lib.hgemm_mi355x_nn_config_name(i).decode() for i in range(4)] == list(NN_MEMBERS)
    tables_unchanged(lib)                                                       # the geometry table's count and name hash
    for nm in MEMBERS:
        assert lib.hgemm_mi355x_config_by_name(nm.encode()) == -1 and lib.hgemm_mi355x_nn_config_by_name(nm.encode()) == -1
        assert lib.hgemm_mi355x_ta_config_by_name(nm.encode()) == -1
    build_py = (PKG / "build.py").read_text()
    for unit in ("g5", "g6", "g7", "g8", "g9", "g10", "g11"):
        assert f"hgemm_inst_{unit}.hip" in build_py


def test_the_tn_table_has_the_four_names_with_the_n_members_geometry(lib):
    assert lib.bgemm_mi355x_tn_num_configs() == len(MEMBERS)
    nn = (ctypes.c_int * 8)()
    for i, nm in enumerate(MEMBERS):
        assert lib.bgemm_mi355x_tn_config_name(i).decode() == nm and lib.bgemm_mi355x_tn_config_by_name(nm.encode()) == i
        bm, bn, wm, wn, mi, nbuf, threads, lds = tn_info(lib, i)
        assert (bm, bn, wm, wn) == tuple(map(int, re.match(r"f(\d+)x(\d+)_w(\d)x(\d)", nm).groups())) == TILES[i] + (2, 2) and mi == 16
        assert threads == 256 and nbuf == NBUF[i] and lds == nbuf * (bm + bn) * 128 <= 160 * 1024   # NBUF stages of (BM + BN) rows x 128 B
        assert lib.hgemm_mi355x_nn_config_info(i, nn) == 0 and list(nn) == [bm, bn, wm, wn, mi, nbuf, threads, lds]
        assert NN_MEMBERS[i] == "n" + nm[1:]
    assert lib.bgemm_mi355x_tn_config_name(-1) is None and lib.bgemm_mi355x_tn_config_name(4) is None
    assert lib.bgemm_mi355x_tn_config_by_name(b"n64x64_w2x2") == -1 and lib.bgemm_mi355x_tn_config_by_name(None) == -1
    assert lib.bgemm_mi355x_tn_config_info(4, nn) != 0
    # the planner's rule is the NN layout's: the same member by position and the same splits
    c, s, c2, s2 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    grid = (64, 136, 264, 1024, 4096, 8192)
    for m, n, k in itertools.product(grid, grid, (64, 128, 320, 1024, 4096, 8192)):
        assert lib.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(c), ctypes.byref(s)) == 0
        assert lib.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(c2), ctypes.byref(s2)) == 0 and (c.value, s.value) == (c2.value, s2.value)
        assert lib.bgemm_mi355x_tn_runs(c.value, m, n, k, k, k, n) == 1
    assert lib.bgemm_mi355x_tn_plan(256, 264, 512, ctypes.byref(c), ctypes.byref(s)) == 0 and (c.value, s.value) == (0, 8)
    assert lib.bgemm_mi355x_tn_plan(0, 64, 64, ctypes.byref(c), ctypes.byref(s)) == -1
    assert lib.bgemm_mi355x_tn_plan(64, 64, 64, None, ctypes.byref(s)) == -1


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------------
def rule(cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out=0):
    """What a bgemm_mi355x_launch_tn call must decide: [status] when refused, else [0, form, dispatches, slab bytes, 0] + per dispatch
    (thunk, grid, epi, splits, k_chunk)."""
    if not 0 <= cid < 4 or lda < k or ldb < k or ldc < n:
        return [-1]
    bm, bn = TILES[cid]
    tiles = -(-m // bm) * -(-n // bn)
    scope = aligned and k % 64 == 0 and n % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0
    reach = (bm * lda + k) * 2 < 2 * GIB and (bn * ldb + k) * 2 < 2 * GIB and (bm * ldc + n) * 2 < 2 * GIB
    if not (scope and reach) or tiles > 0x7FFFFFFF:
        return [0, FORM_REFERENCE, 1, 0, 0, (THUNK_GENERIC, 0, EPI_C16, 1, k)]
    steps = k // 64
    splits = 1 if word & STREAMK else max(1, min(word & 0xFFFF, steps))
    if ruled_out & (1 << FORM_SPLITK) or tiles * splits > 0x7FFFFFFF:
        splits = 1
    per = -(-steps // splits)
    splits = -(-steps // per)
    if splits > 1:
        return [0, FORM_SPLITK, 2, splits * m * n * 4, 0, (THUNK_ENTRY, tiles * splits, EPI_SLAB, splits, per * 64),
                (THUNK_SPLITK_REDUCE, 0, EPI_SLAB, splits, per * 64)]
    return [0, FORM_PLAIN, 1, 0, 0, (THUNK_ENTRY, tiles, EPI_C16, 1, per * 64)]


def answer(lib, cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out=0):
    out = (ctypes.c_longlong * 20)()
    st = lib.bgemm_mi355x_selfcheck_launch_tn(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ruled_out, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


WORDS = (1, 0, 2, 5, 32, 1 | NT_STORE, 2 | NT_STORE, 2 | FUSED, 5 | FUSED, STREAMK, STREAMK | 37, 1 | FUSED)


def test_the_hook_answers_as_the_rules_say_over_the_grid(lib):
    """Plain calls, splits 2 / 5 / 32 clamped to K / 64, a HGEMM_SPLITK_FUSED word run two-pass, a HGEMM_PLAN_STREAMK word run plain, a
    HGEMM_PLAN_NT_STORE word; workspace = 256 KiB + splits M N 4; the scope edges; a form without a workspace."""
    seen = set()
    shapes = [(64, 64, 64), (136, 72, 128), (152, 152, 320), (264, 264, 512), (100, 136, 128), (200, 136, 72), (200, 100, 128), (328, 456, 2048)]
    for cid, (m, n, k), word in itertools.product(range(4), shapes, WORDS):
        for lds in ((k, k, n), (k + 8, k + 16, n + 8), (k, k + 4, n), (k, k, n + 4), (k + 4, k, n)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                want = rule(cid, word, aligned, m, n, k, *lds, ruled_out)
                got = answer(lib, cid, word, aligned, m, n, k, *lds, ruled_out)
                assert got == want, (MEMBERS[cid], (m, n, k), hex(word), lds, aligned, ruled_out)
                seen.add((want[1], want[5][3]))
            if lds == (k, k, n):
                want = rule(cid, word, True, m, n, k, *lds)
                ws = lib.bgemm_mi355x_tn_plan_workspace_bytes(cid, word, m, n, k)
                assert ws == (COUNTER_BYTES + want[3] if want[3] else 0), (MEMBERS[cid], (m, n, k), hex(word))
                assert want[3] == (want[5][3] * m * n * 4 if want[1] == FORM_SPLITK else 0)
            assert lib.bgemm_mi355x_tn_runs(cid, m, n, k, *lds) == (1 if rule(cid, 1, True, m, n, k, *lds)[1] == FORM_PLAIN else 0)
    # every form, and the clamped split counts, occurred: 32 at K = 2048, 32 -> 8 = K / 64 and 5 -> 4 chunks of 2 stages at K = 512
    assert {(FORM_REFERENCE, 1), (FORM_PLAIN, 1), (FORM_SPLITK, 2), (FORM_SPLITK, 5), (FORM_SPLITK, 32), (FORM_SPLITK, 8), (FORM_SPLITK, 4)} <= seen
    # the named edges, spelled out: M = 100 runs the kernel; K = 72, N = 100, ldb = K + 4, ldc = N + 4 do not
    for cid in range(4):
        assert lib.bgemm_mi355x_tn_runs(cid, 100, 136, 128, 128, 128, 136) == 1
        assert answer(lib, cid, 1, True, 100, 136, 128, 128, 128, 136)[1] == FORM_PLAIN
        for m, n, k, lds in ((200, 136, 72, (72, 72, 136)), (200, 100, 128, (128, 128, 100)), (200, 136, 128, (128, 132, 136)), (200, 136, 128, (128, 128, 140))):
            assert lib.bgemm_mi355x_tn_runs(cid, m, n, k, *lds) == 0
            for word in (1, 4):
                assert answer(lib, cid, word, True, m, n, k, *lds) == [0, FORM_REFERENCE, 1, 0, 0, (THUNK_GENERIC, 0, EPI_C16, 1, k)]
        # ldb is the row stride of b_col_major (>= K), not of a row-major B (>= N)
        assert answer(lib, cid, 1, True, 64, 256, 64, 64, 64, 256)[1] == FORM_PLAIN and answer(lib, cid, 1, True, 64, 64, 256, 256, 64, 64) == [-1]


def test_the_reach_edges_at_2_gib(lib):
    """A: (BM lda + K) 2, B: (BN ldb + K) 2, C: (BM ldc + N) 2 bytes, each below 2 GiB: the largest stride that runs is the rule's, and
    around it the form is the kernel's below and the reference kernel's (status 0) from the edge on, plain and split."""
    for cid, (bm, bn) in enumerate(TILES):
        for m, n, k in ((bm + 8, bn + 8, 128), (2 * bm + 8, 3 * bn + 8, 1024)):
            for side in range(3):
                rows, tail = ((bm, 2 * k), (bn, 2 * k), (bm, 2 * n))[side]
                edge = reach_limit(rows, tail)
                assert rows * edge * 2 + tail < 2 * GIB <= rows * (edge + 8) * 2 + tail
                for ld in (edge - 8, edge, edge + 8, edge + 16):
                    lds = [k, k, n]
                    lds[side] = ld
                    for word in (1, 2):
                        got = answer(lib, cid, word, True, m, n, k, *lds)
                        assert got == rule(cid, word, True, m, n, k, *lds), (MEMBERS[cid], (m, n, k), "ABC"[side], ld, word)
                        assert got[1] == (FORM_REFERENCE if ld > edge else FORM_SPLITK if word == 2 else FORM_PLAIN)
                    assert lib.bgemm_mi355x_tn_runs(cid, m, n, k, *lds) == (0 if ld > edge else 1)
        top = (1 << 31) - 8
        for lds in ((top, 128, 64), (128, top, 64), (128, 128, top), (top, top, top)):     # no 32-bit overflow in the resolver
            assert answer(lib, cid, 4, True, 200, 64, 128, *lds)[:2] == [0, FORM_REFERENCE] and lib.bgemm_mi355x_tn_runs(cid, 200, 64, 128, *lds) == 0
        assert lib.bgemm_mi355x_tn_runs(cid, bm + 8, 64, 128, (1 << 31) // bm, 128, 64) == 0  # BM x lda x 2 = 2^32 would wrap to 0
        assert lib.bgemm_mi355x_tn_runs(cid, 64, bn + 8, 128, 128, (1 << 31) // bn, bn + 8) == 0


def test_bad_arguments_are_refused(lib):
    m, n, k = 200, 136, 128
    out = (ctypes.c_longlong * 20)()
    for lds in ((k - 8, k, n), (k, k - 8, n), (k, k, n - 8), (0, k, n), (k, 0, n), (k, k, 0), (-k, k, n), (k, -k, n), (k, k, -n)):
        for aligned in (True, False):
            assert answer(lib, 0, 1, aligned, m, n, k, *lds) == [-1] == rule(0, 1, aligned, m, n, k, *lds), lds
        assert lib.bgemm_mi355x_tn_runs(0, m, n, k, *lds) == 0
    for cid in (-1, 4):
        assert answer(lib, cid, 1, True, m, n, k, k, k, n) == [-1] and lib.bgemm_mi355x_tn_runs(cid, m, n, k, k, k, n) == 0
        assert lib.bgemm_mi355x_tn_plan_workspace_bytes(cid, 4, m, n, k) == 0
    # null pointers and empty shapes return before any HIP call
    null = ctypes.c_void_p(0)
    assert lib.bgemm_mi355x_launch_tn(0, 1, null, null, null, m, n, k, k, k, n, null) == -1
    assert lib.bgemm_mi355x_tn(null, null, null, m, n, k, null) == -1
    for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
        assert lib.bgemm_mi355x_tn(null, null, null, *shape, null) == -1
        assert lib.bgemm_mi355x_launch_tn(0, 1, null, null, null, *shape, k, k, n, null) == -1
        assert lib.bgemm_mi355x_selfcheck_launch_tn(0, 1, 4, *shape, k, k, n, 0, out) == -1
        assert lib.bgemm_mi355x_tn_runs(0, *shape, k, k, n) == 0 and lib.bgemm_mi355x_tn_plan_workspace_bytes(0, 4, *shape) == 0
        assert lib.bgemm_mi355x_tn_reserve_workspace(*shape, null) == -1
    assert lib.bgemm_mi355x_selfcheck_launch_tn(0, 1, 4, m, n, k, k, k, n, 0, None) == -1


# ---- the operand images: the DMA map and the fragment reads, replayed ---------------------------------------------------------------------
KERNEL_LINES = ("const int r  = il * 8 + (lane >> 3);",
                "const int rc = min(r, isA ? g.M - 1 - tc.m0 : g.N - 1 - tc.n0);",
                "const int chunk = (lane & 7) ^ (((il & 1) << 2) | (lane >> 4));",
                "const int lr = lane & 15, lq = lane >> 4, sw = (lr >> 1) & 7;",
                "f_off[ks] = lr * ROW_BYTES + (((ks * 4 + lq) ^ sw) << 4);",
                "bf[j] = *(const ex8*)(st + b_row_base + j * 16 * ROW_BYTES + f_off[ks]);")


def dma_source(il, lane, rows_valid):
    """(source row, source chunk) of the 16 bytes lane `lane` of 1-KiB piece `il` writes at LDS byte il * 1024 + lane * 16: the kernel's
    voff expression, rows clamped to the last valid one."""
    r = il * 8 + (lane >> 3)
    return min(r, rows_valid - 1), (lane & 7) ^ (((il & 1) << 2) | (lane >> 4))


def fragment_offset(lane, ks):
    lr, lq = lane & 15, lane >> 4
    return lr * 128 + (((ks * 4 + lq) ^ ((lr >> 1) & 7)) << 4)


def test_the_replay_helpers_are_the_kernels_expressions():
    text = (CSRC / "hgemm_kernel_tn.hpp").read_text()
    for line in KERNEL_LINES:
        assert line in text, line


@pytest.mark.parametrize("rows", [64, 128])
def test_both_images_hand_every_lane_its_mfma_operand_and_no_row_past_the_edge_is_read(rows):
    """A tile of `rows` rows (BM for A, BN for b_col_major) staged by the DMA map, then read by the fragment offsets: lane
    (n = lane & 15, kq = lane >> 4) of fragment f and K = 32 slice ks receives k = 32 ks + 8 kq .. + 7 of row 16 f + n; with only
    `valid` rows inside the matrix no source row is at or past `valid` (rows past the edge read the last valid row again)."""
    for valid in (rows, rows - 8, 9, 1):
        image = {}
        for il in range(rows // 8):
            for lane in range(64):
                src = dma_source(il, lane, valid)
                assert src[0] < valid
                image[il * 1024 + lane * 16] = src
        assert len(image) == rows * 8
        for f in range(rows // 16):
            for ks in range(2):
                for lane in range(64):
                    row, chunk = image[f * 16 * 128 + fragment_offset(lane, ks)]
                    assert (row, chunk) == (min(16 * f + (lane & 15), valid - 1), 4 * ks + (lane >> 4)), (rows, valid, f, ks, lane)
    # a read that undoes the swizzle wrongly is told apart
    image = {il * 1024 + lane * 16: dma_source(il, lane, rows) for il in range(rows // 8) for lane in range(64)}
    assert any(image[fragment_offset(lane, 0) ^ 16] != (lane & 15, lane >> 4) for lane in range(64))


# ---- ISA audit of unit g11 -------------------------------------------------------------------------------------------------------------
KERNEL = r"_ZN12hgemm_mi355x20hgemm_tn_bf16_kernel\w+"
CFG = "CfgTNB"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    out = tmp_path_factory.mktemp("audit_tn_bf16") / "g11.s"
    done = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S", "--cuda-device-only",
                           str(CSRC / "hgemm_inst_g11.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-2000:]
    text = out.read_text()
    funcs = {m.group(1): [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c]
             for m in re.finditer(rf"^({KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    return text, funcs, meta


def test_the_unit_holds_the_eight_kernels_and_nothing_else(lib, isa):
    text, funcs, meta = isa
    assert set(funcs) == set(meta) and len(funcs) == 8
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family or element type"
    for cid, (bm, bn) in enumerate(TILES):
        for epi in (EPI_C16, EPI_SLAB):
            mine = [f for f in funcs if f"{len(CFG)}{CFG}ILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}EEELi{epi}E" in f]
            assert len(mine) == 1, (MEMBERS[cid], epi)
            md = meta[mine[0]]
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", md), f"{mine[0]}: private segment"
            assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", md).group(1)) == tn_info(lib, cid)[7], f"{mine[0]}: LDS bytes"


def test_k_loops_run_the_bf16_mfma_on_b128_reads_and_only_the_bf16_epilogue_converts(isa):
    """Per K stage 2 FM FN v_mfma_f32_16x16x32_bf16 and no other MFMA, 2 (FM + FN) ds_read_b128 and no transposed read anywhere;
    v_cvt_pk_bf16_f32 behind the loop of the EPI_C16 kernels only, 2 FM FN of them (each accumulator converted once); no conversion to
    fp16, no scratch; the plain and the non-temporal 16-byte stores an instruction each."""
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
        epi = int(re.search(r"EEELi(\d)E", name).group(1))
        mfma = [c for c in body if c.startswith("v_mfma")]
        assert len(mfma) == 2 * fm * fn and all(c.startswith("v_mfma_f32_16x16x32_bf16") for c in mfma), name
        assert not [c for c in codes if c.startswith("v_mfma") and not c.startswith("v_mfma_f32_16x16x32_bf16")], f"{name}: another MFMA"
        assert sum(1 for c in body if c.startswith("ds_read_b128")) == 2 * (fm + fn), name
        assert not [c for c in codes if "_tr_b" in c or "_tr16_" in c or "_tr8_" in c], f"{name}: a transposed read"
        assert not any(c.startswith(("v_mfma", "ds_read")) for c in codes[:lo] + tail), name
        cvt = [c for c in codes if c.startswith("v_cvt_pk_bf16_f32")]
        assert len(cvt) == (2 * fm * fn if epi == EPI_C16 else 0), (name, len(cvt))
        assert not any(c.startswith("v_cvt_pk_bf16_f32") for c in codes[:hi + 1]), f"{name}: a convert in front of the epilogue"
        assert not [c for c in codes if re.match(r"v_cvt_(pk_?)?(rtz_)?f16_|v_cvt_pkrtz_f16|v_cvt_\w*_bf8|v_cvt_\w*_fp8", c)], f"{name}: a conversion to fp16"
        assert not [c for c in codes if c.startswith("scratch_")], f"{name}: scratch"
        stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
        if epi == EPI_C16:
            assert all(c.startswith("buffer_store_dwordx4") for c in stores), name
            assert sum(1 for c in stores if c.endswith(" nt")) == fm * fn // 2 == sum(1 for c in stores if not c.endswith(" nt")), (name, len(stores))
