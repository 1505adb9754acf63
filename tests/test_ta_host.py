"""CPU tests of family "a" (hgemm_kernel_ta.hpp: the TA layout -- A given as a_col_major [K][M], B row-major, both MFMA operands read
through transposed LDS reads): the new entry points and their table, the geometry and NN tables they must leave alone, the planner's
rule, how the explicit call resolves (hgemm_mi355x_selfcheck_launch_ta: nothing is launched), the reach rule of A at its boundary, a
replay of the A image against the MFMA operand contract, and an ISA audit of the family's translation unit."""
import ctypes
import hashlib
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import nn_layout_model as model
from test_nn_host import MEMBERS as NN_MEMBERS, TABLE_COUNT, TABLE_SHA256

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "cuda-l2_amd"
CSRC = PKG / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

MEMBERS = ("a64x64_w2x2", "a128x64_w2x2", "a64x128_w2x2", "a128x128_w2x2")
NBUF = (4, 3, 3, 3)
GRID = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 12288, 16384)
FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000
COUNTER_BYTES = 256 << 10
FORM = {0: "reference", 1: "ragged", 2: "streamk", 3: "splitk", 4: "fused", 5: "hybrid", 6: "plain"}   # hgemm_api.hip: enum Form
THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_GENERIC = 0, 1, 4                                              # hgemm_api.hip: enum Thunk
EPI_C16, EPI_SLAB = 0, 1
GIB = 1 << 30
NEW_NAMES = ("hgemm_mi355x_ta_fp32", "hgemm_mi355x_ta_fp16", "hgemm_mi355x_launch_ta", "hgemm_mi355x_ta_num_configs",
             "hgemm_mi355x_ta_config_name", "hgemm_mi355x_ta_config_by_name", "hgemm_mi355x_ta_config_info", "hgemm_mi355x_ta_plan",
             "hgemm_mi355x_ta_runs", "hgemm_mi355x_ta_plan_workspace_bytes", "hgemm_mi355x_ta_reserve_workspace", "hgemm_rocblas_ta")


@pytest.fixture(scope="module")
def lib():
    import build

    L = ctypes.CDLL(str(build.build_library()))
    for fam in ("", "nn_", "ta_"):
        getattr(L, f"hgemm_mi355x_{fam}config_name").restype = ctypes.c_char_p
        getattr(L, f"hgemm_mi355x_{fam}config_by_name").argtypes = [ctypes.c_char_p]
    L.hgemm_mi355x_ta_plan_workspace_bytes.restype = ctypes.c_size_t
    L.hgemm_mi355x_ta_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    return L


def ta_info(lib, cid):
    out = (ctypes.c_int * 8)()
    assert lib.hgemm_mi355x_ta_config_info(cid, out) == 0
    return list(out)


def resolve(lib, cid, splits, m, n, k, ld=None, aligned=True, ruled_out=0):
    """What hgemm_mi355x_launch_ta decides, nothing launched: (status, form, slab bytes, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    lda, ldb, ldc = ld or (m, n, n)
    st = lib.hgemm_mi355x_selfcheck_launch_ta(cid, splits, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ruled_out, out)
    return st, FORM[out[0]], out[2], [tuple(out[4 + 8 * i:4 + 8 * i + 5]) for i in range(out[1])]


def test_the_header_declares_the_new_names_and_the_library_exports_them(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in NEW_NAMES:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None                                   # (ctypes raises AttributeError for a missing symbol)
    assert lib.hgemm_mi355x_selfcheck_launch_ta is not None
    block = header[header.index("TA layout"):header.index("hgemm_mi355x_strerror")]
    assert "non-temporal" in block and '"nt"' in block                         # the name is explained once, where a caller reads it
    assert "eplace" in block and "reference kernel" in block
    kernel = (CSRC / "hgemm_kernel_ta.hpp").read_text()
    assert '"nt"' in kernel and "non-temporal" in kernel


def test_the_table_of_members(lib):
    assert lib.hgemm_mi355x_ta_num_configs() == len(MEMBERS)
    for i, nm in enumerate(MEMBERS):
        assert lib.hgemm_mi355x_ta_config_name(i).decode() == nm and lib.hgemm_mi355x_ta_config_by_name(nm.encode()) == i
        bm, bn, wm, wn, mi, nbuf, threads, lds = ta_info(lib, i)
        assert (bm, bn, wm, wn) == tuple(map(int, re.match(r"a(\d+)x(\d+)_w(\d)x(\d)", nm).groups())) and mi == 16
        assert threads == 64 * wm * wn == 256 and nbuf == NBUF[i]
        assert lds == nbuf * (bm + bn) * 128 <= 160 * 1024                    # the ring: NBUF stages of 64 k-rows x (BM + BN) halfs
    assert lib.hgemm_mi355x_ta_config_name(-1) is None and lib.hgemm_mi355x_ta_config_name(len(MEMBERS)) is None
    assert lib.hgemm_mi355x_ta_config_by_name(b"n64x64_w2x2") == -1 and lib.hgemm_mi355x_ta_config_by_name(b"t64x64_w2x2_m16_s4") == -1
    assert lib.hgemm_mi355x_ta_config_info(len(MEMBERS), (ctypes.c_int * 8)()) != 0


def test_the_geometry_table_and_the_nn_table_are_unchanged_by_the_family(lib):
    assert lib.hgemm_mi355x_num_configs() == TABLE_COUNT
    names = [lib.hgemm_mi355x_config_name(i).decode() for i in range(TABLE_COUNT)]
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == TABLE_SHA256, "a name or an id of the geometry table moved"
    assert lib.hgemm_mi355x_config_name(TABLE_COUNT) is None
    assert lib.hgemm_mi355x_nn_num_configs() == len(NN_MEMBERS)
    assert [lib.hgemm_mi355x_nn_config_name(i).decode() for i in range(len(NN_MEMBERS))] == list(NN_MEMBERS)
    for nm in MEMBERS:
        assert lib.hgemm_mi355x_config_by_name(nm.encode()) == -1 and lib.hgemm_mi355x_nn_config_by_name(nm.encode()) == -1
    assert "hgemm_inst_g6.hip" in (PKG / "build.py").read_text()


def test_the_planner_returns_a_listed_member_by_its_rule(lib):
    """The largest member whose tiles fill the 256 CUs; otherwise a64x64 with min(ceil(256 / tiles), K / 64, 32) splits -- and on
    every shape the member and split count hgemm_mi355x_nn_plan gives by position (one rule, two tables)."""
    c, s, c2, s2 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    infos = [ta_info(lib, i) for i in range(len(MEMBERS))]
    seen = set()
    for m, n, k in itertools.product(GRID, GRID, GRID):
        assert lib.hgemm_mi355x_ta_plan(m, n, k, ctypes.byref(c), ctypes.byref(s)) == 0
        assert 0 <= c.value < len(MEMBERS) and 1 <= s.value <= max(1, k // 64)
        assert lib.hgemm_mi355x_ta_runs(c.value, m, n, k, m, n, n) == 1
        tiles = [-(-m // bm) * -(-n // bn) for bm, bn, *_ in infos]
        filling = [i for i in range(len(MEMBERS)) if tiles[i] >= 256]
        if filling:
            area = max(infos[i][0] * infos[i][1] for i in filling)
            assert infos[c.value][0] * infos[c.value][1] == area and tiles[c.value] >= 256 and s.value == 1, (m, n, k)
        else:
            assert c.value == 0 and s.value == max(1, min(-(-256 // tiles[0]), k // 64, 32)), (m, n, k)
        assert lib.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(c2), ctypes.byref(s2)) == 0 and (c.value, s.value) == (c2.value, s2.value)
        seen.add(c.value)
    assert {0, 1, 3} <= seen
    for (m, n, k), want in (((256, 264, 512), 8), ((200, 136, 192), 3)):
        assert lib.hgemm_mi355x_ta_plan(m, n, k, ctypes.byref(c), ctypes.byref(s)) == 0 and (c.value, s.value) == (0, want)
    assert lib.hgemm_mi355x_ta_plan(0, 64, 64, ctypes.byref(c), ctypes.byref(s)) != 0
    for shape in ((1, 8, 64), (1000, 520, 72), (333, 100, 64), (5000, 4104, 1088)):
        assert lib.hgemm_mi355x_ta_plan(*shape, ctypes.byref(c), ctypes.byref(s)) == 0 and 0 <= c.value < len(MEMBERS) and s.value >= 1


def test_forms_of_every_plan_word(lib):
    m, n, k = 328, 456, 512
    for cid in range(len(MEMBERS)):
        bm, bn = ta_info(lib, cid)[:2]
        tiles = -(-m // bm) * -(-n // bn)
        for word in (1, 1 | NT_STORE, STREAMK, STREAMK | 37, 1 | FUSED, 0):
            assert resolve(lib, cid, word, m, n, k) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C16, 1, k)]), (cid, hex(word))
            assert lib.hgemm_mi355x_ta_plan_workspace_bytes(cid, word, m, n, k) == 0
        for s in (2, 5, 16):
            chunk = -(-(k // 64) // s) * 64
            real = -(-k // chunk)
            for word in (s, s | FUSED, s | NT_STORE):
                st, form, slab, disp = resolve(lib, cid, word, m, n, k)
                assert (st, form, slab) == (0, "splitk", real * m * n * 4), (cid, hex(word))
                assert disp == [(THUNK_ENTRY, tiles * real, EPI_SLAB, real, chunk), (THUNK_SPLITK_REDUCE, 0, EPI_SLAB, real, chunk)]
                assert lib.hgemm_mi355x_ta_plan_workspace_bytes(cid, word, m, n, k) == COUNTER_BYTES + real * m * n * 4
            assert resolve(lib, cid, s, m, n, k, ruled_out=1 << 3) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C16, 1, k)])
        assert resolve(lib, cid, 16, m, n, 64) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C16, 1, 64)])   # one stage: nothing to split
        assert resolve(lib, cid, 1, m, n, k, ld=(m + 24, n + 24, n + 40))[:2] == (0, "plain")                # padded strides keep the kernel
        assert lib.hgemm_mi355x_ta_runs(cid, m, n, k, m + 24, n + 24, n + 40) == 1


def test_what_the_kernel_does_not_take_falls_back_to_the_reference_kernel(lib):
    m, n, k = 200, 136, 128
    cases = {"K = 72": dict(m=m, n=n, k=72), "M = 100": dict(m=100, n=n, k=k), "N = 100": dict(m=m, n=100, k=k),
             "lda = M + 4": dict(m=m, n=n, k=k, ld=(m + 4, n, n)), "ldb = N + 4": dict(m=m, n=n, k=k, ld=(m, n + 4, n)),
             "ldc = N + 4": dict(m=m, n=n, k=k, ld=(m, n, n + 4)), "misaligned pointer": dict(m=m, n=n, k=k, aligned=False)}
    for cid in range(len(MEMBERS)):
        for what, kw in cases.items():
            for splits in (1, 4):
                st, form, slab, disp = resolve(lib, cid, splits, **kw)
                assert (st, form, slab) == (0, "reference", 0) and len(disp) == 1 and disp[0][0] == THUNK_GENERIC, (cid, what)
            if "aligned" not in kw:
                ld = kw.get("ld") or (kw["m"], kw["n"], kw["n"])
                assert lib.hgemm_mi355x_ta_runs(cid, kw["m"], kw["n"], kw["k"], *ld) == 0, (cid, what)
        assert lib.hgemm_mi355x_ta_runs(cid, m, n, k, m, n, n) == 1


def test_bad_strides_and_ids_are_refused(lib):
    m, n, k = 200, 136, 128
    for ld in ((m - 8, n, n), (m, n - 8, n), (m, n, n - 8), (0, n, n), (m, 0, n), (m, n, -n), (k, n, n)):
        for aligned in (True, False):
            assert resolve(lib, 0, 1, m, n, k, ld=ld, aligned=aligned)[0] == -1, ld
        assert lib.hgemm_mi355x_ta_runs(0, m, n, k, *ld) == 0
    # lda is the row stride of a_col_major (>= M), not of a row-major A (>= K)
    assert resolve(lib, 0, 1, 64, 64, 256, ld=(64, 64, 64))[:2] == (0, "plain")
    assert resolve(lib, 0, 1, 256, 64, 64, ld=(64, 64, 64))[0] == -1
    for cid in (-1, -2, len(MEMBERS)):
        assert resolve(lib, cid, 1, m, n, k)[0] == -1
        assert lib.hgemm_mi355x_ta_runs(cid, m, n, k, m, n, n) == 0
    null = ctypes.c_void_p(0)
    assert lib.hgemm_mi355x_launch_ta(0, 1, null, null, null, m, n, k, m, n, n, null) == -1       # (returns before any HIP call)
    assert lib.hgemm_mi355x_ta_fp32(null, null, null, m, n, k, null) == -1 and lib.hgemm_mi355x_ta_fp16(null, null, null, 0, n, k, null) == -1


# ---- the 32-bit reach rule, at its boundary -------------------------------------------------------------------------------------
def reach_limit(rows, tail):
    """The largest stride (a multiple of 8) with rows x ld x 2 + tail < 2 GiB."""
    return (2 * GIB - tail - 1) // (2 * rows) // 8 * 8


def reach_rule(bm, m, n, k, side):
    """(rows, tail bytes) of the limit on operand `side` (0: A, 1: B, 2: C): rows x ld x 2 + tail < 2 GiB.  A and B are addressed from
    row 0 to the end of the matrix (K - 1 strides, then M or N elements), C from a tile's first row (BM strides, then N elements)."""
    return ((k - 1, 2 * m), (k - 1, 2 * n), (bm, 2 * n))[side]


def largest_ta_stride(lib, cid, m, n, k, side):
    """The largest stride (a multiple of 8) of operand `side` at which the member's kernel still runs, the others contiguous, by
    bisection over hgemm_mi355x_ta_runs."""
    def runs(s):
        lds = [m, n, n]
        lds[side] = s
        return lib.hgemm_mi355x_ta_runs(cid, m, n, k, *lds) == 1

    lo, hi = (m, n, n)[side] // 8, 1 << 27
    assert runs(8 * lo) and not runs(8 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if runs(8 * mid) else (lo, mid)
    return 8 * lo


def test_the_reach_rule_at_its_boundary(lib):
    """Every member, each of A, B and C: the largest stride at which the kernel still runs is the documented rule's, and around it
    status and form are the rule's -- the kernel below, the reference kernel (status 0) from the edge on, plain and split."""
    assert reach_limit(*reach_rule(64, 72, 64, 128, 0)) == 8454656                 # K = 128, M = 72: 127 strides + 144 bytes
    assert lib.hgemm_mi355x_ta_runs(0, 72, 64, 128, 8454656, 64, 64) == 1 and lib.hgemm_mi355x_ta_runs(0, 72, 64, 128, 8454664, 64, 64) == 0
    for cid in range(len(MEMBERS)):
        bm, bn = ta_info(lib, cid)[:2]
        for m, n, k in ((bm + 8, bn + 8, 128), (bm, bn, 128), (2 * bm + 8, 3 * bn + 8, 1024)):
            for side in range(3):
                rows, tail = reach_rule(bm, m, n, k, side)
                edge = reach_limit(rows, tail)
                assert rows * edge * 2 + tail < 2 * GIB <= rows * (edge + 8) * 2 + tail
                assert largest_ta_stride(lib, cid, m, n, k, side) == edge, (MEMBERS[cid], (m, n, k), "ABC"[side], edge)
                for ld in (edge - 8, edge, edge + 8, edge + 16):
                    lds = [m, n, n]
                    lds[side] = ld
                    for splits in (1, 2):
                        st, form, slab, disp = resolve(lib, cid, splits, m, n, k, ld=tuple(lds))
                        want = "reference" if ld > edge else "splitk" if splits == 2 else "plain"
                        assert (st, form) == (0, want), (MEMBERS[cid], (m, n, k), "ABC"[side], ld, splits, st, form)
                        assert (slab > 0) == (want == "splitk") and disp[0][0] == (THUNK_GENERIC if want == "reference" else THUNK_ENTRY)


def test_contiguous_a_past_2_gib_runs_the_reference_kernel(lib):
    for cid in range(len(MEMBERS)):
        # K = 128, contiguous: A spans 127 x M x 2 + M x 2 = 256 M bytes -- the last M below 2 GiB runs, 2 GiB exactly does not
        for m, runs in ((8388600, 1), (8388608, 0), (8388616, 0)):
            assert lib.hgemm_mi355x_ta_runs(cid, m, 64, 128, m, 64, 64) == runs, (cid, m)
            assert resolve(lib, cid, 1, m, 64, 128)[:2] == (0, "plain" if runs else "reference")
        for m, k in ((16384, 65536), (65536, 16448), (32768, 65536), (1 << 20, 4096)):
            assert m * k * 2 >= 2 * GIB
            for splits in (1, 4):
                st, form, slab, disp = resolve(lib, cid, splits, m, 64, k)
                assert (st, form, slab) == (0, "reference", 0) and disp[0][0] == THUNK_GENERIC, (cid, m, k)
            assert lib.hgemm_mi355x_ta_plan_workspace_bytes(cid, 4, m, 64, k) == 0


def test_strides_near_2_31_do_not_overflow_the_resolver(lib):
    top = (1 << 31) - 8
    for cid in range(len(MEMBERS)):
        bm, bn = ta_info(lib, cid)[:2]
        for m, n, k in ((8, 8, 64), (200, 136, 128), (bm + 8, bn + 8, 8192)):
            for lds in ((top, n, n), (m, top, n), (m, n, top), (top, top, top)):
                for splits in (1, 4):
                    st, form, slab, disp = resolve(lib, cid, splits, m, n, k, ld=lds)
                    assert (st, form, slab) == (0, "reference", 0) and len(disp) == 1, (MEMBERS[cid], (m, n, k), lds, st, form)
                assert lib.hgemm_mi355x_ta_runs(cid, m, n, k, *lds) == 0
        # (K - 1 + 1) x ld x 2 = 2^32 and BM x ldc x 2 = 2^32: a 32-bit product would wrap to (almost) 0
        assert lib.hgemm_mi355x_ta_runs(cid, 64, bn, 128, (1 << 31) // 128, bn, bn) == 0
        assert lib.hgemm_mi355x_ta_runs(cid, 64, bn, 128, 64, (1 << 31) // 128, bn) == 0
        assert lib.hgemm_mi355x_ta_runs(cid, bm + 8, bn, 128, bm + 8, bn, (1 << 31) // bm) == 0
        # M near 2^31 with small strides is outside the rule as well (A's k-rows are M elements long): the reference kernel, status 0
        assert resolve(lib, cid, 1, top, 8, 64)[:2] == (0, "reference")


# ---- CPU replay of the A image --------------------------------------------------------------------------------------------------
def ta_read_address(bm, tm, wave_m, ks, h, i, lane):
    """hgemm_kernel_ta.hpp, `a_off[h][i]` + the K = 32 slice: the byte address inside the A image one lane hands a transposed read
    (test_the_lane_address_helper_is_the_kernels_expression pins the source lines this restates)."""
    gq, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
    kr = 8 * gq + 4 * h + q
    chunk = (wave_m * tm + i * 16) // 8 + (p >> 1)
    return ks * 32 * (bm * 2) + kr * (bm * 2) + ((chunk ^ model.swz(bm, kr)) << 4) + 8 * (p & 1)


KERNEL_LINES = ("const int gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;",
                "const int kr = 8 * gq + 4 * h + q;",
                "const int chunk = (wave_m * CFG::TM + i * 16) / 8 + (p >> 1);",
                "a_off[h][i] = kr * CFG::A_ROW_BYTES + ((chunk ^ nn_swz<BM>(kr)) << 4) + 8 * (p & 1);",
                "const char* pa = st + ks * 32 * CFG::A_ROW_BYTES;",
                "const int kr = il * CFG::A_RPP + lane / CFG::A_CH;",
                "const int chunk = (lane % CFG::A_CH) ^ nn_swz<BM>(kr);",
                "static constexpr int A_ROW_BYTES = BM * 2;")


def test_the_lane_address_helper_is_the_kernels_expression():
    src = (CSRC / "hgemm_kernel_ta.hpp").read_text()
    for line in KERNEL_LINES:
        assert line in src, f"hgemm_kernel_ta.hpp no longer holds `{line}`: ta_read_address / the replay restate it"
    assert "ta_read_address" in src                                             # the kernel points back at this file
    nn = (CSRC / "hgemm_kernel_nn.hpp").read_text()
    assert "return BN == 128 ? (((krow & 3) << 2) | ((krow >> 2) & 3)) : ((((krow >> 1) & 1) | (((krow >> 3) & 1) << 1)) << 1);" in nn
    for bm, tm in ((64, 32), (128, 64)):
        for wave_m, ks, h, i in itertools.product(range(2), range(2), range(2), range(tm // 16)):
            assert [ta_read_address(bm, tm, wave_m, ks, h, i, lane) for lane in range(64)] == model.read_addresses(bm, tm, wave_m, ks, h, i)


@pytest.mark.parametrize("cid", range(len(MEMBERS)))
def test_a_image_dma_map_and_transposed_reads_meet_the_mfma_contract(lib, cid):
    """nn_layout_model with bn := BM, tn := TM, wave_n := wave_m: the A image has the shape of family n's B image."""
    bm, bn, wm, wn = ta_info(lib, cid)[:4]
    tm = bm // wm
    image = model.build_image(bm)                                               # (asserts that no LDS byte is written twice)
    assert len(image) == 64 * bm and sorted(image) == list(range(0, 64 * bm * 2, 2))
    assert sorted(image.values()) == [(k, m) for k in range(64) for m in range(bm)]
    assert 64 * bm * 2 // 1024 == bm // 8                                        # the classic piece count
    for il in range(bm // 8):
        rows = {}
        for off, kr, chunk in model.dma_writes(bm)[il * 64:(il + 1) * 64]:
            rows.setdefault(kr, set()).add(chunk)
        assert len(rows) == 512 // bm and all(chunks == set(range(bm // 8)) for chunks in rows.values())
    worst = 1
    for wave_m in range(wm):
        for ks in range(2):
            for i in range(tm // 16):
                got = [[] for _ in range(64)]
                for h in range(2):
                    addrs = [ta_read_address(bm, tm, wave_m, ks, h, i, lane) for lane in range(64)]
                    assert all(a % 8 == 0 and 0 <= a and a + 8 <= 64 * bm * 2 for a in addrs)   # 8-byte aligned, inside the image
                    worst = max(worst, model.bank_conflict_ways(addrs))
                    for lane, elems in enumerate(model.transposed_read(image, addrs)):
                        got[lane] += elems
                for lane in range(64):
                    mm, kq = lane & 15, lane >> 4
                    want = [(ks * 32 + 8 * kq + e, wave_m * tm + i * 16 + mm) for e in range(8)]
                    assert got[lane] == want, (MEMBERS[cid], wave_m, ks, i, lane)
    print(f"{MEMBERS[cid]}: transposed reads of A at most {worst}-way per 32-lane half")
    assert worst == 1


def test_the_replay_tells_a_wrong_image_apart():
    """Swizzle omitted on the read of an image written with it: wrong elements, and the plain addresses conflict 4- / 8-way."""
    for bm, tm, ways in ((64, 32, 4), (128, 64, 8)):
        image = model.build_image(bm)
        right = [ta_read_address(bm, tm, 0, 0, 0, 0, lane) for lane in range(64)]
        plain = [(8 * (lane >> 4) + ((lane >> 2) & 3)) * bm * 2 + (((lane & 3) >> 1) << 4) + 8 * (lane & 1) for lane in range(64)]
        assert plain != right and model.bank_conflict_ways(plain) == ways and model.bank_conflict_ways(right) == 1
        got = model.transposed_read(image, plain)
        assert any(got[lane][q] != (8 * (lane >> 4) + q, lane & 15) for lane in range(64) for q in range(4))
        good = model.transposed_read(image, right)
        assert all(good[lane][q] == (8 * (lane >> 4) + q, lane & 15) for lane in range(64) for q in range(4))


# ---- ISA audit of the family's translation unit alone ---------------------------------------------------------------------------
KERNEL = r"_ZN12hgemm_mi355x15hgemm_ta_kernel\w+"


@pytest.fixture(scope="module")
def ta_isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    out = tmp_path_factory.mktemp("audit_ta") / "g6.s"
    pr = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S",
                         "--cuda-device-only", str(CSRC / "hgemm_inst_g6.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    text = out.read_text()
    funcs = {m.group(1): [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c]
             for m in re.finditer(rf"^({KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    return text, funcs, meta


def test_the_unit_holds_the_family_and_nothing_else(lib, ta_isa):
    text, funcs, meta = ta_isa
    assert set(funcs) == set(meta) and len(funcs) == 2 * len(MEMBERS)      # plain + two-pass slab epilogue per member
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta)    # no kernel of another family is compiled here
    for cid, nm in enumerate(MEMBERS):
        bm, bn = re.match(r"a(\d+)x(\d+)_", nm).groups()
        mine = [f for f in funcs if f"CfgTAILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}E" in f]
        assert len(mine) == 2, nm
        for name in mine:
            md = meta[name]
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", md), f"{name}: private segment"
            assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", md).group(1)) == ta_info(lib, cid)[7], f"{name}: LDS bytes"


EXEC_WRITERS = re.compile(r"^v_cmpx|saveexec|^[sv]_\w+ exec(_lo|_hi)?\b")


def test_k_loop_instruction_streams_and_exec_all_ones_at_the_transposed_reads(ta_isa):
    """Per K stage (the backward branches that hold MFMAs): 4 (FM + FN) ds_read_b64_tr_b16 -- two per fragment and K = 32 slice, for
    BOTH operands --, 2 FM FN v_mfma_f32_16x16x32_f16, and no ds_read_b128 between the first and the last MFMA.  EXEC: no instruction
    between the kernel's entry and its last transposed read writes it, so every read runs with the all-ones mask the dispatcher sets
    for a workgroup of whole waves."""
    _, funcs, _ = ta_isa
    for name, codes in funcs.items():
        labels = {c[:-1]: i for i, c in enumerate(codes) if c.endswith(":")}
        loops = []
        for i, c in enumerate(codes):
            m = re.match(r"s_c?branch\w* (\S+)", c)
            if m and m.group(1) in labels and labels[m.group(1)] < i and any(x.startswith("v_mfma") for x in codes[labels[m.group(1)]:i + 1]):
                loops.append((labels[m.group(1)], i))
        assert loops, f"{name}: no K loop found"
        lo, hi = min(a for a, _ in loops), max(b for _, b in loops)
        body = codes[lo:hi + 1]
        fm, fn = (int(x) // 32 for x in re.search(r"CfgTAILi(\d+)ELi(\d+)E", name).groups())
        mfma = [i for i, c in enumerate(body) if c.startswith("v_mfma")]
        assert len(mfma) == 2 * fm * fn and all(body[i].startswith("v_mfma_f32_16x16x32_f16") for i in mfma), name
        assert sum(1 for c in body if c.startswith("ds_read_b64_tr_b16")) == 4 * (fm + fn), f"{name}: two transposed reads per fragment and slice"
        assert not [c for c in body[mfma[0]:mfma[-1] + 1] if c.startswith("ds_read_b128")], f"{name}: ds_read_b128 in the K loop"
        assert not any(c.startswith(("v_mfma", "ds_read_b64_tr_b16")) for c in codes[:lo] + codes[hi + 1:]), name
        last_tr = max(i for i, c in enumerate(codes) if c.startswith("ds_read_b64_tr_b16"))
        assert not [c for c in codes[:last_tr + 1] if EXEC_WRITERS.search(c)], f"{name}: EXEC is written in front of a transposed read"
