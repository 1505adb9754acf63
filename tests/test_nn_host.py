"""CPU tests of family "n" (hgemm_kernel_nn.hpp: NN layout, row-major B read through transposed LDS reads): the new entry points and
their table, the geometry table they must leave alone, the planner's rule, how the explicit call resolves (hgemm_mi355x_selfcheck_launch_nn:
nothing is launched), a replay of the B image against the MFMA operand contract, and an ISA audit of the family's translation unit."""
import ctypes
import hashlib
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import nn_layout_model as model

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "cuda-l2_amd"
CSRC = PKG / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

MEMBERS = ("n64x64_w2x2", "n128x64_w2x2", "n64x128_w2x2", "n128x128_w2x2")
GRID = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 12288, 16384)          # the 1000 shapes of the tuned table
FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000
COUNTER_BYTES = 256 << 10
FORM = {0: "reference", 1: "ragged", 2: "streamk", 3: "splitk", 4: "fused", 5: "hybrid", 6: "plain"}   # hgemm_api.hip: enum Form
THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_GENERIC = 0, 1, 4                                              # hgemm_api.hip: enum Thunk
EPI_C16, EPI_SLAB = 0, 1
NEW_NAMES = ("hgemm_mi355x_nn_fp32", "hgemm_mi355x_nn_fp16", "hgemm_mi355x_launch_nn", "hgemm_mi355x_nn_num_configs",
             "hgemm_mi355x_nn_config_name", "hgemm_mi355x_nn_config_by_name", "hgemm_mi355x_nn_config_info", "hgemm_mi355x_nn_plan",
             "hgemm_mi355x_nn_runs", "hgemm_mi355x_nn_plan_workspace_bytes", "hgemm_mi355x_nn_reserve_workspace")
# the geometry table as it was before the family: 67 members, their names in id order
TABLE_COUNT = 67
TABLE_SHA256 = "63f6521bf9e7e767c4eb976dce4230a7869a1ca4a62235551e6dd1f58658988e"


@pytest.fixture(scope="module")
def lib():
    import build

    L = ctypes.CDLL(str(build.build_library()))
    L.hgemm_mi355x_config_name.restype = ctypes.c_char_p
    L.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    L.hgemm_mi355x_nn_config_name.restype = ctypes.c_char_p
    L.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    L.hgemm_mi355x_nn_plan_workspace_bytes.restype = ctypes.c_size_t
    L.hgemm_mi355x_nn_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    return L


def nn_info(lib, cid):
    out = (ctypes.c_int * 8)()
    assert lib.hgemm_mi355x_nn_config_info(cid, out) == 0
    return list(out)


def resolve(lib, cid, splits, m, n, k, ld=None, aligned=True, ruled_out=0):
    """What hgemm_mi355x_launch_nn decides, nothing launched: (status, form, slab bytes, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    lda, ldb, ldc = ld or (k, n, n)
    st = lib.hgemm_mi355x_selfcheck_launch_nn(cid, splits, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ruled_out, out)
    return st, FORM[out[0]], out[2], [tuple(out[4 + 8 * i:4 + 8 * i + 5]) for i in range(out[1])]


def test_the_header_declares_the_new_names_and_the_library_exports_them(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in NEW_NAMES:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None                                   # (ctypes raises AttributeError for a missing symbol)
    assert lib.hgemm_mi355x_selfcheck_launch_nn is not None
    # each new block of the header says what it replaces
    block = header[header.index("NN layout"):header.index("hgemm_mi355x_strerror")]
    assert block.count("eplace") >= 3 and "reference" in block


def test_the_table_of_members(lib):
    assert lib.hgemm_mi355x_nn_num_configs() == len(MEMBERS)
    for i, nm in enumerate(MEMBERS):
        assert lib.hgemm_mi355x_nn_config_name(i).decode() == nm and lib.hgemm_mi355x_nn_config_by_name(nm.encode()) == i
        bm, bn, wm, wn, mi, nbuf, threads, lds = nn_info(lib, i)
        assert (bm, bn, wm, wn) == tuple(map(int, re.match(r"n(\d+)x(\d+)_w(\d)x(\d)", nm).groups())) and mi == 16
        assert threads == 64 * wm * wn and nbuf >= 2
        assert lds == nbuf * (bm + bn) * 128 <= 160 * 1024                    # the ring: NBUF stages of BM rows x 128 B + 64 k-rows x BN halfs
    assert lib.hgemm_mi355x_nn_config_name(-1) is None and lib.hgemm_mi355x_nn_config_name(len(MEMBERS)) is None
    assert lib.hgemm_mi355x_nn_config_by_name(b"t64x64_w2x2_m16_s4") == -1
    assert lib.hgemm_mi355x_nn_config_info(len(MEMBERS), (ctypes.c_int * 8)()) != 0


def test_the_geometry_table_is_unchanged_by_the_family(lib):
    assert lib.hgemm_mi355x_num_configs() == TABLE_COUNT
    names = [lib.hgemm_mi355x_config_name(i).decode() for i in range(TABLE_COUNT)]
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == TABLE_SHA256, "a name or an id of the geometry table moved"
    assert names[-1] == "u128x128_w2x2_k4" and not [nm for nm in names if nm[0] == "n"]
    for nm in MEMBERS:
        assert lib.hgemm_mi355x_config_by_name(nm.encode()) == -1
    assert lib.hgemm_mi355x_config_name(TABLE_COUNT) is None


def test_a_b_only_call_of_the_tn_launch_still_runs_the_reference_kernel(lib):
    out = (ctypes.c_longlong * 28)()
    for cfg in (-1, 0, 5):
        assert lib.hgemm_mi355x_selfcheck_launch(cfg, 1, 1, 1 | 4, 512, 512, 512, 512, 512, 512, 0, out) == 0      # operands: b alone
        assert FORM[out[0]] == "reference" and out[1] == 1 and out[4] == THUNK_GENERIC


def test_the_planner_returns_a_listed_member_by_its_rule(lib):
    """The largest member whose tiles fill the 256 CUs; otherwise the 64 x 64 member with min(ceil(256 / tiles), K / 64, 32) splits."""
    c, s = ctypes.c_int(), ctypes.c_int()
    infos = [nn_info(lib, i) for i in range(len(MEMBERS))]
    seen = set()
    for m, n, k in itertools.product(GRID, GRID, GRID):
        assert lib.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(c), ctypes.byref(s)) == 0
        assert 0 <= c.value < len(MEMBERS) and 1 <= s.value <= max(1, k // 64)
        assert lib.hgemm_mi355x_nn_runs(c.value, m, n, k, k, n, n) == 1
        tiles = [-(-m // bm) * -(-n // bn) for bm, bn, *_ in infos]
        filling = [i for i in range(len(MEMBERS)) if tiles[i] >= 256]
        if filling:
            area = max(infos[i][0] * infos[i][1] for i in filling)
            assert infos[c.value][0] * infos[c.value][1] == area and tiles[c.value] >= 256 and s.value == 1, (m, n, k)
        else:
            assert c.value == 0 and s.value == max(1, min(-(-256 // tiles[0]), k // 64, 32)), (m, n, k)
        seen.add(c.value)
    assert {0, 1, 3} <= seen                    # (on the grid 64 x 128 never pads less than 128 x 64, which wins their ties)
    assert lib.hgemm_mi355x_nn_plan(0, 64, 64, ctypes.byref(c), ctypes.byref(s)) != 0
    # off the grid: still a listed member, whether or not the kernel takes the shape
    for shape in ((1, 8, 64), (1000, 520, 72), (333, 100, 64), (5000, 4104, 1088)):
        assert lib.hgemm_mi355x_nn_plan(*shape, ctypes.byref(c), ctypes.byref(s)) == 0 and 0 <= c.value < len(MEMBERS) and s.value >= 1


def test_forms_of_every_plan_word(lib):
    m, n, k = 328, 456, 512
    for cid in range(len(MEMBERS)):
        bm, bn = nn_info(lib, cid)[:2]
        tiles = -(-m // bm) * -(-n // bn)
        for word in (1, 1 | NT_STORE, STREAMK, STREAMK | 37, 1 | FUSED, 0):
            assert resolve(lib, cid, word, m, n, k) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C16, 1, k)]), (cid, hex(word))
            assert lib.hgemm_mi355x_nn_plan_workspace_bytes(cid, word, m, n, k) == 0
        for s in (2, 5, 16):
            chunk = -(-(k // 64) // s) * 64
            real = -(-k // chunk)
            for word in (s, s | FUSED, s | NT_STORE):
                st, form, slab, disp = resolve(lib, cid, word, m, n, k)
                assert (st, form, slab) == (0, "splitk", real * m * n * 4), (cid, hex(word))
                assert disp == [(THUNK_ENTRY, tiles * real, EPI_SLAB, real, chunk), (THUNK_SPLITK_REDUCE, 0, EPI_SLAB, real, chunk)]
                # workspace of a split plan: the counter block + splits x M x N fp32
                assert lib.hgemm_mi355x_nn_plan_workspace_bytes(cid, word, m, n, k) == COUNTER_BYTES + real * m * n * 4
            assert resolve(lib, cid, s, m, n, k, ruled_out=1 << 3) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C16, 1, k)])
        assert resolve(lib, cid, 16, m, n, 64) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C16, 1, 64)])   # one stage: nothing to split
        # padded strides keep the kernel
        assert resolve(lib, cid, 1, m, n, k, ld=(k + 8, n + 24, n + 16))[:2] == (0, "plain")
        assert lib.hgemm_mi355x_nn_runs(cid, m, n, k, k + 8, n + 24, n + 16) == 1


def test_what_the_kernel_does_not_take_falls_back_to_the_reference_kernel(lib):
    for cid in range(len(MEMBERS)):
        cases = {"K = 72": dict(m=200, n=136, k=72), "N = 100": dict(m=200, n=100, k=128),
                 "ldb = N + 4": dict(m=200, n=136, k=128, ld=(128, 140, 136)), "lda = K + 4": dict(m=200, n=136, k=128, ld=(132, 136, 136)),
                 "ldc = N + 4": dict(m=200, n=136, k=128, ld=(128, 136, 140)), "misaligned pointer": dict(m=200, n=136, k=128, aligned=False)}
        for what, kw in cases.items():
            for splits in (1, 4):
                st, form, slab, disp = resolve(lib, cid, splits, **kw)
                assert (st, form, slab) == (0, "reference", 0) and len(disp) == 1 and disp[0][0] == THUNK_GENERIC, (cid, what)
            if "aligned" not in kw:
                ld = kw.get("ld") or (kw["k"], kw["n"], kw["n"])
                assert lib.hgemm_mi355x_nn_runs(cid, kw["m"], kw["n"], kw["k"], *ld) == 0, (cid, what)
        assert lib.hgemm_mi355x_nn_runs(cid, 200, 136, 128, 128, 136, 136) == 1
        # B beyond 2 GiB of 32-bit offsets: the reference kernel as well
        assert resolve(lib, cid, 1, 64, 65536, 16448)[:2] == (0, "reference")


def test_bad_strides_and_ids_are_refused(lib):
    m, n, k = 200, 136, 128
    for ld in ((k - 8, n, n), (k, n - 8, n), (k, n, n - 8), (0, n, n), (k, 0, n), (k, n, -n), (k, k - 8, n)):
        if ld == (k, k - 8, n) and k - 8 >= n:
            continue
        for aligned in (True, False):
            assert resolve(lib, 0, 1, m, n, k, ld=ld, aligned=aligned)[0] == -1, ld
        assert lib.hgemm_mi355x_nn_runs(0, m, n, k, *ld) == 0
    # ldb is B's ROW stride (>= N), not b_col_major's (>= K): K > N is fine with ldb = N, K < N needs ldb >= N
    assert resolve(lib, 0, 1, 64, 64, 256, ld=(256, 64, 64))[:2] == (0, "plain")
    assert resolve(lib, 0, 1, 64, 256, 64, ld=(64, 64, 256))[0] == -1
    for cid in (-1, -2, len(MEMBERS)):
        assert resolve(lib, cid, 1, m, n, k)[0] == -1
        assert lib.hgemm_mi355x_nn_runs(cid, m, n, k, k, n, n) == 0
    null = ctypes.c_void_p(0)
    assert lib.hgemm_mi355x_launch_nn(0, 1, null, null, null, m, n, k, k, n, n, null) == -1       # (returns before any HIP call)
    assert lib.hgemm_mi355x_nn_fp32(null, null, null, m, n, k, null) == -1 and lib.hgemm_mi355x_nn_fp16(null, null, null, 0, n, k, null) == -1


# ---- the 32-bit reach rule (TrLayout::reach_ok), at its boundary ---------------------------------------------------------------------
GIB = 1 << 30


def reach_limit(rows, tail):
    """The largest stride (a multiple of 8) with rows x ld x 2 + tail < 2 GiB."""
    return (2 * GIB - tail - 1) // (2 * rows) // 8 * 8


def test_the_reach_rule_at_its_boundary(lib):
    """For every member and each of A, B and C: the largest stride at which the kernel still runs (bisection over
    hgemm_mi355x_nn_runs, as tests/test_gpu_nn_bars.py finds the strides it executes) is the documented rule's -- A and C:
    BM x ld x 2 + the row's bytes < 2 GiB; B: (K - 1) x ldb x 2 + N x 2 < 2 GiB -- and around it status and form are the rule's:
    the kernel below, the reference kernel (status 0) from the edge on, for plain and split calls."""
    from test_gpu_nn_bars import largest_nn_stride, reach_rule

    for cid in range(len(MEMBERS)):
        bm, bn = nn_info(lib, cid)[:2]
        for m, n, k in ((bm + 8, bn + 8, 128), (bm, bn, 64), (2 * bm + 8, 3 * bn + 8, 1024)):
            for side in range(3):
                rows, tail = reach_rule(bm, m, n, k, side)
                edge = reach_limit(rows, tail)
                assert rows * edge * 2 + tail < 2 * GIB <= rows * (edge + 8) * 2 + tail
                assert largest_nn_stride(lib, cid, m, n, k, side) == edge, (MEMBERS[cid], (m, n, k), "ABC"[side], edge)
                for ld in (edge - 8, edge, edge + 8, edge + 16):
                    lds = [k, n, n]
                    lds[side] = ld
                    for splits in (1, 2):
                        st, form, slab, disp = resolve(lib, cid, splits, m, n, k, ld=tuple(lds))
                        want = ("reference" if ld > edge else "splitk" if splits == 2 and k > 64 else "plain")
                        assert (st, form) == (0, want), (MEMBERS[cid], (m, n, k), "ABC"[side], ld, splits, st, form)
                        assert (slab > 0) == (want == "splitk") and disp[0][0] == (THUNK_GENERIC if want == "reference" else THUNK_ENTRY)


def test_contiguous_b_past_2_gib_runs_the_reference_kernel(lib):
    for cid in range(len(MEMBERS)):
        bm = nn_info(lib, cid)[0]
        # K = 128, contiguous: B spans 127 x N x 2 + N x 2 = 256 N bytes -- the last N below 2 GiB runs (where C's BM rows of N
        # stay below 2 GiB as well: the 64-row members), 2 GiB exactly does not
        for n, runs in ((8388600, int(bm == 64)), (8388608, 0), (8388616, 0)):
            assert lib.hgemm_mi355x_nn_runs(cid, 64, n, 128, 128, n, n) == runs, (cid, n)
            assert resolve(lib, cid, 1, 64, n, 128)[:2] == (0, "plain" if runs else "reference")
        # a contiguous B of 2 GiB, 4 GiB and more
        for n, k in ((16384, 65536), (65536, 16448), (32768, 65536), (1 << 20, 4096)):
            assert n * k * 2 >= 2 * GIB
            for splits in (1, 4):
                st, form, slab, disp = resolve(lib, cid, splits, 64, n, k)
                assert (st, form, slab) == (0, "reference", 0) and disp[0][0] == THUNK_GENERIC, (cid, n, k)
            assert lib.hgemm_mi355x_nn_plan_workspace_bytes(cid, 4, 64, n, k) == 0


def test_strides_near_2_31_do_not_overflow_the_resolver(lib):
    """lda, ldb, ldc up to 2^31 - 8, alone and together, with one row and with many: status 0, the reference kernel, no slabs --
    and a stride that would only pass if a product wrapped round 2^32 or 2^64 is not taken for a small one."""
    top = (1 << 31) - 8
    for cid in range(len(MEMBERS)):
        bm, bn = nn_info(lib, cid)[:2]
        for m, n, k in ((1, 8, 64), (200, 136, 128), (bm + 8, bn + 8, 8192)):
            for lds in ((top, n, n), (k, top, n), (k, n, top), (top, top, top)):
                for splits in (1, 4):
                    st, form, slab, disp = resolve(lib, cid, splits, m, n, k, ld=lds)
                    assert (st, form, slab) == (0, "reference", 0) and len(disp) == 1, (MEMBERS[cid], (m, n, k), lds, st, form)
                assert lib.hgemm_mi355x_nn_runs(cid, m, n, k, *lds) == 0
        # bm x ld x 2 = 2^32 (ld = 2^31 / bm) and (K - 1 + 1) x ldb x 2 = 2^32: a 32-bit product would wrap to 0
        wrap = (1 << 31) // bm
        assert lib.hgemm_mi355x_nn_runs(cid, bm + 8, bn, 128, wrap, bn, bn) == 0 and lib.hgemm_mi355x_nn_runs(cid, bm + 8, bn, 128, 128, bn, wrap) == 0
        assert lib.hgemm_mi355x_nn_runs(cid, 64, bn, 128, 128, (1 << 31) // 128, bn) == 0
        # M near 2^31 with small strides: the tile count and M x ld stay in 64 bits, and the kernel takes it (each tile is small)
        assert resolve(lib, cid, 1, top, 8, 64)[:2] == (0, "plain")


# ---- CPU replay of the B image --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", range(len(MEMBERS)))
def test_b_image_dma_map_and_transposed_reads_meet_the_mfma_contract(lib, cid):
    bm, bn, wm, wn = nn_info(lib, cid)[:4]
    tn = bn // wn
    # every (k, n) of a stage is written exactly once, to bytes inside the image
    image = model.build_image(bn)
    assert len(image) == 64 * bn and sorted(image) == list(range(0, 64 * bn * 2, 2))
    assert sorted(image.values()) == [(k, n) for k in range(64) for n in range(bn)]
    # the DMA's source chunks of one wave instruction stay inside whole k-rows: 64 lanes cover 512 / BN rows x every chunk of them
    for il in range(64 * bn * 2 // 1024):
        rows = {}
        for off, kr, chunk in model.dma_writes(bn)[il * 64:(il + 1) * 64]:
            rows.setdefault(kr, set()).add(chunk)
        assert len(rows) == 512 // bn and all(chunks == set(range(bn // 8)) for chunks in rows.values())
    worst = 1
    for wave_n in range(wn):
        for ks in range(2):
            for jn in range(tn // 16):
                got = [[] for _ in range(64)]
                for h in range(2):
                    addrs = model.read_addresses(bn, tn, wave_n, ks, h, jn)
                    assert all(a % 8 == 0 and 0 <= a and a + 8 <= 64 * bn * 2 for a in addrs)   # 8-byte aligned, inside the image
                    worst = max(worst, model.bank_conflict_ways(addrs))
                    for lane, elems in enumerate(model.transposed_read(image, addrs)):
                        got[lane] += elems
                for lane in range(64):
                    n, kq = lane & 15, lane >> 4
                    want = [(ks * 32 + 8 * kq + e, wave_n * tn + jn * 16 + n) for e in range(8)]
                    assert got[lane] == want, (MEMBERS[cid], wave_n, ks, jn, lane)
    print(f"{MEMBERS[cid]}: transposed reads at most {worst}-way per 32-lane half")
    assert worst <= 2


def test_the_model_tells_a_wrong_image_apart():
    """The replay is not vacuous: without the swizzle the same reads conflict 4- / 8-way, and a read that ignores the swizzle of an
    image written with it delivers wrong elements."""
    for bn, ways in ((64, 4), (128, 8)):
        plain = [(32 * 0 + 8 * (lane >> 4) + ((lane >> 2) & 3)) * bn * 2 + ((lane & 3) >> 1) * 16 + 8 * (lane & 1) for lane in range(64)]
        assert model.bank_conflict_ways(plain) == ways
        image = model.build_image(bn)
        got = model.transposed_read(image, plain)
        assert any(got[lane][q] != (8 * (lane >> 4) + q, lane & 15) for lane in range(64) for q in range(4))


# ---- ISA audit of the family's translation unit alone ---------------------------------------------------------------------------
KERNEL = r"_ZN12hgemm_mi355x15hgemm_nn_kernel\w+"


@pytest.fixture(scope="module")
def nn_isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    out = tmp_path_factory.mktemp("audit_nn") / "g5.s"
    pr = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S",
                         "--cuda-device-only", str(CSRC / "hgemm_inst_g5.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    text = out.read_text()
    funcs = {m.group(1): [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c]
             for m in re.finditer(rf"^({KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    return text, funcs, meta


def test_the_unit_holds_the_family_and_nothing_else(nn_isa):
    text, funcs, meta = nn_isa
    assert set(funcs) == set(meta) and len(funcs) == 2 * len(MEMBERS)      # plain + two-pass slab epilogue per member
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta)    # no kernel of another family is compiled here
    for nm in MEMBERS:
        bm, bn = re.match(r"n(\d+)x(\d+)_", nm).groups()
        assert sum(1 for f in funcs if f"CfgNNILi{bm}ELi{bn}ELi2ELi2E" in f) == 2, nm
    for name, md in meta.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", md), f"{name}: private segment"
        assert not [ln for ln in funcs[name] if "scratch_" in ln], f"{name} uses scratch"
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", md).group(1)) <= 160 * 1024, name


IN_LOOP_EXEC = re.compile(r"^(s_cbranch_exec|v_cmpx|s_and_saveexec)")
EXEC_WRITERS = re.compile(r"^v_cmpx|saveexec|^[sv]_\w+ exec(_lo|_hi)?\b")


def test_k_loop_instruction_streams_and_exec_all_ones_at_the_transposed_reads(nn_isa):
    """The K loop (the backward branches that hold MFMAs) stages by LDS-DMA, waits with a counted vmcnt, meets at ONE barrier and feeds
    v_mfma_f32_16x16x32_f16 from ds_read_b128 (A) and ds_read_b64_tr_b16 (B).  EXEC: nothing between the kernel's entry and its last
    transposed read writes EXEC or branches on it, so every read runs with the all-ones mask the dispatcher sets for a workgroup of
    whole waves.  The plain epilogue has both the plain and the non-temporal store, the slab epilogue 16-byte fp32 stores."""
    _, funcs, _ = nn_isa
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
        mfma = [c for c in body if c.startswith("v_mfma")]
        fm, fn = (int(x) // 32 for x in re.search(r"CfgNNILi(\d+)ELi(\d+)E", name).groups())
        assert len(mfma) == 2 * fm * fn and all(c.startswith("v_mfma_f32_16x16x32_f16") for c in mfma), name
        assert sum(1 for c in body if c.startswith("ds_read_b64_tr_b16")) == 2 * 2 * fn, f"{name}: two transposed reads per operand"
        assert sum(1 for c in body if c.startswith("ds_read_b128")) == 2 * fm, name
        assert any(c.startswith("buffer_load_dwordx4") and c.endswith(" lds") for c in body), f"{name}: no LDS-DMA in the K loop"
        assert sum(1 for c in body if c == "s_barrier") == 1, f"{name}: one barrier per stage"
        assert any(re.match(r"s_waitcnt vmcnt\([1-9]\d*\)", c) for c in body), f"{name}: no counted vmcnt in the K loop"
        assert not any(c.startswith(("global_load", "flat_load", "buffer_store", "global_store")) for c in body), name
        assert not any(c.startswith(("v_mfma", "ds_read_b64_tr_b16")) for c in tail + codes[:lo]), name
        last_tr = max(i for i, c in enumerate(codes) if c.startswith("ds_read_b64_tr_b16"))
        # between the loop head and the last transposed read: no branch on EXEC, no compare that writes it, no saveexec ...
        assert not [c for c in codes[lo:last_tr + 1] if IN_LOOP_EXEC.search(c)], name
        # ... and from the kernel's entry on nothing writes EXEC at all (the prologue may hold the compiler's scalar
        # `s_cbranch_execz`, which reads the all-ones mask and writes nothing)
        assert not [c for c in codes[:last_tr + 1] if EXEC_WRITERS.search(c)], f"{name}: EXEC is written in front of a transposed read"
        stores = [c for c in tail if c.startswith(("buffer_store", "global_store"))]
        if name.endswith("ELi1EEEvNS_8GemmArgsE"):
            assert stores and all(c.startswith("global_store_dwordx4") for c in stores), name
        else:
            assert any(c.startswith("buffer_store_dwordx4") and c.endswith(" nt") for c in stores), f"{name}: no non-temporal store"
            assert any(c.startswith("buffer_store_dwordx4") and not c.endswith(" nt") for c in stores), name
