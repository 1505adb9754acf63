"""CPU tests of family "u" (hgemm_kernel_lu.hpp: the K walk of one output tile split over four K-groups of waves inside the
workgroup, partial accumulators reduced through LDS): the registry rows and the queries that answer for them, the planner's
silence about the family, how the launch resolves its plan words, and an ISA audit of its translation unit."""
import ctypes
import itertools
import random
import re
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "cuda-l2_amd"
CSRC = PKG / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

MEMBERS = ("u64x64_w2x2_k4", "u128x64_w2x2_k4", "u64x128_w2x2_k4", "u128x128_w2x2_k4")
GRID = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 12288, 16384)          # the 1000 shapes of the tuned table
FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000
COUNTER_BYTES = 256 << 10                                                  # arrival counters in front of the slabs
FORM = {0: "reference", 1: "ragged", 2: "streamk", 3: "splitk", 4: "fused", 5: "hybrid", 6: "plain"}   # hgemm_api.hip: enum Form
EPI_C16, EPI_SLAB = 0, 1


@pytest.fixture(scope="module")
def lib():
    import build

    L = ctypes.CDLL(str(build.build_library()))
    L.hgemm_mi355x_config_name.restype = ctypes.c_char_p
    L.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    L.hgemm_mi355x_model_us.restype = ctypes.c_double
    L.hgemm_mi355x_model_us.argtypes = [ctypes.c_int] * 5
    L.hgemm_mi355x_plan_workspace_bytes.restype = ctypes.c_size_t
    L.hgemm_mi355x_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    return L


def names(lib):
    return [lib.hgemm_mi355x_config_name(i).decode() for i in range(lib.hgemm_mi355x_num_configs())]


def info(lib, cid):
    out = (ctypes.c_int * 8)()
    assert lib.hgemm_mi355x_config_info(cid, out) == 0
    return list(out)


def resolve(lib, cid, splits, m, n, k, ld=None, ruled_out=0):
    """What hgemm_mi355x_launch decides, nothing launched: (status, form, slab bytes, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 28)()
    lda, ldb, ldc = ld or (k, k, n)
    st = lib.hgemm_mi355x_selfcheck_launch(cid, splits, 1, 7, m, n, k, lda, ldb, ldc, ruled_out, out)
    return st, FORM[out[0]], out[2], [tuple(out[4 + 8 * i:4 + 8 * i + 5]) for i in range(out[1])]


def test_members_resolve_by_name_behind_family_w(lib):
    all_names = names(lib)
    last_w = max(i for i, nm in enumerate(all_names) if nm[0] == "w")
    ids = []
    for nm in MEMBERS:
        cid = lib.hgemm_mi355x_config_by_name(nm.encode())
        assert cid >= 0, f"{nm} missing from the library"
        assert cid > last_w and lib.hgemm_mi355x_config_name(cid).decode() == nm
        ids.append(cid)
    assert ids == sorted(ids) and ids[-1] == len(all_names) - 1            # appended: nothing behind them, ids of the others unmoved
    assert all(nm[0] != "u" for nm in all_names[:ids[0]])
    assert sorted(nm for nm in all_names if nm[0] == "u") == sorted(MEMBERS)
    # the families in front keep the order of the geometry table: t, then s / q, then r, then w
    order = "".join(ch for ch, _ in itertools.groupby("q" if nm[0] == "s" else nm[0] for nm in all_names))
    assert order == "tqrwu"


def test_geometry_and_local_splits(lib):
    all_names = names(lib)
    for nm in MEMBERS:
        cid = all_names.index(nm)
        bm, bn, wm, wn, mi, nbuf, threads, lds = info(lib, cid)
        assert (bm, bn) == tuple(map(int, re.match(r"u(\d+)x(\d+)_", nm).groups())) and (wm, wn, mi) == (2, 2, 16)
        assert threads == wm * wn * 4 * 64 == 1024 and nbuf >= 2 and lds <= 160 * 1024
        assert lib.hgemm_mi355x_config_local_splits(cid) == 4
        stage = lib.hgemm_mi355x_config_k_granularity(cid)
        assert stage in (64, 128, 256)
        assert lds == nbuf * (bm + bn) * 2 * stage                         # the ring: NBUF stages of (BM + BN) rows x stage halfs
        assert lib.hgemm_mi355x_config_streamk(cid) == 0
        assert lib.hgemm_mi355x_model_us(cid, 1, 1024, 256, 2048) > 0 and lib.hgemm_mi355x_model_us(cid, 4, 1024, 256, 2048) > 0
    for nm in ("q256x256_w2x2", "t64x64_w2x2_m16_s4", "w32x32_k4", "w64x64", "r64x64_k256", "s256x256_w2x2"):
        assert lib.hgemm_mi355x_config_local_splits(all_names.index(nm)) == 1, nm
    assert all(lib.hgemm_mi355x_config_local_splits(i) == (4 if nm[0] == "u" else 1) for i, nm in enumerate(all_names))
    assert lib.hgemm_mi355x_config_local_splits(-1) == -1 and lib.hgemm_mi355x_config_local_splits(-2) == -1
    assert lib.hgemm_mi355x_config_local_splits(len(all_names)) == -1


def test_accepts_k_exactly_the_multiples_of_the_stage_depth(lib):
    all_names = names(lib)
    for nm in MEMBERS:
        cid = all_names.index(nm)
        stage = lib.hgemm_mi355x_config_k_granularity(cid)
        for k in list(range(1, 1100)) + [2048, 2104, 4096, 8192, 8200, 16384]:
            assert lib.hgemm_mi355x_config_accepts_k(cid, k) == (1 if k % stage == 0 else 0), (nm, k)


def test_workspace_and_forms_of_every_plan_word(lib):
    """splits = 1: no workspace whatever flags ride along; an external split count composes as the TWO-PASS form (slab epilogue +
    the combine kernel) with [splits][M][N] fp32 slabs behind the counter block; the single-launch word runs as two-pass, the
    stream-K word as the plain launch; a K that is not whole stages goes to the any-shape kernel with status 0."""
    all_names = names(lib)
    m, n = 328, 456
    for nm in MEMBERS:
        cid = all_names.index(nm)
        bm, bn = info(lib, cid)[:2]
        stage = lib.hgemm_mi355x_config_k_granularity(cid)
        tiles = -(-m // bm) * -(-n // bn)
        k = 8 * stage
        for word in (1, 1 | NT_STORE, STREAMK, STREAMK | 37, 1 | FUSED):
            assert lib.hgemm_mi355x_plan_workspace_bytes(cid, word, m, n, k) == 0, (nm, hex(word))
            assert resolve(lib, cid, word, m, n, k) == (0, "plain", 0, [(0, tiles, EPI_C16, 1, k)]), (nm, hex(word))
        for s in (2, 5, 16):
            chunk = -(-(k // stage) // s) * stage
            real = -(-k // chunk)
            for word in (s, s | FUSED, s | NT_STORE):
                assert lib.hgemm_mi355x_plan_workspace_bytes(cid, word, m, n, k) == COUNTER_BYTES + real * m * n * 4, (nm, hex(word))
                st, form, slab, disp = resolve(lib, cid, word, m, n, k)
                assert (st, form, slab) == (0, "splitk", real * m * n * 4), (nm, hex(word))
                assert disp == [(0, tiles * real, EPI_SLAB, real, chunk), (1, 0, EPI_SLAB, real, chunk)], (nm, hex(word), disp)
            # without workspace the plan runs unsplit, still on the family's own kernel
            assert resolve(lib, cid, s, m, n, k, ruled_out=1 << 3)[:2] == (0, "plain")
        # one stage: nothing to split
        assert resolve(lib, cid, 16, m, n, stage) == (0, "plain", 0, [(0, tiles, EPI_C16, 1, stage)])
        # K not whole stages (a multiple of 64 or not): the any-shape kernel, status 0
        for bad_k in (stage + 64 if stage > 64 else stage + 8, stage + 8, 3 * stage + 40, 64, 200):
            if bad_k % stage == 0:
                continue
            assert resolve(lib, cid, 1, m, n, bad_k)[:2] == (0, "ragged"), (nm, bad_k)
            assert resolve(lib, cid, 4, m, n, bad_k)[:3] == (0, "ragged", 0), (nm, bad_k)
            assert lib.hgemm_mi355x_plan_workspace_bytes(cid, 4, m, n, bad_k) == 0
        # padded strides keep the family's kernel; a stride below K is refused
        assert resolve(lib, cid, 1, m, n, k, ld=(k + 8, k + 24, n + 16))[:2] == (0, "plain")
        assert resolve(lib, cid, 1, m, n, k, ld=(k - 8, k, n))[0] != 0


def test_the_planner_never_returns_a_family_u_geometry(lib):
    u_ids = {i for i, nm in enumerate(names(lib)) if nm[0] == "u"}
    assert len(u_ids) == len(MEMBERS)
    shapes = list(itertools.product(GRID, GRID, GRID))
    shapes += [tuple(map(int, ln.split("_"))) for ln in (PKG / "tools" / "offgrid_shapes.txt").read_text().split()
               if not ln.startswith("#") and "_" in ln]
    rnd = random.Random(20)
    for _ in range(400):   # multiples of the family's stages and tiles: the shapes it could be asked for
        shapes.append((64 * rnd.randint(1, 64), 64 * rnd.randint(1, 64), 128 * rnd.randint(1, 64)))
    for _ in range(200):   # anything
        shapes.append((rnd.randint(1, 5000), 4 * rnd.randint(1, 1200), 8 * rnd.randint(1, 1100)))
    assert len(shapes) > 1600
    c, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cc, ss, gg = (ctypes.c_int * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    for m, n, k in shapes:
        assert lib.hgemm_mi355x_plan(m, n, k, ctypes.byref(c), ctypes.byref(s), ctypes.byref(g)) == 0
        assert c.value not in u_ids, (m, n, k)
        cnt = lib.hgemm_mi355x_insitu_candidates(m, n, k, cc, ss, gg)
        assert not (set(cc[:cnt]) & u_ids), (m, n, k)


# ---- ISA audit of the family's translation unit alone -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lu_isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    out = tmp_path_factory.mktemp("audit_lu") / "g4.s"
    pr = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S",
                         "--cuda-device-only", str(CSRC / "hgemm_inst_g4.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    text = out.read_text()
    funcs = {m.group(1): [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
             for m in re.finditer(r"^(_ZN12hgemm_mi355x18hgemm_tn_lu_kernel\w+):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (_ZN12hgemm_mi355x18hgemm_tn_lu_kernel\w+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    vgprs = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(_ZN12hgemm_mi355x18hgemm_tn_lu_kernel\w+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)}
    return text, funcs, meta, vgprs


def test_the_unit_holds_the_family_and_nothing_else(lu_isa):
    text, funcs, meta, _ = lu_isa
    assert set(funcs) == set(meta) and len(funcs) == 2 * len(MEMBERS)      # plain + two-pass slab epilogue per member
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta)    # no kernel of another family is compiled here
    for nm in MEMBERS:
        bm, bn = re.match(r"u(\d+)x(\d+)_", nm).groups()
        assert sum(1 for f in funcs if f"CfgLUILi{bm}ELi{bn}ELi2ELi2E" in f) == 2, nm


def test_register_and_lds_budget_of_four_waves_per_simd(lu_isa):
    _, funcs, meta, vgprs = lu_isa
    for name, lines in funcs.items():
        md = meta[name]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", md), f"{name}: private segment"
        assert not [ln for ln in lines if "scratch_" in ln], f"{name} uses scratch"
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", md).group(1)) <= 128, name
        assert vgprs[name] <= 128, f"{name}: {vgprs[name]} registers (VGPRs and AGPRs together): not four waves per SIMD"
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", md).group(1)) <= 160 * 1024, name
        print(f"{vgprs[name]:>4} registers  {name}")


def test_k_loop_and_reduce_instruction_streams(lu_isa):
    """The K loop (the innermost backward branch that holds MFMAs) stages by LDS-DMA, waits with a counted vmcnt, meets at ONE
    barrier and feeds v_mfma_f32_16x16x32_f16 from ds_read_b128; behind it the reduce writes and reads LDS in 16-byte pieces
    around a barrier, and the plain epilogue has both the plain and the non-temporal store."""
    _, funcs, _, _ = lu_isa
    for name, codes in funcs.items():
        labels = {c[:-1]: i for i, c in enumerate(codes) if c.endswith(":")}
        loops = []
        for i, c in enumerate(codes):
            m = re.match(r"s_c?branch\w* (\S+)", c)
            if m and m.group(1) in labels and labels[m.group(1)] < i:
                body = codes[labels[m.group(1)]:i + 1]
                if any(x.startswith("v_mfma") for x in body):
                    loops.append((labels[m.group(1)], i))
        assert loops, f"{name}: no K loop found"
        lo = min(a for a, _ in loops)
        hi = max(b for _, b in loops)
        body, tail = codes[lo:hi + 1], codes[hi + 1:]
        mfma = [c for c in body if c.startswith("v_mfma")]
        assert mfma and all(c.startswith("v_mfma_f32_16x16x32_f16") for c in mfma), name
        assert any(c.startswith("buffer_load_dwordx4") and c.endswith(" lds") for c in body), f"{name}: no LDS-DMA in the K loop"
        assert any(c.startswith("ds_read_b128") for c in body), name
        assert sum(1 for c in body if c == "s_barrier") == 1, f"{name}: one barrier per stage"
        # a ring of three or more stages keeps NBUF - 2 of them in flight across the barrier (a two-stage ring waits for all)
        nbuf = int(re.search(r"CfgLUILi\d+ELi\d+ELi\d+ELi\d+ELi\d+ELi(\d+)EEE", name).group(1))
        assert nbuf < 3 or any(re.match(r"s_waitcnt vmcnt\([1-9]\d*\)", c) for c in body), f"{name}: no counted vmcnt in the K loop"
        assert not any(c.startswith(("global_load", "flat_load", "buffer_store", "global_store")) for c in body), name
        # behind the loop: the reduce
        assert not any(c.startswith("v_mfma") for c in tail), name
        w = [i for i, c in enumerate(tail) if c.startswith("ds_write_b128")]
        r = [i for i, c in enumerate(tail) if c.startswith("ds_read_b128")]
        assert w and r and min(w) < min(r), f"{name}: LDS writes and reads of the reduce"
        assert len(r) % 4 == 0                                            # four groups' images per quad
        assert "s_barrier" in tail[:min(w)] and "s_barrier" in tail[max(i for i in w if i < min(r)):min(r)], f"{name}: barriers around the reduce"
        slab = name.endswith("ELi1EEEvNS_8GemmArgsE")
        stores = [c for c in tail if c.startswith(("buffer_store", "global_store"))]
        if slab:
            assert stores and all(c.startswith("global_store_dwordx4") for c in stores), name
        else:
            assert any(c.startswith("buffer_store_dwordx2") and c.endswith(" nt") for c in stores), f"{name}: no non-temporal store"
            assert any(c.startswith("buffer_store_dwordx2") and not c.endswith(" nt") for c in stores), name
