"""CPU tests of family a's fp32-C calls (hgemm_mi355x_ta_c32 / _launch_ta_c32: c32 = A x B or c32 += A x B, EPI_C32 in
hgemm_kernel_ta.hpp, instantiated in hgemm_inst_g7.hip): the names, the tables the calls must leave alone, how a call resolves
(hgemm_mi355x_selfcheck_launch_ta_c32: nothing is launched), the rules in which an fp32 C differs from an fp16 C (ldc % 4, C's reach in
4-byte elements), and an ISA audit of unit g7 alone by the method of test_ta_host.py's audit of unit g6."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from test_ta_host import (COUNTER_BYTES, CSRC, EPI_SLAB, EXEC_WRITERS, FORM, FUSED, HIPCC, MEMBERS, NBUF, NT_STORE, PKG, REPO, STREAMK,
                          THUNK_ENTRY, THUNK_GENERIC, THUNK_SPLITK_REDUCE, ta_info)
from test_ta_host import lib  # noqa: F401  (fixture: the built library)
from test_ta_host import test_the_geometry_table_and_the_nn_table_are_unchanged_by_the_family as tables_unchanged

EPI_C32 = 4                                                     # hgemm_kernel.hpp
GIB = 1 << 30
NEW_NAMES = ("hgemm_mi355x_ta_c32", "hgemm_mi355x_launch_ta_c32", "hgemm_mi355x_ta_c32_runs")


def resolve(lib, cid, splits, m, n, k, ld=None, aligned=True, ruled_out=0, accumulate=0):
    """What hgemm_mi355x_launch_ta_c32 decides, nothing launched: (status, form, slab bytes, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    lda, ldb, ldc = ld or (m, n, n)
    st = lib.hgemm_mi355x_selfcheck_launch_ta_c32(cid, splits, 4 if aligned else 0, m, n, k, lda, ldb, ldc, accumulate, ruled_out, out)
    return st, FORM[out[0]], out[2], [tuple(out[4 + 8 * i:4 + 8 * i + 5]) for i in range(out[1])]


def test_the_header_declares_the_names_and_the_library_exports_them(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in NEW_NAMES:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None
    assert lib.hgemm_mi355x_selfcheck_launch_ta_c32 is not None and "selfcheck_launch_ta_c32" not in header
    block = header[header.index("fp32 C, stored or accumulated"):header.index("hgemm_mi355x_strerror")]
    # the plan, the workspace size and the reserve call are the TA layout's own: said, not copied
    for nm in ("hgemm_mi355x_ta_plan", "hgemm_mi355x_ta_plan_workspace_bytes", "hgemm_mi355x_ta_reserve_workspace"):
        assert nm in block
    for nm in ("ta_c32_plan", "ta_c32_plan_workspace_bytes", "ta_c32_reserve_workspace"):
        assert nm not in header and not hasattr(lib, "hgemm_mi355x_" + nm)
    assert "never read" in block and "ldc % 4" in block and "x 4 bytes" in block


def test_the_tables_are_unchanged(lib):
    assert lib.hgemm_mi355x_ta_num_configs() == 4 == len(MEMBERS)
    assert [lib.hgemm_mi355x_ta_config_name(i).decode() for i in range(4)] == list(MEMBERS)
    tables_unchanged(lib)
    build_py = (PKG / "build.py").read_text()
    assert "hgemm_inst_g7.hip" in build_py and "hgemm_inst_g6.hip" in build_py
    kernel_hpp = (CSRC / "hgemm_kernel.hpp").read_text()
    ids = {nm: int(v) for nm, v in re.findall(r"constexpr int (EPI_\w+)\s*=\s*(\d+);", kernel_hpp)}
    assert ids["EPI_C32"] == EPI_C32 and sum(1 for v in ids.values() if v == EPI_C32) == 1, ids


def test_forms_of_every_plan_word(lib):
    """test_ta_host.py's cut arithmetic: the plain dispatch carries the c32 epilogue, a split plan is the family's slab kernels and the
    c32 combine, the slabs are those of the fp16-C call."""
    m, n, k = 328, 456, 512
    for cid in range(len(MEMBERS)):
        bm, bn = ta_info(lib, cid)[:2]
        tiles = -(-m // bm) * -(-n // bn)
        for acc in (0, 1):
            for word in (1, 1 | NT_STORE, STREAMK, STREAMK | 37, 1 | FUSED, 0):
                assert resolve(lib, cid, word, m, n, k, accumulate=acc) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C32, 1, k)]), (cid, hex(word))
            for s in (2, 5, 16):
                chunk = -(-(k // 64) // s) * 64
                real = -(-k // chunk)
                for word in (s, s | FUSED, s | NT_STORE):
                    st, form, slab, disp = resolve(lib, cid, word, m, n, k, accumulate=acc)
                    assert (st, form, slab) == (0, "splitk", real * m * n * 4), (cid, hex(word))
                    assert disp == [(THUNK_ENTRY, tiles * real, EPI_SLAB, real, chunk), (THUNK_SPLITK_REDUCE, 0, EPI_C32, real, chunk)]
                    assert lib.hgemm_mi355x_ta_plan_workspace_bytes(cid, word, m, n, k) == COUNTER_BYTES + slab
                # the two-pass form ruled out (no workspace): unsplit, status 0
                assert resolve(lib, cid, s, m, n, k, ruled_out=1 << 3, accumulate=acc) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C32, 1, k)])
            assert resolve(lib, cid, 16, m, n, 64, accumulate=acc) == (0, "plain", 0, [(THUNK_ENTRY, tiles, EPI_C32, 1, 64)])
        assert lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m + 24, n + 24, n + 40) == 1


def test_the_first_dispatch_carries_the_start_event_and_the_last_the_stop_event(lib):
    out = (ctypes.c_longlong * 20)()
    for word, want in ((1, [(1, 1)]), (4, [(1, 0), (0, 1)])):
        assert lib.hgemm_mi355x_selfcheck_launch_ta_c32(0, word, 4, 200, 136, 256, 200, 136, 136, 1, 0, out) == 0
        assert [tuple(out[4 + 8 * i + 6:4 + 8 * i + 8]) for i in range(out[1])] == want
    assert lib.hgemm_mi355x_selfcheck_launch_ta_c32(0, 1, 4, 200, 136, 72, 200, 136, 136, 1, 0, out) == 0
    assert (out[0], out[1], tuple(out[10:12])) == (0, 1, (1, 1))


def test_what_the_kernel_does_not_take_falls_back_to_the_reference_kernel(lib):
    m, n, k = 200, 136, 128
    cases = {"K = 72": dict(m=m, n=n, k=72), "M = 100": dict(m=100, n=n, k=k), "N = 100": dict(m=m, n=100, k=k),
             "ldc = N + 2": dict(m=m, n=n, k=k, ld=(m, n, n + 2)), "lda = M + 4": dict(m=m, n=n, k=k, ld=(m + 4, n, n)),
             "misaligned C": dict(m=m, n=n, k=k, aligned=False)}
    for cid in range(len(MEMBERS)):
        for what, kw in cases.items():
            for splits in (1, 4):
                for acc in (0, 1):
                    st, form, slab, disp = resolve(lib, cid, splits, accumulate=acc, **kw)
                    assert (st, form, slab) == (0, "reference", 0) and [d[:3] for d in disp] == [(THUNK_GENERIC, 0, EPI_C32)], (cid, what)
            if "aligned" not in kw:
                ld = kw.get("ld") or (kw["m"], kw["n"], kw["n"])
                assert lib.hgemm_mi355x_ta_c32_runs(cid, kw["m"], kw["n"], kw["k"], *ld) == 0, (cid, what)
        assert lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, n) == 1


def test_rows_of_an_fp32_c_start_every_16_bytes(lib):
    """ldc % 4 == 0 with ldc % 8 != 0: the kernel for an fp32 C, the reference kernel for an fp16 C with the same numbers."""
    m, n, k = 200, 136, 128
    for cid in range(len(MEMBERS)):
        for ldc in (n + 4, n + 12, n + 36):
            assert ldc % 8 == 4
            assert lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, ldc) == 1 and lib.hgemm_mi355x_ta_runs(cid, m, n, k, m, n, ldc) == 0
            assert resolve(lib, cid, 1, m, n, k, ld=(m, n, ldc))[:2] == (0, "plain")
            assert resolve(lib, cid, 3, m, n, k, ld=(m, n, ldc))[:2] == (0, "splitk")
        for ldc in (n + 1, n + 2, n + 6):
            assert lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, ldc) == 0
        # the operands keep their rule
        assert lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m + 4, n, n) == 0 and lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n + 4, n) == 0


def test_the_reach_of_an_fp32_c_at_its_boundary(lib):
    """(BM ldc + N) 4 bytes below 2 GiB.  a64x64, N = 64: ldc = 8388604 is the last stride that runs, 8388608 = 2^23 the first that does
    not ((2^29 + 64) 4 bytes); their neighbours in steps of 4 agree, and every member's edge is the rule's."""
    assert (64 * 8388604 + 64) * 4 < 2 * GIB <= (64 * 8388608 + 64) * 4
    for ldc, runs in ((8388600, 1), (8388604, 1), (8388608, 0), (8388612, 0)):
        assert lib.hgemm_mi355x_ta_c32_runs(0, 72, 64, 64, 72, 64, ldc) == runs, ldc
        for word in (1, 2):
            assert resolve(lib, 0, word, 72, 64, 128, ld=(72, 64, ldc))[:2] == (0, ("plain" if word == 1 else "splitk") if runs else "reference")
    # the fp16 C of the same strides reaches twice as far
    assert lib.hgemm_mi355x_ta_runs(0, 72, 64, 64, 72, 64, 8388608) == 1
    for cid in range(len(MEMBERS)):
        bm, bn = ta_info(lib, cid)[:2]
        for m, n, k in ((bm + 8, bn + 8, 128), (2 * bm + 8, 3 * bn + 8, 1024)):
            edge = (2 * GIB // 4 - n - 1) // bm // 4 * 4
            assert (bm * edge + n) * 4 < 2 * GIB <= (bm * (edge + 4) + n) * 4
            for ldc in (edge - 4, edge, edge + 4, edge + 8):
                assert lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, ldc) == (1 if ldc <= edge else 0), (MEMBERS[cid], (m, n, k), ldc)
        top = (1 << 31) - 4
        assert lib.hgemm_mi355x_ta_c32_runs(cid, 64, bn, 128, 64, bn, top) == 0 and resolve(lib, cid, 2, 64, bn, 128, ld=(64, bn, top))[:2] == (0, "reference")
        assert lib.hgemm_mi355x_ta_c32_runs(cid, bm + 8, bn, 128, bm + 8, bn, (1 << 30) // bm) == 0     # BM x ldc x 4 = 2^32: no 32-bit wrap


def test_bad_arguments_are_refused(lib):
    m, n, k = 200, 136, 128
    null = ctypes.c_void_p(0)
    out = (ctypes.c_longlong * 20)()
    for acc in (2, -1, 256):
        assert lib.hgemm_mi355x_selfcheck_launch_ta_c32(0, 1, 4, m, n, k, m, n, n, acc, 0, out) == -1
        # (a refused accumulate returns before any HIP call: the pointers are never looked at)
        assert lib.hgemm_mi355x_launch_ta_c32(0, 1, null, null, null, m, n, k, m, n, n, acc, null) == -1
        assert lib.hgemm_mi355x_ta_c32(null, null, null, m, n, k, acc, null) == -1
    for ld in ((m - 8, n, n), (m, n - 8, n), (m, n, n - 4), (0, n, n), (m, n, -n), (k, n, n)):
        for aligned in (True, False):
            assert resolve(lib, 0, 1, m, n, k, ld=ld, aligned=aligned)[0] == -1, ld
        assert lib.hgemm_mi355x_ta_c32_runs(0, m, n, k, *ld) == 0
    for cid in (-1, len(MEMBERS)):
        assert resolve(lib, cid, 1, m, n, k)[0] == -1 and lib.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, n) == 0
    for acc in (0, 1):
        assert lib.hgemm_mi355x_launch_ta_c32(0, 1, null, null, null, m, n, k, m, n, n, acc, null) == -1
        assert lib.hgemm_mi355x_ta_c32(null, null, null, m, n, k, acc, null) == -1 and lib.hgemm_mi355x_ta_c32(null, null, null, 0, n, k, acc, null) == -1


# ---- ISA audit of unit g7 alone ---------------------------------------------------------------------------------------------------
KERNEL = r"_ZN12hgemm_mi355x15hgemm_ta_kernel\w+"


@pytest.fixture(scope="module")
def c32_isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    out = tmp_path_factory.mktemp("audit_ta_c32") / "g7.s"
    pr = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S",
                         "--cuda-device-only", str(CSRC / "hgemm_inst_g7.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    text = out.read_text()
    funcs = {m.group(1): [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c]
             for m in re.finditer(rf"^({KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    return text, funcs, meta


def test_the_unit_holds_one_c32_kernel_per_member_and_nothing_else(lib, c32_isa):
    text, funcs, meta = c32_isa
    assert set(funcs) == set(meta) and len(funcs) == len(MEMBERS)
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta)
    for cid, nm in enumerate(MEMBERS):
        bm, bn = re.match(r"a(\d+)x(\d+)_", nm).groups()
        mine = [f for f in funcs if f"CfgTAILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}EEELi{EPI_C32}E" in f]
        assert len(mine) == 1, nm
        md = meta[mine[0]]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", md), f"{nm}: private segment"
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", md).group(1)) == ta_info(lib, cid)[7], f"{nm}: LDS bytes"


def test_the_k_loop_is_the_familys_and_the_epilogue_stores_fp32(c32_isa):
    """Per K stage 4 (FM + FN) ds_read_b64_tr_b16 and 2 FM FN v_mfma_f32_16x16x32_f16, no ds_read_b128 between the MFMAs, no EXEC writer
    in front of the last transposed read.  Behind the K loop: FM FN buffer_store_dwordx4 of each hint form (plain and nt: an
    instruction of its own each), the old value through buffer_load_dwordx4 that are not LDS-DMA, and no fp16 conversion anywhere."""
    _, funcs, _ = c32_isa
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
        fm, fn = (int(x) // 32 for x in re.search(r"CfgTAILi(\d+)ELi(\d+)E", name).groups())
        mfma = [i for i, c in enumerate(body) if c.startswith("v_mfma")]
        assert len(mfma) == 2 * fm * fn and all(body[i].startswith("v_mfma_f32_16x16x32_f16") for i in mfma), name
        assert sum(1 for c in body if c.startswith("ds_read_b64_tr_b16")) == 4 * (fm + fn), name
        assert not [c for c in body[mfma[0]:mfma[-1] + 1] if c.startswith("ds_read_b128")], f"{name}: ds_read_b128 in the K loop"
        assert not any(c.startswith(("v_mfma", "ds_read_b64_tr_b16")) for c in codes[:lo] + tail), name
        last_tr = max(i for i, c in enumerate(codes) if c.startswith("ds_read_b64_tr_b16"))
        assert not [c for c in codes[:last_tr + 1] if EXEC_WRITERS.search(c)], f"{name}: EXEC is written in front of a transposed read"
        assert not any(c.startswith(("buffer_store", "global_store", "global_load", "flat_load")) for c in codes[:hi + 1]), name
        stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
        assert all(c.startswith("buffer_store_dwordx4") for c in stores), name
        assert sum(1 for c in stores if c.endswith(" nt")) == fm * fn == sum(1 for c in stores if not c.endswith(" nt")), (name, len(stores))
        old = [c for c in tail if c.startswith("buffer_load_dwordx4") and not c.endswith(" lds")]
        assert len(old) == fm * fn, f"{name}: {len(old)} loads of the old value"
        assert not any(c.startswith("buffer_load") and not c.endswith(" lds") for c in codes[:hi + 1]), f"{name}: C is read in front of the epilogue"
        assert not [c for c in codes if re.match(r"v_cvt_\w*f16_f32", c)], f"{name}: an fp16 conversion"
