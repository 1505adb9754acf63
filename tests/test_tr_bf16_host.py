"""CPU tests of the bfloat16 calls on the two transposed-read layouts (bgemm_mi355x_nn / _ta / _ta_c32 and their launch_ / _runs
forms; kernels: CfgNNB / CfgTAB in hgemm_kernel_nn.hpp / hgemm_kernel_ta.hpp, instantiated in hgemm_inst_g8.hip, g9 and g10): the
names, the tables the calls must leave alone, that every call resolves exactly as its fp16 twin over the grid of
tests/golden/tr_resolve_golden.json (the element kind selects a kernel set and nothing else), bad arguments, and an ISA audit of the
three new units by the method of test_ta_host.py's audit of unit g6."""
import concurrent.futures as cf
import ctypes
import json
import re
import subprocess
from pathlib import Path

import pytest

from test_nn_host import MEMBERS as NN_MEMBERS
from test_ta_host import CSRC, EXEC_WRITERS, HIPCC, MEMBERS as TA_MEMBERS, NBUF, PKG, REPO, ta_info
from test_ta_host import lib  # noqa: F401  (fixture: the built library)
from test_ta_host import test_the_geometry_table_and_the_nn_table_are_unchanged_by_the_family as tables_unchanged
from test_tr_resolve_golden import GOLDEN

EPI_C16, EPI_SLAB, EPI_C32 = 0, 1, 4
PUBLIC = ("bgemm_mi355x_nn", "bgemm_mi355x_ta", "bgemm_mi355x_ta_c32", "bgemm_mi355x_launch_nn", "bgemm_mi355x_launch_ta",
          "bgemm_mi355x_launch_ta_c32", "bgemm_mi355x_nn_runs", "bgemm_mi355x_ta_runs", "bgemm_mi355x_ta_c32_runs")
HOOKS = ("bgemm_mi355x_selfcheck_launch_nn", "bgemm_mi355x_selfcheck_launch_ta", "bgemm_mi355x_selfcheck_launch_ta_c32")


def test_the_header_declares_the_names_and_the_library_exports_them(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None                                   # (ctypes raises AttributeError for a missing symbol)
    for nm in HOOKS:
        assert getattr(lib, nm) is not None and nm not in header
    block = header[header.index("bfloat16 on the NN and TA layouts"):header.index("hgemm_mi355x_strerror")]
    # plan, workspace and reserve are the fp16 layouts' own: said, not copied
    for nm in ("hgemm_mi355x_nn_plan", "_nn_plan_workspace_bytes", "_nn_reserve_workspace"):
        assert nm in block
    for nm in ("nn_plan", "ta_plan", "ta_reserve_workspace", "nn_reserve_workspace", "ta_plan_workspace_bytes", "ta_config_name"):
        assert not hasattr(lib, "bgemm_mi355x_" + nm)
    assert "nearest even" in block and "b_col_major" in block and "NO bf16 form" in block and "eplace" in block


def test_the_tables_and_their_name_hashes_are_unchanged(lib):
    assert lib.hgemm_mi355x_ta_num_configs() == 4 and [lib.hgemm_mi355x_ta_config_name(i).decode() for i in range(4)] == list(TA_MEMBERS)
    assert lib.hgemm_mi355x_nn_num_configs() == 4 and [lib.hgemm_mi355x_nn_config_name(i).decode() for i in range(4)] == list(NN_MEMBERS)
    tables_unchanged(lib)                                                       # the geometry table's count and name hash
    build_py = (PKG / "build.py").read_text()
    for unit in ("g5", "g6", "g7", "g8", "g9", "g10"):
        assert f"hgemm_inst_{unit}.hip" in build_py


def answer(fn, *args):
    out = (ctypes.c_longlong * 20)()
    st = fn(*args, out)
    return [st] + list(out[:4 + 8 * max(0, out[1])]) if st == 0 else [st]


def test_every_call_resolves_as_its_fp16_twin_over_the_recorded_grid(lib):
    """Status, form, grids, cuts, workspace: the rows of the golden file (scope, reach and stride edges included), then the fp32-C
    twins over the TA rows in both modes, and the ldc % 4 versus % 8 edge."""
    golden = json.loads(GOLDEN.read_text())
    seen = set()
    for fam in ("nn", "ta"):
        h, b = getattr(lib, f"hgemm_mi355x_selfcheck_launch_{fam}"), getattr(lib, f"bgemm_mi355x_selfcheck_launch_{fam}")
        for row in golden[fam]["resolve"]:
            got = answer(b, *row[:10])
            assert got == answer(h, *row[:10]), (fam, row[:10])
            assert got[0] == row[10] and (got[0] != 0 or got == row[10:]), (fam, row[:10])   # and the recording's
            seen.add((got[0], got[1] if len(got) > 1 else None))
        for row in golden[fam]["runs"]:
            assert getattr(lib, f"bgemm_mi355x_{fam}_runs")(*row[:7]) == row[7], (fam, row)
    assert {(0, 0), (0, 3), (0, 6)} <= seen and any(st != 0 for st, _ in seen)   # reference, split, plain and refused calls all occur
    hc, bc = lib.hgemm_mi355x_selfcheck_launch_ta_c32, lib.bgemm_mi355x_selfcheck_launch_ta_c32
    forms = set()
    for row in golden["ta"]["resolve"]:
        for acc in (0, 1):
            args = row[:9] + [acc, row[9]]
            got = answer(bc, *args)
            assert got == answer(hc, *args), args
            forms.add((got[0], got[1] if len(got) > 1 else None))
    assert {(0, 0), (0, 3), (0, 6)} <= forms
    for row in golden["ta"]["runs"]:
        assert lib.bgemm_mi355x_ta_c32_runs(*row[:7]) == lib.hgemm_mi355x_ta_c32_runs(*row[:7]), row
    m, n, k = 200, 136, 128
    for cid in range(4):
        for ldc in (n + 4, n + 12):          # rows of an fp32 C start every 16 bytes: the kernel; of a bf16 C they do not: the reference
            assert lib.bgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, ldc) == 1 and lib.bgemm_mi355x_ta_runs(cid, m, n, k, m, n, ldc) == 0
            assert answer(bc, cid, 3, 4, m, n, k, m, n, ldc, 1, 0)[:2] == [0, 3] and answer(lib.bgemm_mi355x_selfcheck_launch_ta, cid, 3, 4, m, n, k, m, n, ldc, 0)[:2] == [0, 0]
            assert lib.bgemm_mi355x_nn_runs(cid, m, n, k, k, n, ldc) == 0 and lib.bgemm_mi355x_nn_runs(cid, m, n, k, k, n, n + 8) == 1
    # C's reach: 2-byte elements for the bf16 C (twice the fp32 C's stride)
    assert lib.bgemm_mi355x_ta_c32_runs(0, 72, 64, 64, 72, 64, 8388604) == 1 and lib.bgemm_mi355x_ta_c32_runs(0, 72, 64, 64, 72, 64, 8388608) == 0
    assert lib.bgemm_mi355x_ta_runs(0, 72, 64, 64, 72, 64, 8388608) == 1 and lib.bgemm_mi355x_ta_runs(0, 72, 64, 64, 72, 64, 16777216) == 0


def test_bad_arguments_are_refused(lib):
    m, n, k = 200, 136, 128
    null = ctypes.c_void_p(0)
    out = (ctypes.c_longlong * 20)()
    for acc in (2, -1, 256):
        assert lib.bgemm_mi355x_selfcheck_launch_ta_c32(0, 1, 4, m, n, k, m, n, n, acc, 0, out) == -1
        # (a refused accumulate returns before any HIP call: the pointers are never looked at)
        assert lib.bgemm_mi355x_launch_ta_c32(0, 1, null, null, null, m, n, k, m, n, n, acc, null) == -1
        assert lib.bgemm_mi355x_ta_c32(null, null, null, m, n, k, acc, null) == -1
    for ld in ((m - 8, n, n), (m, n - 8, n), (m, n, n - 4), (0, n, n), (m, n, -n)):
        for aligned in (4, 0):
            assert lib.bgemm_mi355x_selfcheck_launch_ta(0, 1, aligned, m, n, k, *ld, 0, out) == -1, ld
            assert lib.bgemm_mi355x_selfcheck_launch_ta_c32(0, 1, aligned, m, n, k, *ld, 1, 0, out) == -1, ld
        assert lib.bgemm_mi355x_ta_runs(0, m, n, k, *ld) == 0 and lib.bgemm_mi355x_ta_c32_runs(0, m, n, k, *ld) == 0
    for ld in ((k - 8, n, n), (k, n - 8, n), (k, n, n - 8), (k, 0, n)):
        assert lib.bgemm_mi355x_selfcheck_launch_nn(0, 1, 4, m, n, k, *ld, 0, out) == -1, ld
        assert lib.bgemm_mi355x_nn_runs(0, m, n, k, *ld) == 0
    for cid in (-1, 4):
        assert lib.bgemm_mi355x_selfcheck_launch_nn(cid, 1, 4, m, n, k, k, n, n, 0, out) == -1
        assert lib.bgemm_mi355x_selfcheck_launch_ta(cid, 1, 4, m, n, k, m, n, n, 0, out) == -1
        assert lib.bgemm_mi355x_selfcheck_launch_ta_c32(cid, 1, 4, m, n, k, m, n, n, 0, 0, out) == -1
        assert lib.bgemm_mi355x_nn_runs(cid, m, n, k, k, n, n) == 0 and lib.bgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, n) == 0
    # null pointers and empty shapes return before any HIP call
    assert lib.bgemm_mi355x_launch_nn(0, 1, null, null, null, m, n, k, k, n, n, null) == -1
    assert lib.bgemm_mi355x_launch_ta(0, 1, null, null, null, m, n, k, m, n, n, null) == -1
    assert lib.bgemm_mi355x_nn(null, null, null, m, n, k, null) == -1 and lib.bgemm_mi355x_ta(null, null, null, m, n, k, null) == -1
    for acc in (0, 1):
        assert lib.bgemm_mi355x_launch_ta_c32(0, 1, null, null, null, m, n, k, m, n, n, acc, null) == -1
        assert lib.bgemm_mi355x_ta_c32(null, null, null, m, n, k, acc, null) == -1 and lib.bgemm_mi355x_ta_c32(null, null, null, 0, n, k, acc, null) == -1
    assert lib.bgemm_mi355x_selfcheck_launch_nn(0, 1, 4, 0, n, k, k, n, n, 0, out) == -1


# ---- ISA audit of units g8 (family n), g9 (family a) and g10 (family a, fp32 C) ---------------------------------------------------
UNITS = {"g8": ("nn", "CfgNNB", (EPI_C16, EPI_SLAB)), "g9": ("ta", "CfgTAB", (EPI_C16, EPI_SLAB)), "g10": ("ta", "CfgTAB", (EPI_C32,))}


def compile_unit(unit, out):
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S",
                           "--cuda-device-only", str(CSRC / f"hgemm_inst_{unit}.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_tr_bf16")
    with cf.ThreadPoolExecutor(max_workers=3) as ex:
        done = dict(zip(UNITS, ex.map(lambda u: compile_unit(u, tmp / f"{u}.s"), UNITS)))
    units = {}
    for unit, (fam, cfg, epis) in UNITS.items():
        assert done[unit].returncode == 0, done[unit].stderr[-2000:]
        kernel = rf"_ZN12hgemm_mi355x15hgemm_{fam}_kernel\w+"
        text = (tmp / f"{unit}.s").read_text()
        funcs = {m.group(1): [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c]
                 for m in re.finditer(rf"^({kernel}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
        meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({kernel})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
        units[unit] = (text, funcs, meta)
    return units


def test_each_unit_holds_its_bf16_kernels_and_nothing_else(lib, isa):
    for unit, (fam, cfg, epis) in UNITS.items():
        text, funcs, meta = isa[unit]
        assert set(funcs) == set(meta) and len(funcs) == 4 * len(epis), unit
        assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), f"{unit}: a kernel of another family or element type"
        info = ta_info if fam == "ta" else (lambda L, cid: (lambda o: (L.hgemm_mi355x_nn_config_info(cid, o), list(o))[1])((ctypes.c_int * 8)()))
        for cid, nm in enumerate(TA_MEMBERS):
            bm, bn = re.match(r"a(\d+)x(\d+)_", nm).groups()
            for epi in epis:
                mine = [f for f in funcs if f"{len(cfg)}{cfg}ILi{bm}ELi{bn}ELi2ELi2ELi{NBUF[cid]}EEELi{epi}E" in f]
                assert len(mine) == 1, (unit, nm, epi)
                md = meta[mine[0]]
                assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", md), f"{mine[0]}: private segment"
                assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", md).group(1)) == info(lib, cid)[7], f"{mine[0]}: LDS bytes"


def test_k_loops_run_the_bf16_mfma_and_only_the_16_bit_epilogue_converts(isa):
    """Per K stage: the family's transposed reads (a: 4 (FM + FN), none of A's through ds_read_b128; n: 4 FN and 2 FM ds_read_b128),
    2 FM FN v_mfma_f32_16x16x32_bf16 and no other MFMA; v_cvt_pk_bf16_f32 behind the loop of the EPI_C16 kernels only, 2 FM FN of them
    (each accumulator converted once); no conversion to fp16 and no scratch anywhere; no EXEC writer between entry and the last
    transposed read."""
    for unit, (fam, cfg, epis) in UNITS.items():
        _, funcs, _ = isa[unit]
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
            fm, fn = (int(x) // 32 for x in re.search(rf"{cfg}ILi(\d+)ELi(\d+)E", name).groups())
            epi = int(re.search(r"EEELi(\d)E", name).group(1))
            mfma = [i for i, c in enumerate(body) if c.startswith("v_mfma")]
            assert len(mfma) == 2 * fm * fn and all(body[i].startswith("v_mfma_f32_16x16x32_bf16") for i in mfma), name
            assert not [c for c in codes if c.startswith("v_mfma") and not c.startswith("v_mfma_f32_16x16x32_bf16")], f"{name}: another MFMA"
            tr = sum(1 for c in body if c.startswith("ds_read_b64_tr_b16"))
            b128 = sum(1 for c in body if c.startswith("ds_read_b128"))
            if fam == "ta":
                assert tr == 4 * (fm + fn) and b128 == 0, (name, tr, b128)
            else:
                assert tr == 4 * fn and b128 == 2 * fm, (name, tr, b128)
            assert not any(c.startswith(("v_mfma", "ds_read_b64_tr_b16")) for c in codes[:lo] + tail), name
            last_tr = max(i for i, c in enumerate(codes) if c.startswith("ds_read_b64_tr_b16"))
            assert not [c for c in codes[:last_tr + 1] if EXEC_WRITERS.search(c)], f"{name}: EXEC is written in front of a transposed read"
            cvt = [c for c in codes if c.startswith("v_cvt_pk_bf16_f32")]
            assert len(cvt) == (2 * fm * fn if epi == EPI_C16 else 0), (name, len(cvt))
            assert not any(c.startswith("v_cvt_pk_bf16_f32") for c in codes[:hi + 1]), f"{name}: a convert in front of the epilogue"
            assert not [c for c in codes if re.match(r"v_cvt_(pk_?)?(rtz_)?f16_|v_cvt_pkrtz_f16|v_cvt_\w*_bf8|v_cvt_\w*_fp8", c)], f"{name}: a conversion to fp16"
            assert not [c for c in codes if c.startswith("scratch_")], f"{name}: scratch"
            stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
            if epi != EPI_SLAB:       # plain and non-temporal 16-byte stores, an instruction of its own each
                per = fm * fn // 2 if epi == EPI_C16 else fm * fn
                assert all(c.startswith("buffer_store_dwordx4") for c in stores), name
                assert sum(1 for c in stores if c.endswith(" nt")) == per == sum(1 for c in stores if not c.endswith(" nt")), (name, len(stores))
