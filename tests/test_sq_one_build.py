"""ISA audit of the one-tile-per-workgroup kernel of q256x256_w2x2 (hgemm_kernel_sq_one.hpp, unit hgemm_inst_g13.hip) -- runs on CPU
(hipcc cross-compiles gfx950).  The kernel keeps its accumulators in named AGPRs and writes its MFMAs and LDS-DMA pieces as asm
statements, as family q does, so the same properties of the generated code are checked; and the units whose kernels are
fingerprinted (g0-g3) must not have gained a symbol of it."""
import re
import subprocess
from pathlib import Path

import pytest

from test_build_audit import CSRC, HIPCC, REPO, _outside_asm, m0_provenance_violations, valu_to_mfma_source_hazards

KERNEL = "hgemm_tn_sq_one_kernel"


def _device_isa(tmp_path_factory, unit: str) -> str:
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("sq_one") / f"{unit}.s"
    res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S", "--cuda-device-only",
                          str(CSRC / f"{unit}.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


@pytest.fixture(scope="module")
def one_kernel(tmp_path_factory):
    text = _device_isa(tmp_path_factory, "hgemm_inst_g13")
    funcs = {m.group(1): m.group(2).splitlines()
             for m in re.finditer(r"^(_ZN12hgemm_mi355x\d+" + KERNEL + r"\w+):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    meta = {m.group(1): m.group(2)
            for m in re.finditer(r"\.amdhsa_kernel (_ZN12hgemm_mi355x\d+" + KERNEL + r"\w+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    assert len(funcs) == 1 and set(funcs) == set(meta), sorted(funcs)
    name = next(iter(funcs))
    assert "CfgSQILi256ELi256ELi2ELi2ELi1ELi16E" in name
    notes = re.search(r"\.name:\s+" + re.escape(name) + r"\n(.*?)\.wavefront_size", text, re.S)
    assert notes, "no metadata note of the kernel"
    return name, funcs[name], meta[name], notes.group(1), text


def test_the_unit_holds_the_one_kernel_and_nothing_else(one_kernel):
    *_, text = one_kernel
    assert len(re.findall(r"\.amdhsa_kernel ", text)) == 1


def test_no_private_segment_and_no_spills(one_kernel):
    _, lines, meta, notes, _ = one_kernel
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", notes)
    assert re.search(r"\.sgpr_spill_count:\s+0\b", notes) and re.search(r"\.vgpr_spill_count:\s+0\b", notes)
    assert not [ln for ln in lines if "scratch_" in ln]


def test_all_256_agprs_are_reserved_below_at_most_224_vgprs(one_kernel):
    _, _, meta, _, _ = one_kernel
    nxt = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    accum = int(re.search(r"\.amdhsa_accum_offset (\d+)", meta).group(1))
    print(f"accum_offset {accum} next_free_vgpr {nxt}")
    assert nxt - accum == 256
    assert accum <= 224


def test_the_compiler_touches_no_agpr(one_kernel):
    _, lines, *_ = one_kernel
    bad = [ln for ln in _outside_asm(lines) if re.search(r"\bv_accvgpr_|\bv_mfma_|\ba\[?\d+", ln.split(";")[0])]
    assert not bad, bad[:3]


def test_no_valu_write_within_two_wait_states_of_an_mfma_that_reads_it(one_kernel):
    _, lines, *_ = one_kernel
    n_mfma = sum(1 for ln in lines if ln.split(";")[0].strip().startswith("v_mfma"))
    # head step, two steps of the hot loop, three peeled steps: 128 MFMAs each
    assert n_mfma == 6 * 128, n_mfma
    bad = valu_to_mfma_source_hazards(lines)
    assert not bad, bad[:2]


def test_every_asm_lds_dma_sees_an_asm_m0_write_on_every_path(one_kernel):
    _, lines, *_ = one_kernel
    loads = [ln for ln in lines if ln.split(";")[0].strip().startswith("buffer_load") and ln.split(";")[0].strip().endswith(" lds")]
    # prologue: two tiles + the early A pieces (compiler form); per full step 16 pieces, the first peeled step lacks the early A pieces
    assert len(loads) > 3 * 16
    bad = m0_provenance_violations(lines)
    assert not bad, bad[:2]


def test_the_peeled_tail_issues_no_piece_behind_the_last_real_one(one_kernel):
    """Behind the hot loop: one step with every piece but the early A pieces of interval B, then two steps without any LDS-DMA; the
    last sync point's wait is vmcnt(0), and the kernel does not wait for its stores."""
    _, lines, *_ = one_kernel
    text = "\n".join(lines)
    tail = re.split(r"s_cbranch_scc\d", text.split("This Inner Loop Header")[-1], 1)[1]
    codes = [ln.split(";")[0].strip() for ln in tail.splitlines()]
    mfma = [i for i, c in enumerate(codes) if c.startswith("v_mfma")]
    dma = [i for i, c in enumerate(codes) if c.startswith("buffer_load") and c.endswith(" lds")]
    assert len(mfma) == 3 * 128
    assert dma and max(dma) < mfma[128], "an LDS-DMA piece behind the first peeled step"
    assert not [c for c in codes[mfma[-1]:] if c.startswith("s_waitcnt vmcnt(0)")], "the kernel waits for its stores"


def test_the_kernel_keeps_the_instruction_stream_that_was_measured(one_kernel):
    """profiles/sq_one_isa_fingerprint.json is unit g13 as the commit that added the kernel compiled it: the kernel of
    profiles/sq_one_bench_*.jsonl and profiles/sq_one_check_q256x256.log.  Its K-steps are instantiations of sq_interval, shared
    with every kernel of family q (hgemm_kernel_sq.hpp): a change there shows here as well as in test_build_audit's 348 kernels."""
    import json
    import sys

    sys.path.insert(0, str(REPO / "cuda-l2_amd" / "tools"))
    import isa_fingerprint

    name, *_, text = one_kernel
    recorded = json.loads((REPO / "profiles" / "sq_one_isa_fingerprint.json").read_text())["kernels"]
    assert isa_fingerprint.fingerprints(text) == recorded and list(recorded) == [name]


@pytest.mark.parametrize("grp", [0, 1, 2, 3])
def test_the_fingerprinted_units_hold_no_symbol_of_the_kernel(tmp_path_factory, grp):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    # device side: preprocess-free and cheap -- the kernel's name must not appear among the unit's device symbols; the full device
    # compile of these units is test_build_audit's (the 348 names).  Host side: the unit only CALLS the out-of-line launcher.
    out = tmp_path_factory.mktemp("sq_one_host") / f"g{grp}.o"
    res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-c", "--cuda-host-only",
                          str(CSRC / f"hgemm_inst_g{grp}.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    syms = subprocess.run(["nm", "-C", str(out)], capture_output=True, text=True).stdout
    assert KERNEL not in syms, [ln for ln in syms.splitlines() if KERNEL in ln][:3]
    calls = [ln for ln in syms.splitlines() if "launch_sq_one" in ln]
    assert all(ln.split()[0] == "U" for ln in calls), calls
