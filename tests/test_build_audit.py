"""ISA audit of the software-pipelined kernel families ("s": hgemm_kernel_sp.hpp, "q": hgemm_kernel_sq.hpp) -- runs on CPU (hipcc cross-compiles gfx950).

The SP kernels keep their 256 accumulators in explicitly named AGPRs (a[0..255], inline asm only).
That is only sound while the compiler itself never touches AGPRs, never spills, and keeps the LDS-DMA
descriptors in SGPRs; those are properties of the generated code, so they are checked on the ISA.
"""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "cuda-l2_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _sp_groups() -> list[int]:
    groups = sorted({int(m.group(1)) for m in re.finditer(r"^\s*HGEMM_S[PQ]\((\d+),", (CSRC / "hgemm_configs.def").read_text(), re.M)})
    assert groups, "no HGEMM_SP / HGEMM_SQ entry in hgemm_configs.def"
    return groups


def _compile_groups(tmp_path_factory, opt: str) -> str:
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    procs = []
    for grp in _sp_groups():
        out = tmp_path_factory.mktemp("audit") / f"sp{grp}{opt}.s"
        src = CSRC / f"hgemm_inst_g{grp}.hip"
        procs.append((out, subprocess.Popen([HIPCC, "--offload-arch=gfx950", opt, "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S",
                                             "--cuda-device-only", str(src), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)))
    text = ""
    for out, pr in procs:
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, err.decode()[-2000:]
        text += out.read_text()
    return text


@pytest.fixture(scope="module")
def isa_text(tmp_path_factory):
    return _compile_groups(tmp_path_factory, "-O3")


@pytest.fixture(scope="module")
def sp_functions(isa_text):
    text = isa_text
    funcs = {}
    for m in re.finditer(r"^(_ZN12hgemm_mi355x18hgemm_tn_s[pq]_kernel\w+):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        funcs[m.group(1)] = m.group(2).splitlines()
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (_ZN12hgemm_mi355x18hgemm_tn_s[pq]_kernel\w+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        meta[m.group(1)] = m.group(2)
    assert funcs and set(funcs) == set(meta)
    return funcs, meta


def _outside_asm(lines):
    inside = False
    for ln in lines:
        if "#ASMSTART" in ln:
            inside = True
        elif "#ASMEND" in ln:
            inside = False
        elif not inside:
            yield ln


def test_sp_accumulators_are_only_touched_by_the_asm_statements(sp_functions):
    funcs, _ = sp_functions
    for name, lines in funcs.items():
        bad = [ln for ln in _outside_asm(lines) if re.search(r"\bv_accvgpr_|\bv_mfma_|\ba\[?\d+", ln.split(";")[0])]
        assert not bad, f"{name}: compiler-generated AGPR access: {bad[:3]}"


def test_sp_kernels_do_not_spill_and_leave_room_for_the_agprs(sp_functions):
    funcs, meta = sp_functions
    for name, lines in funcs.items():
        assert not [ln for ln in lines if "scratch_" in ln], f"{name} uses scratch"
        m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta[name])
        accum = re.search(r"\.amdhsa_accum_offset (\d+)", meta[name])
        assert m and accum
        agprs = int(m.group(1)) - int(accum.group(1))
        # two-resident members of family q (round 5, CfgSQ::WGS == 2: two stages <= 80 KiB): exactly their accumulators are
        # reserved, and the plain-epilogue kernels must leave room for a second wave on the SIMD (<= 256 registers, no LDS but the
        # stages); everything else owns the SIMD's file and reserves all 256 AGPRs
        sq = re.search(r"CfgSQILi(\d+)ELi(\d+)ELi\d+ELi\d+ELi(\d+)ELi(\d+)EEELi(\d+)EEEvNS", name)
        two_resident = bool(sq) and 2 * 2 * int(sq.group(3)) * (int(sq.group(1)) + int(sq.group(2))) * 128 <= 160 * 1024
        if two_resident:
            acc = int(sq.group(1)) * int(sq.group(2)) // 256
            assert acc <= agprs <= acc + 7, f"{name}: expected {acc} AGPRs (allocation granule 8), got {agprs}"
            lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta[name]).group(1))
            if (int(sq.group(5)) & 7) != 3:
                assert int(m.group(1)) <= 256 and 2 * lds <= 160 * 1024, f"{name}: {m.group(1)} registers, {lds} B of LDS: not two per CU"
        else:
            assert agprs == 256, f"{name}: expected 256 AGPRs"
        assert int(m.group(1)) <= 512
        # VGPR headroom below the reserved AGPRs, per epilogue class (the last template argument): the plain epilogues
        # (narrow 0 / wide 1) are what the compute-bound plans run and keep >= 32 registers of margin, the slab epilogue
        # (2) >= 16; only the single-launch split-K form (3: fragments + a combine row live together) may use the file
        # up to the last register -- a compiler bump that costs one more there fails the 256-AGPR check above instead of
        # silently spilling.  The table is printed (pytest -s / on failure) so a creeping allocation is visible early.
        # (family q's "ktail" variants carry EPI_KTAIL = 8 on top of the epilogue id: same classes, same bounds -- the tail's
        # fragments live in the registers of the two fragment sets that are dead at an item's end)
        epi = int(re.search(r"ELi(\d+)EEEvNS", name).group(1))
        bound = {0: 224, 1: 224, 2: 240, 3: 256}[epi & 7]
        print(f"accum_offset {accum.group(1):>3} (bound {bound})  {name}")
        assert int(accum.group(1)) <= bound, f"{name}: {accum.group(1)} VGPRs > {bound} (epilogue class {epi})"


def test_sp_k_loops_are_mfma_streams_with_scalar_dma_descriptors(sp_functions):
    funcs, _ = sp_functions
    for name, lines in funcs.items():
        # K loops = innermost loops that contain MFMAs; split the function at loop headers
        text = "\n".join(lines)
        loops = re.split(r"This Inner Loop Header", text)[1:]
        # (round 5: family q's prologue has one loop before the K loops -- the phase offset's sleep; it holds nothing but s_sleep and
        # scalar arithmetic, checked here, and is skipped)
        while loops and not re.search(r"\bv_mfma_", loops[0].split("s_cbranch_scc")[0]):
            pre = [ln.split(";")[0].strip() for ln in loops[0].split("s_cbranch_scc")[0].splitlines()]
            assert "sq_kernel" in name and any(c.startswith("s_sleep") for c in pre), name
            assert all(re.match(r"(s_\w+|\.LBB\S*:?|)(\s|$)", c) for c in pre[1:]), (name, [c for c in pre[1:] if not re.match(r"(s_\w+|\.LBB\S*:?|)(\s|$)", c)][:3])
            loops = loops[1:]
        assert len(loops) >= 2, f"{name}: expected a hot and a tail K loop"
        hot = loops[0].split("s_cbranch_scc")[0]
        n16 = len(re.findall(r"\bv_mfma_f32_16x16x32_f16", hot))
        n32 = len(re.findall(r"\bv_mfma_f32_32x32x16_f16", hot))
        assert (n16 == 0) != (n32 == 0), f"{name}: one MFMA shape per kernel ({n16} / {n32})"
        # a trip is a whole number of K-steps (K = 64) of the wave tile: (BM / WM) x (BN / WN) x 64 per K-step = FM * FN * 2
        # 16x16x32 MFMAs or FM * FN * 4 32x32x16 MFMAs (geometry from the mangled CfgSP / CfgSQ template arguments)
        bm, bn, wm, wn = map(int, re.search(r"Cfg\w+?ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).groups())
        mi = 16 if n16 else 32
        per_step = (bm // wm // mi) * (bn // wn // mi) * (2 if n16 else 4)
        n = n16 or n32
        assert n >= per_step and n % per_step == 0, f"{name}: {n16} / {n32} MFMAs in the hot loop, {per_step} per K-step"
        body = list(_outside_asm(hot.splitlines()))
        # LDS-DMA with a divergent descriptor is wrapped in a waterfall loop (readfirstlane + exec masking)
        assert not [ln for ln in body if re.search(r"v_readfirstlane|s_and_saveexec|s_cbranch_execn?z", ln)], name
        # fragment registers are written by ds_read only; no VALU moves between the MFMAs
        assert not [ln for ln in body if re.search(r"\bv_mov_b32|\bv_accvgpr", ln)], name
        # (family q writes its LDS-DMA loads as asm statements, so they are counted on the whole loop text)
        assert len([ln for ln in hot.splitlines() if "buffer_load_dwordx4" in ln and " lds" in ln.split(";")[0]]) >= 8, name


def test_m0_writes_and_lds_dma_loads_alternate_in_the_k_loops(sp_functions):
    """Family q issues an LDS-DMA piece as two asm statements in two MFMA gaps (hgemm_kernel_sq.hpp, sq_interval): M0 = the
    LDS destination, then the load.  M0 is the compiler's register, so the pairing is checked where it counts, on the ISA:
    in every MFMA loop of the q kernels an M0 write is followed by exactly one LDS-DMA load before the next M0 write,
    the loop neither starts with a load nor ends with a dangling M0 write, and at least one MFMA sits between the two
    (the wait state an LDS-DMA needs behind an M0 write)."""
    funcs, _ = sp_functions
    checked = 0
    for name, lines in funcs.items():
        if "sq_kernel" not in name:
            continue
        text = "\n".join(lines)
        for loop in re.split(r"This Inner Loop Header", text)[1:]:
            body = loop.split("s_cbranch_scc")[0]
            if len(re.findall(r"\bv_mfma_", body)) < 32:
                continue
            events = []
            for ln in body.splitlines():
                code = ln.split(";")[0].strip()
                if re.match(r"s_\w+\s+m0\b", code):
                    events.append("m0")
                elif code.startswith("buffer_load_dwordx4") and code.endswith(" lds"):
                    events.append("dma")
                elif code.startswith("v_mfma_") and events and events[-1] == "m0":
                    events.append("mfma")
            seq = [e for e in events if e != "mfma"]
            if not seq and int(re.search(r"ELi(\d+)EEEvNS", name).group(1)) & 8:
                continue   # the slice loop of a ktail variant's direct tail: MFMAs on fragments from plain buffer loads, no LDS-DMA
            assert seq and seq[0] == "m0" and seq[-1] == "dma", f"{name}: {seq[:4]} ... {seq[-4:]}"
            assert all(a != b for a, b in zip(seq, seq[1:])), f"{name}: M0 writes and LDS-DMA loads do not alternate"
            # an MFMA between every M0 write and its load
            for i, e in enumerate(events):
                if e == "m0":
                    assert events[i + 1] == "mfma", f"{name}: LDS-DMA right behind its M0 write"
            checked += 1
    assert checked >= 6


def m0_provenance_violations(lines):
    """Whole-function M0 audit: family q writes M0 and issues the LDS-DMA load as two asm statements without telling the
    compiler (an "m0" clobber makes hipcc pad every pair with an s_nop in the MFMA gaps).  So nothing but the ISA can show that
    the compiler never slips an M0 write of its own between a pair, on ANY path: every asm-statement `buffer_load ... lds` must
    be reached only by asm-statement M0 writes -- over the control-flow graph, not just textually.  Returns the offending loads.
    (Compiler-generated LDS-DMA, the builtin form used outside the K loops, sets M0 itself and is not subject to this.)"""
    blocks, cur, in_asm = [], {"label": None, "code": []}, False
    for ln in lines:
        if "#ASMSTART" in ln:
            in_asm = True
            continue
        if "#ASMEND" in ln:
            in_asm = False
            continue
        code = ln.split(";")[0].strip()
        if not code or code.startswith("#") or (code.startswith(".") and not code.endswith(":")):
            continue
        if code.endswith(":"):
            if cur["code"] or cur["label"] is not None:
                blocks.append(cur)
            cur = {"label": code[:-1], "code": []}
            continue
        cur["code"].append((code, in_asm))
        if re.match(r"s_(branch|cbranch_\w+|endpgm|setpc_b64|trap)\b", code):
            blocks.append(cur)
            cur = {"label": None, "code": []}
    if cur["code"] or cur["label"] is not None:
        blocks.append(cur)
    index = {b["label"]: i for i, b in enumerate(blocks) if b["label"] is not None}
    preds = [set() for _ in blocks]
    for i, b in enumerate(blocks):
        last = b["code"][-1][0] if b["code"] else ""
        m = re.match(r"s_(branch|cbranch_\w+)\s+(\S+)", last)
        if m and m.group(2) in index:
            preds[index[m.group(2)]].add(i)
        if i + 1 < len(blocks) and not re.match(r"s_(branch|endpgm|setpc_b64)\b", last):
            preds[i + 1].add(i)
    # per-block summary: the last M0 writer inside the block (None: the entry state passes through) and the asm loads, each with
    # the writer it sees inside the block (None: it sees the entry state)
    last_w, loads = [], []
    for b in blocks:
        w, ls = None, []
        for code, in_asm in b["code"]:
            if re.match(r"s_\w+\s+m0\b", code):
                w = "asm" if in_asm else "compiler"
            elif in_asm and code.startswith("buffer_load") and code.endswith(" lds"):
                ls.append((code, w))
        last_w.append(w)
        loads.append(ls)
    entry = [frozenset() for _ in blocks]          # who wrote M0 last, over all paths: subset of {"asm", "compiler"}
    for _ in range(len(blocks) + 2):
        changed = False
        for i in range(len(blocks)):
            e = frozenset().union(*[(frozenset({last_w[p]}) if last_w[p] else entry[p]) for p in preds[i]]) if preds[i] else frozenset()
            if e != entry[i]:
                entry[i], changed = e, True
        if not changed:
            break
    else:
        raise AssertionError("M0 audit did not reach a fixpoint")
    bad = []
    for i, ls in enumerate(loads):
        for code, w in ls:
            st = frozenset({w}) if w else entry[i]
            if st != frozenset({"asm"}):
                bad.append((code, sorted(st)))
    return bad


def test_every_asm_lds_dma_is_fed_by_an_asm_m0_write_on_every_path(sp_functions):
    funcs, _ = sp_functions
    pairs = 0
    for name, lines in funcs.items():
        if "sq_kernel" not in name:
            continue
        bad = m0_provenance_violations(lines)
        assert not bad, f"{name}: {len(bad)} LDS-DMA loads can see a compiler-written M0, first: {bad[0]}"
        pairs += sum(1 for ln in lines if ln.split(";")[0].strip().startswith("buffer_load") and ln.split(";")[0].strip().endswith(" lds"))
    assert pairs > 500
    # the audit catches a compiler M0 write between a pair, directly and through a side entry
    a_m0, a_ld = ["#ASMSTART", "s_mov_b32 m0, s5", "#ASMEND"], ["#ASMSTART", "buffer_load_dwordx4 v1, s[0:3], s9 offen lds", "#ASMEND"]
    assert not m0_provenance_violations(a_m0 + ["v_mfma_f32_16x16x32_f16 a[0:3], v[0:3], v[4:7], a[0:3]"] + a_ld)
    assert m0_provenance_violations(a_m0 + ["s_mov_b32 m0, -1"] + a_ld)
    assert m0_provenance_violations(["s_cbranch_scc1 .LBB0_2"] + a_m0 + ["s_branch .LBB0_3", ".LBB0_2:", "s_mov_b32 m0, s7", ".LBB0_3:"] + a_ld)
    assert m0_provenance_violations(a_ld)          # no M0 write at all in front of the load


def test_staged_epilogue_has_no_scalar_load_inside_its_counted_lds_window(sp_functions):
    """sp_epilogue_staged waits with `s_waitcnt lgkmcnt(4)` for its two ds_read_b128 while the next group's four
    ds_write_b64 are already queued -- sound only while nothing else counts on lgkmcnt there: SMEM loads share the counter and
    return out of order.  On the ISA: between the first ds_write_b64 of a staged epilogue and its last buffer_store there is no
    s_load / s_buffer_load."""
    funcs, _ = sp_functions
    seen = 0
    for name, lines in funcs.items():
        codes = [ln.split(";")[0].strip() for ln in lines]
        idx_w = [i for i, c in enumerate(codes) if c.startswith("ds_write_b64")]
        if not idx_w:
            continue
        # runs of the staged epilogue: from a ds_write_b64 to the last buffer_store_dwordx4 before the next K-loop MFMA
        i = 0
        while i < len(idx_w):
            start = idx_w[i]
            end = start
            j = start
            while j < len(codes) and not codes[j].startswith("v_mfma"):
                if codes[j].startswith("buffer_store_dwordx4"):
                    end = j
                j += 1
            window = codes[start:end + 1]
            assert not [c for c in window if c.startswith(("s_load", "s_buffer_load"))], f"{name}: scalar load inside the staged epilogue's LDS window"
            seen += 1
            while i < len(idx_w) and idx_w[i] <= max(end, start):
                i += 1
    assert seen >= 4


def _vgprs(tok: str, bank: str = "v") -> set:
    """register numbers of a v / a operand (`a` registers are offset by 1000 so both banks share one set)"""
    base = 0 if bank == "v" else 1000
    m = re.match(bank + r"\[(0x[0-9a-f]+|\d+):(0x[0-9a-f]+|\d+)\]$", tok)
    if m:
        return set(range(base + int(m.group(1), 0), base + int(m.group(2), 0) + 1))
    m = re.match(bank + r"(\d+)$", tok)
    return {base + int(m.group(1))} if m else set()


def _audit_step(recent, code, bad):
    """One instruction of the hazard scan: `recent` = [(registers written, wait states since, text)] of the VALU writes younger
    than two wait states; returns the list behind this instruction."""
    ops = code.replace(",", " ").split()
    mn = ops[0]
    if mn.startswith("v_mfma"):
        src = set()
        for tok in ops[2:4]:
            src |= _vgprs(tok)
        if len(ops) > 4:
            src |= _vgprs(ops[4], "a")        # the accumulator input: v_accvgpr_write (the clears) is a VALU write, too
        bad += [(txt, code) for (w, age, txt) in recent if age < 2 and w & src]
        return [(w, age + 1, t) for (w, age, t) in recent if age + 1 < 2]
    step = int(ops[1]) + 1 if mn == "s_nop" else 1
    recent = [(w, age + step, t) for (w, age, t) in recent if age + step < 2]
    if mn.startswith("v_") and not mn.startswith("v_cmp") and len(ops) > 1:
        w = _vgprs(ops[1]) | _vgprs(ops[1], "a")
        if w:
            recent.append((frozenset(w), 0, code))
    return recent


def valu_to_mfma_source_hazards(lines):
    """(VALU line, MFMA line) pairs where an MFMA reads a VGPR as A / B operand fewer than two wait states behind a VALU write of
    it.  hipcc's hazard recognizer pads its own MFMAs for this; the persistent families write theirs as asm statements, which
    it does not see -- the MFMA would read the OLD register value.  (ds_read results are ordered by lgkmcnt, not by wait
    states, and are not VALU writes.)
    The scan follows the CONTROL FLOW (the 192 x 192 bug sat at a control-flow merge, and a straight-line scan only
    sees textual fall-through): the stream is cut into basic blocks at labels and behind branches; a block is entered with the
    union of the young VALU writes at the end of ALL its predecessors -- the block above it unless that ends in s_branch /
    s_endpgm, and every block that branches to its label, loop back-edges included -- iterated to a fixpoint (a block shorter
    than two wait states passes its own entry state on).  A branch counts as one wait state whether taken or not
    (conservative: a taken branch refills the instruction buffer)."""
    blocks, cur = [], {"label": None, "code": []}
    for ln in lines:
        code = ln.split(";")[0].strip()
        if not code or code.startswith("#") or (code.startswith(".") and not code.endswith(":")):
            continue
        if code.endswith(":"):
            if cur["code"] or cur["label"] is not None:
                blocks.append(cur)
            cur = {"label": code[:-1], "code": []}
            continue
        cur["code"].append(code)
        if re.match(r"s_(branch|cbranch_\w+|endpgm|setpc_b64|trap)\b", code):
            blocks.append(cur)
            cur = {"label": None, "code": []}
    if cur["code"] or cur["label"] is not None:
        blocks.append(cur)
    index = {b["label"]: i for i, b in enumerate(blocks) if b["label"] is not None}
    preds = [set() for _ in blocks]
    for i, b in enumerate(blocks):
        last = b["code"][-1] if b["code"] else ""
        m = re.match(r"s_(branch|cbranch_\w+)\s+(\S+)", last)
        if m and m.group(2) in index:
            preds[index[m.group(2)]].add(i)
        if i + 1 < len(blocks) and not re.match(r"s_(branch|endpgm|setpc_b64)\b", last):
            preds[i + 1].add(i)
    entry = [frozenset() for _ in blocks]
    exits = [frozenset() for _ in blocks]
    bad = []
    for _ in range(8):                      # ages are < 2: the state space is tiny, two or three sweeps reach the fixpoint
        changed = False
        bad = []
        for i, b in enumerate(blocks):
            recent = sorted(entry[i], key=str)
            for code in b["code"]:
                recent = _audit_step(recent, code, bad)
            out = frozenset(recent)
            if out != exits[i]:
                exits[i], changed = out, True
        for i in range(len(blocks)):
            e = frozenset().union(*[exits[p] for p in preds[i]]) if preds[i] else frozenset()
            if e != entry[i]:
                entry[i], changed = e, True
        if not changed:
            break
    else:
        raise AssertionError("hazard scan did not reach a fixpoint")
    return sorted(set(bad))


def test_no_valu_write_sits_within_two_wait_states_of_an_asm_mfma_that_reads_it(sp_functions):
    """Round 3: a 192 x 192 member of family q produced one wrong output tile whenever the K-step count was odd -- hipcc had
    moved an A fragment from v[2:5] to v[0:3] with four v_perm_b32 directly in front of its first MFMA (a control-flow merge
    in front of the odd K-step), and an asm MFMA gets no hazard padding.  The shipped 192 x 256 member had the same pattern in
    its narrow-epilogue variant.  sq_settle() now pins the fragment sets and spends the wait states at that merge; this test
    keeps EVERY MFMA of every persistent kernel clear of the condition, whatever a future compiler does with the copies."""
    funcs, _ = sp_functions
    total = 0
    for name, lines in funcs.items():
        bad = valu_to_mfma_source_hazards(lines)
        assert not bad, f"{name}: {len(bad)} MFMA source hazards, first: {bad[0]}"
        total += sum(1 for ln in lines if ln.split(";")[0].strip().startswith("v_mfma"))
    assert total > 5000      # the audit really saw the MFMA streams


def test_the_hazard_audit_catches_the_pattern():
    stream = ["v_perm_b32 v2, v123, v4, s68", "v_perm_b32 v3, v122, v5, s68",
              "v_mfma_f32_16x16x32_f16 a[120:123], v[74:77], v[0:3], a[120:123]"]
    assert len(valu_to_mfma_source_hazards(stream)) == 2
    assert not valu_to_mfma_source_hazards(stream[:2] + ["s_nop 1"] + stream[2:])
    assert not valu_to_mfma_source_hazards(["ds_read_b128 v[0:3], v9"] + stream[2:])          # LDS results: lgkmcnt's business
    assert len(valu_to_mfma_source_hazards([stream[1], stream[2]])) == 1                      # no wait state
    assert len(valu_to_mfma_source_hazards([stream[1], "s_nop 0", stream[2]])) == 1           # one wait state: still too close
    assert len(valu_to_mfma_source_hazards([stream[1], "s_add_u32 m0, m0, 0x1000", stream[2]])) == 1
    assert not valu_to_mfma_source_hazards([stream[1], "s_add_u32 m0, m0, 0x1000", "s_nop 0", stream[2]])   # two
    assert len(valu_to_mfma_source_hazards(["v_accvgpr_write_b32 a121, 0", stream[2]])) == 1  # a cleared accumulator read as SrcC
    assert not valu_to_mfma_source_hazards(["v_accvgpr_write_b32 a124, 0", stream[2]])


def test_the_hazard_audit_follows_branches():
    """Edges other than fall-through: a VALU write at the end of a block that JUMPS to a block opening with an asm MFMA,
    a loop back-edge, and a merge where only one predecessor carries the write."""
    mfma = "v_mfma_f32_16x16x32_f16 a[120:123], v[74:77], v[0:3], a[120:123]"
    # taken branch: the write sits textually far away from the MFMA
    taken = ["s_cmp_eq_u32 s0, 0", "s_cbranch_scc1 .LBB0_2", "v_perm_b32 v2, v9, v4, s68", "s_branch .LBB0_3",
             ".LBB0_2:", "s_nop 4", "s_endpgm", ".LBB0_3:", mfma]
    # (the branch is the one wait state between the write and the MFMA: still a hazard)
    assert len(valu_to_mfma_source_hazards(taken)) == 1
    assert not valu_to_mfma_source_hazards(taken[:-1] + ["s_nop 0", mfma])
    # the same layout with the write in front of the OTHER exit is clean
    other = ["s_cmp_eq_u32 s0, 0", "s_cbranch_scc1 .LBB0_2", "s_nop 0", "s_branch .LBB0_3",
             ".LBB0_2:", "v_perm_b32 v2, v9, v4, s68", "s_endpgm", ".LBB0_3:", mfma]
    assert not valu_to_mfma_source_hazards(other)
    # loop back-edge: the write closes the loop body, the MFMA opens it
    loop = ["s_mov_b32 s4, 8", ".LBB0_1:", mfma, "s_add_i32 s4, s4, -1", "s_cmp_lg_u32 s4, 0", "v_mov_b32 v1, v8", "s_cbranch_scc1 .LBB0_1", "s_nop 0"]
    assert len(valu_to_mfma_source_hazards(loop)) == 1
    assert not valu_to_mfma_source_hazards([ln for ln in loop if not ln.startswith("v_mov")])
    # merge: fall-through predecessor is clean, the side entry is not
    merge = ["s_cbranch_scc1 .LBB0_5", "s_nop 1", "s_branch .LBB0_6", ".LBB0_5:", "v_perm_b32 v3, v9, v4, s68", ".LBB0_6:", mfma]
    assert len(valu_to_mfma_source_hazards(merge)) == 1
    # a block shorter than two wait states hands its entry state on
    short = ["v_perm_b32 v0, v9, v4, s68", "s_branch .LBB0_7", ".LBB0_7:", mfma]
    assert len(valu_to_mfma_source_hazards(short)) == 1
    short_ok = ["v_perm_b32 v0, v9, v4, s68", "s_branch .LBB0_7", ".LBB0_7:", "s_nop 0", mfma]
    assert not valu_to_mfma_source_hazards(short_ok)


def test_the_audits_hold_at_a_second_optimisation_level(tmp_path_factory):
    """VERDICT r3 item 8 asks that the hazard class be removed rather than audited.  It is still audited -- but the audit must not depend
    on one lucky register allocation: the persistent kernels compiled at -O2 (another schedule, another allocation) pass the same
    control-flow-aware hazard scan, the M0 provenance audit, the AGPR rule and the no-scratch rule.  (Exactness of an -O2 library is a
    GPU question; the shipped build is -O3.)"""
    text = _compile_groups(tmp_path_factory, "-O2")
    funcs = {m.group(1): m.group(2).splitlines()
             for m in re.finditer(r"^(_ZN12hgemm_mi355x18hgemm_tn_s[pq]_kernel\w+):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}
    assert len(funcs) >= 40
    for name, lines in funcs.items():
        assert not valu_to_mfma_source_hazards(lines), name
        assert not [ln for ln in lines if "scratch_" in ln], name
        assert not [ln for ln in _outside_asm(lines) if re.search(r"\bv_accvgpr_|\bv_mfma_|\ba\[?\d+", ln.split(";")[0])], name
        if "sq_kernel" in name:
            assert not m0_provenance_violations(lines), name


def _r6_change_allowed(name: str) -> bool:
    """Kernels round 6 touched on purpose (see the test below)."""
    epi = re.search(r"EEELi(\d+)EEEvNS", name)
    epi = int(epi.group(1)) if epi else -1
    if "15hgemm_tn_kernel" in name or "18hgemm_tn_wd_kernel" in name:
        return epi == 2                                   # EPI_FUSED
    if "18hgemm_tn_rs_kernel" in name:
        return epi in (2, 10)                             # EPI_FUSED, EPI_FUSED | ktail
    if "18hgemm_tn_sq_kernel" in name:
        # the row-ahead combine of the fused variants (epilogue ids 3, 3 | ktail, 3 | kstagger) of the members with <= 128 accumulators
        return (epi & 3) == 3 and re.search(r"CfgSQILi(256ELi128E|128ELi128E|192ELi128E|128ELi192E)", name) is not None
    return False


def test_kernels_of_the_measured_library_keep_their_instruction_streams(isa_text):
    """A round's grid records (plan reports, parity / tolerance records, PMC table, bench) stay valid only while the kernels they
    ran are untouched, and "I did not edit that function" is not evidence: variants are instantiations of the same templates and
    share non-inlined helpers.  So the kernels are fingerprinted (tools/isa_fingerprint.py: instruction stream modulo basic-block
    numbering) against the library a closing run measured.

    Round 6 against round 5's closing library (profiles/r05_isa_fingerprint_closing_run_library.json, 348 kernels): the SAME 348
    kernels, none added, and exactly 76 changed, knowingly -- the single-launch split-K ("fused") variants, whose last arriver now
    adds the slabs in batches (fused_combine): 28 of the classic family, 24 of family r (plain + ktail), 9 of family w, and the 15
    fused variants of the five family-q members with at most 128 accumulator registers.  (A prologue for a phase offset inside a CU
    was tried on the two-resident members in calls B - F and withdrawn: no gain, profiles/withdrawn/r06_cuphase_*.)
    Every other kernel -- all plain / two-pass / stream-K kernels of every family, and every variant of q256x256 (the headline
    kernel), q192x256, q256x192, q128x256 -- is instruction-for-instruction round 5's: 272 kernels, checked below.  The closing run of round 6 fingerprints its own library
    (profiles/r06_isa_fingerprint_closing_run_library.json, when present: everything must match it)."""
    import json
    import sys

    sys.path.insert(0, str(REPO / "cuda-l2_amd" / "tools"))
    import isa_fingerprint

    now = isa_fingerprint.fingerprints(isa_text)
    base = json.loads((REPO / "profiles" / "r05_isa_fingerprint_closing_run_library.json").read_text())["kernels"]
    assert len(base) == 348 and set(base) == set(now), (sorted(set(base) ^ set(now))[:4])
    changed = [k for k in base if now[k] != base[k]]
    assert not [k for k in changed if not _r6_change_allowed(k)], [k for k in changed if not _r6_change_allowed(k)][:4]
    assert len(changed) == 76, len(changed)
    # the headline kernel and its variants are round 5's
    assert not [k for k in changed if "CfgSQILi256ELi256E" in k]
    r6 = REPO / "profiles" / "r06_isa_fingerprint_closing_run_library.json"
    if r6.exists():
        closing = json.loads(r6.read_text())["kernels"]
        assert set(closing) == set(now) and not [k for k in closing if now[k] != closing[k]], [k for k in closing if now.get(k) != closing[k]][:4]
    # round 4 -> round 5 (kept: what round 5 changed knowingly): of round 4's 296 kernels the classic family, family r and both
    # stream-K kernels came through round 5 untouched
    r4 = json.loads((REPO / "profiles" / "r04_isa_fingerprint_call_k_library.json").read_text())["kernels"]
    assert len(r4) == 296 and not set(r4) - set(base)
    same = [k for k in r4 if base[k] == r4[k]]
    ch5 = [k for k in r4 if base[k] != r4[k]]
    assert len(same) == 212 and all(re.search(r"hgemm_tn_(sq|sp|wd)_kernel", k) for k in ch5)
    added = sorted(set(base) - set(r4))
    # kstagger variants (epilogue id + 16) of the 16x16x32 members of family q, and every variant of the two-resident members
    assert added and all(re.search(r"hgemm_tn_sq_kernel.*(ELi(16|17|18|19)EEEvNS|CfgSQILi(192ELi128|128ELi192)E)", k) for k in added), added[:3]
