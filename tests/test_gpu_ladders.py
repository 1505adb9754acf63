"""GPU ladders (run with `-m gpu` on an MI355X): every table geometry at short and odd K-step counts, the item seams of the
persistent walks (families s and q), and sliver tiles -- explicit plans through the C ABI against the CPU oracle.

Nothing here names a geometry: the table is read through the C ABI (hgemm_mi355x_config_info: BM, BN, MI; the stage depth is
the smallest K of 64 / 128 / 256 that hgemm_mi355x_config_accepts_k takes; a K tail is taken when stage + 40 is accepted;
hgemm_mi355x_config_streamk), persistence and the resident workgroup count G come from the launch-decision hook
(gpu_common.resolve: grid < items), so a new member is covered the day it joins the table.  One case per family letter.

Bar: 0/1 inputs (oracle.zero_one_inputs) BIT-EXACT AND UNMASKED against oracle.truth_numpy / truth_prefix_k -- every partial
sum is an integer < 2**24, exact in fp32 in any order, then one round-to-nearest-even to fp16 (tests/test_oracle.py pins
the restatements together).  C is NaN-prefilled and every padding element compared (gpu_common.gemm).  Each launch is first
resolved through the hook: status 0, never the any-shape kernel, and the form / split count / grid it really runs as.
N(0,1) inputs: oracle.relative_error <= 1e-3 (the project's REL_TOL) against the fp32 product on the CPU."""
import ctypes
import math
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

from gpu_common import resolve

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3
FAMILIES = ("t", "s", "q", "r", "w", "u")
PERSISTENT_FAMILIES = ("s", "q")
NO_FUSED_KERNEL = ("u",)     # include/hgemm_mi355x.h: HGEMM_SPLITK_FUSED on a family-u geometry runs as the two-pass form
FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000
XCD_STAGGER, RS_NT_LOADS = 0x80000, 0x100000
PHASE_OFFSET, WAVE_PRIORITY, PHASE_OFFSET4 = 0x200000, 0x400000, 0x800000
PHASE_OFFSET8 = PHASE_OFFSET | PHASE_OFFSET4
SPLIT_MASK = 0xFFFF
EDGE = 24                    # rows / columns of the ragged last tile (a multiple of 8: the wide epilogue stays possible)
TAIL = 40                    # K remainder of the tail rungs: one whole K = 32 slice and a partial one

Geo = namedtuple("Geo", "name cid family bm bn mi stage tail streamk grid")   # grid: resident workgroups G (0: not persistent)


@pytest.fixture(scope="module")
def g():
    import gpu_common

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return gpu_common


@pytest.fixture(scope="module")
def oracle():
    from oracle import hgemm_oracle

    return hgemm_oracle


def read_table(g):
    """Every table geometry, described through the C ABI and the launch-decision hook alone."""
    L = g.lib()
    out = []
    for cid, name in enumerate(g.config_names()):
        info = (ctypes.c_int * 8)()
        assert L.hgemm_mi355x_config_info(cid, info) == 0
        bm, bn, mi = info[0], info[1], info[4]
        stages = [k for k in (64, 128, 256) if L.hgemm_mi355x_config_accepts_k(cid, k) == 1]
        assert stages, f"{name}: no stage depth among 64 / 128 / 256"
        stage = stages[0]
        tail = L.hgemm_mi355x_config_accepts_k(cid, stage + TAIL) == 1
        # persistence: 1600 one-stage tiles (more than any resident wave; one K-step, so the hybrid rule cannot fire)
        st, form, disp = resolve(cid, 1, 40 * bm, 40 * bn, stage, (stage, stage, 40 * bn))
        assert st == 0 and form == "plain" and len(disp) == 1, (name, st, form, disp)
        grid, items = disp[0][1], disp[0][5]
        assert items == 1600 and 0 < grid <= items, (name, disp)
        out.append(Geo(name, cid, name[0], bm, bn, mi, stage, tail, L.hgemm_mi355x_config_streamk(cid) > 0, grid if grid < items else 0))
    return out


@pytest.fixture(scope="module")
def geos(g):
    return read_table(g)


def bits(x):
    return x.view(np.uint16)


class Operands:
    """One pair of 0/1 operands at the largest shape of a test part; every case takes a top-left sub-block (rows of A, columns
    of B, a K prefix) and the same sub-block of the truth of that K -- exact for 0/1 inputs (oracle.truth_prefix_k)."""

    def __init__(self, oracle, m, n, ks, seed):
        ks = sorted(set(ks))
        self.a, self.b = oracle.zero_one_inputs(m, n, ks[-1], np.random.default_rng(seed))
        self.truth = dict(oracle.truth_prefix_k(self.a, self.b, ks))
        assert all(not np.isnan(t).any() for t in self.truth.values())

    def sub(self, m, n, k):
        return self.a[:m, :k], self.b[:k, :n], self.truth[k][:m, :n]


class Normals:
    """The same for N(0,1) operands: the reference is the fp32 product of the fp16 values on the CPU."""

    def __init__(self, m, n, kmax, seed):
        rng = np.random.default_rng(seed)
        self.a = rng.standard_normal((m, kmax), dtype=np.float32).astype(np.float16)
        self.b = rng.standard_normal((kmax, n), dtype=np.float32).astype(np.float16)
        self.ref = {}

    def sub(self, m, n, k, with_ref=True):
        if with_ref and k not in self.ref:
            self.ref[k] = self.a[:, :k].astype(np.float32) @ self.b[:k].astype(np.float32)
        return self.a[:m, :k], self.b[:k, :n], self.ref[k][:m, :n] if with_ref else None


class Findings:
    """Failures of one test case, gathered so that the report shows the pattern (which rung, which form, which rows and columns),
    raised together at the end; a wrong result is no fault, the walk goes on."""

    def __init__(self):
        self.lines, self.runs = [], 0

    def exact(self, g, geo, splits, a, b, truth, what, ld=None, group=2):
        got = g.gemm(a, b, plan=(geo.cid, splits, group), ld=ld)
        self.runs += 1
        bad = bits(got) != bits(truth)
        if bad.any():
            rows, cols = np.flatnonzero(bad.any(axis=1)), np.flatnonzero(bad.any(axis=0))
            self.lines.append(f"{geo.name} splits {hex(splits)} {a.shape[0]}x{b.shape[1]}x{a.shape[1]} ld={ld} {what}: {int(bad.sum())} of "
                              f"{bad.size} elements differ; rows {rows[0]}..{rows[-1]} ({len(rows)}), columns {cols[0]}..{cols[-1]} "
                              f"({len(cols)}); first: got {got[rows[0], cols[0]]} want {truth[rows[0], cols[0]]}")
        return got

    def check(self, ok, line):
        if not ok:
            self.lines.append(line)

    def close(self, label, t0):
        print(f"{label}: {self.runs} runs, {time.perf_counter() - t0:.1f} s")
        assert not self.lines, f"{len(self.lines)} findings:\n" + "\n".join(self.lines[:40])


def fast(geo, splits, m, n, k, lds=None):
    """The hook's decision for a run that must take the geometry's own kernel: (form, the first dispatch)."""
    st, form, disp = resolve(geo.cid, splits, m, n, k, lds or (k, k, n))
    assert st == 0 and form not in ("ragged", "reference") and disp, (geo.name, hex(splits), (m, n, k), lds, st, form)
    return form, disp[0]


def as_requested(geo, splits, form, dispatch):
    """Whether a run resolved to the form its plan word names: stream-K on the named number of workgroups, a split count of
    its own in the two-pass / single-launch form (the latter runs as two-pass on a family without that kernel), plain."""
    low = splits & SPLIT_MASK
    if splits & STREAMK:
        return form == "stream-K" and dispatch[1] == low
    if low > 1:
        want = "fused" if splits & FUSED and geo.family not in NO_FUSED_KERNEL else "split-K"
        return form == want and dispatch[3] == low
    return form == "plain" and dispatch[3] == 1


def test_the_table_is_what_the_ladders_assume(geos):
    """Every geometry belongs to a family letter the cases below run; a K tail is taken by families t and r and by the
    16x16x32 members of family q; families s and q are the persistent ones, all of their members and nobody else."""
    assert len(geos) >= 60
    for geo in geos:
        assert geo.family in FAMILIES, f"{geo.name}: add its family letter to FAMILIES"
        assert geo.tail == (geo.family in "tr" or (geo.family == "q" and geo.mi == 16)), geo
        assert (geo.grid > 0) == (geo.family in PERSISTENT_FAMILIES), geo
    assert {geo.family for geo in geos} == set(FAMILIES)


# ---- A. K-step ladder ---------------------------------------------------------------------------------------------------------
RUNGS = range(1, 10)           # past twice the deepest ring (4), both parities
TAIL_RUNGS = (1, 2, 3)


def ladder_forms(geo):
    forms = [1, 1 | NT_STORE, 2, 3, 2 | FUSED, 3 | FUSED]
    if geo.streamk:
        forms.append(STREAMK | 5)
    if geo.family == "q":
        forms.append(1 | XCD_STAGGER)
    if geo.family == "r":
        forms.append(1 | XCD_STAGGER | RS_NT_LOADS)
    return forms


@pytest.fixture(scope="module")
def ladder_operands(oracle, geos):
    ks = {geo.stage * n for geo in geos for n in RUNGS} | {geo.stage * n + TAIL for geo in geos if geo.tail for n in TAIL_RUNGS}
    m, n = max(geo.bm for geo in geos) + EDGE, max(geo.bn for geo in geos) + EDGE
    return Operands(oracle, m, n, ks, seed=101), Normals(m, n, max(ks), seed=102)


@pytest.mark.parametrize("family", FAMILIES)
def test_k_step_ladder_of_every_geometry(g, oracle, geos, ladder_operands, family):
    """K = 1 ... 9 pipeline stages (a ring's prologue longer than the walk, odd and even step counts, the early-A split's step
    parity) on one whole tile plus a 24-row / 24-column sliver each way, in every form; a K tail of 40 behind 1, 2, 3 stages where
    the geometry takes one.  Per geometry every requested form must have run AS ITSELF on some whole-stage rung (the host
    clamps splits to one per stage: a degraded rung is no coverage of that form).  One N(0,1) run per rung at splits = 1."""
    L = g.lib()
    zo, nrm = ladder_operands
    f, t0 = Findings(), time.perf_counter()
    members = [geo for geo in geos if geo.family == family]
    assert members
    never = []
    for geo in members:
        m, n = geo.bm + EDGE, geo.bn + EDGE
        forms = ladder_forms(geo)
        ran_as_itself = {s: [] for s in forms}
        rungs = [(i, geo.stage * i) for i in RUNGS] + ([(i, geo.stage * i + TAIL) for i in TAIL_RUNGS] if geo.tail else [])
        for i, k in rungs:
            assert L.hgemm_mi355x_config_accepts_k(geo.cid, k) == 1, (geo.name, k)
            a, b, truth = zo.sub(m, n, k)
            for s in forms:
                form, d = fast(geo, s, m, n, k)
                if k % geo.stage == 0 and as_requested(geo, s, form, d):
                    ran_as_itself[s].append(i)
                f.exact(g, geo, s, a, b, truth, f"rung {i} ({form}, {d[3]} splits, grid {d[1]})")
            ar, br, ref = nrm.sub(m, n, k)
            got = g.gemm(ar, br, plan=(geo.cid, 1, 2))
            f.runs += 1
            err = oracle.relative_error(got, ref)
            f.check(err <= REL_TOL, f"{geo.name} N(0,1) {m}x{n}x{k}: relative error {err:.3e} > {REL_TOL}")
        for s, where in ran_as_itself.items():
            f.check(where, f"{geo.name}: form {hex(s)} never ran as itself on rungs 1 ... 9")
        if any(s & FUSED for s in forms) and geo.family in NO_FUSED_KERNEL:
            never.append(f"{geo.name}: single-launch split-K runs as two-pass")
    print(f"ladder {family}: forms that cannot run as requested: {never or 'none'}")
    f.close(f"ladder {family}: {len(members)} geometries", t0)


# ---- B. item seams of the persistent walks ------------------------------------------------------------------------------------
def seam_tiles(grid):
    """The smallest near-square tile grid with more tiles than resident workgroups."""
    tm = math.isqrt(grid) + 1
    return tm, grid // tm + 1


def seam_shape(geo):
    tm, tn = seam_tiles(geo.grid)
    assert tm * tn > geo.grid and (tm - 1) * tn <= geo.grid and abs(tm - tn) <= 1
    return (tm - 1) * geo.bm + EDGE, (tn - 1) * geo.bn + EDGE


def seam_ks(geo):
    return [geo.stage * i for i in range(1, 6)] + ([geo.stage * 3 + TAIL] if geo.tail else [])


@pytest.fixture(scope="module")
def seam_operands(oracle, geos):
    walkers = [geo for geo in geos if geo.grid]
    shapes = [seam_shape(geo) for geo in walkers]
    ks = {k for geo in walkers for k in seam_ks(geo)}
    m, n = max(s[0] for s in shapes), max(s[1] for s in shapes)
    return Operands(oracle, m, n, ks, seed=201), Normals(m, n, max(geo.stage for geo in walkers) * 3, seed=202)


@pytest.mark.parametrize("family", PERSISTENT_FAMILIES)
def test_item_seams_when_tiles_exceed_the_resident_workgroups(g, geos, seam_operands, family):
    """More tiles than resident workgroups (the smallest near-square grid that has), both edges ragged, 1 ... 5 K-steps per item
    and a K tail behind three: the pipeline carried across items, first / middle / last item of a walk, with plain and
    non-temporal stores.  The hook must show items > grid in the plain form (under 8 K-steps the hybrid rule cannot fire)."""
    zo, _ = seam_operands
    f, t0 = Findings(), time.perf_counter()
    members = [geo for geo in geos if geo.family == family and geo.grid]
    assert members
    for geo in members:
        m, n = seam_shape(geo)
        for k in seam_ks(geo):
            a, b, truth = zo.sub(m, n, k)
            for s in (1, 1 | NT_STORE):
                form, d = fast(geo, s, m, n, k)
                assert form == "plain" and d[5] > d[1] == geo.grid and d[3] == 1, (geo.name, (m, n, k), form, d)
                f.exact(g, geo, s, a, b, truth, f"{d[5]} items on {d[1]} workgroups")
    f.close(f"seams by tiles {family}: {len(members)} geometries", t0)


def split_rule(steps, splits):
    """The host's K cut (hgemm_mi355x.h: at most one split per stage, no empty split, chunks of whole stages)."""
    per = -(-steps // max(1, min(splits, steps)))
    return -(-steps // per), per


def three_item_splits(geo, m, n):
    """The smallest split count with which some workgroup walks three items: items >= 2 x grid + 1 (through the hook)."""
    for s in range(2, 4096):
        form, d = fast(geo, s, m, n, s * geo.stage)
        assert form == "split-K" and d[3] == s, (geo.name, s, form, d)
        if d[5] >= 2 * d[1] + 1:
            return s
    raise AssertionError(f"{geo.name}: no split count below 4096 gives a three-item walk")


def split_seam_ks(geo, s):
    """s x n stages (items of n = 1, 2, 3 steps); (2 s + 1) stages as the host cuts them: chunks of three stages and a last
    chunk of one (fewer items, a short item at every tile's end); (2 s - 1) stages: s chunks of two stages and a last chunk
    of ONE, so that the step parity changes at a seam of a three-item walk."""
    return [s * i * geo.stage for i in (1, 2, 3)] + [(2 * s + 1) * geo.stage, (2 * s - 1) * geo.stage]


@pytest.fixture(scope="module")
def split_seam_operands(oracle, geos):
    plans = {}
    for geo in geos:
        if geo.grid:
            m, n = 2 * geo.bm + EDGE, 2 * geo.bn + EDGE
            plans[geo.name] = (m, n, three_item_splits(geo, m, n))
    ks = {k for geo in geos if geo.grid for k in split_seam_ks(geo, plans[geo.name][2])}
    m, n = max(p[0] for p in plans.values()), max(p[1] for p in plans.values())
    return plans, Operands(oracle, m, n, ks, seed=301)


@pytest.mark.parametrize("family", PERSISTENT_FAMILIES)
def test_item_seams_when_splits_make_the_items(g, geos, split_seam_operands, family):
    """Nine tiles (two whole ones and a sliver each way) cut into so many K splits that a workgroup walks three items, two-pass
    and single-launch: items of 1, 2 and 3 K-steps, and two K at which a tile's last item is shorter than the others.  The hook
    must show the split count the host rule gives and the form asked for."""
    plans, zo = split_seam_operands
    f, t0 = Findings(), time.perf_counter()
    members = [geo for geo in geos if geo.family == family and geo.grid]
    assert members
    for geo in members:
        m, n, s = plans[geo.name]
        assert s * 9 >= 2 * geo.grid + 1 > (s - 1) * 9, (geo.name, s)
        for k in split_seam_ks(geo, s):
            steps = k // geo.stage
            want_splits, per = split_rule(steps, s)
            a, b, truth = zo.sub(m, n, k)
            for plan, want_form in ((s, "split-K"), (s | FUSED, "fused")):
                form, d = fast(geo, plan, m, n, k)
                assert form == want_form and d[3] == want_splits and d[4] == per * geo.stage and d[5] == 9 * want_splits, (geo.name, k, form, d)
                assert d[5] > d[1], (geo.name, k, d)                        # a walk of several items
                if steps != 2 * s + 1:
                    assert want_splits == s and d[5] >= 2 * geo.grid + 1, (geo.name, k, d)   # ... of three
                f.exact(g, geo, plan, a, b, truth, f"{d[5]} items of {per} steps (last of a tile: {steps - per * (want_splits - 1)}) on {d[1]} workgroups")
    f.close(f"seams by splits {family}: {len(members)} geometries", t0)


def test_phase_flags_of_family_q_change_no_bit(g, geos, seam_operands):
    """HGEMM_PLAN_PHASE_OFFSET / _OFFSET4 / _OFFSET8 / _WAVE_PRIORITY on a walk of several items of three K-steps: exact on 0/1
    inputs, and on N(0,1) inputs bit-identical to the run without the flag (include/hgemm_mi355x.h: "Results are bit-identical
    with and without them")."""
    zo, nrm = seam_operands
    f, t0 = Findings(), time.perf_counter()
    members = [geo for geo in geos if geo.family == "q" and geo.grid]
    assert members
    for geo in members:
        m, n = seam_shape(geo)
        k = 3 * geo.stage
        a, b, truth = zo.sub(m, n, k)
        ar, br, _ = nrm.sub(m, n, k, with_ref=False)
        base = g.gemm(ar, br, plan=(geo.cid, 1, 2))
        f.runs += 1
        assert not np.isnan(base).any()
        for flag in (PHASE_OFFSET, PHASE_OFFSET4, PHASE_OFFSET8, WAVE_PRIORITY):
            form, d = fast(geo, 1 | flag, m, n, k)
            assert form == "plain" and d[5] > d[1], (geo.name, hex(flag), form, d)
            f.exact(g, geo, 1 | flag, a, b, truth, "phase flag")
            got = g.gemm(ar, br, plan=(geo.cid, 1 | flag, 2))
            f.runs += 1
            f.check(np.array_equal(bits(got), bits(base)), f"{geo.name} flag {hex(flag)} {m}x{n}x{k}: N(0,1) result differs from the flag-less run")
    f.close(f"phase flags: {len(members)} geometries", t0)


# ---- C. sliver tiles ----------------------------------------------------------------------------------------------------------
def sliver_shapes(geo):
    n0, m0 = geo.bn + 4, geo.bm + 1         # N % 8 == 4: the narrow epilogue, a 4-column last tile; a 1-row last tile
    ms = sorted({1, 15, 16, 17, geo.bm - 1, geo.bm + 1})
    ns = sorted({4, 8, 12, 20, geo.bn - 4, geo.bn + 4})
    return [(m, n0) for m in ms] + [(m0, n) for n in ns if (m0, n) != (m0, n0)]


@pytest.fixture(scope="module")
def sliver_operands(oracle, geos):
    return Operands(oracle, max(geo.bm for geo in geos) + 1, max(geo.bn for geo in geos) + 4, {2 * geo.stage for geo in geos}, seed=401)


@pytest.mark.parametrize("family", FAMILIES)
def test_sliver_tiles_of_every_geometry(g, geos, sliver_operands, family):
    """K = two stages.  M = 1 / 15 / 16 / 17 / BM - 1 / BM + 1 (whole wave rows out of range, a 1-row last tile) against
    N = BN + 4, and N = 4 / 8 / 12 / 20 / BN - 4 / BN + 4 (4-column slivers, the narrow epilogue) against M = BM + 1: plain,
    two-pass, single-launch and (where the geometry has the kernel) stream-K, never the any-shape kernel; the largest of them
    once more at padded strides (K + 8, K + 24, N + 4)."""
    zo = sliver_operands
    f, t0 = Findings(), time.perf_counter()
    members = [geo for geo in geos if geo.family == family]
    assert members
    for geo in members:
        k = 2 * geo.stage
        forms = [1, 2, 2 | FUSED] + ([STREAMK | 3] if geo.streamk else [])
        shapes = sliver_shapes(geo)
        assert len(shapes) >= 7
        for m, n in shapes:
            a, b, truth = zo.sub(m, n, k)
            for s in forms:
                form, d = fast(geo, s, m, n, k)
                f.exact(g, geo, s, a, b, truth, f"sliver ({form})")
        m, n = geo.bm + 1, geo.bn + 4
        ld = (k + 8, k + 24, n + 4)
        a, b, truth = zo.sub(m, n, k)
        for s in forms:
            form, d = fast(geo, s, m, n, k, ld)
            f.exact(g, geo, s, a, b, truth, f"sliver, padded strides ({form})", ld=ld)
    f.close(f"slivers {family}: {len(members)} geometries", t0)
