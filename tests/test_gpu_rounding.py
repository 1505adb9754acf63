"""GPU rounding tests (run with `-m gpu` on an MI355X): the fp32 -> fp16 conversion of every kernel path, which the 0/1 ladders
cannot see -- their sums are integers <= 2047, exact in fp16 under every rounding mode.

Inputs: oracle.dyadic_inputs (A in {-1, 0, 1}, B in {0, 1 + e / 1024}).  Every sum over any subset of K, in any order and
grouping, is a multiple of 2^-10 below 2^13: exact in fp32 like a 0/1 sum, but about three quarters of the results need a real
rounding to fp16, a tenth and more are exact ties, and half of them are negative.  The truth is the exact fp64 product rounded
to fp16 once (oracle.truth_exact); every case is BIT-EXACT AND UNMASKED against it through gpu_common.gemm (NaN prefill, every
padding element compared).  No tolerance anywhere.  tests/test_oracle.py proves on the CPU, for these very operands, that the
truth is order-independent and that a truncating convert, a round-half-away convert and fp16-held partials each show in every
16x16 block of C.  A wrong result is reported with the mutant its differing elements equal, which names the fault.

The table test names no geometry: the table reader, the findings, the hook helpers and the flag words are the ladders'.  The
hybrid tail's four geometries are those of tests/test_gpu_parity.py's 0/1 test of that schedule."""
import ctypes
import time

import numpy as np
import pytest

import kernel_layout_model as klm
from gpu_common import lib, resolve
from test_gpu_ladders import (EDGE, FAMILIES, FUSED, NT_STORE, RS_NT_LOADS, SPLIT_MASK, STREAMK, TAIL, XCD_STAGGER,
                              Findings, Geo, as_requested, bits, fast, read_table, split_rule)
from test_gpu_ladders import g, geos, oracle  # noqa: F401  (the ladders' fixtures: the GPU helpers, the CPU oracle, the table)

pytestmark = pytest.mark.gpu

SEED = 501                   # of the table operands (tests/test_oracle.py draws the same)
STREAMK_WGS = 5              # workgroups of the stream-K plan word
NARROW = 20                  # columns of the last tile of the second N: N % 8 = 4, the narrow epilogue
HYBRID_MN = (4352, 4352)     # of test_hybrid_tail_schedule_is_exact_on_zero_one_inputs (tests/test_gpu_parity.py)
HYBRID_GEOMETRIES = ("s256x256_w2x2", "s128x256_w2x2", "q256x256_w2x2", "q256x128_w2x2")   # the four of that test


def rounding_ks(geo):
    """Three stages (the 2-way cut is two stages and one, the 3-way cut one each); two stages and a K tail of 40."""
    return [3 * geo.stage] + ([2 * geo.stage + TAIL] if geo.tail else [])


def rounding_forms(geo):
    forms = [1, 1 | NT_STORE, 3, 3 | FUSED]
    if geo.streamk:
        forms.append(STREAMK | STREAMK_WGS)
    if geo.family == "q":
        forms.append(1 | XCD_STAGGER)
    if geo.family == "r":
        forms.append(1 | XCD_STAGGER | RS_NT_LOADS)
    return forms


def streamk_cut(geo):
    """(K, [K offsets of the cuts]) of the smallest K of three or more whole stages at which stream-K on five workgroups runs on
    five AND cuts a tile between two of them.  The host snaps a run boundary onto a tile boundary while a tile has fewer than
    2 x min_steps stages (kernel_layout_model.streamk_start), so below that K every segment is a whole tile, stored directly:
    only from here on do the slab stores, the arrival vote and the finisher's K-order slab reduce run.  The partition is the
    model's, checked against the library's own (hgemm_mi355x_selfcheck_streamk)."""
    m, n = geo.bm + EDGE, geo.bn + EDGE
    tiles, grid, min_steps = 4, STREAMK_WGS, klm.streamk_min_steps(geo.stage)
    form, d = fast(geo, STREAMK | 64, m, n, 3 * geo.stage)          # the launch's own min_steps: 12 stages feed 12 // min_steps workgroups
    assert form == "stream-K" and d[1] == 3 * tiles // min_steps, (geo.name, min_steps, form, d)
    out = (ctypes.c_int * 2)()
    for steps in range(3, 17):
        k = steps * geo.stage
        form, d = fast(geo, STREAMK | grid, m, n, k)
        if not as_requested(geo, STREAMK | grid, form, d):
            continue
        assert d[5] == tiles, (geo.name, d)
        for w in range(grid + 1):
            assert lib().hgemm_mi355x_selfcheck_streamk(tiles, steps, grid, min_steps, w, 0, out) == 0
            assert out[0] == klm.streamk_start(tiles, steps, grid, min_steps, w), (geo.name, steps, w)
        partial = [seg for segs in klm.streamk_partition(tiles, steps, grid, min_steps) for seg in segs if seg[3] is not None]
        if partial:
            return k, sorted({seg[1] * geo.stage for seg in partial if seg[1]})
    raise AssertionError(f"{geo.name}: stream-K on five workgroups cuts no tile up to sixteen stages")


def table_cuts(geos):
    return {geo.name: streamk_cut(geo) for geo in geos if geo.streamk}


def table_extent(geos, cuts):
    """(M, N, every K) of the one operand pair all table cases cut their sub-blocks from."""
    ks = {k for geo in geos for k in rounding_ks(geo)} | {k for k, _ in cuts.values()}
    return max(geo.bm for geo in geos) + EDGE, max(geo.bn for geo in geos) + EDGE, sorted(ks)


def stage_cuts(k, stage, splits):
    """Where the host cuts K into `splits` chunks of whole stages (a K tail rides on the last chunk)."""
    n, per = split_rule(k // stage, splits)
    return [per * stage * i for i in range(1, n)]


class DyadicOperands:
    """One pair of dyadic operands at the largest shape; a case takes a top-left sub-block and the same sub-block of the truth of
    its K (an element of C depends on its row of A and its column of B alone)."""

    def __init__(self, oracle, m, n, ks, seed):
        self.ks = sorted(set(ks))
        self.a, self.b = oracle.dyadic_inputs(m, n, self.ks[-1], np.random.default_rng(seed))
        self.truth = {k: oracle.truth_exact(self.a[:, :k], self.b[:k]) for k in self.ks}

    def sub(self, m, n, k):
        return self.a[:m, :k], self.b[:k, :n], self.truth[k][:m, :n]


def name_the_fault(oracle, a, b, got, truth, cut_sets):
    """Which mutant the differing elements equal: a truncating convert, ties away from zero, partials held in fp16."""
    bad = bits(got) != bits(truth)
    x = oracle.exact_product(a, b)
    mutants = [("RTZ", oracle.round_toward_zero(x)), ("round-half-away", oracle.round_half_away(x))]
    mutants += [(f"fp16-partials (K cut at {cuts})", oracle.fp16_partials(a, b, cuts)) for cuts in cut_sets if cuts]
    said = [f"{int((bits(got)[bad] == bits(mu)[bad]).sum())} of {int(bad.sum())} differing elements equal the {name} mutant" for name, mu in mutants]
    return "; ".join(said) + f"; {int((np.abs(got[bad].astype(np.float64)) < np.abs(x[bad])).sum())} of them lie nearer to zero than the exact sum"


def exact_and_named(f, g, oracle, geo, splits, a, b, truth, what, cut_sets, ld=None, group=2):
    """Findings.exact, and for a wrong result the mutant it matches appended to the finding."""
    got = f.exact(g, geo, splits, a, b, truth, what, ld=ld, group=group)
    if (bits(got) != bits(truth)).any():
        f.lines[-1] += "\n    " + name_the_fault(oracle, a, b, got, truth, cut_sets)
    return got


@pytest.fixture(scope="module")
def table_operands(oracle, geos):
    cuts = table_cuts(geos)
    m, n, ks = table_extent(geos, cuts)
    return DyadicOperands(oracle, m, n, ks, SEED), cuts


def shapes_of(geo, k):
    """(N, strides): wide, narrow, and the wide case at padded strides."""
    return ((geo.bn + EDGE, None), (geo.bn + NARROW, None), (geo.bn + EDGE, (k + 8, k + 24, geo.bn + EDGE + 4)))


@pytest.mark.parametrize("family", FAMILIES)
def test_every_form_of_every_geometry_rounds_to_nearest_even(g, oracle, geos, table_operands, family):
    """M = BM + 24; N = BN + 24 (wide epilogue) and BN + 20 (N % 8 = 4: narrow): a whole tile and a sliver each way, so every lane
    and accumulator register of a tile converts a value that needs rounding.  K = three stages, and two stages + 40 where the
    geometry takes a K tail.  Plain, non-temporal store, two-pass and single-launch split-K in three, stream-K on five
    workgroups, family q's and r's staggered plans; the wide case once more at padded strides (K + 8, K + 24, N + 4).  At three
    stages every form must have run as itself (single-launch split-K as two-pass on a family without that kernel).  Stream-K is
    the one form the host may clamp there (12 K-steps feed three or four workgroups, not five: asserted as stream-K on two or
    more), and at these K it cuts no tile: every segment is a whole tile, stored by the stream-K kernel's direct epilogue.  So
    stream-K runs once more per shape at streamk_cut's K -- on five workgroups, a tile cut between two of them -- where the slab
    stores and the finisher's reduce carry values that need rounding."""
    ops, cuts = table_operands
    f, t0 = Findings(), time.perf_counter()
    members = [geo for geo in geos if geo.family == family]
    assert members
    clamped, cut_runs = set(), 0
    for geo in members:
        m = geo.bm + EDGE
        for k in rounding_ks(geo):
            cut_sets = [stage_cuts(k, geo.stage, 3), stage_cuts(k, geo.stage, 2)]
            for n, ld in shapes_of(geo, k):
                assert (n % 8 == 4) == (n == geo.bn + NARROW)
                a, b, truth = ops.sub(m, n, k)
                for s in rounding_forms(geo):
                    form, d = fast(geo, s, m, n, k, ld)
                    if k == 3 * geo.stage:
                        ok = as_requested(geo, s, form, d)
                        if s & STREAMK and not ok:
                            ok = form == "stream-K" and 2 <= d[1] < (s & SPLIT_MASK)
                            clamped.add(geo.name)
                        assert ok, f"{geo.name}: plan {hex(s)} at {m}x{n}x{k} ld={ld} runs as {form} {d}"
                    exact_and_named(f, g, oracle, geo, s, a, b, truth, f"({form}, {d[3]} splits, grid {d[1]})", cut_sets, ld=ld)
        if geo.streamk:
            k, at = cuts[geo.name]
            s = STREAMK | STREAMK_WGS
            for n, ld in shapes_of(geo, k):
                form, d = fast(geo, s, m, n, k, ld)
                assert as_requested(geo, s, form, d) and d[5] == 4, (geo.name, k, ld, form, d)   # the four tiles streamk_cut cut
                exact_and_named(f, g, oracle, geo, s, *ops.sub(m, n, k), f"({form}, grid {d[1]}, a tile cut at K = {at})", [at], ld=ld)
                cut_runs += 1
    print(f"rounding {family}: stream-K clamped below five workgroups at three stages: {len(clamped)} geometries; "
          f"stream-K runs with a tile cut between workgroups: {cut_runs}")
    f.close(f"rounding {family}: {len(members)} geometries", t0)


def smallest_hybrid_k(geo, m, n, max_k):
    """The smallest K of whole stages at which the launch of one split resolves to the hybrid tail schedule (None: no K does)."""
    for k in range(geo.stage, max_k + 1, geo.stage):
        st, form, disp = resolve(geo.cid, 1, m, n, k, (k, k, n), group=4)
        assert st == 0, (geo.name, k, st)
        if form == "hybrid":
            return k
    return None


def hybrid_case(geo, max_k):
    """(M, N, K) of a geometry's hybrid run: HYBRID_MN where some K <= max_k resolves to the schedule there; where the host's
    cost rule never takes it (half-size tiles leave 66 tail tiles, three K slices each), the shape with 16 tiles more than
    resident workgroups, which it does take."""
    for m, n in (HYBRID_MN, ((geo.grid // 16 + 1) * geo.bm, 16 * geo.bn)):
        k = smallest_hybrid_k(geo, m, n, max_k)
        if k:
            return m, n, k
    raise AssertionError(f"{geo.name}: no K up to {max_k} runs as the hybrid tail schedule")


def test_paths_outside_the_table_round_to_nearest_even(g, oracle, geos):
    """The register-staged any-shape kernel (-2) and the plain-FMA kernel (-1) on shapes no table geometry takes; both entry
    points at their own plans; the hybrid tail schedule of the persistent families (full rounds, K-split tail tiles, the tail
    reduce over fp32 slabs) at the smallest K that resolves to it, contiguous and at ldc = N + 4."""
    f, t0 = Findings(), time.perf_counter()
    rng = np.random.default_rng(SEED + 1)
    for cid, name in ((-2, "ragged"), (-1, "generic")):
        special = Geo(name, cid, "", 0, 0, 0, 0, False, False, 0)
        for m, n, k in ((65, 30, 100), (129, 67, 257)):
            st, form, _ = resolve(cid, 1, m, n, k, (k, k, n), group=1)
            assert st == 0 and form == ("ragged" if cid == -2 else "reference"), (name, st, form)
            a, b = oracle.dyadic_inputs(m, n, k, rng)
            exact_and_named(f, g, oracle, special, 1, a, b, oracle.truth_exact(a, b), f"({form})", [], group=1)
    for m, n, k in ((64, 64, 64), (256, 256, 512), (200, 136, 192)):
        a, b = oracle.dyadic_inputs(m, n, k, rng)
        truth = oracle.truth_exact(a, b)
        for entry in ("fp32", "fp16"):
            got = g.gemm(a, b, entry=entry)
            f.runs += 1
            bad = bits(got) != bits(truth)
            f.check(not bad.any(), f"entry {entry} {m}x{n}x{k}: {int(bad.sum())} of {bad.size} elements differ\n    "
                    + (name_the_fault(oracle, a, b, got, truth, [[k // 2]]) if bad.any() else ""))
    # the hybrid tail: its truth is the fp32 BLAS product (tests/test_oracle.py: equal to truth_exact for this class)
    members = [geo for geo in geos if geo.name in HYBRID_GEOMETRIES]
    assert len(members) == len(HYBRID_GEOMETRIES), [geo.name for geo in members]
    ks = {geo.name: hybrid_case(geo, oracle.DYADIC_MAX_K) for geo in members}
    assert any(case[:2] == HYBRID_MN for case in ks.values())
    a, b = oracle.dyadic_inputs(*(max(case[i] for case in ks.values()) for i in range(3)), rng)
    oracle.assert_dyadic(a, b)
    truths = {(m, n, k): oracle.truth_numpy(a[:m, :k], b[:k, :n]) for m, n, k in set(ks.values())}
    for geo in members:
        m, n, k = ks[geo.name]
        for ld in (None, (k, k, n + 4)):
            st, form, disp = resolve(geo.cid, 1, m, n, k, ld or (k, k, n), group=4)
            assert st == 0 and form == "hybrid" and len(disp) == 3, (geo.name, k, ld, st, form, disp)
            tail = disp[1]
            cuts = list(range(tail[4], k, tail[4]))
            exact_and_named(f, g, oracle, geo, 1, a[:m, :k], b[:k, :n], truths[m, n, k], f"(hybrid, tail of {tail[5]} items in {tail[3]} K slices)", [cuts], ld=ld, group=4)
    print(f"hybrid M, N, K: {ks}")
    f.close("rounding outside the table", t0)
