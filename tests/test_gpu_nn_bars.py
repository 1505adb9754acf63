"""GPU tests that hold family "n" (the NN layout, hgemm_kernel_nn.hpp and its host path in hgemm_api.hip) to the bars the other
families are held to (run with `-m gpu` on an MI355X); tests/test_gpu_nn.py is the family's first look, whose fixtures and helpers
these tests use.

1. Rounding: dyadic operands (oracle.dyadic_inputs), bit-exact against oracle.truth_exact -- the hand-written fp16 epilogue
   (convert, v_permlane16_swap, 16-byte buffer store and its non-temporal twin), the slab epilogue + reduce of the two-pass form,
   both planned entries (the planned SPLIT path) and the reference kernel.  tests/test_oracle.py proves on the CPU, for these
   very operands, that the truth is order-independent and that each mutant shows in every 16 x 16 block of every case.
2. Special values: inf, NaN, -0, denormal operands and results, overflow at 65520, in rows of A AND in rows of B (the operand of
   the transposed reads), against the reference's CPU expression.
3. The 32-bit reach rule of TrLayout::reach_ok, executed on both sides of its edge for A, B and C.
4. Rasters of more than eight tile rows (group_m = 8 with a ragged last group), split items across them.
5. The workspace behaviour of hgemm_mi355x_launch_nn: capture without and with a reserved workspace, a lent buffer, two streams.
6. Misaligned A, B or C: the reference kernel answers.

Every comparison is bit-exact and unmasked, C prefilled with NaN and every padding element compared (gemm_nn); section 2 compares
the NaN pattern and the bits of everything else against a C prefilled with 7.0, as test_special_values_round_like_the_reference."""
import ctypes
import time

import numpy as np
import pytest
import torch

from test_gpu_nn import FORMS, MEMBERS, NT_STORE, bits, check_exact, gemm_nn
from test_gpu_nn import L, g, members, oracle  # noqa: F401  (the first look's fixtures: GPU helpers, the library, the CPU oracle)
from test_gpu_parity import special_value_operands
from test_gpu_rounding import DyadicOperands, name_the_fault
from test_gpu_strides import all_bits_equal

pytestmark = pytest.mark.gpu

GIB = 1 << 30
BK = 64                                   # K of one stage
FORM_REFERENCE, FORM_SPLITK, FORM_PLAIN = 0, 3, 6            # hgemm_api.hip: enum Form
COUNTER_BYTES = 256 << 10                 # the counter block in front of the slabs (hgemm_plan.hpp)

# ---- 1. rounding -------------------------------------------------------------------------------------------------------------------
SEED = 601                                # of the member operands (tests/test_oracle.py draws the same)
PLANNED_SEED = 602                        # of the planned entries' operands
EDGE, NARROW = 24, 20                     # M = BM + 24; N = BN + 24: a whole tile and an 8-column sliver; BN + 20: N % 8 = 4, outside the kernel
ROUNDING_FORMS = (1, 1 | NT_STORE, 2, 3, 5)
LONG = (64, 64, 8128)                     # 127 stages: the largest multiple of 64 within oracle.DYADIC_MAX_K
LONG_FORMS = (1, 5)
PLANNED = ((256, 264, 512, 8), (200, 136, 192, 3))           # (M, N, K, the splits tr_model_plan gives the 64 x 64 member)


def nn_infos(lib):
    """[(name, id, BM, BN, NBUF)] of the family's members, from any handle of the library (no GPU)."""
    lib.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    out = []
    for name in MEMBERS:
        cid = lib.hgemm_mi355x_nn_config_by_name(name.encode())
        info = (ctypes.c_int * 8)()
        assert cid >= 0 and lib.hgemm_mi355x_nn_config_info(cid, info) == 0, name
        out.append((name, cid, info[0], info[1], info[5]))
    return out


def two_pass(k, word):
    """(splits, K per chunk) of the two-pass form, tr_resolve's clamp rule: at most one split per stage, per = ceil(steps / splits)
    stages per chunk, no empty chunk."""
    steps = k // BK
    splits = max(1, min(word & 0xFFFF, steps))
    per = -(-steps // splits)
    return -(-steps // per), per * BK


def two_pass_cuts(k, word):
    splits, chunk = two_pass(k, word)
    return [chunk * i for i in range(1, splits)]


def member_ks(nbuf):
    """Three stages; NBUF + 1 stages: the ring wraps."""
    return (3 * BK, (nbuf + 1) * BK)


def member_extent(infos):
    """(M, N, every K) of the one operand pair all member cases cut their sub-blocks from."""
    ks = {k for *_, nbuf in infos for k in member_ks(nbuf)} | {LONG[2]}
    return max(bm for _, _, bm, _, _ in infos) + EDGE, max(bn for _, _, _, bn, _ in infos) + EDGE, sorted(ks)


def member_cases(infos):
    """{(M, N, K): the cut sets of the forms run there} of every member case below (tests/test_oracle.py proves the operands on it)."""
    cases = {}
    for _, _, bm, bn, nbuf in infos:
        for k in member_ks(nbuf):
            cases.setdefault((bm + EDGE, bn + EDGE, k), set()).update(tuple(two_pass_cuts(k, w)) for w in ROUNDING_FORMS if w & 0xFFFF > 1)
        cases.setdefault((bm + EDGE, bn + NARROW, 3 * BK), set())                    # the reference kernel: no cut
    cases.setdefault(LONG, set()).update(tuple(two_pass_cuts(LONG[2], w)) for w in LONG_FORMS if w > 1)
    return {shape: sorted(cuts) for shape, cuts in cases.items()}


def planned_cases():
    return {(m, n, k): [tuple(two_pass_cuts(k, splits))] for m, n, k, splits in PLANNED}


def planned_extent():
    return max(c[0] for c in PLANNED), max(c[1] for c in PLANNED), sorted({c[2] for c in PLANNED})


def decision(L, cid, word, m, n, k, ld=None, aligned=True):
    """What hgemm_mi355x_launch_nn decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    st = L.hgemm_mi355x_selfcheck_launch_nn(cid, word, 4 if aligned else 0, m, n, k, *(ld or (k, n, n)), 0, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def runs_as_requested(L, cid, word, m, n, k, ld=None):
    """Plain for a split count of 1, else two-pass with the split count and chunk the clamp rule gives."""
    st, form, disp = decision(L, cid, word, m, n, k, ld)
    splits, chunk = two_pass(k, word)
    if splits == 1:
        return st == 0 and form == FORM_PLAIN and len(disp) == 1 and disp[0][3:] == (1, k)
    return st == 0 and form == FORM_SPLITK and len(disp) == 2 and disp[0][3:] == (splits, chunk)


@pytest.fixture(scope="module")
def infos(L):
    return nn_infos(L)


@pytest.fixture(scope="module")
def member_operands(oracle, infos):
    m, n, ks = member_extent(infos)
    return DyadicOperands(oracle, m, n, ks, SEED)


class Rounding:
    """Runs of one test: every wrong result is kept with the mutant it matches, and all of them fail the test at the end."""

    def __init__(self, g, L, oracle):
        self.g, self.L, self.oracle, self.lines, self.runs, self.t0 = g, L, oracle, [], 0, time.perf_counter()

    def run(self, what, a, b, truth, cut_sets, **how):
        got = gemm_nn(self.g, self.L, a, b, **how)
        self.runs += 1
        bad = bits(got) != bits(truth)
        if bad.any():
            self.lines.append(f"{what} {a.shape[0]}x{b.shape[1]}x{a.shape[1]} ld={how.get('ld')}: {int(bad.sum())} of {bad.size} elements differ\n    "
                              + name_the_fault(self.oracle, a, b, got, truth, cut_sets))

    def close(self, what):
        print(f"{what}: {self.runs} runs, {len(self.lines)} wrong, {time.perf_counter() - self.t0:.2f} s")
        assert not self.lines, f"{what}: {len(self.lines)} of {self.runs} runs are not round-to-nearest-even:\n" + "\n".join(self.lines)


@pytest.mark.parametrize("member", MEMBERS)
def test_every_form_of_every_member_rounds_to_nearest_even(g, L, oracle, infos, member_operands, member):
    """M = BM + 24, N = BN + 24: a whole tile and a sliver each way, so every lane and accumulator register of a tile converts a
    value that needs rounding, through the plain store, its non-temporal twin and the slab epilogue + reduce (2, 3 and 5 splits,
    clamped to one per stage).  K = three stages and NBUF + 1 stages (the ring wraps); the three-stage case once more at padded
    strides (K + 8, N + 24, N + 16).  Each form must have run as requested.  N = BN + 20 is outside the kernel: the reference
    kernel answers, and must round the same way."""
    name, cid, bm, bn, nbuf = next(i for i in infos if i[0] == member)
    r = Rounding(g, L, oracle)
    m, n = bm + EDGE, bn + EDGE
    assert n % 8 == 0 and bm < m < 2 * bm and bn < n < 2 * bn
    for k, ld in [(k, None) for k in member_ks(nbuf)] + [(3 * BK, (3 * BK + 8, n + 24, n + 16))]:
        a, b, truth = member_operands.sub(m, n, k)
        assert L.hgemm_mi355x_nn_runs(cid, m, n, k, *(ld or (k, n, n))) == 1
        for word in ROUNDING_FORMS:
            assert runs_as_requested(L, cid, word, m, n, k, ld), (name, hex(word), k, ld, decision(L, cid, word, m, n, k, ld))
            cuts = [two_pass_cuts(k, word)] if word & 0xFFFF > 1 else sorted({tuple(two_pass_cuts(k, w)) for w in (2, 3)})
            r.run(f"{name} plan {hex(word)}", a, b, truth, cuts, plan=(cid, word), ld=ld)
    n, k = bn + NARROW, 3 * BK
    assert L.hgemm_mi355x_nn_runs(cid, m, n, k, k, n, n) == 0 and decision(L, cid, 1, m, n, k)[:2] == (0, FORM_REFERENCE)
    a, b, truth = member_operands.sub(m, n, k)
    for word in (1, 4):
        r.run(f"{name} plan {hex(word)} (reference kernel)", a, b, truth, [], plan=(cid, word))
    r.close(f"rounding {name}")
    assert r.runs == 3 * len(ROUNDING_FORMS) + 2


def test_long_k_rounds_to_nearest_even(g, L, oracle, infos, member_operands):
    """64 x 64 x 8128: 127 stages, sums up to a few hundred where fp16 spacing is 2^-4 ... 2^-2; plain, and five chunks of 26 / 23
    stages through the slabs."""
    m, n, k = LONG
    assert k % BK == 0 and k <= oracle.DYADIC_MAX_K < k + BK
    a, b, truth = member_operands.sub(m, n, k)
    r = Rounding(g, L, oracle)
    for name, cid, *_ in infos:
        for word in LONG_FORMS:
            assert runs_as_requested(L, cid, word, m, n, k), (name, word)
            r.run(f"{name} plan {hex(word)}", a, b, truth, [two_pass_cuts(k, 5)], plan=(cid, word))
    assert two_pass(k, 5) == (5, 26 * BK)
    r.close("rounding long K")
    assert r.runs == len(MEMBERS) * len(LONG_FORMS)


def test_the_planned_entries_round_to_nearest_even_through_their_split_plans(g, L, oracle):
    """hgemm_mi355x_nn_fp32 / _fp16 at two shapes whose 64 x 64 tiles do not fill the chip: the planner splits (8 and 3 ways), so the
    planned split path -- tr_model_plan's split branch, the stream workspace, the slab epilogue and the reduce -- carries values
    that need rounding."""
    ops = DyadicOperands(oracle, *planned_extent(), PLANNED_SEED)
    r = Rounding(g, L, oracle)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for m, n, k, want in PLANNED:
        assert L.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0
        assert MEMBERS[cfg.value] == "n64x64_w2x2" and splits.value == want > 1, (m, n, k, cfg.value, splits.value)
        assert runs_as_requested(L, cfg.value, splits.value, m, n, k) and two_pass(k, want)[0] == want
        a, b, truth = ops.sub(m, n, k)
        for entry in ("fp32", "fp16"):
            r.run(f"entry {entry} ({want} splits)", a, b, truth, planned_cases()[m, n, k], entry=entry)
    r.close("rounding planned entries")
    assert r.runs == 2 * len(PLANNED)


# ---- 2. special values -------------------------------------------------------------------------------------------------------------
def nn_special_operands(n):
    """special_value_operands at 128 x n x 512 (hot = 300), plus rows of B that carry specials -- in the NN form B's values sit in the
    operand of the transposed reads -- which gives C a column pattern next to the row pattern.  Row 3 of B: -0.0 in even columns.
    Row 4 of B: the denormal 2^-24 in columns = 3 mod 16.  The matching A entries keep every product and sum exact in fp32."""
    m, k, hot = 128, 512, 300
    a, b = special_value_operands(m, n, k, hot)
    b[3, 0::2] = -0.0
    b[4, 3::16] = 2.0 ** -24
    a[15, 3] = 1.0                                     # 1 x -0 joins a sum of +0 terms: +0, in every column
    a[16, 3] = 1.0; a[16, 2] = 2.0 ** -14              # 2^-24 + -0
    a[17, 4] = 1.0                                     # a denormal operand of B, a denormal result: 2^-24 in columns 3 mod 16
    a[18, 4] = 0.5                                     # 2^-25: the tie between 0 and 2^-24 rounds to even = 0
    a[19, 4] = 1.5                                     # 1.5 x 2^-24: the tie between 2^-24 and 2^-23 rounds to even = 2^-23
    a[20, 4] = 1024.0                                  # 2^-14: a normal result from a denormal operand
    a[21, 4] = float("inf")                            # inf in columns 3 mod 16, inf x 0 = NaN in every other column
    a[22, 3] = 1.0; a[22, 4] = -1.0                    # -0 - 2^-24 / +0 - 0
    a[23, 4] = 65504.0                                 # 65504 x 2^-24, rounded once
    a[64:, :] = a[:64, :].clone()
    truth = (a.float() @ b.float()).half()
    z = torch.zeros(n, dtype=torch.half)
    col = torch.arange(n) % 16 == 3
    assert torch.equal(truth[15].view(torch.int16), z.view(torch.int16)) and (truth[16] == 2.0 ** -24).all()
    assert torch.equal(truth[17], torch.where(col, 2.0 ** -24, 0.0).half()) and (truth[18] == 0).all()
    assert torch.equal(truth[19], torch.where(col, 2.0 ** -23, 0.0).half()) and torch.equal(truth[20], torch.where(col, 2.0 ** -14, 0.0).half())
    assert torch.equal(torch.isinf(truth[21]), col) and torch.equal(torch.isnan(truth[21]), ~col)
    assert torch.equal(truth[22], torch.where(col, -2.0 ** -24, 0.0).half())
    assert torch.isinf(truth[1]).all() and truth[2, 0] == 65504 and torch.isnan(truth[4, 5]) and truth[9, 0] == 0 and truth[13, 0] == 2048
    assert torch.equal(truth[64:].view(torch.int16), truth[:64].view(torch.int16))
    return a, b, truth


def specials_differ(got, truth):
    """None, or how `got` differs from the reference: the NaN pattern, then the bits of everything else."""
    if not torch.equal(torch.isnan(got), torch.isnan(truth)):
        return f"NaN pattern differs from the reference in {int((torch.isnan(got) != torch.isnan(truth)).sum())} elements"
    same = torch.where(torch.isnan(truth), torch.zeros_like(truth), truth).view(torch.int16) == torch.where(torch.isnan(got), torch.zeros_like(got), got).view(torch.int16)
    bad = (~same).nonzero()
    if bad.numel():
        return f"{bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()} want {truth[tuple(bad[0])].item()}"
    return None


@pytest.mark.parametrize("n", [192, 200])
def test_special_values_round_like_the_reference_in_the_nn_layout(g, L, members, n):
    """n = 192: every member x every form, and both planned entries, contiguous.  n = 200 is ragged against both tile widths; the
    members run at ldb = n + 24 with B's padding holding alternating +inf and NaN (it enters the LDS image of the edge tiles, and
    must only meet accumulators that are never stored), the planned entries contiguous.  B is compared bit for bit afterwards."""
    m, k = 128, 512
    a, b, truth = nn_special_operands(n)
    ldb = n if n == 192 else n + 24
    ad = a.cuda()
    bd = torch.empty((k, ldb), dtype=torch.half, device="cuda")
    bd[:, 0::2] = float("inf")
    bd[:, 1::2] = float("nan")
    bd[:, :n] = b.cuda()
    before = bd.clone()
    bc = b.cuda()
    plans = [(f"{name}/{word:#x}", (cid, word)) for name, cid in members for word in FORMS] + [("entry fp32", None), ("entry fp16", None)]
    for label, plan in plans:
        c = torch.full((m, n), 7.0, dtype=torch.half, device="cuda")
        if plan is None:
            fn = L.hgemm_mi355x_nn_fp16 if label.endswith("fp16") else L.hgemm_mi355x_nn_fp32
            st = fn(ad.data_ptr(), bc.data_ptr(), c.data_ptr(), m, n, k, g.stream())
        else:
            assert L.hgemm_mi355x_nn_runs(plan[0], m, n, k, k, ldb, n) == 1
            st = L.hgemm_mi355x_launch_nn(plan[0], plan[1], ad.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, k, ldb, n, g.stream())
        assert st == 0, label
        torch.cuda.synchronize()
        said = specials_differ(c.cpu(), truth)
        assert said is None, f"{label} (n = {n}, ldb = {ldb}): {said}"
    assert torch.equal(bd.view(torch.int16), before.view(torch.int16)) and torch.equal(bc.view(torch.int16), b.cuda().view(torch.int16))
    print(f"special values n = {n}: {len(plans)} runs")


# ---- 3. the reach rule, both sides executed ----------------------------------------------------------------------------------------
def largest_nn_stride(lib, cid, m, n, k, side):
    """The largest stride (a multiple of 8) of operand `side` (0: A, 1: B, 2: C) at which the member's kernel still runs, the other two
    contiguous -- by bisection over hgemm_mi355x_nn_runs, which is monotone in the stride."""
    def runs(s):
        lds = [k, n, n]
        lds[side] = s
        return lib.hgemm_mi355x_nn_runs(cid, m, n, k, *lds) == 1

    lo, hi = (k, n, n)[side] // 8, 1 << 27             # 8 x 2^27 = 2^30 elements: beyond the reach of every member and K >= 64
    assert runs(8 * lo) and not runs(8 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if runs(8 * mid) else (lo, mid)
    return 8 * lo


def reach_rule(bm, m, n, k, side):
    """(rows, tail bytes) of TrLayout::reach_ok's limit on operand `side`: rows x ld x 2 + tail < 2 GiB.  A and C are addressed from a tile's
    first row (BM rows, then the row's K or N elements), B from row 0 to the end of the matrix (K - 1 rows, then N elements)."""
    return ((bm, 2 * k), (k - 1, 2 * n), (bm, 2 * n))[side]


REACH_CASES = [  # (member, M, N, K, operand (0: A, 1: B, 2: C))
    ("n128x128_w2x2", 128 + 8, 64, 128, 0),            # a second row band whose base lies just below the limit, ragged
    ("n64x64_w2x2", 64, 64 + 8, 128, 1),               # a second column tile, descriptor base n0 = 64: the last k-row's sliver ends with the descriptor
    ("n64x128_w2x2", 64 + 8, 136, 128, 2),             # the C descriptor of the buffer stores; the reduce's 64-bit stores in the split form
]


@pytest.mark.parametrize("case", REACH_CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1:4]))}-{'ABC'[c[4]]}")
def test_nn_reach_edges_run_exact_on_both_sides(g, L, oracle, infos, case):
    """The largest stride at which the member's kernel still runs and the next multiple of 8 (the reference kernel, 64-bit
    addressing), both executed, plain and in two splits.  The operand lives in a flat buffer filled with NaN (C: with -3.0) that
    must come back unchanged outside the operand's window."""
    name, m, n, k, side = case
    _, cid, bm, bn, _ = next(i for i in infos if i[0] == name)
    s = largest_nn_stride(L, cid, m, n, k, side)
    rows_rule, tail = reach_rule(bm, m, n, k, side)
    assert rows_rule * s * 2 + tail < 2 * GIB <= rows_rule * (s + 8) * 2 + tail, (s, rows_rule, tail)     # the documented rule
    a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(s % 100003))
    truth = torch.from_numpy(oracle.truth_numpy(a_np, b_np))
    rows, cols = [(m, k), (k, n), (m, n)][side]
    pad_value = -3.0 if side == 2 else float("nan")
    flat = torch.full((rows * (s + 8),), pad_value, dtype=torch.half, device="cuda")
    a, b = torch.from_numpy(a_np).cuda(), torch.from_numpy(b_np).cuda()
    ran = 0
    for stride, runs in ((s, 1), (s + 8, 0)):
        lds = [k, n, n]
        lds[side] = stride
        assert L.hgemm_mi355x_nn_runs(cid, m, n, k, *lds) == runs
        window = flat.as_strided((rows, cols), (stride, 1))
        for word in (1, 2):
            st, form, disp = decision(L, cid, word, m, n, k, lds)
            assert (st, form) == (0, FORM_REFERENCE if not runs else FORM_PLAIN if word == 1 else FORM_SPLITK), (stride, word, st, form)
            assert not runs or disp[0][3] == word
            c = torch.full((m, n), float("nan"), dtype=torch.half, device="cuda")
            if side == 2:
                window.fill_(float("nan"))
                c = window
            else:
                window.copy_([a, b][side])
            ops = [a, b, c]
            ops[side] = flat
            st = L.hgemm_mi355x_launch_nn(cid, word, ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), m, n, k, *lds, g.stream())
            assert st == 0, L.hgemm_mi355x_strerror(st)
            torch.cuda.synchronize()
            got = c.contiguous().cpu()
            assert torch.equal(got.view(torch.int16), truth.view(torch.int16)), (name, "ABC"[side], stride, word, int((got.view(torch.int16) != truth.view(torch.int16)).sum()))
            window.fill_(pad_value)
            assert all_bits_equal(flat, pad_value), (name, "ABC"[side], stride, word, "the buffer changed outside the operand's window")
            ran += 1
    print(f"reach {name} {'ABC'[side]}: edge stride {s}, {ran} runs, buffer {flat.numel() * 2 / 1e9:.2f} GB")
    del flat, window, c
    torch.cuda.empty_cache()


# ---- 4. rasters of more than eight tile rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1160, 136, 128), (520, 1096, 64)])
def test_rasters_of_more_than_eight_tile_rows_are_exact(g, L, oracle, infos, members, shape):
    """group_m = min(tiles_m, 8): (1160, 136, 128) has 19 / 10 tile rows -- two whole groups and a ragged third, ragged M, split
    items walking the same raster; (520, 1096, 64) has 9 / 5 tile rows against 18 / 9 column tiles and one stage, so every split
    count is clamped to 1."""
    m, n, k = shape
    tiles_m = {name: -(-m // bm) for name, _, bm, _, _ in infos}
    assert all(tiles_m[name] > 8 and tiles_m[name] % 8 for name, _, bm, _, _ in infos if bm == 64), tiles_m
    for name, cid, *_ in infos:
        for word in FORMS:
            assert runs_as_requested(L, cid, word, m, n, k), (name, hex(word))
    assert check_exact(g, L, oracle, members, m, n, k, seed=m + n + k)[0] == len(MEMBERS) * len(FORMS)


# ---- 5. the workspace behaviour of hgemm_mi355x_launch_nn ---------------------------------------------------------------------------
WS_SHAPE = (200, 264, 512)
WS_SPLITS = 4


@pytest.fixture(scope="module")
def W(L):
    L.hgemm_mi355x_nn_reserve_workspace.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    L.hgemm_mi355x_set_workspace.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    return L


def replays_exactly(oracle, graph, bufs, seeds):
    """Replays a captured chain of GEMMs on NEW operand values written into the captured buffers; the labels of the wrong results."""
    m, n, k = WS_SHAPE
    wrong = []
    for seed in seeds:
        truths = []
        for i, (a, b, c) in enumerate(bufs):
            a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(1000 * seed + i))
            a.copy_(torch.from_numpy(a_np)); b.copy_(torch.from_numpy(b_np))
            c.fill_(float("nan"))
            truths.append(oracle.truth_numpy(a_np, b_np))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        wrong += [(seed, i) for i, ((_, _, c), truth) in enumerate(zip(bufs, truths)) if not np.array_equal(bits(c.cpu().numpy()), bits(truth))]
    return wrong


def device_buffers(count):
    m, n, k = WS_SHAPE
    return [(torch.empty((m, k), dtype=torch.half, device="cuda"), torch.empty((k, n), dtype=torch.half, device="cuda"),
             torch.empty((m, n), dtype=torch.half, device="cuda")) for _ in range(count)]


def test_a_split_call_captured_without_a_workspace_runs_unsplit(g, W, oracle, members):
    """Nothing may be allocated while a stream captures: a split call on a fresh stream with nothing reserved returns 0, runs without
    the two-pass form (hgemm_mi355x_launch_nn resolves again with that form ruled out) and replays exactly.  One stream, one chain."""
    m, n, k = WS_SHAPE
    for name, cid in members:
        assert decision(W, cid, WS_SPLITS, m, n, k)[1] == FORM_SPLITK and W.hgemm_mi355x_nn_plan_workspace_bytes(cid, WS_SPLITS, m, n, k) > COUNTER_BYTES
    bufs = device_buffers(len(members))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rcs = []
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        for (name, cid), (a, b, c) in zip(members, bufs):
            rcs.append(W.hgemm_mi355x_launch_nn(cid, WS_SPLITS, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, k, n, n, st))
    assert rcs == [0] * len(members), rcs
    assert replays_exactly(oracle, graph, bufs, (1, 2)) == []


def test_the_planned_split_call_captures_after_the_nn_reserve_call(g, W, oracle):
    """hgemm_mi355x_nn_reserve_workspace sizes the stream's workspace for the plan hgemm_mi355x_nn_fp32 will take (8 splits here), so the
    capture finds it and the graph holds the slab epilogue and the reduce."""
    m, n, k = WS_SHAPE
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert W.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value > 1
    assert W.hgemm_mi355x_nn_plan_workspace_bytes(cfg.value, splits.value, m, n, k) == COUNTER_BYTES + splits.value * m * n * 4
    s = torch.cuda.Stream()
    assert W.hgemm_mi355x_nn_reserve_workspace(m, n, k, s.cuda_stream) == 0
    bufs = device_buffers(2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rcs = []
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        for fn, (a, b, c) in zip((W.hgemm_mi355x_nn_fp32, W.hgemm_mi355x_nn_fp16), bufs):
            rcs.append(fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, st))
    assert rcs == [0, 0], rcs
    assert replays_exactly(oracle, graph, bufs, (1, 2)) == []


def test_a_lent_workspace_too_small_runs_unsplit_and_one_of_the_plan_size_runs_split(g, W, oracle, members):
    """The lent buffer is filled with a byte pattern no slab holds (0xA5A5A5A5 is a negative fp32 below 1e-15; a 0/1 partial sum is a
    non-negative integer).  Too small for the slabs: the result is exact and the bytes behind the counters are untouched, so the
    plan ran unsplit.  hgemm_mi355x_nn_plan_workspace_bytes: exact, and every fp32 of the four slabs has been written."""
    m, n, k = WS_SHAPE
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(31))
    truth = oracle.truth_numpy(a, b)
    try:
        for name, cid in members:
            need = int(W.hgemm_mi355x_nn_plan_workspace_bytes(cid, WS_SPLITS, m, n, k))
            assert need == COUNTER_BYTES + WS_SPLITS * m * n * 4
            for size, split in ((COUNTER_BYTES + 1024, False), (need, True)):
                buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
                assert W.hgemm_mi355x_set_workspace(buf.data_ptr(), size) == 0
                got = gemm_nn(g, W, a, b, plan=(cid, WS_SPLITS))
                assert np.array_equal(bits(got), bits(truth)), (name, size)
                slabs = buf[COUNTER_BYTES:]
                if split:
                    words = slabs.view(torch.int32)
                    assert int((words == words.new_tensor(0xA5A5A5A5 - (1 << 32))).sum()) == 0, (name, "a slab element was not written: the plan did not run split")
                else:
                    assert bool((slabs == 0xA5).all()), (name, "the plan wrote behind a buffer too small for its slabs")
                assert W.hgemm_mi355x_set_workspace(None, 0) == 0
    finally:
        assert W.hgemm_mi355x_set_workspace(None, 0) == 0
    assert np.array_equal(bits(gemm_nn(g, W, a, b, plan=(members[0][1], WS_SPLITS))), bits(truth))


def test_nn_split_k_on_two_streams_does_not_share_partials(g, W, oracle, members):
    """The same split plan on two streams at once, different operands: each stream has slabs of its own."""
    m, n, k = WS_SHAPE
    rng = np.random.default_rng(41)
    probs = []
    for _ in range(2):
        a_np, b_np = oracle.zero_one_inputs(m, n, k, rng)
        probs.append((torch.from_numpy(a_np).cuda(), torch.from_numpy(b_np).cuda(), oracle.truth_numpy(a_np, b_np)))
    assert not np.array_equal(probs[0][2], probs[1][2])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for name, cid in members:
        assert decision(W, cid, WS_SPLITS, m, n, k)[1] == FORM_SPLITK
        outs = [torch.full((m, n), float("nan"), dtype=torch.half, device="cuda") for _ in probs]
        for rep in range(20):
            for (a, b, _), st, c in zip(probs, streams, outs):
                assert W.hgemm_mi355x_launch_nn(cid, WS_SPLITS, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, k, n, n, st.cuda_stream) == 0
        torch.cuda.synchronize()
        for i, ((_, _, truth), c) in enumerate(zip(probs, outs)):
            assert np.array_equal(bits(c.cpu().numpy()), bits(truth)), (name, i)


# ---- 6. misaligned pointers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1, 2], ids=["A", "B", "C"])
def test_a_misaligned_pointer_is_answered_exactly_by_the_reference_kernel(g, L, oracle, members, side):
    """One operand starts 4 elements (8 bytes) into a larger tensor, strides unchanged: 8-byte aligned, not 16.  Status 0, exact, and
    the backing tensor unchanged around the operand -- whatever split count is named."""
    m, n, k = 200, 136, 128
    off = 4
    a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(60 + side))
    truth = oracle.truth_f32acc(a_np, b_np)
    shapes = [(m, k), (k, n), (m, n)]
    fills = [float("nan"), float("nan"), g.C_PAD]
    for name, cid in members:
        assert L.hgemm_mi355x_nn_runs(cid, m, n, k, k, n, n) == 1 and decision(L, cid, 1, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
        for word in (1, 4):
            flats, views = [], []
            for i, (rows, cols) in enumerate(shapes):
                lead = off if i == side else 0
                flat = torch.full((rows * cols + 2 * off,), fills[i], dtype=torch.half, device="cuda")
                view = flat[lead:lead + rows * cols].view(rows, cols)
                assert view.data_ptr() % 16 == (8 if i == side else 0)
                flats.append(flat); views.append(view)
            views[0].copy_(torch.from_numpy(a_np)); views[1].copy_(torch.from_numpy(b_np)); views[2].fill_(float("nan"))
            before = [f.clone() for f in flats]
            st = L.hgemm_mi355x_launch_nn(cid, word, views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), m, n, k, k, n, n, g.stream())
            assert st == 0, (name, word, L.hgemm_mi355x_strerror(st))
            torch.cuda.synchronize()
            assert np.array_equal(bits(views[2].cpu().numpy()), bits(truth)), (name, word, "ABC"[side])
            views[2].fill_(float("nan"))
            for f, was in zip(flats, before):
                assert torch.equal(f.view(torch.int16), was.view(torch.int16)), (name, word, "ABC"[side], "the backing tensor changed")


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the fp16 NN set (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit."""
    sets = [g.HelperKernelSet(lambda cfg, word, p, d, acc: L.hgemm_mi355x_launch_nn(cfg, word, p["a"], p["b"], p["c"], *d[:6], g.stream()),
                              lambda cfg, word, d, aligned, acc: decision(L, cfg, word, *d[:3], d[3:6], aligned), torch.float16)]
    for s in sets:
        s.check_combine(128, 2, 9101)
        s.check_combine(704, 11, 9101 + 1)
        s.check_reference(9101 + 2)
