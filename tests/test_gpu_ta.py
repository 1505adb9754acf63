"""GPU tests of family "a" (run with `-m gpu` on an MI355X): the TA layout -- A given as a_col_major [K][lda] (M contiguous), B row-major,
both staged as they lie in memory and read through ds_read_b64_tr_b16 (hgemm_kernel_ta.hpp) -- through the C ABI against the CPU oracle.

Bar: 0/1 and dyadic inputs BIT-EXACT AND UNMASKED (tests/test_gpu_nn.py states why the sums are exact in any order); N(0,1) inputs
oracle.relative_error <= 1e-3, the project's REL_TOL.  Device operands as in test_gpu_nn.gemm_nn: a_col_major = a.T placed in a
[K][lda] buffer whose padding columns hold NaN, B in [K][ldb] likewise, C's padding holds gpu_common.C_PAD, and every padding element
must come back bit-unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_nn import NT_STORE, REL_TOL, bits, truth_of
from test_gpu_nn import g, oracle  # noqa: F401  (fixtures: the GPU helpers, the CPU oracle)
from test_ta_host import largest_ta_stride, reach_limit, reach_rule

pytestmark = pytest.mark.gpu

MEMBERS = ("a64x64_w2x2", "a128x64_w2x2", "a64x128_w2x2", "a128x128_w2x2")
FORMS = (1, 1 | NT_STORE, 2, 5)   # plain, non-temporal stores, two-pass splits 2 / 5 (clamped to one split per K stage)
GIB = 1 << 30
BK = 64
FORM_REFERENCE, FORM_SPLITK, FORM_PLAIN = 0, 3, 6            # hgemm_api.hip: enum Form
COUNTER_BYTES = 256 << 10


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    lib.hgemm_mi355x_ta_config_name.restype = ctypes.c_char_p
    lib.hgemm_mi355x_ta_config_by_name.argtypes = [ctypes.c_char_p]
    lib.hgemm_mi355x_launch_ta.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    lib.hgemm_mi355x_ta_fp32.argtypes = lib.hgemm_mi355x_ta_fp16.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.hgemm_mi355x_ta_plan_workspace_bytes.restype = ctypes.c_size_t
    lib.hgemm_mi355x_ta_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    lib.hgemm_mi355x_ta_reserve_workspace.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.hgemm_rocblas_ta.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    ids = [L.hgemm_mi355x_ta_config_by_name(nm.encode()) for nm in MEMBERS]
    assert all(i >= 0 for i in ids), f"family a members missing from the library: {list(zip(MEMBERS, ids))}"
    return list(zip(MEMBERS, ids))


@pytest.fixture(scope="module")
def infos(L, members):
    out = []
    for name, cid in members:
        info = (ctypes.c_int * 8)()
        assert L.hgemm_mi355x_ta_config_info(cid, info) == 0
        out.append((name, cid, info[0], info[1], info[5]))   # (name, id, BM, BN, NBUF)
    return out


def decision(L, cid, word, m, n, k, ld=None, aligned=True):
    """What hgemm_mi355x_launch_ta decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    st = L.hgemm_mi355x_selfcheck_launch_ta(cid, word, 4 if aligned else 0, m, n, k, *(ld or (m, n, n)), 0, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def two_pass_cuts(k, word):
    """K cuts of the two-pass form: at most one split per stage, ceil(steps / splits) stages per chunk, no empty chunk."""
    steps = k // BK
    splits = max(1, min(word & 0xFFFF, steps))
    per = -(-steps // splits)
    return [per * BK * i for i in range(1, -(-steps // per))]


def gemm_ta(g, L, a_np, b_np, plan=None, entry="fp32", ld=None):
    """C = A.B through the TA entry points, A handed over as a_col_major; plan = (ta_config, splits) for the explicit call.
    ld = (lda, ldb, ldc) places a_col_major ([K][lda], lda >= M), the row-major B and C in wider buffers."""
    m, k = a_np.shape
    n = b_np.shape[1]
    assert ld is None or plan is not None, "the planned entry points take contiguous operands"
    lda, ldb, ldc = ld or (m, n, n)
    at = torch.full((k, lda), float("nan"), dtype=torch.half, device="cuda")
    at[:, :m] = torch.from_numpy(np.ascontiguousarray(a_np.T)).cuda()
    b = torch.full((k, ldb), float("nan"), dtype=torch.half, device="cuda")
    b[:, :n] = torch.from_numpy(np.ascontiguousarray(b_np)).cuda()
    c = torch.full((m, ldc), g.C_PAD, dtype=torch.half, device="cuda")
    c[:, :n] = float("nan")  # unwritten outputs stay NaN
    pads = [(x[:, w:], x[:, w:].clone()) for x, w in ((at, m), (b, n), (c, n))]
    if plan is None:
        fn = L.hgemm_mi355x_ta_fp16 if entry == "fp16" else L.hgemm_mi355x_ta_fp32
        st = fn(at.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, g.stream())
    else:
        st = L.hgemm_mi355x_launch_ta(plan[0], plan[1], at.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, lda, ldb, ldc, g.stream())
    assert st == 0, L.hgemm_mi355x_strerror(st)
    torch.cuda.synchronize()
    for pad, before in pads:
        assert torch.equal(pad.view(torch.int16), before.view(torch.int16)), f"padding changed (lda, ldb, ldc = {lda}, {ldb}, {ldc})"
    return c[:, :n].contiguous().cpu().numpy()


def check_exact(g, L, oracle, members, m, n, k, seed, forms=FORMS, ld=None, runs=1):
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(seed))
    truth = truth_of(oracle, a, b)
    assert not np.isnan(truth).any()
    ran = 0
    for name, cid in members:
        assert L.hgemm_mi355x_ta_runs(cid, m, n, k, *(ld or (m, n, n))) == runs, (name, m, n, k, ld)
        for splits in forms:
            got = gemm_ta(g, L, a, b, plan=(cid, splits), ld=ld)
            bad = int((bits(got) != bits(truth)).sum())
            assert bad == 0, f"{name} splits {hex(splits)} {m}x{n}x{k} ld={ld}: {bad} of {m * n} elements differ from the oracle"
            ran += 1
    return ran


# ---- orientation ---------------------------------------------------------------------------------------------------------------------
def test_an_untransposed_a_is_told_apart(g, L, oracle, members):
    """B = identity (K = N = 128, M = 136): C must be A itself, an asymmetric 0/1 matrix -- a kernel that reads a_col_major as [M][K],
    swaps two k-rows or two 16-byte chunks of a row, or hands a lane another lane's column gives another matrix.  Then B = a column
    permutation of the identity: C = the permuted columns of A."""
    m, k = 136, 128
    rng = np.random.default_rng(7)
    a = (rng.random((m, k)) < 0.5).astype(np.float16)
    assert not np.array_equal(a[:128, :128], a[:128, :128].T)
    perm = rng.permutation(k)
    for b, want in ((np.eye(k, dtype=np.float16), a), (np.eye(k, dtype=np.float16)[:, perm], a[:, perm])):
        for name, cid in members:
            for splits in FORMS:
                got = gemm_ta(g, L, a, b, plan=(cid, splits))
                assert np.array_equal(bits(got), bits(want)), (name, hex(splits), int((bits(got) != bits(want)).sum()))


def test_square_shapes_do_not_hide_an_untransposed_read(g, L, oracle, members):
    """M = K = 128, where a_col_major could be read as [M][K] without leaving the buffer: asymmetric A and B."""
    m = k = 128
    n = 136
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(8))
    assert not np.array_equal(a, a.T)
    truth = oracle.truth_f32acc(a, b)
    assert not np.array_equal(bits(truth), bits(oracle.truth_f32acc(np.ascontiguousarray(a.T), b)))
    for name, cid in members:
        for splits in FORMS:
            got = gemm_ta(g, L, a, b, plan=(cid, splits))
            assert np.array_equal(bits(got), bits(truth)), (name, hex(splits), int((bits(got) != bits(truth)).sum()))


# ---- exact 0/1 -----------------------------------------------------------------------------------------------------------------------
# one stage (fewer than the prologue) / a sliver tile, every chunk past M or N / NBUF + 1 stages, ragged in M and N for every member /
# a second tile row that is an 8-row sliver whose last k-row ends with the A descriptor
SHAPES = [(64, 64, 64), (8, 8, 64), (200, 136, 320), (72, 264, 192)]


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_and_form_is_exact(g, L, oracle, members, shape, padded):
    m, n, k = shape
    ld = (m + 24, n + 24, n + 40) if padded else None
    assert check_exact(g, L, oracle, members, m, n, k, seed=m + 3 * n + 5 * k, ld=ld) == len(MEMBERS) * len(FORMS)


# ---- planned entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(256, 264, 512, 8), (200, 136, 192, 3)], ids=lambda c: "x".join(map(str, c[:3])))
def test_the_planned_entries_are_exact_through_their_split_plans(g, L, oracle, case):
    m, n, k, want = case
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.hgemm_mi355x_ta_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0
    assert (MEMBERS[cfg.value], splits.value) == ("a64x64_w2x2", want) and L.hgemm_mi355x_ta_runs(cfg.value, m, n, k, m, n, n) == 1
    assert decision(L, cfg.value, splits.value, m, n, k)[1] == FORM_SPLITK
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(m + n + k))
    truth = truth_of(oracle, a, b)
    for entry in ("fp32", "fp16"):
        got = gemm_ta(g, L, a, b, entry=entry)
        assert np.array_equal(bits(got), bits(truth)), (case, entry, int((bits(got) != bits(truth)).sum()))


def test_randn_inputs_meet_the_relative_tolerance(g, L, oracle, members):
    m, n, k = 256, 256, 1024
    rng = np.random.default_rng(13)
    a = rng.standard_normal((m, k), dtype=np.float32).astype(np.float16)
    b = rng.standard_normal((k, n), dtype=np.float32).astype(np.float16)
    ref = a.astype(np.float32) @ b.astype(np.float32)
    runs = [("entry fp32", dict(entry="fp32")), ("entry fp16", dict(entry="fp16"))]
    runs += [(f"{name} {hex(w)}", dict(plan=(cid, w))) for name, cid in members for w in FORMS]
    for what, how in runs:
        err = oracle.relative_error(gemm_ta(g, L, a, b, **how), ref)
        print(f"{what} {m}x{n}x{k}: relative error {err:.3e}")
        assert err <= REL_TOL, (what, err)


# ---- rounding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("member", MEMBERS)
def test_every_member_rounds_to_nearest_even(g, L, oracle, infos, member):
    """Dyadic operands (oracle.dyadic_inputs) against oracle.truth_exact, M = BM + 24, N = BN + 24 (a whole tile and a sliver each
    way): the fp16 epilogue (plain) and the slab epilogue + reduce (3 splits), at K = 192 and K = 64 (NBUF + 1), where the ring wraps.
    A wrong result names the mutant it matches, as tests/test_gpu_rounding.py does."""
    from test_gpu_rounding import DyadicOperands, name_the_fault

    name, cid, bm, bn, nbuf = next(i for i in infos if i[0] == member)
    m, n = bm + 24, bn + 24
    ks = (192, BK * (nbuf + 1))
    ops = DyadicOperands(oracle, m, n, ks, 701)
    lines, runs = [], 0
    for k in ks:
        a, b, truth = ops.sub(m, n, k)
        assert L.hgemm_mi355x_ta_runs(cid, m, n, k, m, n, n) == 1
        for word in (1, 3):
            st, form, disp = decision(L, cid, word, m, n, k)
            # (3 splits of four stages run as 2 x 2 stages: at most ceil(stages / splits) stages per chunk, no empty chunk)
            assert (st, form) == (0, FORM_PLAIN if word == 1 else FORM_SPLITK) and disp[0][3] == len(two_pass_cuts(k, word)) + 1, (name, word, k, form, disp)
            got = gemm_ta(g, L, a, b, plan=(cid, word))
            runs += 1
            bad = bits(got) != bits(truth)
            if bad.any():
                cuts = [two_pass_cuts(k, 3)] if word == 3 else sorted({tuple(two_pass_cuts(k, w)) for w in (2, 3)})
                lines.append(f"{name} plan {word} {m}x{n}x{k}: {int(bad.sum())} of {bad.size} elements differ\n    "
                             + name_the_fault(oracle, a, b, got, truth, cuts))
    assert not lines, f"{len(lines)} of {runs} runs are not round-to-nearest-even:\n" + "\n".join(lines)
    assert runs == 4


# ---- special values ------------------------------------------------------------------------------------------------------------------
def ta_special_operands(m, n):
    """test_gpu_parity.special_value_operands (the builder tests/test_gpu_nn_bars.py uses) at 128 x n x 512 (hot = 300), grown to m
    rows, plus rows of A -- COLUMNS of a_col_major, the operand of the new transposed reads -- that carry -0 and the denormal 2^-24 in
    the last eight rows (for m = 200 the 8-row sliver).  Rows 3 and 19 of B, which no other row of A meets, select them."""
    from test_gpu_parity import special_value_operands

    k, hot = 512, 300
    a0, b = special_value_operands(128, n, k, hot)
    a = torch.zeros((m, k), dtype=torch.half)
    a[:128] = a0
    a[128:184] = a0[:56]
    r = m - 6
    b[3, :] = 1.0
    b[19, :] = 0.5
    a[r, 0::2] = -0.0                                  # -0 x anything joins +0 terms: +0 in every column
    a[r + 1, 3::16] = 2.0 ** -24                       # a denormal operand of A (k = 3 meets the ones, k = 19 the halves): 1.5 x 2^-24,
    #                                                    the tie between 2^-24 and 2^-23 rounds to even = 2^-23
    a[r + 2, 3] = 2.0 ** -24                           # a denormal operand, a denormal result 2^-24
    a[r + 3, 0::2] = -0.0; a[r + 3, 3] = 2.0 ** -24    # -0 + 2^-24
    a[r + 4, 19] = 2.0 ** -24                          # 2^-25: the tie between 0 and 2^-24 rounds to even = 0
    a[r + 5, 3] = -(2.0 ** -24); a[r + 5, 2] = -0.0    # -2^-24
    truth = (a.float() @ b.float()).half()
    z = torch.zeros(n, dtype=torch.half)
    assert torch.equal(truth[r].view(torch.int16), z.view(torch.int16)) and (truth[r + 1] == 2.0 ** -23).all()
    assert (truth[r + 2] == 2.0 ** -24).all() and (truth[r + 3] == 2.0 ** -24).all() and (truth[r + 4] == 0).all()
    assert (truth[r + 5] == -(2.0 ** -24)).all()
    assert torch.isinf(truth[1]).all() and truth[2, 0] == 65504 and torch.isnan(truth[4, 5]) and truth[9, 0] == 0 and truth[13, 0] == 2048
    assert torch.equal(truth[128:184].view(torch.int16), truth[:56].view(torch.int16))
    return a, b, truth


@pytest.mark.parametrize("m", [192, 200])
def test_special_values_round_like_the_reference_in_the_ta_layout(g, L, members, m):
    """m = 192: every member x every form and both planned entries, contiguous.  m = 200 is ragged against both tile heights; the
    members run at lda = m + 24 with a_col_major's padding holding alternating +inf and NaN (it enters the LDS image of the edge tiles
    and must only meet accumulators that are never stored), the planned entries contiguous.  a_col_major is compared bit for bit."""
    from test_gpu_nn_bars import specials_differ

    n, k = 136, 512
    a, b, truth = ta_special_operands(m, n)
    lda = m if m == 192 else m + 24
    atd = torch.empty((k, lda), dtype=torch.half, device="cuda")
    atd[:, 0::2] = float("inf")
    atd[:, 1::2] = float("nan")
    atd[:, :m] = a.t().cuda()
    before = atd.clone()
    atc = a.t().contiguous().cuda()
    bd = b.cuda()
    plans = [(f"{name}/{word:#x}", (cid, word)) for name, cid in members for word in FORMS] + [("entry fp32", None), ("entry fp16", None)]
    for label, plan in plans:
        c = torch.full((m, n), 7.0, dtype=torch.half, device="cuda")
        if plan is None:
            fn = L.hgemm_mi355x_ta_fp16 if label.endswith("fp16") else L.hgemm_mi355x_ta_fp32
            st = fn(atc.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, g.stream())
        else:
            assert L.hgemm_mi355x_ta_runs(plan[0], m, n, k, lda, n, n) == 1
            st = L.hgemm_mi355x_launch_ta(plan[0], plan[1], atd.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, lda, n, n, g.stream())
        assert st == 0, label
        torch.cuda.synchronize()
        said = specials_differ(c.cpu(), truth)
        assert said is None, f"{label} (m = {m}, lda = {lda}): {said}"
    assert torch.equal(atd.view(torch.int16), before.view(torch.int16)) and torch.equal(atc.view(torch.int16), a.t().contiguous().cuda().view(torch.int16))
    print(f"special values m = {m}: {len(plans)} runs")


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["K=72", "M=100", "N=100"])
def test_what_the_kernel_does_not_take_is_still_answered_exactly(g, L, oracle, members, case):
    """Outside the kernel's scope the reference kernel answers: status 0 (gemm_ta asserts it), exact, whatever split count is named."""
    m, n, k = {"K=72": (200, 136, 72), "M=100": (100, 136, 128), "N=100": (200, 100, 128)}[case]
    for name, cid in members:
        assert decision(L, cid, 1, m, n, k)[:2] == (0, FORM_REFERENCE)
    assert check_exact(g, L, oracle, members, m, n, k, seed=k + n + m, forms=(1, 4), runs=0) == 2 * len(MEMBERS)


@pytest.mark.parametrize("side", [0, 1, 2], ids=["A", "B", "C"])
def test_a_misaligned_pointer_is_answered_exactly_by_the_reference_kernel(g, L, oracle, members, side):
    """One operand starts 4 elements (8 bytes) into a larger tensor, strides unchanged.  Status 0, exact, and the backing tensor
    unchanged around the operand -- whatever split count is named."""
    m, n, k = 200, 136, 128
    off = 4
    a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(70 + side))
    truth = oracle.truth_f32acc(a_np, b_np)
    shapes = [(k, m), (k, n), (m, n)]
    fills = [float("nan"), float("nan"), g.C_PAD]
    for name, cid in members:
        assert L.hgemm_mi355x_ta_runs(cid, m, n, k, m, n, n) == 1 and decision(L, cid, 1, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
        for word in (1, 4):
            flats, views = [], []
            for i, (rows, cols) in enumerate(shapes):
                lead = off if i == side else 0
                flat = torch.full((rows * cols + 2 * off,), fills[i], dtype=torch.half, device="cuda")
                view = flat[lead:lead + rows * cols].view(rows, cols)
                assert view.data_ptr() % 16 == (8 if i == side else 0)
                flats.append(flat); views.append(view)
            views[0].copy_(torch.from_numpy(np.ascontiguousarray(a_np.T))); views[1].copy_(torch.from_numpy(b_np)); views[2].fill_(float("nan"))
            before = [f.clone() for f in flats]
            st = L.hgemm_mi355x_launch_ta(cid, word, views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), m, n, k, m, n, n, g.stream())
            assert st == 0, (name, word, L.hgemm_mi355x_strerror(st))
            torch.cuda.synchronize()
            assert np.array_equal(bits(views[2].cpu().numpy()), bits(truth)), (name, word, "ABC"[side])
            views[2].fill_(float("nan"))
            for f, was in zip(flats, before):
                assert torch.equal(f.view(torch.int16), was.view(torch.int16)), (name, word, "ABC"[side], "the backing tensor changed")


# ---- the reach rule of A, both sides executed ----------------------------------------------------------------------------------------
def test_the_lda_reach_edge_runs_exact_on_both_sides(g, L, oracle, infos):
    """K = 128, M = 72, a64x64: the largest lda at which the kernel still runs (127 x lda x 2 + 144 bytes < 2 GiB; the second tile row
    is an 8-row sliver whose last k-row ends with the descriptor, just below 2 GiB) and the next multiple of 8 (the reference kernel,
    64-bit addressing), both executed in ONE flat buffer of NaN, plain and in two splits.  The buffer must come back unchanged outside
    a_col_major's window and C holds nothing but the result."""
    from test_gpu_strides import all_bits_equal

    name, cid, bm, bn, _ = infos[0]
    m, n, k = 72, 64, 128
    s = largest_ta_stride(L, cid, m, n, k, 0)
    rows_rule, tail = reach_rule(bm, m, n, k, 0)
    assert s == reach_limit(rows_rule, tail) == 8454656 and rows_rule * s * 2 + tail < 2 * GIB <= rows_rule * (s + 8) * 2 + tail
    a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(s % 100003))
    truth = torch.from_numpy(oracle.truth_numpy(a_np, b_np))
    flat = torch.full((k * (s + 8),), float("nan"), dtype=torch.half, device="cuda")
    at, b = torch.from_numpy(np.ascontiguousarray(a_np.T)).cuda(), torch.from_numpy(b_np).cuda()
    ran = 0
    for stride, runs in ((s, 1), (s + 8, 0)):
        assert L.hgemm_mi355x_ta_runs(cid, m, n, k, stride, n, n) == runs
        window = flat.as_strided((k, m), (stride, 1))
        for word in (1, 2):
            st, form, disp = decision(L, cid, word, m, n, k, (stride, n, n))
            assert (st, form) == (0, FORM_REFERENCE if not runs else FORM_PLAIN if word == 1 else FORM_SPLITK), (stride, word, st, form)
            window.copy_(at)
            cbuf = torch.full((m + 2, n), g.C_PAD, dtype=torch.half, device="cuda")      # a guard row in front of and behind C
            c = cbuf[1:m + 1]
            c.fill_(float("nan"))
            st = L.hgemm_mi355x_launch_ta(cid, word, flat.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, stride, n, n, g.stream())
            assert st == 0, L.hgemm_mi355x_strerror(st)
            torch.cuda.synchronize()
            got = c.cpu()
            assert torch.equal(got.view(torch.int16), truth.view(torch.int16)), (stride, word, int((got.view(torch.int16) != truth.view(torch.int16)).sum()))
            assert all_bits_equal(cbuf[0], g.C_PAD) and all_bits_equal(cbuf[m + 1], g.C_PAD), "something outside C's window changed"
            window.fill_(float("nan"))
            assert all_bits_equal(flat, float("nan")), (stride, word, "the buffer changed outside the operand's window")
            ran += 1
    print(f"reach {name} A: edge stride {s}, {ran} runs, buffer {flat.numel() * 2 / 1e9:.2f} GB")
    del flat, window
    torch.cuda.empty_cache()


# ---- workspace -----------------------------------------------------------------------------------------------------------------------
WS_SHAPE = (200, 264, 512)


def device_buffers(count):
    m, n, k = WS_SHAPE
    return [(torch.empty((k, m), dtype=torch.half, device="cuda"), torch.empty((k, n), dtype=torch.half, device="cuda"),
             torch.empty((m, n), dtype=torch.half, device="cuda")) for _ in range(count)]


def replays_exactly(oracle, graph, bufs, seeds):
    """Replays a captured single-stream chain of GEMMs on NEW operand values written into the captured buffers."""
    m, n, k = WS_SHAPE
    wrong = []
    for seed in seeds:
        truths = []
        for i, (at, b, c) in enumerate(bufs):
            a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(2000 * seed + i))
            at.copy_(torch.from_numpy(np.ascontiguousarray(a_np.T))); b.copy_(torch.from_numpy(b_np))
            c.fill_(float("nan"))
            truths.append(oracle.truth_numpy(a_np, b_np))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        wrong += [(seed, i) for i, ((_, _, c), truth) in enumerate(zip(bufs, truths)) if not np.array_equal(bits(c.cpu().numpy()), bits(truth))]
    return wrong


def test_a_split_call_captured_without_a_workspace_runs_unsplit(g, L, oracle, members):
    """Nothing may be allocated while a stream captures: a 2-split call on a fresh stream with nothing reserved returns 0, runs without
    the two-pass form and replays exactly.  One stream, one chain: no parallel branches."""
    m, n, k = WS_SHAPE
    for name, cid in members:
        assert decision(L, cid, 2, m, n, k)[1] == FORM_SPLITK and L.hgemm_mi355x_ta_plan_workspace_bytes(cid, 2, m, n, k) == COUNTER_BYTES + 2 * m * n * 4
    bufs = device_buffers(len(members))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rcs = []
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        for (name, cid), (at, b, c) in zip(members, bufs):
            rcs.append(L.hgemm_mi355x_launch_ta(cid, 2, at.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, m, n, n, st))
    assert rcs == [0] * len(members), rcs
    assert replays_exactly(oracle, graph, bufs, (1, 2)) == []


def test_the_planned_split_call_captures_after_the_ta_reserve_call(g, L, oracle):
    """hgemm_mi355x_ta_reserve_workspace sizes the stream's workspace for the plan hgemm_mi355x_ta_fp32 will take (8 splits here), so the
    capture finds it and the graph holds the slab epilogue and the reduce."""
    m, n, k = WS_SHAPE
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.hgemm_mi355x_ta_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == 8
    assert L.hgemm_mi355x_ta_plan_workspace_bytes(cfg.value, splits.value, m, n, k) == COUNTER_BYTES + splits.value * m * n * 4
    s = torch.cuda.Stream()
    assert L.hgemm_mi355x_ta_reserve_workspace(m, n, k, s.cuda_stream) == 0
    bufs = device_buffers(2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rcs = []
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        for fn, (at, b, c) in zip((L.hgemm_mi355x_ta_fp32, L.hgemm_mi355x_ta_fp16), bufs):
            rcs.append(fn(at.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, st))
    assert rcs == [0, 0], rcs
    assert replays_exactly(oracle, graph, bufs, (1, 2)) == []


# ---- baseline ------------------------------------------------------------------------------------------------------------------------
def test_the_rocblas_ta_baseline_agrees_with_the_oracle(g, L, oracle):
    m, n, k = 128, 136, 256
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(17))
    truth = oracle.truth_f32acc(a, b)
    at = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    bd = torch.from_numpy(b).cuda()
    for acc in (0, 1):
        c = torch.full((m, n), float("nan"), dtype=torch.half, device="cuda")
        st = L.hgemm_rocblas_ta(at.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, acc, g.stream())
        assert st == 0, L.hgemm_mi355x_strerror(st)
        torch.cuda.synchronize()
        assert np.array_equal(bits(c.cpu().numpy()), bits(truth)), (acc, int((bits(c.cpu().numpy()) != bits(truth)).sum()))


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the fp16 TA set (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit."""
    sets = [g.HelperKernelSet(lambda cfg, word, p, d, acc: L.hgemm_mi355x_launch_ta(cfg, word, p["a"], p["b"], p["c"], *d[:6], g.stream()),
                              lambda cfg, word, d, aligned, acc: decision(L, cfg, word, *d[:3], d[3:6], aligned), torch.float16, a_col=True)]
    for s in sets:
        s.check_combine(128, 2, 9111)
        s.check_combine(704, 11, 9111 + 1)
        s.check_reference(9111 + 2)
