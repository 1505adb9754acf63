"""GPU tests of family a's fp32-C calls (run with `-m gpu` on an MI355X): hgemm_mi355x_ta_c32 / _launch_ta_c32, c32 = A x B or
c32 += A x B with A given as a_col_major -- the EPI_C32 epilogue of hgemm_kernel_ta.hpp, the c32 combine of the two-pass form and the
reference kernel of the output kind.

Bar: operands are integers in -2 .. 2 with K <= 512, so every partial sum is an integer of magnitude <= 2048, the old C32 holds integers
in +-1000, and every value on the way stays far below 2^24: exact in fp32 in ANY order.  The expected result is numpy's int64 product
(plus the old value) cast to fp32, compared bit for bit and unmasked.  The pad columns of C32 and a guard row behind it hold a sentinel
that is no integer and must come back bit-unchanged; the operands' padding holds NaN."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_nn import NT_STORE
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, MEMBERS, two_pass_cuts

pytestmark = pytest.mark.gpu

SENTINEL = -12345.625                       # no integer: no result and no old value is this
THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_GENERIC = 0, 1, 4
EPI_SLAB, EPI_C32 = 1, 4
GIB = 1 << 30


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    lib.hgemm_mi355x_ta_config_by_name.argtypes = [ctypes.c_char_p]
    lib.hgemm_mi355x_launch_ta_c32.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    lib.hgemm_mi355x_ta_c32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.hgemm_mi355x_ta_fp32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.hgemm_mi355x_ta_plan_workspace_bytes.restype = ctypes.c_size_t
    lib.hgemm_mi355x_ta_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    lib.hgemm_mi355x_ta_reserve_workspace.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    ids = [L.hgemm_mi355x_ta_config_by_name(nm.encode()) for nm in MEMBERS]
    assert all(i >= 0 for i in ids)
    return list(zip(MEMBERS, ids))


def decision(L, cid, word, m, n, k, ld=None, aligned=True, accumulate=0):
    """What hgemm_mi355x_launch_ta_c32 decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    st = L.hgemm_mi355x_selfcheck_launch_ta_c32(cid, word, 4 if aligned else 0, m, n, k, *(ld or (m, n, n)), accumulate, 0, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def i32(t):
    return t.contiguous().view(torch.int32)


class Case:
    """Integer operands of one shape on the device, a_col_major in [K][lda] and B in [K][ldb] with NaN in the padding, and the exact
    product as fp32 (computed once, in int64)."""

    def __init__(self, m, n, k, seed, ld=None, a=None, b=None):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k = m, n, k
        self.ld = ld or (m, n, n)
        lda, ldb, _ = self.ld
        a = rng.integers(-2, 3, (m, k)) if a is None else a
        b = rng.integers(-2, 3, (k, n)) if b is None else b
        self.a, self.b = a, b
        prod = a.astype(np.int64) @ b.astype(np.int64)
        assert np.abs(prod).max() < 2 ** 24
        self.product = torch.from_numpy(prod.astype(np.float32)).cuda()
        self.at = torch.full((k, lda), float("nan"), dtype=torch.half, device="cuda")
        self.at[:, :m] = torch.from_numpy(np.ascontiguousarray(a.T).astype(np.float16)).cuda()
        self.bd = torch.full((k, ldb), float("nan"), dtype=torch.half, device="cuda")
        self.bd[:, :n] = torch.from_numpy(b.astype(np.float16)).cuda()
        self.before = (self.at.clone(), self.bd.clone())

    def old_values(self, seed):
        return torch.from_numpy(np.random.default_rng(seed).integers(-1000, 1001, (self.m, self.n)).astype(np.float32)).cuda()

    def c_buffer(self, old=None):
        """C32 in [M + 1][ldc]: the window holds `old` (NaN if none), the pad columns and the guard row behind it the sentinel."""
        buf = torch.full((self.m + 1, self.ld[2]), SENTINEL, dtype=torch.float32, device="cuda")
        buf[:self.m, :self.n] = float("nan") if old is None else old
        return buf

    def launch(self, g, L, buf, plan, accumulate):
        if plan is None:
            assert self.ld == (self.m, self.n, self.n)
            st = L.hgemm_mi355x_ta_c32(self.at.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), self.m, self.n, self.k, accumulate, g.stream())
        else:
            st = L.hgemm_mi355x_launch_ta_c32(plan[0], plan[1], self.at.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), self.m, self.n, self.k,
                                              *self.ld, accumulate, g.stream())
        assert st == 0, (plan, accumulate, L.hgemm_mi355x_strerror(st))

    def check(self, buf, want, what):
        torch.cuda.synchronize()
        got = buf[:self.m, :self.n]
        bad = int((i32(got) != i32(want)).sum())
        assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements differ"
        sent = torch.full((1,), SENTINEL, dtype=torch.float32, device="cuda").view(torch.int32)
        assert bool((i32(buf[:self.m, self.n:]) == sent).all()) and bool((i32(buf[self.m]) == sent).all()), f"{what}: the pad or the guard row changed"

    def operands_intact(self):
        return all(torch.equal(x.view(torch.int16), was.view(torch.int16)) for x, was in zip((self.at, self.bd), self.before))


# ---- orientation ---------------------------------------------------------------------------------------------------------------------
def test_an_untransposed_a_is_told_apart(g, L, members):
    """M = 136, K = 128, N = 72: non-square, and A^T (cut to shape) times B is another matrix."""
    m, n, k = 136, 72, 128
    case = Case(m, n, k, 7)
    sq = case.a[:128, :128].astype(np.int64)
    assert not np.array_equal(sq, sq.T) and not np.array_equal(sq @ case.b, sq.T @ case.b)
    for name, cid in members:
        for word in FORMS:
            buf = case.c_buffer()
            case.launch(g, L, buf, (cid, word), 0)
            case.check(buf, case.product, f"{name} {hex(word)}")


# ---- every member x form x mode ------------------------------------------------------------------------------------------------------
SHAPES = [(64, 64, 64), (8, 8, 64), (200, 136, 320), (72, 264, 192)]


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_form_and_mode_is_exact(g, L, members, shape, padded):
    """Store, then accumulate twice in a row on one buffer (old + P, then old + 2 P: a stale read or a double add shows)."""
    m, n, k = shape
    ld = (m + 8, n + 16, n + 4) if padded else None
    case = Case(m, n, k, m + 3 * n + 5 * k, ld)
    old = case.old_values(11)
    ran = 0
    for name, cid in members:
        assert L.hgemm_mi355x_ta_c32_runs(cid, m, n, k, *case.ld) == 1, (name, shape, ld)
        for word in FORMS:
            st, form, disp = decision(L, cid, word, m, n, k, ld)
            cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
            assert (st, form) == (0, FORM_SPLITK if cuts else FORM_PLAIN), (name, hex(word), form)
            assert [d[0] for d in disp] == ([THUNK_ENTRY, THUNK_SPLITK_REDUCE] if cuts else [THUNK_ENTRY])
            assert [d[2] for d in disp] == ([EPI_SLAB, EPI_C32] if cuts else [EPI_C32]) and disp[0][3] == len(cuts) + 1
            what = f"{name} {hex(word)} {m}x{n}x{k} ld={ld}"
            buf = case.c_buffer()
            case.launch(g, L, buf, (cid, word), 0)
            case.check(buf, case.product, what + " store")
            buf = case.c_buffer(old)
            case.launch(g, L, buf, (cid, word), 1)
            case.check(buf, old + case.product, what + " accumulate")
            case.launch(g, L, buf, (cid, word), 1)
            case.check(buf, old + 2 * case.product, what + " accumulate twice")
            ran += 1
    assert ran == len(MEMBERS) * len(FORMS) and case.operands_intact()


# ---- what the old value does ---------------------------------------------------------------------------------------------------------
def test_store_mode_never_reads_c(g, L, members):
    """C32 prefilled with NaN (Case.c_buffer's default): finite and exact, unsplit and split, kernel and reference kernel."""
    for m, n, k in ((200, 136, 320), (100, 100, 72)):
        case = Case(m, n, k, 23)
        for name, cid in members:
            for word in FORMS:
                buf = case.c_buffer()
                assert bool(torch.isnan(buf[:m, :n]).all())
                case.launch(g, L, buf, (cid, word), 0)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(buf[:m, :n]).all()), (name, hex(word), "store mode added the old value")
                case.check(buf, case.product, f"{name} {hex(word)} {m}x{n}x{k}")


def test_accumulate_mode_keeps_a_nan_or_inf_of_the_old_value_where_it_is(g, L, members):
    m, n, k = 200, 136, 320
    case = Case(m, n, k, 29)
    old = case.old_values(31)
    spots = {(0, 0): float("nan"), (199, 135): float("inf"), (63, 64): float("nan"), (64, 63): float("inf"), (130, 7): float("-inf")}
    for (r, c), v in spots.items():
        old[r, c] = v
    want = old + case.product
    assert int(torch.isnan(want).sum()) == 2 and int(torch.isinf(want).sum()) == 3
    for name, cid in members:
        for word in FORMS:
            buf = case.c_buffer(old)
            case.launch(g, L, buf, (cid, word), 1)
            case.check(buf, want, f"{name} {hex(word)}")          # bit for bit: the NaN and inf patterns are the old value's own
            torch.cuda.synchronize()
            assert int((~torch.isfinite(buf[:m, :n])).sum()) == len(spots)


# ---- no fp16 anywhere on the path ----------------------------------------------------------------------------------------------------
def test_a_sum_beyond_the_fp16_range_is_exact(g, L, members):
    """A = B = 16, K = 512: every output is 131072, twice fp16's largest number; hgemm_mi355x_ta_fp32 on the same operands gives inf."""
    m, n, k = 72, 136, 512
    case = Case(m, n, k, 0, a=np.full((m, k), 16), b=np.full((k, n), 16))
    assert bool((case.product == 131072.0).all())
    c16 = torch.zeros((m, n), dtype=torch.half, device="cuda")
    assert L.hgemm_mi355x_ta_fp32(case.at.data_ptr(), case.bd.data_ptr(), c16.data_ptr(), m, n, k, g.stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isinf(c16).all())
    for name, cid in members:
        for word in FORMS:
            for acc in (0, 1):
                buf = case.c_buffer(torch.zeros((m, n), device="cuda") if acc else None)
                case.launch(g, L, buf, (cid, word), acc)
                case.check(buf, case.product, f"{name} {hex(word)} accumulate={acc}")
    for acc in (0, 1):
        buf = case.c_buffer(torch.zeros((m, n), device="cuda") if acc else None)
        case.launch(g, L, buf, None, acc)
        case.check(buf, case.product, f"planned accumulate={acc}")


def test_the_old_value_meets_the_sum_in_one_fp32_add(g, L, members):
    """old = 2^24: + 1 gives 2^24 (the tie rounds to even), + 3 gives 2^24 + 4 -- one round-to-nearest-even fp32 add of the whole sum, not
    a chain of adds of the parts (2^24 + 1 + 1 + 1 stays 2^24)."""
    m, n, k = 72, 72, 192
    a = np.zeros((m, k), dtype=np.int64)
    b = np.zeros((k, n), dtype=np.int64)
    a[:, 0] = a[:, 70] = a[:, 150] = 1                         # three terms, one per K stage (and per split of a 3-split plan)
    b[0, :] = 1
    b[70, 1::2] = 1
    b[150, 1::2] = 1                                           # even columns sum to 1, odd columns to 3
    case = Case(m, n, k, 0, a=a, b=b)
    old = torch.full((m, n), 2.0 ** 24, dtype=torch.float32, device="cuda")
    want = old.clone()
    want[:, 1::2] = 2.0 ** 24 + 4
    assert torch.equal(want, old + case.product)
    for name, cid in members:
        for word in (1, 1 | NT_STORE, 2, 3):
            buf = case.c_buffer(old)
            case.launch(g, L, buf, (cid, word), 1)
            case.check(buf, want, f"{name} {hex(word)}")


# ---- planned entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 264, 512, 8), (200, 136, 192, 3)], ids=lambda c: "x".join(map(str, c[:3])))
def test_the_planned_entry_is_exact_through_its_split_plan(g, L, shape):
    m, n, k, want = shape
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.hgemm_mi355x_ta_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0
    assert (MEMBERS[cfg.value], splits.value) == ("a64x64_w2x2", want) and L.hgemm_mi355x_ta_c32_runs(cfg.value, m, n, k, m, n, n) == 1
    st, form, disp = decision(L, cfg.value, splits.value, m, n, k, accumulate=1)
    assert (st, form, len(disp)) == (0, FORM_SPLITK, 2) and disp[0][3] == len(two_pass_cuts(k, splits.value)) + 1
    assert (disp[0][0], disp[0][2], disp[1][0], disp[1][2]) == (THUNK_ENTRY, EPI_SLAB, THUNK_SPLITK_REDUCE, EPI_C32)
    case = Case(m, n, k, m + n + k)
    old = case.old_values(5)
    buf = case.c_buffer()
    case.launch(g, L, buf, None, 0)
    case.check(buf, case.product, "planned store")
    buf = case.c_buffer(old)
    case.launch(g, L, buf, None, 1)
    case.check(buf, old + case.product, "planned accumulate")
    case.launch(g, L, buf, None, 1)
    case.check(buf, old + 2 * case.product, "planned accumulate twice")


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["K=72", "M=100", "N=100"])
def test_what_the_kernel_does_not_take_is_still_answered_exactly(g, L, members, what):
    m, n, k = {"K=72": (200, 136, 72), "M=100": (100, 136, 128), "N=100": (200, 100, 128)}[what]
    case = Case(m, n, k, m + n + k)
    old = case.old_values(3)
    for name, cid in members:
        assert L.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, n) == 0
        for word in (1, 4):
            st, form, disp = decision(L, cid, word, m, n, k)
            assert (st, form) == (0, FORM_REFERENCE) and [d[0] for d in disp] == [THUNK_GENERIC]
            buf = case.c_buffer()
            case.launch(g, L, buf, (cid, word), 0)
            case.check(buf, case.product, f"{name} {word} store")
            buf = case.c_buffer(old)
            case.launch(g, L, buf, (cid, word), 1)
            case.check(buf, old + case.product, f"{name} {word} accumulate")


def test_a_c32_pointer_off_by_4_bytes_is_answered_exactly_by_the_reference_kernel(g, L, members):
    m, n, k = 200, 136, 128
    case = Case(m, n, k, 41)
    old = case.old_values(43)
    for name, cid in members:
        assert L.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, n) == 1 and decision(L, cid, 1, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
        for word in (1, 4):
            for acc in (0, 1):
                flat = torch.full((m * n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
                view = flat[1:1 + m * n].view(m, n)
                assert view.data_ptr() % 16 == 4
                view.copy_(old if acc else torch.full_like(old, float("nan")))
                st = L.hgemm_mi355x_launch_ta_c32(cid, word, case.at.data_ptr(), case.bd.data_ptr(), view.data_ptr(), m, n, k, m, n, n, acc, g.stream())
                assert st == 0, (name, word, acc)
                torch.cuda.synchronize()
                want = old + case.product if acc else case.product
                assert torch.equal(i32(view), i32(want)), (name, word, acc)
                assert bool((flat[:1] == SENTINEL).all()) and bool((flat[1 + m * n:] == SENTINEL).all()), "the backing tensor changed"


# ---- N(0,1) operands -----------------------------------------------------------------------------------------------------------------
def test_randn_operands_meet_the_first_order_bound(g, L, members):
    """Per element |got - ref| <= (K + 1) 2^-23 sum_k |a_k b_k| + 2^-23 |old| against the fp64 product of the fp16 operands: the
    first-order bound of ANY summation order with a relative error of 2^-23 per add (twice the unit roundoff: the MFMA's internal adder
    is not documented to round to nearest), K adds of the sum, one of the old value."""
    m, n, k = 200, 136, 320
    rng = np.random.default_rng(13)
    a = rng.standard_normal((m, k)).astype(np.float16)
    b = rng.standard_normal((k, n)).astype(np.float16)
    old_np = (rng.standard_normal((m, n)) * 30).astype(np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ref = a64 @ b64
    mag = np.abs(a64) @ np.abs(b64)
    at = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    bd = torch.from_numpy(b).cuda()
    eps = 2.0 ** -23
    for name, cid in members:
        for word in FORMS:
            for acc in (0, 1):
                c = torch.from_numpy(old_np).cuda() if acc else torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
                assert L.hgemm_mi355x_launch_ta_c32(cid, word, at.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, m, n, n, acc, g.stream()) == 0
                torch.cuda.synchronize()
                got = c.cpu().numpy().astype(np.float64)
                want = ref + (old_np.astype(np.float64) if acc else 0.0)
                bound = (k + 1) * eps * mag + (eps * np.abs(old_np) if acc else 0.0)
                err = np.abs(got - want)
                worst = float((err / bound).max())
                print(f"{name} {hex(word)} accumulate={acc}: worst error {worst:.3f} of the bound")
                assert bool((err <= bound).all()), (name, hex(word), acc, worst)


# ---- C's reach, both sides executed --------------------------------------------------------------------------------------------------
def test_the_ldc_reach_edge_runs_exact_on_both_sides(g, L, members):
    """a64x64, M = 72, N = 64, K = 64: (64 ldc + 64) 4 bytes < 2 GiB holds at ldc = 8388604 (the kernel) and fails at 8388608 (the
    reference kernel, 64-bit addressing), both executed in ONE flat buffer of the sentinel.  Row 71 (the 8-row sliver of the second tile
    row) and the element behind the window are checked, and the whole buffer outside the window."""
    name, cid = members[0]
    m, n, k = 72, 64, 64
    below, above = 8388604, 8388608
    assert (64 * below + 64) * 4 < 2 * GIB <= (64 * above + 64) * 4
    case = Case(m, n, k, 57)
    old = case.old_values(59)
    flat = torch.full(((m - 1) * above + n + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    sent = torch.full((1,), SENTINEL, dtype=torch.float32, device="cuda").view(torch.int32)
    for ldc, runs in ((below, 1), (above, 0)):
        assert L.hgemm_mi355x_ta_c32_runs(cid, m, n, k, m, n, ldc) == runs
        assert decision(L, cid, 1, m, n, k, (m, n, ldc))[:2] == (0, FORM_PLAIN if runs else FORM_REFERENCE)
        window = flat.as_strided((m, n), (ldc, 1))
        for acc in (0, 1):
            window.copy_(old if acc else torch.full_like(old, float("nan")))
            st = L.hgemm_mi355x_launch_ta_c32(cid, 1, case.at.data_ptr(), case.bd.data_ptr(), flat.data_ptr(), m, n, k, m, n, ldc, acc, g.stream())
            assert st == 0, (ldc, acc)
            torch.cuda.synchronize()
            want = old + case.product if acc else case.product
            assert torch.equal(i32(window[71]), i32(want[71])), (ldc, acc, "row 71")
            assert torch.equal(i32(window), i32(want)), (ldc, acc)
            assert int(flat[(m - 1) * ldc + n].view(torch.int32)) == int(sent), (ldc, acc, "the element behind the window changed")
            window.fill_(SENTINEL)
            assert bool((flat.view(torch.int32) == sent).all()), (ldc, acc, "the buffer changed outside the window")
    print(f"reach {name} C32: ldc {below} | {above}, buffer {flat.numel() * 4 / 1e9:.2f} GB")
    del flat, window
    torch.cuda.empty_cache()


# ---- capture -------------------------------------------------------------------------------------------------------------------------
WS_SHAPE = (200, 264, 512)


def replays_exactly(case, graph, buf, rounds=3):
    wrong = []
    for r in range(rounds):
        old = case.old_values(100 + r)                          # fresh old values in the captured buffer
        buf[:case.m, :case.n] = old
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        if not torch.equal(i32(buf[:case.m, :case.n]), i32(old + case.product)) or not bool((buf[case.m] == SENTINEL).all()):
            wrong.append(r)
    return wrong


def test_a_split_accumulate_call_captured_without_a_workspace_runs_unsplit(g, L, members):
    """Nothing may be allocated while a stream captures: on a fresh stream with nothing reserved the 2-split call returns 0, runs
    unsplit and replays exactly.  One stream, one chain: no parallel branches."""
    m, n, k = WS_SHAPE
    case = Case(m, n, k, 61)
    bufs = [case.c_buffer(case.old_values(1)) for _ in members]
    for name, cid in members:
        assert decision(L, cid, 2, m, n, k, accumulate=1)[1] == FORM_SPLITK
        assert L.hgemm_mi355x_ta_plan_workspace_bytes(cid, 2, m, n, k) == COUNTER_BYTES + 2 * m * n * 4
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rcs = []
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        for (name, cid), buf in zip(members, bufs):
            rcs.append(L.hgemm_mi355x_launch_ta_c32(cid, 2, case.at.data_ptr(), case.bd.data_ptr(), buf.data_ptr(), m, n, k, m, n, n, 1, st))
    assert rcs == [0] * len(members), rcs
    wrong = []
    for r in range(3):
        olds = [case.old_values(200 + 10 * r + i) for i in range(len(bufs))]
        for buf, old in zip(bufs, olds):
            buf[:m, :n] = old
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        wrong += [(r, i) for i, (buf, old) in enumerate(zip(bufs, olds)) if not torch.equal(i32(buf[:m, :n]), i32(old + case.product))]
    assert wrong == []


def test_the_planned_accumulate_call_captures_through_its_split_plan_after_the_reserve_call(g, L):
    """hgemm_mi355x_ta_reserve_workspace serves the fp32-C form too (the slabs are the same): the capture finds the workspace and the
    graph holds the slab kernel and the c32 combine."""
    m, n, k = WS_SHAPE
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.hgemm_mi355x_ta_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == 8
    assert decision(L, cfg.value, splits.value, m, n, k, accumulate=1)[1] == FORM_SPLITK
    case = Case(m, n, k, 67)
    buf = case.c_buffer(case.old_values(1))
    s = torch.cuda.Stream()
    assert L.hgemm_mi355x_ta_reserve_workspace(m, n, k, s.cuda_stream) == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rc = L.hgemm_mi355x_ta_c32(case.at.data_ptr(), case.bd.data_ptr(), buf.data_ptr(), m, n, k, 1, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert replays_exactly(case, graph, buf) == []


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the fp16 TA set with an fp32 C (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit, accumulate = 0 and accumulate = 1 on a non-zero C32."""
    sets = [g.HelperKernelSet(lambda cfg, word, p, d, acc: L.hgemm_mi355x_launch_ta_c32(cfg, word, p["a"], p["b"], p["c"], *d[:6], acc, g.stream()),
                              lambda cfg, word, d, aligned, acc: decision(L, cfg, word, *d[:3], d[3:6], aligned, acc), torch.float16, a_col=True,
                              c32=True, accs=(0, 1))]
    for s in sets:
        s.check_combine(128, 2, 9121)
        s.check_combine(704, 11, 9121 + 1)
        s.check_reference(9121 + 2)
