"""GPU tests of the bfloat16 forward product (run with `-m gpu` on an MI355X): bgemm_mi355x_tn / bgemm_mi355x_launch_tn -- Y = X W^T with B
given as b_col_major [N][ldb]; family f (hgemm_kernel_tn.hpp, CfgTNB) with v_mfma_f32_16x16x32_bf16 on ds_read_b128 fragments, the bf16
combine of the two-pass form and the bf16 reference kernel that reads B as [N][ldb].

Bar and method are tests/test_gpu_tr_bf16.py's, imported from there: every comparison is bit for bit and unmasked.  Operands are integers
in -2 .. 2 (exact in bf16) with K <= 512, so every fp32 partial sum is an integer of magnitude <= 2048: exact in any order.  The expected
value is numpy's int64 product cast to fp32 (exact), then torch's round-to-nearest-even to bfloat16.  Before any launch the module shows on
the CPU that the expected matrices hold ties to both sides and plain round-ups, and that slabs rounded to bf16 before the add give another
matrix for the split plans at K >= 320.  C lies in [M + 1][ldc]: pad columns and a guard row hold a sentinel that is no integer and must
come back bit-unchanged; the operands' padding holds NaN and the operands must be unchanged afterwards."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, two_pass_cuts
from test_gpu_tr_bf16 import SENTINEL, ibits, operands, rounding_classes, seed_of, special_product, through_slabs, to_bf16

pytestmark = pytest.mark.gpu

MEMBERS = ("f64x64_w2x2", "f128x64_w2x2", "f64x128_w2x2", "f128x128_w2x2")
# one tile and one stage; ragged M and N tiles with clamped B rows; the ring wraps and the cuts are uneven; three tiles each way for
# the largest member
SHAPES = [(64, 64, 64), (136, 72, 128), (152, 152, 320), (264, 264, 512)]


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    lib.bgemm_mi355x_tn.argtypes = [p] * 3 + [i] * 3 + [p]
    lib.bgemm_mi355x_tn_reserve_workspace.argtypes = [i] * 3 + [p]
    lib.bgemm_mi355x_tn_plan_workspace_bytes.restype, lib.bgemm_mi355x_tn_plan_workspace_bytes.argtypes = ctypes.c_size_t, [i] * 5
    lib.bgemm_mi355x_nn.argtypes = [p] * 3 + [i] * 3 + [p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    ids = [(nm, L.bgemm_mi355x_tn_config_by_name(nm.encode())) for nm in MEMBERS]
    assert [cid for _, cid in ids] == [0, 1, 2, 3]
    return ids


def decision(L, cid, word, m, n, k, ld=None, aligned=True):
    """What the call decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    st = L.bgemm_mi355x_selfcheck_launch_tn(cid, word, 4 if aligned else 0, m, n, k, *(ld or (k, k, n)), 0, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


class Case:
    """One shape's operands on the device: A in [M][lda], B as b_col_major [N][ldb] (w[n][k] = b[k][n]), NaN in all padding; the exact
    product as fp32 and as bf16, computed once on the CPU."""

    def __init__(self, m, n, k, seed, padded=False, a=None, b=None, scale=(1.0, 1.0)):
        self.m, self.n, self.k = m, n, k
        if a is None:
            a, b = operands(m, n, k, seed)
        self.a, self.b = a, b
        prod = a.astype(np.int64) @ b.astype(np.int64)
        assert np.abs(prod).max() < 2 ** 24 and np.abs(a).max() <= 16 and np.abs(b).max() <= 16
        self.prod32_np = (prod.astype(np.float64) * scale[0] * scale[1]).astype(np.float32)
        assert np.array_equal(self.prod32_np.astype(np.float64), prod.astype(np.float64) * scale[0] * scale[1])   # the cast was exact
        self.product16 = to_bf16(torch.from_numpy(self.prod32_np).cuda())
        self.ld = (k + 8, k + 16, n + 8) if padded else (k, k, n)
        af = torch.from_numpy(a.astype(np.float32) * np.float32(scale[0])).to(torch.bfloat16)
        bf = torch.from_numpy(b.astype(np.float32) * np.float32(scale[1])).to(torch.bfloat16)
        assert np.array_equal(af.float().numpy().astype(np.float64), a * scale[0]) and np.array_equal(bf.float().numpy().astype(np.float64), b * scale[1])
        self.ad = torch.full((m, self.ld[0]), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.ad[:, :k] = af.cuda()
        self.wd = torch.full((n, self.ld[1]), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.wd[:, :k] = bf.t().contiguous().cuda()
        self.b_rows = bf.cuda()                                    # the row-major B of bgemm_mi355x_nn (the cross-check)
        self.before = [x.clone() for x in (self.ad, self.wd)]

    def c_buffer(self):
        """C in [M + 1][ldc]: the window holds NaN, the pad columns and the guard row behind it the sentinel."""
        buf = torch.full((self.m + 1, self.ld[2]), SENTINEL, dtype=torch.bfloat16, device="cuda")
        buf[:self.m, :self.n] = float("nan")
        return buf

    def launch(self, g, L, buf, plan):
        m, n, k = self.m, self.n, self.k
        if plan is None:
            assert self.ld == (k, k, n)
            st = L.bgemm_mi355x_tn(self.ad.data_ptr(), self.wd.data_ptr(), buf.data_ptr(), m, n, k, g.stream())
        else:
            st = L.bgemm_mi355x_launch_tn(plan[0], plan[1], self.ad.data_ptr(), self.wd.data_ptr(), buf.data_ptr(), m, n, k, *self.ld, g.stream())
        assert st == 0, (plan, L.hgemm_mi355x_strerror(st))

    def check(self, buf, what, want=None):
        torch.cuda.synchronize()
        want = self.product16 if want is None else want
        bad = int((ibits(buf[:self.m, :self.n]) != ibits(want)).sum())
        assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements differ"
        sent = ibits(torch.full((1,), SENTINEL, dtype=buf.dtype, device="cuda"))
        assert bool((ibits(buf[:self.m, self.n:]) == sent).all()) and bool((ibits(buf[self.m]) == sent).all()), f"{what}: the pad or the guard row changed"

    def run(self, g, L, plan, what):
        buf = self.c_buffer()
        self.launch(g, L, buf, plan)
        self.check(buf, what)
        return buf

    def operands_intact(self):
        return all(torch.equal(ibits(x), ibits(was)) for x, was in zip((self.ad, self.wd), self.before))


@pytest.fixture(scope="module")
def cases():
    """The sweep's operands and expected matrices, built once per (shape, padded) and shared; nothing writes to them."""
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            built[(shape, padded)] = Case(*shape, seed_of(shape), padded)
        return built[(shape, padded)]

    return get


@pytest.fixture(scope="module")
def evidence():
    """On the CPU, before any launch: over the expected matrices of SHAPES ties to both sides and plain round-ups occur, truncation and
    round-half-away give other matrices, and -- for every split plan of the two shapes with K >= 320 whose slabs span more than one K
    stage -- so do slabs rounded to bf16 before the add."""
    seen = {"ties to even downwards": 0, "ties to even upwards": 0, "round-ups": 0, "truncation differs": 0, "half-away differs": 0}
    slab_diffs = {}
    for shape in SHAPES:
        m, n, k = shape
        a, b = operands(m, n, k, seed_of(shape))
        prod32 = (a.astype(np.int64) @ b.astype(np.int64)).astype(np.float32)
        down, up, ups, trunc, away, rne = rounding_classes(prod32)
        want = to_bf16(torch.from_numpy(prod32))
        assert np.array_equal(rne.astype(np.uint16), want.view(torch.int16).numpy().view(np.uint16)), "torch's bf16 conversion is not RNE"
        for key, v in zip(seen, (down, up, ups, int((trunc != rne).sum()), int((away != rne).sum()))):
            seen[key] += v
        if k >= 320:
            assert min(down, up, ups) > 0 and int((trunc != rne).sum()) > 0 and int((away != rne).sum()) > 0, (shape, down, up, ups)
            for word in (2, 5):
                cuts = [0] + two_pass_cuts(k, word) + [k]
                d = int((ibits(through_slabs(a, b, k, word, torch.bfloat16)) != ibits(want)).sum())
                slab_diffs[(shape, word)] = d
                if max(hi - lo for lo, hi in zip(cuts, cuts[1:])) == 64:
                    assert d == 0      # a slab of one K stage holds sums of magnitude <= 64 x 4 = 256: bf16 values, nothing to tell apart
                else:
                    assert d > 0, (shape, word, "slabs rounded to bf16 before the add give the same matrix")
    assert all(v > 0 for v in seen.values()), seen
    return seen, slab_diffs


def test_the_expected_matrices_tell_the_rounding_mistakes_apart(evidence):
    seen, slab_diffs = evidence
    print(f"rounding classes over the expected matrices: {seen}; elements a bf16-rounded slab moves: {slab_diffs}")
    assert all(v > 0 for v in seen.values()) and len(slab_diffs) == 4 and sum(1 for d in slab_diffs.values() if d > 0) == 3


# ---- every member x form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_and_form_is_exact(g, L, members, cases, evidence, shape, padded):
    m, n, k = shape
    case = cases(shape, padded)
    if shape == (136, 72, 128):       # b_col_major read as if it were row-major (cut to shape) is another matrix
        w = case.b.T[:72, :72].astype(np.int64)
        assert not np.array_equal(w, w.T) and not np.array_equal(case.a[:, :72].astype(np.int64) @ w, case.a[:, :72].astype(np.int64) @ w.T)
    ran = 0
    for name, cid in members:
        assert L.bgemm_mi355x_tn_runs(cid, m, n, k, *case.ld) == 1, (name, shape)
        for word in FORMS:
            st, form, disp = decision(L, cid, word, m, n, k, case.ld)
            cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
            assert (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1), (name, hex(word))
            case.run(g, L, (cid, word), f"{name} {hex(word)} {m}x{n}x{k} ld={case.ld}")
            ran += 1
    assert ran == 4 * len(FORMS) and case.operands_intact()


def test_the_integer_cases_equal_bgemm_mi355x_nn_on_the_transposed_weight_bit_for_bit(g, L, cases, evidence):
    """bgemm_mi355x_tn(a, w) against bgemm_mi355x_nn(a, w^T contiguous), both planned, on every shape of the sweep."""
    for shape in SHAPES:
        m, n, k = shape
        case = cases(shape)
        c_tn = case.run(g, L, None, f"planned tn {shape}")
        c_nn = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_nn(case.ad.data_ptr(), case.b_rows.data_ptr(), c_nn.data_ptr(), m, n, k, g.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ibits(c_tn[:m, :n]), ibits(c_nn)), shape


def test_m_100_goes_through_the_kernel_and_is_exact(g, L, members):
    m, n, k = 100, 136, 128
    case = Case(m, n, k, m + n + k)
    for name, cid in members:
        assert L.bgemm_mi355x_tn_runs(cid, m, n, k, *case.ld) == 1 and decision(L, cid, 1, m, n, k)[:2] == (0, FORM_PLAIN)
        for word in FORMS:
            case.run(g, L, (cid, word), f"M=100 {name} {hex(word)}")
    assert case.operands_intact()


# ---- bf16, not fp16 --------------------------------------------------------------------------------------------------------------------
def test_operands_and_results_outside_the_fp16_range_are_exact(g, L, members, evidence):
    """A scaled by 2^40 and B by 2^-20: A is far beyond fp16's largest number, B below its normal range, C is an integer x 2^20 -- finite
    in bf16, beyond fp16 wherever it is not zero.  On the CPU first: slabs rounded through fp16 give inf here, another matrix."""
    m, n, k = 152, 152, 320
    case = Case(m, n, k, 77, scale=(2.0 ** 40, 2.0 ** -20))
    assert bool(torch.isfinite(case.product16).all()) and float(case.product16.float().abs().max()) > 65504 * 16
    assert bool(torch.isinf(case.ad.half()[case.ad != 0]).all())   # what a cast of A to fp16 would do
    for word in (2, 5):
        cuts = [0] + two_pass_cuts(k, word) + [k]
        total = sum(torch.from_numpy(((case.a[:, lo:hi].astype(np.float64) @ case.b[lo:hi].astype(np.float64)) * 2.0 ** 20).astype(np.float32)).half().float()
                    for lo, hi in zip(cuts, cuts[1:]))
        assert int((ibits(to_bf16(total)) != ibits(case.product16.cpu())).sum()) > 0, "slabs rounded through fp16 give the same matrix"
    for name, cid in members:
        for word in FORMS:
            case.run(g, L, (cid, word), f"scaled {name} {hex(word)}")
    assert case.operands_intact()


def test_a_sum_beyond_the_fp16_maximum_is_finite_in_the_bf16_c(g, L, members):
    """16 x 16 x 512 of 16s: every output is 131072 = 2^17, a bf16 value, twice fp16's largest."""
    m, n, k = 16, 16, 512
    case = Case(m, n, k, 0, a=np.full((m, k), 16), b=np.full((k, n), 16))
    assert bool((case.product16.float() == 131072.0).all())
    buf = case.run(g, L, None, "bgemm_mi355x_tn")
    assert bool(torch.isfinite(buf[:m, :n]).all())
    for name, cid in members:
        for word in FORMS:
            case.run(g, L, (cid, word), f"2^17 {name} {hex(word)}")


# ---- special values --------------------------------------------------------------------------------------------------------------------
def test_special_values_propagate_as_the_cpu_product_says(g, L, members):
    """NaN, +-inf and -0 in a row of A and in a row of b_col_major (a column of B).  NaN carries no defined payload: the NaN pattern is
    compared first, then the bits of every other element."""
    m, n, k = 72, 72, 128
    a, b = operands(m, n, k, 5)
    a, b = a.astype(np.float64), b.astype(np.float64)
    a[3, :] = -0.0                                                 # a row of -0: C row 3 is +0
    a[9, 70] = np.inf
    a[21, 5] = -np.inf
    a[40, 100] = np.nan
    a[50, 7], a[50, 90] = np.inf, -np.inf                          # both infinities in one row: NaN wherever both meet non-zero b
    w = np.ascontiguousarray(b.T)                                  # b_col_major [N][K]
    w[64, :] = -0.0                                                # a row of -0: C column 64 is +0
    w[17, 3::16] = np.inf                                          # one row of b_col_major holds all four kinds
    w[17, 5::16] = -np.inf
    w[17, 11] = np.nan
    w[17, 12] = -0.0
    w[33, 99] = np.inf
    want32 = special_product(a, np.ascontiguousarray(w.T))
    assert np.isnan(want32).any() and (want32 == np.inf).any() and (want32 == -np.inf).any() and np.isfinite(want32).sum() > m * n // 2
    assert not np.signbit(want32[3][np.isfinite(want32[3])]).any() and not np.signbit(want32[:, 64][np.isfinite(want32[:, 64])]).any()
    ad, wd = torch.from_numpy(a).to(torch.bfloat16).cuda(), torch.from_numpy(w).to(torch.bfloat16).cuda()
    want = to_bf16(torch.from_numpy(want32).cuda())
    clean = torch.where(torch.isnan(want), torch.zeros_like(want), want)
    for name, cid in members:
        for word in FORMS:
            got = torch.full((m, n), SENTINEL, dtype=torch.bfloat16, device="cuda")
            assert L.bgemm_mi355x_launch_tn(cid, word, ad.data_ptr(), wd.data_ptr(), got.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, hex(word), "NaN pattern")
            assert torch.equal(ibits(torch.where(torch.isnan(got), torch.zeros_like(got), got)), ibits(clean)), (name, hex(word))


# ---- planned entries -------------------------------------------------------------------------------------------------------------------
def test_the_planned_entry_is_exact_through_a_split_plan_and_an_unsplit_one(g, L, evidence):
    """256 x 264 x 512: 20 tiles of 64 x 64, eight two-pass splits.  1024 x 1024 x 64: 256 tiles fill the chip, one stage, unsplit."""
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for (m, n, k), want in (((256, 264, 512), 8), ((1024, 1024, 64), 1)):
        assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and (cfg.value, splits.value) == (0, want)
        assert L.bgemm_mi355x_tn_runs(cfg.value, m, n, k, k, k, n) == 1
        st, form, disp = decision(L, cfg.value, splits.value, m, n, k)
        assert (st, form, len(disp), disp[0][3]) == ((0, FORM_SPLITK, 2, 8) if want > 1 else (0, FORM_PLAIN, 1, 1))
        case = Case(m, n, k, m + n + k)
        case.run(g, L, None, f"planned {m}x{n}x{k}")
        assert case.operands_intact()


# ---- fallbacks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["K=72", "N=100", "ldb=K+4"])
def test_what_the_kernels_do_not_take_is_answered_exactly_by_the_reference_kernel(g, L, members, what):
    m, n, k = {"K=72": (200, 136, 72), "N=100": (200, 100, 128), "ldb=K+4": (200, 136, 128)}[what]
    case = Case(m, n, k, m + n + k)
    if what == "ldb=K+4":
        case.ld = (k, k + 4, n)
        case.wd = torch.full((n, k + 4), float("nan"), dtype=torch.bfloat16, device="cuda")
        case.wd[:, :k] = case.b_rows.t()
        case.before = [case.ad.clone(), case.wd.clone()]
    for name, cid in members:
        assert L.bgemm_mi355x_tn_runs(cid, m, n, k, *case.ld) == 0
        for word in (1, 4):
            assert decision(L, cid, word, m, n, k, case.ld)[:2] == (0, FORM_REFERENCE)
            case.run(g, L, (cid, word), f"{what} {name} {word}")
    assert case.operands_intact()


def test_a_pointer_8_bytes_off_is_answered_exactly_by_the_reference_kernel(g, L, members):
    m, n, k = 200, 136, 128
    case = Case(m, n, k, 41)
    for name, cid in members[::3]:
        assert L.bgemm_mi355x_tn_runs(cid, m, n, k, *case.ld) == 1 and decision(L, cid, 1, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
        for word in (1, 4):
            flat = torch.full((m * n + 16,), SENTINEL, dtype=torch.bfloat16, device="cuda")
            view = flat[4:4 + m * n].view(m, n)
            assert view.data_ptr() % 16 == 8
            view.fill_(float("nan"))
            assert L.bgemm_mi355x_launch_tn(cid, word, case.ad.data_ptr(), case.wd.data_ptr(), view.data_ptr(), m, n, k, *case.ld, g.stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(ibits(view), ibits(case.product16)), (name, word)
            assert bool((flat[:4] == SENTINEL).all()) and bool((flat[4 + m * n:] == SENTINEL).all()), "the backing tensor changed"
    assert case.operands_intact()


# ---- N(0,1) operands -------------------------------------------------------------------------------------------------------------------
def test_randn_operands_meet_the_first_order_bound(g, L, members):
    """Per element |got - ref| <= K 2^-24 sum_k |a_k b_k| (the first-order bound of K fp32 adds at unit roundoff 2^-24; the products of
    two bf16 values are exact in fp32) + half a bf16 ulp of the result, against the fp64 product of the bf16-rounded operands: the bound
    of test_gpu_tr_bf16.py, derived there, not measured.  No element is skipped."""
    m, n, k = 264, 264, 512
    rng = np.random.default_rng(13)
    a16 = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).to(torch.bfloat16)
    w16 = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32)).to(torch.bfloat16)
    a64, w64 = a16.double().numpy(), w16.double().numpy()
    ref = a64 @ w64.T
    mag = np.abs(a64) @ np.abs(w64).T
    half_ulp = 2.0 ** (np.floor(np.log2(np.abs(ref))) - 8)
    assert (ref != 0).all()
    bound = k * 2.0 ** -24 * mag + half_ulp
    ad, wd = a16.cuda(), w16.cuda()
    for name, cid in members:
        for word in FORMS:
            c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            assert L.bgemm_mi355x_launch_tn(cid, word, ad.data_ptr(), wd.data_ptr(), c.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
            torch.cuda.synchronize()
            err = np.abs(c.double().cpu().numpy() - ref)
            worst = float((err / bound).max())
            print(f"{name} {hex(word)}: worst error {worst:.3f} of the bound")
            assert bool((err <= bound).all()), (name, hex(word), worst)


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
def test_a_split_call_captured_without_a_workspace_runs_unsplit_and_split_after_the_reserve_call(g, L, evidence):
    """Nothing may be allocated while a stream captures: on a fresh stream with nothing reserved the split bgemm_mi355x_launch_tn call
    returns 0 and replays unsplit; after bgemm_mi355x_tn_reserve_workspace on another fresh stream it replays through its slabs.  Both
    exact (and the same bits: the sums are exact in any order).  One stream, one chain per graph: no parallel branches."""
    m, n, k = 200, 264, 512
    case = Case(m, n, k, 61)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == 8
    cid = cfg.value
    assert decision(L, cid, splits.value, m, n, k)[1] == FORM_SPLITK
    assert L.bgemm_mi355x_tn_plan_workspace_bytes(cid, splits.value, m, n, k) == COUNTER_BYTES + 8 * m * n * 4
    for reserve in (False, True):
        buf = case.c_buffer()
        s = torch.cuda.Stream()
        if reserve:
            assert L.bgemm_mi355x_tn_reserve_workspace(m, n, k, s.cuda_stream) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            rc = L.bgemm_mi355x_launch_tn(cid, splits.value, case.ad.data_ptr(), case.wd.data_ptr(), buf.data_ptr(), m, n, k, k, k, n,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, reserve
        buf[:m, :n] = float("nan")
        torch.cuda.synchronize()
        graph.replay()
        case.check(buf, f"replay, reserved={reserve}")
    assert case.operands_intact()


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the bf16 TN set (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit."""
    sets = [g.HelperKernelSet(lambda cfg, word, p, d, acc: L.bgemm_mi355x_launch_tn(cfg, word, p["a"], p["b"], p["c"], *d[:6], g.stream()),
                              lambda cfg, word, d, aligned, acc: decision(L, cfg, word, *d[:3], d[3:6], aligned), torch.bfloat16, b_col=True)]
    for s in sets:
        s.check_combine(128, 2, 9141)
        s.check_combine(704, 11, 9141 + 1)
        s.check_reference(9141 + 2)
