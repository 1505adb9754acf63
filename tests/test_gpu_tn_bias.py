"""GPU tests of the forward product with a fused bias (run with `-m gpu` on an MI355X): bgemm_mi355x_tn_bias / bgemm_mi355x_launch_tn_bias --
Y = X W^T + b; family f's EPI_C16_BIAS kernels (hgemm_inst_g12.hip), the bias combine of the two-pass form and the bias reference kernel.

The semantics under test, bit for bit and unmasked:  C[m][n] = bf16_rne( fl32( S[m][n] + float(bias[n]) ) ), S the finished fp32 sum, the bias
added LAST as one fp32 add, the result rounded ONCE.

Operands are tests/test_gpu_tr_bf16.py's integers in -2 .. 2 with K <= 512: S is an exact integer of magnitude <= 2048 in any order.  The
bias holds bf16 values that are multiples of 2^-8 with |b| <= 256, all N pairwise distinct: quarters, halves, odd integers and a few large
ones.  S + b then needs at most 12 + 8 = 20 significand bits: exact in fp32, so the expected matrix is (S32 + b.float()).to(bfloat16) from the
CPU.  Before any launch the module shows on the CPU that this matrix holds ties to both sides and plain round-ups and differs from what
each mistake would give: the bias added after the bf16 rounding, added into every slab, taken from the neighbouring column tile.  The bias
as the accumulators' initial value gives the same bits on integers (every order is exact); the scaled case below tells it apart.
On integers the twice-rounded bias cannot show at K = 64 (TWICE_ROUNDED_FLOOR[(64, 64, 64)] == 0: every |S| <= 256 is a bf16 value); that
blind spot is covered by tests/test_gpu_tn_bars.py, whose operands have live mantissa bits (152 elements differ at (64, 64, 64) there).

C lies in [M + 1][ldc] with a sentinel in the pad and the guard row, NaN sits in the operands' padding, the bias vector is followed by a NaN
guard element, and operands and bias must be bit-unchanged afterwards."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, two_pass_cuts
from test_gpu_tn_bf16 import MEMBERS, SHAPES, Case
from test_gpu_tr_bf16 import SENTINEL, ibits, operands, rounding_classes, seed_of, to_bf16

pytestmark = pytest.mark.gpu

EPI_SLAB, EPI_C16_BIAS = 1, 5
# Elements of the expected matrix that the twice-rounded value must differ in, per shape.  At K = 64 every |S| <= 4 x 64 = 256 is a bf16
# value, so rounding S first changes nothing: the mistake cannot show there and the floor is 0.  From K = 128 on, odd sums beyond 256
# are no bf16 values (rows m % 3 == 2 x odd columns centre at 2.25 K); the floors are a twentieth of the elements or less.
TWICE_ROUNDED_FLOOR = {(64, 64, 64): 0, (136, 72, 128): 100, (152, 152, 320): 2000, (264, 264, 512): 10000}


def bias_pool():
    """bf16 values, multiples of 2^-8, |b| <= 256, pairwise distinct: odd quarters below 32, halves from 32.5 to 63.5, odd integers from
    65 to 255, a few large even ones, and the granularity itself with a zero: 400 values."""
    quarters = [q / 4.0 for q in range(-127, 128) if q % 2]                       # |b| <= 31.75: 7 significand bits
    halves = [s * (32 + h / 2.0) for h in range(1, 64, 2) for s in (1, -1)]
    odd = [s * float(v) for v in range(65, 256, 2) for s in (1, -1)]              # 8 significand bits
    large = [256.0, -256.0, 192.0, -192.0, 224.0, -160.0, 128.0, -96.0]
    small = [q / 256.0 for q in (1, -1, 3, -5, 7, 96, -80)] + [0.0]
    pool = quarters + halves + odd + large + small
    assert len(set(pool)) == len(pool) == 400
    return pool


def make_bias(n, seed):
    """N pairwise distinct values of the pool in a seeded order; a longer vector (N = 1024) goes on with other bf16 multiples of 2^-8."""
    rng = np.random.default_rng(1000 + seed)
    pool = rng.permutation(np.array(bias_pool(), dtype=np.float32))
    if n > len(pool):
        grid = torch.arange(-65536, 65537, dtype=torch.float32) / 256
        rest = grid[grid.to(torch.bfloat16).float() == grid].numpy()
        pool = np.concatenate([pool, rng.permutation(np.setdiff1d(rest, pool))])
    b = np.ascontiguousarray(pool[:n])
    t = torch.from_numpy(b).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy(), b), "a bias value is no bf16 value"
    assert len(set(b.tolist())) == n and np.abs(b).max() <= 256 and np.array_equal(b * 256, np.round(b * 256))
    return t


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    lib.bgemm_mi355x_tn.argtypes = [p] * 3 + [i] * 3 + [p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    lib.bgemm_mi355x_tn_bias.argtypes = [p] * 4 + [i] * 3 + [p]
    lib.bgemm_mi355x_tn_reserve_workspace.argtypes = [i] * 3 + [p]
    lib.bgemm_mi355x_tn_plan_workspace_bytes.restype, lib.bgemm_mi355x_tn_plan_workspace_bytes.argtypes = ctypes.c_size_t, [i] * 5
    return lib


@pytest.fixture(scope="module")
def members(L):
    ids = [(nm, L.bgemm_mi355x_tn_config_by_name(nm.encode())) for nm in MEMBERS]
    assert [cid for _, cid in ids] == [0, 1, 2, 3]
    return ids


def decision(L, cid, word, m, n, k, ld=None, aligned=True):
    """What the bias call decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    st = L.bgemm_mi355x_selfcheck_launch_tn_bias(cid, word, 4 if aligned else 0, m, n, k, *(ld or (k, k, n)), 0, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


class BiasCase(Case):
    """test_gpu_tn_bf16.Case with a bias vector: N bf16 values on the device followed by a NaN guard element, and the expected matrix
    bf16(S32 + bias) from the CPU."""

    def __init__(self, m, n, k, seed, padded=False, bias=None, **kw):
        super().__init__(m, n, k, seed, padded, **kw)
        self.bias = make_bias(n, seed) if bias is None else bias
        self.set_bias(self.bias)

    def set_bias(self, bias, offset=0):
        """`offset` elements of NaN in front (a pointer 2 x offset bytes off a 16-byte boundary), the NaN guard behind."""
        self.bias = bias
        self.bias_buf = torch.full((offset + self.n + 1,), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.bias_buf[offset:offset + self.n] = bias.cuda()
        self.bias_d = self.bias_buf[offset:offset + self.n]
        assert self.bias_d.data_ptr() % 16 == (2 * offset) % 16
        self.bias_before = self.bias_buf.clone()
        with np.errstate(invalid="ignore"):
            self.want32 = torch.from_numpy(self.prod32_np) + bias.float()[None, :]      # one fp32 add per element (exact on the integer cases)
        self.product16 = to_bf16(self.want32).cuda()                                     # what Case.check compares with

    def launch(self, g, L, buf, plan):
        m, n, k = self.m, self.n, self.k
        if plan is None:
            assert self.ld == (k, k, n)
            st = L.bgemm_mi355x_tn_bias(self.ad.data_ptr(), self.wd.data_ptr(), self.bias_d.data_ptr(), buf.data_ptr(), m, n, k, g.stream())
        else:
            st = L.bgemm_mi355x_launch_tn_bias(plan[0], plan[1], self.ad.data_ptr(), self.wd.data_ptr(), self.bias_d.data_ptr(), buf.data_ptr(), m, n, k,
                                               *self.ld, g.stream())
        assert st == 0, (plan, L.hgemm_mi355x_strerror(st))

    def operands_intact(self):
        nan_same = torch.equal(ibits(self.bias_buf), ibits(self.bias_before))
        return super().operands_intact() and nan_same


@pytest.fixture(scope="module")
def cases():
    """The sweep's operands, biases and expected matrices, built once per (shape, padded) and shared; nothing writes to them."""
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            built[(shape, padded)] = BiasCase(*shape, seed_of(shape), padded)
        return built[(shape, padded)]

    return get


def mutants_on_the_cpu(shape):
    """The expected matrix of `shape` and what each mistake would store instead, all on the CPU: (expected, {mistake: matrix})."""
    m, n, k = shape
    a, b = operands(m, n, k, seed_of(shape))
    s32 = torch.from_numpy((a.astype(np.int64) @ b.astype(np.int64)).astype(np.float32))
    bias = make_bias(n, seed_of(shape)).float()
    assert np.array_equal((s32.double() + bias.double()).float().double().numpy(), (s32.double() + bias.double()).numpy()), "S + b is not exact in fp32"
    want = to_bf16(s32 + bias)
    out = {"rounded twice": to_bf16(to_bf16(s32).float() + bias)}
    for word in (2, 5):
        splits = len(two_pass_cuts(k, word)) + 1
        if splits > 1:
            out[f"bias in each of {splits} slabs"] = to_bf16(s32 + splits * bias)
    out["bias of column tile j + 1"] = to_bf16(s32 + torch.roll(bias, -16))
    out["bias of the post-swap columns"] = to_bf16(s32 + bias.view(-1, 2, 4)[:, [1, 0], :].reshape(-1))   # (4 q + e <-> the store's 8-column groups)
    out["no bias"] = to_bf16(s32)
    return s32 + bias, want, out


@pytest.fixture(scope="module")
def evidence():
    """On the CPU, before any launch: the expected matrices hold ties to both sides and plain round-ups, and every mistake gives another
    matrix at every shape where it can (the twice-rounded one from K = 128 on: TWICE_ROUNDED_FLOOR)."""
    report = {}
    for shape in SHAPES:
        want32, want, wrong = mutants_on_the_cpu(shape)
        down, up, ups, trunc, away, rne = rounding_classes(want32.numpy())
        assert np.array_equal(rne.astype(np.uint16), want.view(torch.int16).numpy().view(np.uint16)), "torch's bf16 conversion is not RNE"
        assert min(down, up, ups) > 0, (shape, down, up, ups)
        diffs = {what: int((ibits(x) != ibits(want)).sum()) for what, x in wrong.items()}
        assert diffs["rounded twice"] >= TWICE_ROUNDED_FLOOR[shape], (shape, diffs)
        assert all(d > shape[0] * shape[1] // 4 for what, d in diffs.items() if what != "rounded twice"), (shape, diffs)
        report[shape] = {"ties down": down, "ties up": up, "round-ups": ups, **diffs}
    return report


def test_the_expected_matrices_tell_the_mistakes_apart(evidence):
    for shape, row in evidence.items():
        print(shape, row)
    assert len(evidence) == 4 and sum(1 for s in evidence if evidence[s]["rounded twice"] > 0) == 3


# ---- every member x form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_and_form_is_exact(g, L, members, cases, evidence, shape, padded):
    m, n, k = shape
    case = cases(shape, padded)
    ran = 0
    for name, cid in members:
        assert L.bgemm_mi355x_tn_bias_runs(cid, m, n, k, *case.ld) == 1, (name, shape)
        for word in FORMS:
            st, form, disp = decision(L, cid, word, m, n, k, case.ld)
            cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
            assert (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1), (name, hex(word))
            assert [d[2] for d in disp] == ([EPI_SLAB, EPI_C16_BIAS] if cuts else [EPI_C16_BIAS])
            case.run(g, L, (cid, word), f"{name} {hex(word)} {m}x{n}x{k} ld={case.ld}")
            ran += 1
    assert ran == 4 * len(FORMS) and case.operands_intact()


def test_a_zero_bias_equals_bgemm_mi355x_tn_bit_for_bit(g, L, cases, evidence):
    for shape in SHAPES:
        m, n, k = shape
        case = BiasCase(*shape, seed_of(shape), bias=torch.zeros(n, dtype=torch.bfloat16))
        c_bias = case.run(g, L, None, f"planned, zero bias {shape}")
        c_tn = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_tn(case.ad.data_ptr(), case.wd.data_ptr(), c_tn.data_ptr(), m, n, k, g.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ibits(c_bias[:m, :n]), ibits(c_tn)), shape


def test_m_100_goes_through_the_kernel_and_is_exact(g, L, members):
    m, n, k = 100, 136, 128
    case = BiasCase(m, n, k, m + n + k)
    for name, cid in members:
        assert L.bgemm_mi355x_tn_bias_runs(cid, m, n, k, *case.ld) == 1 and decision(L, cid, 1, m, n, k)[:2] == (0, FORM_PLAIN)
        for word in FORMS:
            case.run(g, L, (cid, word), f"M=100 {name} {hex(word)}")
    assert case.operands_intact()


# ---- the order of the add ----------------------------------------------------------------------------------------------------------------
def init_value_model(a, b, bias, scale):
    """What the accumulators would hold had they STARTED at the bias: fp32, K walked in MFMA blocks of 32 (each block's exact sum added
    to the accumulator with one rounding)."""
    acc = np.broadcast_to(bias.astype(np.float32), (a.shape[0], b.shape[1])).copy()
    for lo in range(0, a.shape[1], 32):
        block = (a[:, lo:lo + 32].astype(np.float64) @ b[lo:lo + 32].astype(np.float64)) * scale
        acc = (acc.astype(np.float64) + block).astype(np.float32)
    return acc


def test_the_bias_is_added_last_and_not_the_accumulators_initial_value(g, L, members):
    """A scaled by 2^40 and B by 2^-10 (test_gpu_tn_bf16.py's scaled case, moved up): S is an integer x 2^30, and a bias of magnitude
    below 32 is below half an ulp of every non-zero S.  Added last, C = bf16(S) where S != 0 and C = bias where S == 0.  As the initial value the bias is absorbed by
    the first non-zero partial sum, so an element whose partial sums leave zero and return to it ends as 0: another matrix, shown on the
    CPU first.  (On the integer cases every order gives the same bits; this case tells the two apart.)"""
    m, n, k = 152, 152, 320
    bias = torch.from_numpy(((np.arange(n) + 1) * 0.125 * np.where(np.arange(n) % 2, -1, 1)).astype(np.float32)).to(torch.bfloat16)
    assert len(set(bias.tolist())) == n and float(bias.float().abs().max()) < 32 == 2.0 ** 30 * 2.0 ** -25
    case = BiasCase(m, n, k, 77, bias=bias, scale=(2.0 ** 40, 2.0 ** -10))
    zero = case.prod32_np == 0
    want = case.product16.cpu()
    assert zero.sum() > 20 and torch.equal(ibits(want[torch.from_numpy(zero)]), ibits(bias[None, :].expand(m, n)[torch.from_numpy(zero)]))
    assert torch.equal(ibits(want[torch.from_numpy(~zero)]), ibits(to_bf16(torch.from_numpy(case.prod32_np))[torch.from_numpy(~zero)]))
    init = to_bf16(torch.from_numpy(init_value_model(case.a, case.b, bias.float().numpy(), 2.0 ** 30)))
    assert int((ibits(init) != ibits(want)).sum()) > 20, "the bias as the initial value gives the same matrix"
    for name, cid in members:
        for word in FORMS:
            case.run(g, L, (cid, word), f"scaled {name} {hex(word)}")
    assert case.operands_intact()


# ---- special values --------------------------------------------------------------------------------------------------------------------
def test_special_values_in_the_bias_and_in_the_sum(g, L, members):
    """NaN in one bias element gives a NaN column; +inf bias gives +inf; an S of +inf from the operands with -inf bias gives NaN; -0 bias on
    an S of +0 gives +0.  The NaN pattern is compared first, then the bits of every other element."""
    m, n, k = 72, 72, 128
    a, b = operands(m, n, k, 5)
    a, b = a.astype(np.float64), b.astype(np.float64)
    a[3, :] = 0.0                                                   # S row 3 is +0
    a[9, 70] = np.inf                                               # S row 9 is +-inf wherever b[70] != 0
    b[70, 20] = 2.0
    bias = make_bias(n, 5).float().numpy()
    bias[11], bias[30], bias[20], bias[40] = np.nan, np.inf, -np.inf, -0.0
    with np.errstate(invalid="ignore"):
        terms = a[:, :, None] * b[None, :, :]
        s32 = np.where(np.isfinite(terms), terms, 0.0).sum(1) + 0.0
        s32[(terms == np.inf).any(1)] = np.inf
        s32[(terms == -np.inf).any(1)] = -np.inf
        s32[np.isnan(terms).any(1) | ((terms == np.inf).any(1) & (terms == -np.inf).any(1))] = np.nan
        want32 = s32.astype(np.float32) + bias[None, :].astype(np.float32)
    assert s32[9, 20] == np.inf and np.isnan(want32[9, 20]) and np.isnan(want32[:, 11]).all() and (want32[:8, 30] == np.inf).all()
    assert want32[3, 40] == 0 and not np.signbit(want32[3, 40]) and np.isfinite(want32).sum() > m * n // 2
    want = to_bf16(torch.from_numpy(want32)).cuda()
    clean = torch.where(torch.isnan(want), torch.zeros_like(want), want)
    ad = torch.from_numpy(a).to(torch.bfloat16).cuda()
    wd = torch.from_numpy(np.ascontiguousarray(b.T)).to(torch.bfloat16).cuda()
    bd = torch.from_numpy(bias).to(torch.bfloat16).cuda()
    for name, cid in members:
        for word in FORMS:
            got = torch.full((m, n), SENTINEL, dtype=torch.bfloat16, device="cuda")
            assert L.bgemm_mi355x_launch_tn_bias(cid, word, ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), got.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, hex(word), "NaN pattern")
            assert torch.equal(ibits(torch.where(torch.isnan(got), torch.zeros_like(got), got)), ibits(clean)), (name, hex(word))


# ---- planned entries -------------------------------------------------------------------------------------------------------------------
def test_the_planned_entry_is_exact_through_a_split_plan_and_an_unsplit_one(g, L, evidence):
    """256 x 264 x 512: 20 tiles of 64 x 64, eight two-pass splits.  1024 x 1024 x 64: 256 tiles fill the chip, one stage, unsplit."""
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for (m, n, k), want in (((256, 264, 512), 8), ((1024, 1024, 64), 1)):
        assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and (cfg.value, splits.value) == (0, want)
        assert L.bgemm_mi355x_tn_bias_runs(cfg.value, m, n, k, k, k, n) == 1
        st, form, disp = decision(L, cfg.value, splits.value, m, n, k)
        assert (st, form, len(disp), disp[0][3]) == ((0, FORM_SPLITK, 2, 8) if want > 1 else (0, FORM_PLAIN, 1, 1))
        case = BiasCase(m, n, k, m + n + k)
        case.run(g, L, None, f"planned {m}x{n}x{k}")
        assert case.operands_intact()
    null = ctypes.c_void_p(0)
    assert L.bgemm_mi355x_tn_bias(case.ad.data_ptr(), case.wd.data_ptr(), null, case.c_buffer().data_ptr(), m, n, k, g.stream()) == -1


# ---- fallbacks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["K=72", "N=100", "ldb=K+4"])
def test_what_the_kernels_do_not_take_is_answered_exactly_by_the_reference_kernel(g, L, members, what):
    m, n, k = {"K=72": (200, 136, 72), "N=100": (200, 100, 128), "ldb=K+4": (200, 136, 128)}[what]
    case = BiasCase(m, n, k, m + n + k)
    if what == "ldb=K+4":
        case.ld = (k, k + 4, n)
        case.wd = torch.full((n, k + 4), float("nan"), dtype=torch.bfloat16, device="cuda")
        case.wd[:, :k] = case.b_rows.t()
        case.before = [case.ad.clone(), case.wd.clone()]
    for name, cid in members:
        assert L.bgemm_mi355x_tn_bias_runs(cid, m, n, k, *case.ld) == 0
        for word in (1, 4):
            assert decision(L, cid, word, m, n, k, case.ld)[:2] == (0, FORM_REFERENCE)
            case.run(g, L, (cid, word), f"{what} {name} {word}")
    assert case.operands_intact()


@pytest.mark.parametrize("what", ["C 8 bytes off", "bias 2 bytes off"])
def test_a_misaligned_pointer_is_answered_exactly_by_the_reference_kernel(g, L, members, what):
    m, n, k = 200, 136, 128
    case = BiasCase(m, n, k, 41)
    if what == "bias 2 bytes off":
        case.set_bias(case.bias, offset=1)
        assert case.bias_d.data_ptr() % 16 == 2
    for name, cid in members[::3]:
        assert L.bgemm_mi355x_tn_bias_runs(cid, m, n, k, *case.ld) == 1 and decision(L, cid, 1, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
        for word in (1, 4):
            flat = torch.full((m * n + 16,), SENTINEL, dtype=torch.bfloat16, device="cuda")
            off = 4 if what == "C 8 bytes off" else 8
            view = flat[off:off + m * n].view(m, n)
            assert view.data_ptr() % 16 == (8 if what == "C 8 bytes off" else 0)
            view.fill_(float("nan"))
            assert L.bgemm_mi355x_launch_tn_bias(cid, word, case.ad.data_ptr(), case.wd.data_ptr(), case.bias_d.data_ptr(), view.data_ptr(), m, n, k,
                                                 *case.ld, g.stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(ibits(view), ibits(case.product16)), (name, word)
            assert bool((flat[:off] == SENTINEL).all()) and bool((flat[off + m * n:] == SENTINEL).all()), "the backing tensor changed"
    assert case.operands_intact()


# ---- N(0,1) operands and bias ------------------------------------------------------------------------------------------------------------
def test_randn_operands_and_bias_meet_the_first_order_bound(g, L, members):
    """Per element |got - ref| <= K 2^-24 sum_k |a_k b_k| (K fp32 adds at unit roundoff 2^-24; products of bf16 values are exact in fp32)
    + 2^-24 |S + bias| (the one fp32 add of the bias) + half a bf16 ulp of the result, against the fp64 value of the bf16-rounded
    operands and bias: DESIGN.md 4.24's bound with the bias term.  No element is skipped."""
    m, n, k = 264, 264, 512
    rng = np.random.default_rng(13)
    a16 = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).to(torch.bfloat16)
    w16 = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32)).to(torch.bfloat16)
    b16 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(torch.bfloat16)
    a64, w64, b64 = a16.double().numpy(), w16.double().numpy(), b16.double().numpy()
    ref = a64 @ w64.T + b64[None, :]
    mag = np.abs(a64) @ np.abs(w64).T
    assert (ref != 0).all()
    half_ulp = 2.0 ** (np.floor(np.log2(np.abs(ref))) - 8)
    bound = k * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(ref) + half_ulp
    ad, wd, bd = a16.cuda(), w16.cuda(), b16.cuda()
    for name, cid in members:
        for word in FORMS:
            c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            assert L.bgemm_mi355x_launch_tn_bias(cid, word, ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
            torch.cuda.synchronize()
            err = np.abs(c.double().cpu().numpy() - ref)
            worst = float((err / bound).max())
            print(f"{name} {hex(word)}: worst error {worst:.3f} of the bound")
            assert bool((err <= bound).all()), (name, hex(word), worst)


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
def test_a_split_call_captured_without_a_workspace_runs_unsplit_and_split_after_the_reserve_call(g, L, evidence):
    """On a fresh stream with nothing reserved the split bgemm_mi355x_launch_tn_bias call returns 0 while capturing and replays unsplit;
    after bgemm_mi355x_tn_reserve_workspace on another fresh stream it replays through its slabs and the bias combine.  Both replays equal
    the eager call bit for bit.  One stream, one chain per graph: no parallel branches."""
    m, n, k = 200, 264, 512
    case = BiasCase(m, n, k, 61)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == 8
    cid = cfg.value
    assert decision(L, cid, splits.value, m, n, k)[1] == FORM_SPLITK
    assert L.bgemm_mi355x_tn_plan_workspace_bytes(cid, splits.value, m, n, k) == COUNTER_BYTES + 8 * m * n * 4
    eager = case.run(g, L, (cid, splits.value), "eager")
    for reserve in (False, True):
        buf = case.c_buffer()
        s = torch.cuda.Stream()
        if reserve:
            assert L.bgemm_mi355x_tn_reserve_workspace(m, n, k, s.cuda_stream) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            rc = L.bgemm_mi355x_launch_tn_bias(cid, splits.value, case.ad.data_ptr(), case.wd.data_ptr(), case.bias_d.data_ptr(), buf.data_ptr(), m, n, k,
                                               k, k, n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, reserve
        buf[:m, :n] = float("nan")
        torch.cuda.synchronize()
        graph.replay()
        case.check(buf, f"replay, reserved={reserve}")
        assert torch.equal(ibits(buf), ibits(eager))
    assert case.operands_intact()


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the fused-bias set (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit."""
    sets = [g.HelperKernelSet(lambda cfg, word, p, d, acc: L.bgemm_mi355x_launch_tn_bias(cfg, word, p["a"], p["b"], p["bias"], p["c"], *d[:6], g.stream()),
                              lambda cfg, word, d, aligned, acc: decision(L, cfg, word, *d[:3], d[3:6], aligned), torch.bfloat16, b_col=True, bias=True)]
    for s in sets:
        s.check_combine(128, 2, 9151)
        s.check_combine(704, 11, 9151 + 1)
        s.check_reference(9151 + 2)
