"""GPU tests of the bfloat16 calls on the two transposed-read layouts (run with `-m gpu` on an MI355X): bgemm_mi355x_nn / _ta / _ta_c32
and their launch_ forms -- families n and a with v_mfma_f32_16x16x32_bf16 (CfgNNB / CfgTAB), the bf16 combine of the two-pass form and
the bf16 reference kernels.

Bar: every comparison is bit for bit and unmasked.  Operands are integers in -2 .. 2 (exact in bf16) with K <= 512, so every fp32 partial
sum is an integer of magnitude <= 2048: exact in any order.  The expected value is numpy's int64 product cast to fp32 (exact), then --
for the 16-bit C -- torch's round-to-nearest-even to bfloat16; the fp32 C has no rounding at all.  Two thirds of A's rows follow the
sign pattern of B's k-rows, so their sums reach K and 1.5 K, far past 256 = 2^8 where bf16 stops holding every integer: the rounding
is exercised, and the module shows on the CPU, before any launch, that truncation, round-half-away and slabs rounded before the add
each give another matrix.  Slabs rounded through fp16 are told apart on the scaled case only: an integer partial sum of magnitude
<= 2048 is an fp16 value, so on the unscaled cases that mistake cannot show; at a scale of 2^20 it overflows fp16.
C lies in [M + 1][ldc]: pad columns and a guard row hold a sentinel that is no integer and must come back bit-unchanged; the operands'
padding holds NaN and the operands must be unchanged afterwards."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_nn import MEMBERS as NN_MEMBERS, NT_STORE
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, MEMBERS as TA_MEMBERS, two_pass_cuts

pytestmark = pytest.mark.gpu

SENTINEL = -0.3125                          # a bf16 and an fp32 value, no integer and no integer x 2^20: no result is this
KINDS = ("nn", "ta", "c32")                 # bf16 C through family n, through family a, fp32 C through family a
SHAPES = [(64, 64, 64), (136, 72, 128), (152, 152, 320), (264, 264, 512)]
WS_SHAPE = (200, 264, 512)


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    for fam in ("nn", "ta"):
        getattr(lib, f"hgemm_mi355x_{fam}_config_by_name").argtypes = [ctypes.c_char_p]
        getattr(lib, f"bgemm_mi355x_launch_{fam}").argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
        getattr(lib, f"bgemm_mi355x_{fam}").argtypes = [p] * 3 + [i] * 3 + [p]
        getattr(lib, f"hgemm_mi355x_{fam}_reserve_workspace").argtypes = [i] * 3 + [p]
        fn = getattr(lib, f"hgemm_mi355x_{fam}_plan_workspace_bytes")
        fn.restype, fn.argtypes = ctypes.c_size_t, [i] * 5
    lib.bgemm_mi355x_launch_ta_c32.argtypes = [i] * 2 + [p] * 3 + [i] * 7 + [p]
    lib.bgemm_mi355x_ta_c32.argtypes = [p] * 3 + [i] * 4 + [p]
    lib.hgemm_mi355x_ta_fp32.argtypes = [p] * 3 + [i] * 3 + [p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    """kind -> [(name, id)]; the ids of a family's bf16 kernels are those of its table"""
    nn = [(nm, L.hgemm_mi355x_nn_config_by_name(nm.encode())) for nm in NN_MEMBERS]
    ta = [(nm, L.hgemm_mi355x_ta_config_by_name(nm.encode())) for nm in TA_MEMBERS]
    assert all(cid >= 0 for _, cid in nn + ta)
    return {"nn": nn, "ta": ta, "c32": ta}


def decision(L, kind, cid, word, m, n, k, ld=None, aligned=True, accumulate=0):
    """What the bf16 call decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    ld = ld or ((k if kind == "nn" else m), n, n)
    if kind == "c32":
        st = L.bgemm_mi355x_selfcheck_launch_ta_c32(cid, word, 4 if aligned else 0, m, n, k, *ld, accumulate, 0, out)
    else:
        st = getattr(L, f"bgemm_mi355x_selfcheck_launch_{kind}")(cid, word, 4 if aligned else 0, m, n, k, *ld, 0, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def runs(L, kind, cid, m, n, k, ld):
    return getattr(L, {"nn": "bgemm_mi355x_nn_runs", "ta": "bgemm_mi355x_ta_runs", "c32": "bgemm_mi355x_ta_c32_runs"}[kind])(cid, m, n, k, *ld)


def ibits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def operands(m, n, k, seed):
    """Integers in -2 .. 2.  B's k-row kk carries the sign s[kk]; rows m % 3 == 1 of A carry it too with magnitudes 0 .. 2 (sums near
    +-K), rows m % 3 == 2 with magnitudes 1 .. 2 (near +-1.5 K), rows m % 3 == 0 are uniform (sums near 0); B's odd columns have
    magnitudes 1 .. 2, which raises the sums of those columns by half again.  Row and column signs make both signs of every size occur."""
    rng = np.random.default_rng(seed)
    s = rng.choice([-1, 1], k)
    a = rng.integers(-2, 3, (m, k))
    a[1::3] = s * rng.integers(0, 3, a[1::3].shape)
    a[2::3] = s * rng.integers(1, 3, a[2::3].shape)
    a *= rng.choice([-1, 1], (m, 1))
    mag = rng.integers(0, 3, (k, n))
    mag[:, 1::2] = rng.integers(1, 3, mag[:, 1::2].shape)        # odd columns: magnitudes 1 .. 2 (sums up to 2.25 K)
    b = s[:, None] * mag * rng.choice([-1, 1], (1, n))
    return a, b


def to_bf16(x32):
    """fp32 tensor -> bf16, round to nearest even (torch's conversion: the reference of every 16-bit C here)"""
    return x32.to(torch.bfloat16)


def f32bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def rounding_classes(prod32):
    """How each exact fp32 value meets the bf16 grid: (ties whose even neighbour is the truncation, ties whose even neighbour is the
    next one up in magnitude, plain round-ups), and the matrices truncation and round-half-away would give (as bf16 bit patterns)."""
    u = f32bits(prod32)
    low, keep = u & 0xFFFF, u >> 16
    tie = low == 0x8000
    rne = (u + 0x7FFF + (keep & 1)) >> 16
    return int((tie & (rne == keep)).sum()), int((tie & (rne == keep + 1)).sum()), int((low > 0x8000).sum()), keep, (u + 0x8000) >> 16, rne


def through_slabs(a, b, k, word, fmt):
    """The two-pass result if every slab were rounded through `fmt` before the add (fp32 adds in split order, then bf16 once)."""
    cuts = [0] + two_pass_cuts(k, word) + [k]
    total = None
    for lo, hi in zip(cuts, cuts[1:]):
        slab = torch.from_numpy((a[:, lo:hi].astype(np.float64) @ b[lo:hi].astype(np.float64)).astype(np.float32)).to(fmt).float()
        total = slab if total is None else total + slab
    return to_bf16(total)


class Case:
    """One shape's operands on the device in both layouts of A -- [M][lda] for family n, a_col_major [K][lda'] for family a --, B in
    [K][ldb], NaN in all padding; the exact product as fp32 and as bf16, computed once on the CPU."""

    def __init__(self, m, n, k, seed, padded=False, a=None, b=None, scale=(1.0, 1.0)):
        self.m, self.n, self.k = m, n, k
        if a is None:
            a, b = operands(m, n, k, seed)
        self.a, self.b = a, b
        prod = a.astype(np.int64) @ b.astype(np.int64)
        assert np.abs(prod).max() < 2 ** 24 and np.abs(a).max() <= 16 and np.abs(b).max() <= 16
        self.prod32_np = (prod.astype(np.float64) * scale[0] * scale[1]).astype(np.float32)
        assert np.array_equal(self.prod32_np.astype(np.float64), prod.astype(np.float64) * scale[0] * scale[1])   # the cast was exact
        self.product = torch.from_numpy(self.prod32_np).cuda()
        self.product16 = to_bf16(self.product)
        pa, pb = (8, 16) if padded else (0, 0)
        self.ld = {"nn": (k + pa, n + pb, n + (8 if padded else 0)), "ta": (m + pa, n + pb, n + (8 if padded else 0)),
                   "c32": (m + pa, n + pb, n + (4 if padded else 0))}
        af = torch.from_numpy(a.astype(np.float32) * np.float32(scale[0])).to(torch.bfloat16)
        bf = torch.from_numpy(b.astype(np.float32) * np.float32(scale[1])).to(torch.bfloat16)
        assert np.array_equal(af.float().numpy().astype(np.float64), a * scale[0]) and np.array_equal(bf.float().numpy().astype(np.float64), b * scale[1])
        self.a_rows = torch.full((m, k + pa), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.a_rows[:, :k] = af.cuda()
        self.a_cols = torch.full((k, m + pa), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.a_cols[:, :m] = af.t().contiguous().cuda()
        self.bd = torch.full((k, n + pb), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.bd[:, :n] = bf.cuda()
        self.before = [x.clone() for x in (self.a_rows, self.a_cols, self.bd)]

    def old_values(self, seed):
        return torch.from_numpy(np.random.default_rng(seed).integers(-1000, 1001, (self.m, self.n)).astype(np.float32)).cuda()

    def c_buffer(self, kind, old=None):
        """C in [M + 1][ldc]: the window holds `old` (NaN if none), the pad columns and the guard row behind it the sentinel."""
        buf = torch.full((self.m + 1, self.ld[kind][2]), SENTINEL, dtype=torch.float32 if kind == "c32" else torch.bfloat16, device="cuda")
        buf[:self.m, :self.n] = float("nan") if old is None else old
        return buf

    def launch(self, g, L, kind, buf, plan, accumulate=0):
        a = self.a_rows if kind == "nn" else self.a_cols
        m, n, k = self.m, self.n, self.k
        if plan is None:
            assert self.ld[kind] == ((k if kind == "nn" else m), n, n)
            if kind == "c32":
                st = L.bgemm_mi355x_ta_c32(a.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), m, n, k, accumulate, g.stream())
            else:
                st = getattr(L, f"bgemm_mi355x_{kind}")(a.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), m, n, k, g.stream())
        elif kind == "c32":
            st = L.bgemm_mi355x_launch_ta_c32(plan[0], plan[1], a.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), m, n, k, *self.ld[kind], accumulate, g.stream())
        else:
            st = getattr(L, f"bgemm_mi355x_launch_{kind}")(plan[0], plan[1], a.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), m, n, k, *self.ld[kind], g.stream())
        assert st == 0, (kind, plan, accumulate, L.hgemm_mi355x_strerror(st))

    def check(self, buf, want, what):
        torch.cuda.synchronize()
        got = buf[:self.m, :self.n]
        bad = int((ibits(got) != ibits(want)).sum())
        assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements differ"
        sent = ibits(torch.full((1,), SENTINEL, dtype=buf.dtype, device="cuda"))
        assert bool((ibits(buf[:self.m, self.n:]) == sent).all()) and bool((ibits(buf[self.m]) == sent).all()), f"{what}: the pad or the guard row changed"

    def run_all_modes(self, g, L, kind, plan, what):
        """bf16 C: the product rounded once.  fp32 C: store over NaN, then accumulate twice on one buffer (old + P, old + 2 P)."""
        if kind != "c32":
            buf = self.c_buffer(kind)
            self.launch(g, L, kind, buf, plan)
            self.check(buf, self.product16, what)
            return
        buf = self.c_buffer(kind)
        self.launch(g, L, kind, buf, plan, 0)
        self.check(buf, self.product, what + " store")
        old = self.old_values(11)
        buf = self.c_buffer(kind, old)
        self.launch(g, L, kind, buf, plan, 1)
        self.check(buf, old + self.product, what + " accumulate")
        self.launch(g, L, kind, buf, plan, 1)
        self.check(buf, (old + self.product) + self.product, what + " accumulate twice")   # (two fp32 adds, as the calls make them)

    def operands_intact(self):
        return all(torch.equal(ibits(x), ibits(was)) for x, was in zip((self.a_rows, self.a_cols, self.bd), self.before))


def seed_of(shape):
    return shape[0] + 3 * shape[1] + 5 * shape[2]


@pytest.fixture(scope="module")
def evidence():
    """On the CPU, before any launch: over the expected matrices of SHAPES the three rounding classes occur, truncation and
    round-half-away give other matrices, and -- for every split plan of the two long-K shapes whose slabs span more than one K stage -- so
    do slabs rounded to bf16 before the add.  Returns the counts for the report."""
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
                d = int((ibits(through_slabs(a, b, k, word, torch.bfloat16)) != ibits(want)).sum())
                slab_diffs[(shape, word)] = d
                if max(hi - lo for lo, hi in zip([0] + two_pass_cuts(k, word), two_pass_cuts(k, word) + [k])) == 64:
                    assert d == 0      # a slab of one K stage holds sums of magnitude <= 64 x 4 = 256: bf16 values, nothing to tell apart
                    continue
                assert d > 0, (shape, word, "slabs rounded to bf16 before the add give the same matrix")
                # (an integer partial sum <= 2048 is an fp16 value: the fp16 mistake shows on the scaled case, see the module docstring)
                assert int((ibits(through_slabs(a, b, k, word, torch.float16)) != ibits(want)).sum()) == 0
    assert all(v > 0 for v in seen.values()), seen
    return seen, slab_diffs


def test_the_expected_matrices_tell_the_rounding_mistakes_apart(evidence):
    seen, slab_diffs = evidence
    print(f"rounding classes over the expected matrices: {seen}; elements a bf16-rounded slab moves: {slab_diffs}")
    assert all(v > 0 for v in seen.values()) and len(slab_diffs) == 4 and sum(1 for d in slab_diffs.values() if d > 0) == 3


# ---- every member x form x kind ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_form_and_kind_is_exact(g, L, members, evidence, shape, padded):
    m, n, k = shape
    case = Case(m, n, k, seed_of(shape), padded)
    if shape == (136, 72, 128):       # non-square: A^T (cut to shape) times B is another matrix
        sq = case.a[:128, :128].astype(np.int64)
        assert not np.array_equal(sq, sq.T) and not np.array_equal(sq @ case.b, sq.T @ case.b)
    ran = 0
    for kind in KINDS:
        for name, cid in members[kind]:
            assert runs(L, kind, cid, m, n, k, case.ld[kind]) == 1, (kind, name, shape)
            for word in FORMS:
                st, form, disp = decision(L, kind, cid, word, m, n, k, case.ld[kind])
                cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
                assert (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1), (kind, name, hex(word))
                case.run_all_modes(g, L, kind, (cid, word), f"{kind} {name} {hex(word)} {m}x{n}x{k} ld={case.ld[kind]}")
                ran += 1
    assert ran == len(KINDS) * 4 * len(FORMS) and case.operands_intact()


# ---- bf16, not fp16 ------------------------------------------------------------------------------------------------------------------
def test_operands_and_results_outside_the_fp16_range_are_exact(g, L, members, evidence):
    """A scaled by 2^40 and B by 2^-20: A is far beyond fp16's largest number, B below its normal range, C is an integer x 2^20 -- finite
    in bf16, beyond fp16 wherever it is not zero.  On the CPU first: slabs rounded through fp16 give inf here, another matrix."""
    m, n, k = 152, 152, 320
    case = Case(m, n, k, 77, scale=(2.0 ** 40, 2.0 ** -20))
    assert bool(torch.isfinite(case.product16).all()) and float(case.product.abs().max()) > 65504 * 16
    assert bool(torch.isinf(case.a_rows.half()[case.a_rows != 0]).all())   # what a cast of A to fp16 would do
    for word in (2, 5):
        cuts = [0] + two_pass_cuts(k, word) + [k]
        total = sum(torch.from_numpy(((case.a[:, lo:hi].astype(np.float64) @ case.b[lo:hi].astype(np.float64)) * 2.0 ** 20).astype(np.float32)).half().float()
                    for lo, hi in zip(cuts, cuts[1:]))
        assert int((ibits(to_bf16(total)) != ibits(case.product16.cpu())).sum()) > 0, "slabs rounded through fp16 give the same matrix"
    for kind in KINDS:
        for name, cid in members[kind]:
            for word in FORMS:
                case.run_all_modes(g, L, kind, (cid, word), f"scaled {kind} {name} {hex(word)}")
    assert case.operands_intact()


def test_a_sum_beyond_the_fp16_maximum_is_finite_in_the_bf16_c(g, L, members):
    """16 x 16 x 512 of 16s: every output is 131072 = 2^17, a bf16 value, twice fp16's largest; hgemm_mi355x_ta_fp32 on the fp16 twins
    of these operands gives inf."""
    m, n, k = 16, 16, 512
    case = Case(m, n, k, 0, a=np.full((m, k), 16), b=np.full((k, n), 16))
    assert bool((case.product16.float() == 131072.0).all())
    c16 = torch.zeros((m, n), dtype=torch.half, device="cuda")
    assert L.hgemm_mi355x_ta_fp32(case.a_cols.half().data_ptr(), case.bd.half().data_ptr(), c16.data_ptr(), m, n, k, g.stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isinf(c16).all())
    buf = case.c_buffer("ta")
    case.launch(g, L, "ta", buf, None)
    case.check(buf, case.product16, "bgemm_mi355x_ta")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf[:m, :n]).all())
    for kind in ("nn", "ta"):
        for name, cid in members[kind]:
            for word in FORMS:
                case.run_all_modes(g, L, kind, (cid, word), f"2^17 {kind} {name} {hex(word)}")


# ---- special values ------------------------------------------------------------------------------------------------------------------
def special_product(a, b):
    """The IEEE result of sum_k a[m][k] b[k][n] whatever the order, for operands that are integers, +-inf, NaN or -0: NaN if a term is
    NaN (inf x 0 is one) or terms of both infinities occur, else the infinity that occurs, else the exact integer sum (+0 for an empty
    one: the accumulators start at +0, and +0 + -0 = +0)."""
    with np.errstate(invalid="ignore"):
        terms = a[:, :, None] * b[None, :, :]                      # [M][K][N], fp64: exact products
    nan = np.isnan(terms).any(1) | ((terms == np.inf).any(1) & (terms == -np.inf).any(1))
    out = np.where(np.isfinite(terms), terms, 0.0).sum(1) + 0.0
    out[(terms == np.inf).any(1)] = np.inf
    out[(terms == -np.inf).any(1)] = -np.inf
    out[nan] = np.nan
    return out.astype(np.float32)


def test_special_values_propagate_as_the_cpu_product_says(g, L, members):
    """NaN, +-inf and -0 in a row of A and in a row of B (a column pattern through the transposed reads).  NaN carries no defined
    payload: the NaN pattern is compared, then the bits of every other element."""
    m, n, k = 72, 72, 128
    a, b = operands(m, n, k, 5)
    a, b = a.astype(np.float64), b.astype(np.float64)
    a[3, :] = -0.0                                                 # a row of -0: C row 3 is +0
    a[9, 70] = np.inf
    a[21, 5] = -np.inf
    a[40, 100] = np.nan
    a[50, 7], a[50, 90] = np.inf, -np.inf                          # both infinities in one row: NaN wherever both meet non-zero b
    b[64, :] = -0.0                                                # a k-row of -0
    b[17, 3::16] = np.inf                                          # a column pattern
    b[33, 5::16] = -np.inf
    b[99, 11] = np.nan
    want32 = special_product(a, b)
    assert np.isnan(want32).any() and (want32 == np.inf).any() and (want32 == -np.inf).any() and np.isfinite(want32).sum() > m * n // 2
    assert not np.signbit(want32[3][np.isfinite(want32[3])]).any()
    case = Case.__new__(Case)
    case.m, case.n, case.k = m, n, k
    case.ld = {"nn": (k, n, n), "ta": (m, n, n), "c32": (m, n, n)}
    af, bf = torch.from_numpy(a).to(torch.bfloat16), torch.from_numpy(b).to(torch.bfloat16)
    case.a_rows, case.a_cols, case.bd = af.cuda(), af.t().contiguous().cuda(), bf.cuda()
    want = {"c32": torch.from_numpy(want32).cuda()}
    want["nn"] = want["ta"] = to_bf16(want["c32"])
    for kind in KINDS:
        w = want[kind]
        clean = torch.where(torch.isnan(w), torch.zeros_like(w), w)
        for name, cid in members[kind]:
            for word in FORMS:
                buf = case.c_buffer(kind)
                case.launch(g, L, kind, buf, (cid, word))
                torch.cuda.synchronize()
                got = buf[:m, :n]
                assert torch.equal(torch.isnan(got), torch.isnan(w)), (kind, name, hex(word), "NaN pattern")
                assert torch.equal(ibits(torch.where(torch.isnan(got), torch.zeros_like(got), got)), ibits(clean)), (kind, name, hex(word))


# ---- planned entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 264, 512, 8), (200, 136, 192, 3)], ids=lambda c: "x".join(map(str, c[:3])))
def test_the_planned_entries_are_exact_through_their_split_plans(g, L, members, evidence, shape):
    m, n, k, want = shape
    case = Case(m, n, k, m + n + k)
    for kind in KINDS if m == 256 else ("nn", "ta"):
        fam = "nn" if kind == "nn" else "ta"
        cfg, splits = ctypes.c_int(), ctypes.c_int()
        assert getattr(L, f"hgemm_mi355x_{fam}_plan")(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0
        assert (cfg.value, splits.value) == (members[kind][0][1], want) and runs(L, kind, cfg.value, m, n, k, case.ld[kind]) == 1
        st, form, disp = decision(L, kind, cfg.value, splits.value, m, n, k, accumulate=1)
        assert (st, form, len(disp)) == (0, FORM_SPLITK, 2) and disp[0][3] == len(two_pass_cuts(k, splits.value)) + 1
        case.run_all_modes(g, L, kind, None, f"planned {kind}")
    assert case.operands_intact()


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["K=72", "M=100", "N=100"])
def test_what_the_kernels_do_not_take_is_answered_exactly_by_the_bf16_reference_kernels(g, L, members, what):
    m, n, k = {"K=72": (200, 136, 72), "M=100": (100, 136, 128), "N=100": (200, 100, 128)}[what]
    case = Case(m, n, k, m + n + k)
    for kind in KINDS:
        if what == "M=100" and kind == "nn":
            assert all(runs(L, kind, cid, m, n, k, case.ld[kind]) == 1 for _, cid in members[kind])   # (family n takes any M)
            continue
        for name, cid in members[kind]:
            assert runs(L, kind, cid, m, n, k, case.ld[kind]) == 0
            for word in (1, 4):
                assert decision(L, kind, cid, word, m, n, k)[:2] == (0, FORM_REFERENCE)
                case.run_all_modes(g, L, kind, (cid, word), f"{what} {kind} {name} {word}")
    assert case.operands_intact()


def test_a_pointer_8_bytes_off_is_answered_exactly_by_the_reference_kernels(g, L, members):
    m, n, k = 200, 136, 128
    case = Case(m, n, k, 41)
    old = case.old_values(43)
    for kind in KINDS:
        a = case.a_rows if kind == "nn" else case.a_cols
        dt, shift = (torch.float32, 2) if kind == "c32" else (torch.bfloat16, 4)
        for name, cid in members[kind][::3]:
            assert runs(L, kind, cid, m, n, k, case.ld[kind]) == 1 and decision(L, kind, cid, 1, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
            for word in (1, 4):
                for acc in (0, 1) if kind == "c32" else (0,):
                    flat = torch.full((m * n + 16,), SENTINEL, dtype=dt, device="cuda")
                    view = flat[shift:shift + m * n].view(m, n)
                    assert view.data_ptr() % 16 == 8
                    view.copy_(old if acc else torch.full_like(old, float("nan")))
                    if kind == "c32":
                        st = L.bgemm_mi355x_launch_ta_c32(cid, word, a.data_ptr(), case.bd.data_ptr(), view.data_ptr(), m, n, k, m, n, n, acc, g.stream())
                    else:
                        st = getattr(L, f"bgemm_mi355x_launch_{kind}")(cid, word, a.data_ptr(), case.bd.data_ptr(), view.data_ptr(), m, n, k, *case.ld[kind], g.stream())
                    assert st == 0, (kind, name, word, acc)
                    torch.cuda.synchronize()
                    want = case.product16 if kind != "c32" else (old + case.product if acc else case.product)
                    assert torch.equal(ibits(view), ibits(want)), (kind, name, word, acc)
                    assert bool((flat[:shift] == SENTINEL).all()) and bool((flat[shift + m * n:] == SENTINEL).all()), "the backing tensor changed"


# ---- N(0,1) operands -----------------------------------------------------------------------------------------------------------------
def test_randn_operands_meet_the_first_order_bound(g, L, members):
    """Per element |got - ref| <= K 2^-24 sum_k |a_k b_k| (the first-order bound of K fp32 adds at unit roundoff 2^-24; the products of
    two bf16 values are exact in fp32) + half a bf16 ulp of the result for the 16-bit C, against the fp64 product of the bf16-rounded
    operands.  The fp32 C has no ulp term.  Derived, not measured; no element is skipped.
    Half a bf16 ulp of a result in [2^e, 2^(e+1)) is 2^(e-8) -- eight bits of significand --, which lies between 2^-9 |ref| and 2^-8 |ref|.
    The flat figure 2^-9 |ref| is below it everywhere but at the top of a binade, and no implementation meets it: the test first shows
    that the fp64 product rounded to bf16 CORRECTLY misses 2^-9 |ref| on thousands of elements while it meets half an ulp on all.  (One run
    on one MI355X with the flat figure: worst error 1.82 of the bound for n64x64, plain.)"""
    m, n, k = 264, 264, 512
    rng = np.random.default_rng(13)
    a16 = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).to(torch.bfloat16)
    b16 = torch.from_numpy(rng.standard_normal((k, n)).astype(np.float32)).to(torch.bfloat16)
    a64, b64 = a16.double().numpy(), b16.double().numpy()
    ref = a64 @ b64
    mag = np.abs(a64) @ np.abs(b64)
    dev = {"nn": a16.cuda(), "ta": a16.t().contiguous().cuda()}
    dev["c32"] = dev["ta"]
    bd = b16.cuda()
    half_ulp = 2.0 ** (np.floor(np.log2(np.abs(ref))) - 8)
    assert (ref != 0).all() and (2.0 ** -9 * np.abs(ref) <= half_ulp).all() and (half_ulp <= 2.0 ** -8 * np.abs(ref)).all()
    ideal = np.abs(np.rint(ref / (2 * half_ulp)) * (2 * half_ulp) - ref)                  # the correctly rounded result's own error
    assert (ideal <= half_ulp).all() and int((ideal > 2.0 ** -9 * np.abs(ref)).sum()) > 1000
    for kind in KINDS:
        bound = k * 2.0 ** -24 * mag + (0.0 if kind == "c32" else half_ulp)
        ld = ((k if kind == "nn" else m), n, n)
        for name, cid in members[kind]:
            for word in FORMS:
                c = torch.full((m, n), float("nan"), dtype=torch.float32 if kind == "c32" else torch.bfloat16, device="cuda")
                if kind == "c32":
                    st = L.bgemm_mi355x_launch_ta_c32(cid, word, dev[kind].data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, *ld, 0, g.stream())
                else:
                    st = getattr(L, f"bgemm_mi355x_launch_{kind}")(cid, word, dev[kind].data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, *ld, g.stream())
                assert st == 0
                torch.cuda.synchronize()
                err = np.abs(c.double().cpu().numpy() - ref)
                worst = float((err / bound).max())
                print(f"{kind} {name} {hex(word)}: worst error {worst:.3f} of the bound")
                assert bool((err <= bound).all()), (kind, name, hex(word), worst)


# ---- capture -------------------------------------------------------------------------------------------------------------------------
def test_a_split_call_captured_without_a_workspace_runs_unsplit_and_split_after_the_reserve_call(g, L, members, evidence):
    """Nothing may be allocated while a stream captures: on a fresh stream with nothing reserved the split bgemm_mi355x_launch_ta call
    returns 0 and replays unsplit; after hgemm_mi355x_ta_reserve_workspace on another fresh stream it replays through its slabs.  Both
    exact (and the same bits: the sums are exact in any order).  One stream, one chain per graph: no parallel branches."""
    m, n, k = WS_SHAPE
    case = Case(m, n, k, 61)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.hgemm_mi355x_ta_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == 8
    cid = cfg.value
    assert decision(L, "ta", cid, splits.value, m, n, k)[1] == FORM_SPLITK
    assert L.hgemm_mi355x_ta_plan_workspace_bytes(cid, splits.value, m, n, k) == COUNTER_BYTES + 8 * m * n * 4
    for reserve in (False, True):
        buf = case.c_buffer("ta")
        s = torch.cuda.Stream()
        if reserve:
            assert L.hgemm_mi355x_ta_reserve_workspace(m, n, k, s.cuda_stream) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            rc = L.bgemm_mi355x_launch_ta(cid, splits.value, case.a_cols.data_ptr(), case.bd.data_ptr(), buf.data_ptr(), m, n, k, m, n, n,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, reserve
        for r in range(2):
            buf[:m, :n] = float("nan")
            torch.cuda.synchronize()
            graph.replay()
            case.check(buf, case.product16, f"replay {r}, reserved={reserve}")
    assert case.operands_intact()


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the bf16 NN and TA sets, 16-bit and fp32 C (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit, the fp32 C with accumulate = 0 and accumulate = 1 on a non-zero C32."""
    def one(kind, fn, **kw):
        c32 = kind == "c32"
        return g.HelperKernelSet(lambda cfg, word, p, d, acc: fn(cfg, word, p["a"], p["b"], p["c"], *d[:6], *([acc] if c32 else []), g.stream()),
                                 lambda cfg, word, d, aligned, acc: decision(L, kind, cfg, word, *d[:3], d[3:6], aligned, acc), torch.bfloat16, **kw)
    sets = [one("nn", L.bgemm_mi355x_launch_nn), one("ta", L.bgemm_mi355x_launch_ta, a_col=True),
            one("c32", L.bgemm_mi355x_launch_ta_c32, a_col=True, c32=True, accs=(0, 1))]
    for s in sets:
        s.check_combine(128, 2, 9131)
        s.check_combine(704, 11, 9131 + 1)
        s.check_reference(9131 + 2)
