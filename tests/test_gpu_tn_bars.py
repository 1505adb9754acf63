"""GPU tests that hold family "f" (hgemm_kernel_tn.hpp: bgemm_mi355x_tn, bgemm_mi355x_tn_bias and their launch_ forms) to the bars family n
is held to by tests/test_gpu_nn_bars.py (run with `-m gpu` on an MI355X); tests/test_gpu_tn_bf16.py and tests/test_gpu_tn_bias.py are the
family's first look, whose helpers these tests use.

Operands: oracle.bf16_dyadic_inputs -- bf16 values whose two lowest mantissa bits are live, in B (class "B"), in A ("A") or in both ("AB").
Every sum over any subset of K, in any order and grouping, is a whole number of 2^-7 (AB: 2^-14) below 2^23 of them: exact in fp32 like an
integer sum, but most results need a real rounding to bf16.  The expected C is the exact product (fp64, cast to fp32 with the cast asserted
exact; with a bias: one fp32 add of float(bias[n]) to it) rounded to bf16 once by torch's conversion, which Exact.want shows to be round to
nearest even.  tests/test_bf16_dyadic.py proves on the CPU, for these very operands and shapes, that the sums are order-independent, that
the expected matrices hold ties to both sides and plain round-ups, and that each mistake (truncation, ties away from zero, slabs held in
bf16, the bias added after the rounding, no bias) gives another matrix; it also feeds every such matrix to `compare` below, which must
reject it and name it.

1. Rounding: every member x form, _tn and _tn_bias, classes A / B / AB; the planned entries.
2. Long K: 127 stages.
3. The same operands through the other bf16 calls (families n and a, bf16 and fp32 C).
4. The 32-bit reach rule of TrLayout::reach_ok for family f, executed on both sides of its edge for A, b_col_major and C.
5. Rasters of more than eight tile rows (group_m = 8 with a ragged last group), with a per-column bias.
6. The workspace behaviour of bgemm_mi355x_launch_tn / _tn_bias: a lent buffer, two streams.
7. Misaligned A or b_col_major: the reference kernel answers.

Every comparison is bit for bit and unmasked.  C lies in [M + 1][ldc]: the window is prefilled with NaN, the pad columns and the guard row
hold a sentinel (-5 x 2^-20: no sum and no sum + bias is that) that must come back bit-unchanged; operand padding holds NaN, the bias
vector is followed by a NaN guard element, and operands and bias must be bit-unchanged afterwards: the conventions of
test_gpu_tn_bf16.Case / test_gpu_tn_bias.BiasCase, whose classes assert integer operands -- BarCase is their sibling for these."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from oracle import hgemm_oracle as O
from test_gpu_nn import MEMBERS as NN_MEMBERS
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import BK, COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, GIB, MEMBERS as TA_MEMBERS, two_pass_cuts
from test_gpu_tn_bf16 import MEMBERS, SHAPES
from test_gpu_tn_bf16 import decision as tn_decision
from test_gpu_tn_bias import EPI_C16_BIAS, EPI_SLAB, make_bias
from test_gpu_tn_bias import decision as bias_decision
from test_gpu_tr_bf16 import decision as tr_decision
from test_gpu_tr_bf16 import ibits

pytestmark = pytest.mark.gpu

SENTINEL = -5.0 * 2.0 ** -20                # a bf16 and an fp32 value; no multiple of 2^-14, so no sum and no sum + bias
TILES = dict(zip(MEMBERS, ((64, 64), (128, 64), (64, 128), (128, 128))))    # asserted against bgemm_mi355x_tn_config_info (infos)
CALLS = (False, True)                       # bgemm_mi355x_launch_tn, bgemm_mi355x_launch_tn_bias

# ---- the cases (tests/test_bf16_dyadic.py reads them through operand_sets) -------------------------------------------------------------
ROUNDING_SHAPES = {"A": SHAPES, "B": SHAPES, "AB": [(64, 64, 64), (136, 72, 128), (152, 152, 256)]}
PADDED_SHAPE = (136, 72, 128)               # run once more at Case's padded strides (K + 8, K + 16, N + 8)
PLANNED = (256, 264, 512)                   # 20 tiles of 64 x 64: the planner splits 8 ways
PLANNED_SPLITS = 8
LONG = (64, 64, 8128)                       # 127 stages, class B
LONG_FORMS = (1, 5)
OTHER_CALLS = [("A", (136, 72, 128)), ("B", (136, 72, 128)), ("A", (264, 264, 512)), ("B", (264, 264, 512)), ("AB", (152, 152, 256))]
OTHER_FORMS = (1, 5)
REACH_CASES = [  # (member, M, N, K, operand (0: A, 1: b_col_major, 2: C), bias form)
    ("f128x128_w2x2", 136, 64, 128, 0, False),         # a second, ragged row band whose base lies just below the limit
    ("f64x128_w2x2", 64, 136, 128, 1, False),          # a second, ragged column tile: descriptor base at row 128 of b_col_major
    ("f64x64_w2x2", 72, 136, 128, 2, False),           # the C descriptor of the buffer stores; the combine's 64-bit stores when split
    ("f64x64_w2x2", 72, 136, 128, 2, True),
]
RASTERS = [(1160, 136, 128), (520, 1096, 64)]
WS_SHAPE = (200, 264, 512)
WS_SPLITS = 4
WS_FILL = 0xA5A5A5A5                        # of a lent workspace: as fp32 a negative number below 1e-15 in magnitude
MISALIGNED = (200, 136, 128)


def cut_sets_of(k, words):
    return sorted({tuple(two_pass_cuts(k, w)) for w in words if (w & 0xFFFF) > 1 and two_pass_cuts(k, w)})


def operand_sets():
    """[(class, shape, seed, K cut sets of the split forms run there, section)] of every operand pair the tests below draw."""
    sets = [(side, shape, sum(shape), cut_sets_of(shape[2], FORMS), "rounding") for side in ("A", "B", "AB") for shape in ROUNDING_SHAPES[side]]
    sets += [(side, PLANNED, sum(PLANNED), cut_sets_of(PLANNED[2], (PLANNED_SPLITS,)), "planned") for side in ("A", "B")]
    sets += [("B", LONG, sum(LONG), cut_sets_of(LONG[2], LONG_FORMS), "long K")]
    sets += [("B", (m, n, k), m + n + k, cut_sets_of(k, (2,)), "reach") for _, m, n, k, side, biased in REACH_CASES if not biased]
    sets += [("B", shape, sum(shape), cut_sets_of(shape[2], FORMS), "raster") for shape in RASTERS]
    sets += [("B", WS_SHAPE, sum(WS_SHAPE) + i, cut_sets_of(WS_SHAPE[2], (WS_SPLITS,)), "workspace") for i in (0, 1)]
    sets += [("B", MISALIGNED, sum(MISALIGNED), [], "misaligned")]
    assert all(shape in ROUNDING_SHAPES[side] and set(OTHER_FORMS) <= set(FORMS) for side, shape in OTHER_CALLS)     # section 3 draws nothing new
    return sets


# ---- the reference, all on the CPU -----------------------------------------------------------------------------------------------------
class Exact:
    """One operand pair of a class at a shape (seed M + N + K unless named), its exact product as fp32, the bias of
    test_gpu_tn_bias.make_bias for its N, and what each call must store -- as bf16 bit patterns -- next to what each mistake would."""

    def __init__(self, side, shape, seed=None):
        self.side, self.shape, self.seed = side, tuple(shape), sum(shape) if seed is None else seed
        m, n, k = shape
        self.a, self.b = O.bf16_dyadic_inputs(m, n, k, np.random.default_rng(self.seed), side)
        self.s32 = O.bf16_exact_product(self.a, self.b, side)                     # asserts the class and the exactness rule
        self.bias = make_bias(n, self.seed).float().numpy()
        self.sb32 = self.s32 + self.bias[None, :]                                 # the one fp32 add of the bias form
        self.bias_add_exact = np.array_equal(self.sb32.astype(np.float64), self.s32.astype(np.float64) + self.bias.astype(np.float64)[None, :])
        self._want, self._mutants = {}, {}

    def value32(self, biased):
        return self.sb32 if biased else self.s32

    def want(self, biased):
        if biased not in self._want:
            rne = O.bf16_roundings(self.value32(biased))[0]
            by_torch = torch.from_numpy(self.value32(biased)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            assert np.array_equal(rne, by_torch), "torch's bf16 conversion is not round to nearest even"
            self._want[biased] = rne
        return self._want[biased]

    def mutants(self, biased, cut_sets=()):
        """{name: bit patterns} of what each mistake would store."""
        key = (biased, tuple(map(tuple, cut_sets)))
        if key not in self._mutants:
            _, trunc, away = O.bf16_roundings(self.value32(biased))
            out = {"truncation": trunc, "round-half-away": away}
            for cuts in cut_sets:
                if cuts:
                    out[f"bf16 slabs (K cut at {list(cuts)})"] = O.bf16_partials(self.a, self.b, self.side, cuts, self.bias if biased else None)
            if biased:
                out["twice-rounded bias"] = O.bf16_roundings(O.bf16_to_f32(self.want(False)) + self.bias[None, :])[0]
                out["no bias"] = self.want(False)
            self._mutants[key] = out
        return self._mutants[key]

    def slab_sums(self, cuts):
        edges = [0, *cuts, self.shape[2]]
        return [O.bf16_exact_product(self.a[:, lo:hi], self.b[lo:hi], self.side) for lo, hi in zip(edges, edges[1:])]


@functools.lru_cache(maxsize=None)
def _exact(side, shape, seed):
    return Exact(side, shape, seed)


def exact(side, shape, seed=None):
    """Built once per (class, shape, seed) and shared by every test; nothing writes to it."""
    return _exact(side, tuple(shape), sum(shape) if seed is None else seed)


def compare(ex, biased, got_bits, cut_sets=(), what=""):
    """None if `got_bits` (uint16 bf16 patterns, [M][N]) is what the call must store, else the finding: how many elements differ and
    which mistake they equal (as test_gpu_rounding.name_the_fault)."""
    want = ex.want(biased)
    assert got_bits.dtype == np.uint16 and got_bits.shape == want.shape
    bad = got_bits != want
    if not bad.any():
        return None
    said = []
    for name, mu in ex.mutants(biased, cut_sets).items():
        if np.array_equal(got_bits, mu):
            said.append(f"the whole result equals the {name} mutant")
        else:
            said.append(f"{int((got_bits[bad] == mu[bad]).sum())} of {int(bad.sum())} differing elements equal the {name} mutant")
    nearer = int((np.abs(O.bf16_to_f32(got_bits)[bad].astype(np.float64)) < np.abs(ex.value32(biased)[bad].astype(np.float64))).sum())
    first = tuple(int(i) for i in np.argwhere(bad)[0])
    return (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {first}: got {O.bf16_to_f32(got_bits)[first]!r} for "
            f"{ex.value32(biased)[first]!r}\n    " + "; ".join(said) + f"; {nearer} of them lie nearer to zero than the exact value")


# ---- the device side -------------------------------------------------------------------------------------------------------------------
def to_device_bf16(x32):
    t = torch.from_numpy(np.ascontiguousarray(x32)).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy().view(np.uint32), np.ascontiguousarray(x32).view(np.uint32)), "an operand is no bf16 value"
    return t.cuda()


def same_bits(x, value):
    want = ibits(torch.full((1,), value, dtype=x.dtype, device=x.device))
    return bool((ibits(x) == want).all())


class BarCase:
    """An Exact on the device as family f reads it: A in [M][lda], B as b_col_major [N][ldb], NaN in all padding, the bias vector with
    a NaN guard element behind it."""

    def __init__(self, ex, padded=False):
        self.ex = ex
        self.m, self.n, self.k = m, n, k = ex.shape
        self.ld = (k + 8, k + 16, n + 8) if padded else (k, k, n)
        self.ad = torch.full((m, self.ld[0]), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.ad[:, :k] = to_device_bf16(ex.a)
        self.wd = torch.full((n, self.ld[1]), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.wd[:, :k] = to_device_bf16(ex.b.T)
        self.bias_buf = torch.full((n + 1,), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.bias_buf[:n] = to_device_bf16(ex.bias)
        self.bias_d = self.bias_buf[:n]
        assert self.bias_d.data_ptr() % 16 == 0
        self.before = [x.clone() for x in (self.ad, self.wd, self.bias_buf)]

    def c_buffer(self):
        buf = torch.full((self.m + 1, self.ld[2]), SENTINEL, dtype=torch.bfloat16, device="cuda")
        buf[:self.m, :self.n] = float("nan")
        return buf

    def launch(self, g, L, buf, plan, biased, stream=None):
        m, n, k = self.m, self.n, self.k
        ptrs = [self.ad.data_ptr(), self.wd.data_ptr()] + ([self.bias_d.data_ptr()] if biased else []) + [buf.data_ptr()]
        stream = g.stream() if stream is None else stream
        if plan is None:
            assert self.ld == (k, k, n)
            st = (L.bgemm_mi355x_tn_bias if biased else L.bgemm_mi355x_tn)(*ptrs, m, n, k, stream)
        else:
            st = (L.bgemm_mi355x_launch_tn_bias if biased else L.bgemm_mi355x_launch_tn)(plan[0], plan[1], *ptrs, m, n, k, *self.ld, stream)
        assert st == 0, (plan, biased, L.hgemm_mi355x_strerror(st))

    def verdict(self, buf, biased, what, cut_sets=()):
        """None, or what is wrong with a finished call's C buffer."""
        torch.cuda.synchronize()
        said = compare(self.ex, biased, ibits(buf[:self.m, :self.n]).cpu().numpy().view(np.uint16), cut_sets, what)
        if not (same_bits(buf[:self.m, self.n:], SENTINEL) and same_bits(buf[self.m], SENTINEL)):
            said = (said + "\n" if said else "") + f"{what}: the pad or the guard row changed"
        return said

    def operands_intact(self):
        return all(torch.equal(ibits(x), ibits(was)) for x, was in zip((self.ad, self.wd, self.bias_buf), self.before))


class Runs:
    """The runs of one test: every wrong result is kept with the mistake it matches, and all of them fail the test at the end."""

    def __init__(self, g, L):
        self.g, self.L, self.lines, self.runs, self.t0 = g, L, [], 0, time.perf_counter()

    def run(self, case, plan, biased, what, cut_sets=()):
        buf = case.c_buffer()
        case.launch(self.g, self.L, buf, plan, biased)
        self.runs += 1
        said = case.verdict(buf, biased, f"{'tn_bias' if biased else 'tn'} {what} {case.m}x{case.n}x{case.k} ld={case.ld} class {case.ex.side}", cut_sets)
        if said:
            self.lines.append(said)

    def close(self, what, expect_runs):
        print(f"{what}: {self.runs} launches, {len(self.lines)} wrong, {time.perf_counter() - self.t0:.2f} s")
        assert not self.lines, f"{what}: {len(self.lines)} of {self.runs} runs are wrong:\n" + "\n".join(self.lines)
        assert self.runs == expect_runs, (self.runs, expect_runs)


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    lib.bgemm_mi355x_tn.argtypes = [p] * 3 + [i] * 3 + [p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    lib.bgemm_mi355x_tn_bias.argtypes = [p] * 4 + [i] * 3 + [p]
    lib.bgemm_mi355x_tn_plan_workspace_bytes.restype, lib.bgemm_mi355x_tn_plan_workspace_bytes.argtypes = ctypes.c_size_t, [i] * 5
    lib.hgemm_mi355x_set_workspace.argtypes = [p, ctypes.c_size_t]
    for fam in ("nn", "ta"):
        getattr(lib, f"hgemm_mi355x_{fam}_config_by_name").argtypes = [ctypes.c_char_p]
        getattr(lib, f"bgemm_mi355x_launch_{fam}").argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    lib.bgemm_mi355x_launch_ta_c32.argtypes = [i] * 2 + [p] * 3 + [i] * 7 + [p]
    return lib


@pytest.fixture(scope="module")
def infos(L):
    """[(name, id, BM, BN)] of the family's members."""
    out = []
    for want, name in enumerate(MEMBERS):
        cid = L.bgemm_mi355x_tn_config_by_name(name.encode())
        info = (ctypes.c_int * 8)()
        assert cid == want and L.bgemm_mi355x_tn_config_info(cid, info) == 0 and (info[0], info[1]) == TILES[name], name
        out.append((name, cid, info[0], info[1]))
    return out


def decide(L, biased, *args, **kw):
    return (bias_decision if biased else tn_decision)(L, *args, **kw)


def kernel_runs(L, biased, cid, m, n, k, ld):
    return (L.bgemm_mi355x_tn_bias_runs if biased else L.bgemm_mi355x_tn_runs)(cid, m, n, k, *ld)


def runs_as_requested(L, biased, cid, word, m, n, k, ld=None):
    """Plain for a split count of 1, else two-pass with the split count the clamp rule gives; the bias form's epilogue ids."""
    st, form, disp = decide(L, biased, cid, word, m, n, k, ld)
    cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
    epis = [d[2] for d in disp]
    ok = (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1)
    return ok and (not biased or epis == ([EPI_SLAB, EPI_C16_BIAS] if cuts else [EPI_C16_BIAS]))


def sweep(r, L, infos, case, words, cut_sets):
    """Every member x word x call on one case, each asserted to run as the word asks."""
    m, n, k = case.ex.shape
    for name, cid, *_ in infos:
        for biased in CALLS:
            assert kernel_runs(L, biased, cid, m, n, k, case.ld) == 1, (name, biased, case.ex.shape, case.ld)
            for word in words:
                assert runs_as_requested(L, biased, cid, word, m, n, k, case.ld), (name, biased, hex(word), decide(L, biased, cid, word, m, n, k, case.ld))
                r.run(case, (cid, word), biased, f"{name} {hex(word)}", cut_sets)


# ---- 1. rounding -----------------------------------------------------------------------------------------------------------------------
ROUNDING_PARAMS = [(side, shape, False) for side in ("A", "B", "AB") for shape in ROUNDING_SHAPES[side]] + [(side, PADDED_SHAPE, True) for side in ("A", "B", "AB")]


@pytest.mark.parametrize("side,shape,padded", ROUNDING_PARAMS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else {True: "padded", False: "contiguous"}.get(v, v))
def test_every_member_form_and_call_rounds_to_nearest_even(g, L, infos, side, shape, padded):
    """One tile and one stage; ragged M and N tiles with clamped b_col_major rows; the ring wraps and the cuts are uneven; three tiles
    each way for the largest member -- on operands whose mantissa bits are live, through the plain store, its non-temporal twin, the
    slab epilogue + combine (2 and 5 splits, clamped to one per stage) and, with the bias, the EPI_C16_BIAS kernels and the bias combine."""
    case = BarCase(exact(side, shape), padded)
    r = Runs(g, L)
    sweep(r, L, infos, case, FORMS, cut_sets_of(shape[2], FORMS))
    assert case.operands_intact()
    r.close(f"rounding class {side} {shape} {'padded' if padded else 'contiguous'}", len(MEMBERS) * len(FORMS) * len(CALLS))


@pytest.mark.parametrize("side", ["A", "B"])
def test_the_planned_entries_round_to_nearest_even_through_their_split_plan(g, L, side):
    """bgemm_mi355x_tn / _tn_bias at 256 x 264 x 512: the planner takes the 64 x 64 member in eight two-pass splits, so the planned split
    path -- the stream workspace, the slab epilogue and both combines -- carries values that need rounding."""
    m, n, k = PLANNED
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and (cfg.value, splits.value) == (0, PLANNED_SPLITS)
    case = BarCase(exact(side, PLANNED))
    r = Runs(g, L)
    for biased in CALLS:
        assert kernel_runs(L, biased, cfg.value, m, n, k, case.ld) == 1 and runs_as_requested(L, biased, cfg.value, splits.value, m, n, k)
        r.run(case, None, biased, "planned entry", cut_sets_of(k, (PLANNED_SPLITS,)))
    assert case.operands_intact()
    r.close(f"rounding planned entries class {side}", len(CALLS))


# ---- 2. long K -------------------------------------------------------------------------------------------------------------------------
def test_long_k_rounds_to_nearest_even(g, L, infos):
    """64 x 64 x 8128: 127 stages through the family's own kbyte advance and ring, plain and in five chunks of 26 / 23 stages."""
    m, n, k = LONG
    assert k % BK == 0 and k // BK == 127 and two_pass_cuts(k, 5) == [26 * BK * i for i in range(1, 5)]
    case = BarCase(exact("B", LONG))
    r = Runs(g, L)
    sweep(r, L, infos, case, LONG_FORMS, cut_sets_of(k, LONG_FORMS))
    assert case.operands_intact()
    r.close("rounding long K", len(MEMBERS) * len(LONG_FORMS) * len(CALLS))


# ---- 3. the same operands through the other bf16 calls -----------------------------------------------------------------------------------
class TrBarCase:
    """An Exact laid out as test_gpu_tr_bf16.Case lays its operands out, contiguous: A in [M][K] for family n, a_col_major [K][M] for
    family a, B in [K][N]."""

    def __init__(self, ex):
        self.ex = ex
        self.m, self.n, self.k = m, n, k = ex.shape
        self.ld = {"nn": (k, n, n), "ta": (m, n, n), "c32": (m, n, n)}
        self.a_rows, self.a_cols, self.bd = to_device_bf16(ex.a), to_device_bf16(ex.a.T), to_device_bf16(ex.b)
        self.before = [x.clone() for x in (self.a_rows, self.a_cols, self.bd)]
        self.want32 = torch.from_numpy(ex.s32.view(np.int32)).cuda()

    def run(self, g, L, kind, plan, what, cut_sets):
        m, n, k = self.m, self.n, self.k
        buf = torch.full((m + 1, n), SENTINEL, dtype=torch.float32 if kind == "c32" else torch.bfloat16, device="cuda")
        buf[:m] = float("nan")
        a = self.a_rows if kind == "nn" else self.a_cols
        if kind == "c32":
            st = L.bgemm_mi355x_launch_ta_c32(plan[0], plan[1], a.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), m, n, k, *self.ld[kind], 0, g.stream())
        else:
            st = getattr(L, f"bgemm_mi355x_launch_{kind}")(plan[0], plan[1], a.data_ptr(), self.bd.data_ptr(), buf.data_ptr(), m, n, k, *self.ld[kind], g.stream())
        assert st == 0, (kind, plan, L.hgemm_mi355x_strerror(st))
        torch.cuda.synchronize()
        if kind == "c32":                     # the fp32 C: the exact sum, no rounding at all
            bad = int((ibits(buf[:m]) != self.want32).sum())
            said = f"{what}: {bad} of {m * n} elements differ from the exact fp32 sum" if bad else None
        else:
            said = compare(self.ex, False, ibits(buf[:m]).cpu().numpy().view(np.uint16), cut_sets, what)
        if not same_bits(buf[m], SENTINEL):
            said = (said + "\n" if said else "") + f"{what}: the guard row changed"
        return said


@pytest.mark.parametrize("side,shape", OTHER_CALLS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_the_other_bf16_calls_round_the_same_operands_to_nearest_even(g, L, side, shape):
    """bgemm_mi355x_launch_nn, _launch_ta and _launch_ta_c32 (store mode) on the operand pairs of section 1: the bf16 MFMA paths of
    families n and a had only integer operands in their bit-exact tests.  Plain and five splits, every member."""
    m, n, k = shape
    case = TrBarCase(exact(side, shape))
    members = {"nn": NN_MEMBERS, "ta": TA_MEMBERS, "c32": TA_MEMBERS}
    lines, ran, t0 = [], 0, time.perf_counter()
    for kind in ("nn", "ta", "c32"):
        for name in members[kind]:
            cid = getattr(L, f"hgemm_mi355x_{'nn' if kind == 'nn' else 'ta'}_config_by_name")(name.encode())
            assert cid >= 0, name
            for word in OTHER_FORMS:
                st, form, disp = tr_decision(L, kind, cid, word, m, n, k)
                cuts = two_pass_cuts(k, word) if word > 1 else []
                assert (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1), (kind, name, word)
                said = case.run(g, L, kind, (cid, word), f"{kind} {name} {hex(word)} {m}x{n}x{k} class {side}", cut_sets_of(k, OTHER_FORMS))
                ran += 1
                if said:
                    lines.append(said)
    print(f"other bf16 calls class {side} {shape}: {ran} launches, {len(lines)} wrong, {time.perf_counter() - t0:.2f} s")
    assert not lines, "\n".join(lines)
    assert ran == 3 * 4 * len(OTHER_FORMS) and all(torch.equal(ibits(x), ibits(was)) for x, was in zip((case.a_rows, case.a_cols, case.bd), case.before))


# ---- 4. the reach rule, both sides executed ----------------------------------------------------------------------------------------------
def largest_stride(runs, least):
    """The largest stride (a multiple of 8, from `least` on) at which runs(stride) still holds -- by bisection; runs is monotone in the
    stride (a call's _runs function with every other argument fixed)."""
    lo, hi = least // 8, 1 << 27                       # 8 x 2^27 = 2^30 elements: beyond the reach of every member and K >= 64
    assert runs(8 * lo) and not runs(8 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if runs(8 * mid) else (lo, mid)
    return 8 * lo


def largest_tn_stride(L, biased, cid, m, n, k, side):
    """The largest stride (a multiple of 8) of operand `side` at which the member's kernel still runs, the other two contiguous -- by
    bisection over bgemm_mi355x_tn_runs (_tn_bias_runs), which is monotone in the stride."""
    def runs(s):
        lds = [k, k, n]
        lds[side] = s
        return kernel_runs(L, biased, cid, m, n, k, lds) == 1

    return largest_stride(runs, (k, k, n)[side])


def reach_rule(bm, bn, n, k, side):
    """(rows, tail bytes) of TrLayout::reach_ok's limit on operand `side` of family f: rows x ld x 2 + tail < 2 GiB.  All three are
    addressed from a tile's first row: BM rows of A and then the row's K elements, BN rows of b_col_major and K, BM rows of C and N."""
    return ((bm, 2 * k), (bn, 2 * k), (bm, 2 * n))[side]


def all_same_bits(flat, value):
    step = 1 << 28
    return all(same_bits(flat[i:i + step], value) for i in range(0, flat.numel(), step))


@pytest.mark.parametrize("case", REACH_CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1:4]))}-{'ABC'[c[4]]}{'-bias' if c[5] else ''}")
def test_tn_reach_edges_run_exact_on_both_sides(g, L, infos, case):
    """The largest stride at which the member's kernel still runs and the next multiple of 8 (the reference kernel, 64-bit addressing),
    both executed, plain and in two splits.  The operand lives in a flat buffer filled with NaN (C: with -3.0) that must come back
    unchanged outside the operand's window."""
    name, m, n, k, side, biased = case
    _, cid, bm, bn = next(i for i in infos if i[0] == name)
    s = largest_tn_stride(L, biased, cid, m, n, k, side)
    rows_rule, tail = reach_rule(bm, bn, n, k, side)
    assert rows_rule * s * 2 + tail < 2 * GIB <= rows_rule * (s + 8) * 2 + tail, (s, rows_rule, tail)     # the documented rule
    if side == 1:
        assert n > bn and (rows_rule, tail) == (bn, 2 * k)         # a second column tile: its descriptor starts at row BN of b_col_major
    ex = exact("B", (m, n, k))
    want = torch.from_numpy(ex.want(biased).view(np.int16))
    rows, cols = [(m, k), (n, k), (m, n)][side]
    pad_value = -3.0 if side == 2 else float("nan")
    flat = torch.full((rows * (s + 8),), pad_value, dtype=torch.bfloat16, device="cuda")
    a, w, bias = to_device_bf16(ex.a), to_device_bf16(ex.b.T), to_device_bf16(ex.bias)
    ran = 0
    for stride, runs in ((s, 1), (s + 8, 0)):
        lds = [k, k, n]
        lds[side] = stride
        assert kernel_runs(L, biased, cid, m, n, k, lds) == runs
        window = flat.as_strided((rows, cols), (stride, 1))
        for word in (1, 2):
            st, form, disp = decide(L, biased, cid, word, m, n, k, lds)
            assert (st, form) == (0, FORM_REFERENCE if not runs else FORM_PLAIN if word == 1 else FORM_SPLITK), (stride, word, st, form)
            assert not runs or disp[0][3] == word
            c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            if side == 2:
                window.fill_(float("nan"))
                c = window
            else:
                window.copy_([a, w][side])
            ops = [a, w, c]
            ops[side] = flat
            ptrs = [ops[0].data_ptr(), ops[1].data_ptr()] + ([bias.data_ptr()] if biased else []) + [ops[2].data_ptr()]
            st = (L.bgemm_mi355x_launch_tn_bias if biased else L.bgemm_mi355x_launch_tn)(cid, word, *ptrs, m, n, k, *lds, g.stream())
            assert st == 0, L.hgemm_mi355x_strerror(st)
            torch.cuda.synchronize()
            got = ibits(c).cpu()
            said = compare(ex, biased, got.numpy().view(np.uint16), cut_sets_of(k, (2,)), f"{name} {'ABC'[side]} stride {stride} word {word}")
            assert said is None and torch.equal(got, want), said
            window.fill_(pad_value)
            assert all_same_bits(flat, pad_value), (name, "ABC"[side], stride, word, "the buffer changed outside the operand's window")
            ran += 1
    print(f"reach {name} {'ABC'[side]}{' bias' if biased else ''}: edge stride {s}, {ran} launches, buffer {flat.numel() * 2 / 1e9:.2f} GB")
    del flat, window, c
    torch.cuda.empty_cache()


# ---- 5. rasters of more than eight tile rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RASTERS, ids=lambda s: "x".join(map(str, s)))
def test_rasters_of_more_than_eight_tile_rows_are_exact(g, L, infos, shape):
    """group_m = min(tiles_m, 8): (1160, 136, 128) has 19 / 10 tile rows -- two whole groups and a ragged third, ragged M, split items
    walking the same raster; (520, 1096, 64) has 9 / 5 tile rows against 18 / 9 column tiles and one stage, so every split count is
    clamped to 1.  The bias is pairwise distinct over all N columns: a tile that adds another column tile's bias shows."""
    m, n, k = shape
    tiles_m = {name: -(-m // bm) for name, _, bm, _ in infos}
    assert all(tiles_m[name] > 8 and tiles_m[name] % 8 for name, _, bm, _ in infos if bm == 64), tiles_m
    ex = exact("B", shape)
    assert len(set(ex.bias.tolist())) == n and ex.bias_add_exact
    case = BarCase(ex)
    r = Runs(g, L)
    sweep(r, L, infos, case, FORMS, cut_sets_of(k, FORMS))
    assert case.operands_intact()
    r.close(f"raster {shape}", len(MEMBERS) * len(FORMS) * len(CALLS))


# ---- 6. the workspace behaviour of bgemm_mi355x_launch_tn / _tn_bias -----------------------------------------------------------------------
def test_a_lent_workspace_too_small_runs_unsplit_and_one_of_the_plan_size_runs_split(g, L, infos):
    """The lent buffer is filled with a byte pattern no slab holds (0xA5A5A5A5 is a negative fp32 below 1e-15 in magnitude; a class-B
    partial sum is a multiple of 2^-7 -- checked on the four slabs' own sums).  Too small for the slabs: the result is exact and the bytes
    behind the counters are untouched, so the plan ran unsplit.  bgemm_mi355x_tn_plan_workspace_bytes: exact, and every fp32 of the four
    slabs has been written."""
    m, n, k = WS_SHAPE
    ex = exact("B", WS_SHAPE, sum(WS_SHAPE))
    cuts = two_pass_cuts(k, WS_SPLITS)
    assert len(cuts) == WS_SPLITS - 1 and not any((s.view(np.uint32) == WS_FILL).any() for s in ex.slab_sums(cuts))
    assert -1e-15 < np.array([WS_FILL], dtype=np.uint32).view(np.float32)[0] < 0
    case = BarCase(ex)
    r = Runs(g, L)
    try:
        for name, cid, *_ in infos:
            need = int(L.bgemm_mi355x_tn_plan_workspace_bytes(cid, WS_SPLITS, m, n, k))
            assert need == COUNTER_BYTES + WS_SPLITS * m * n * 4
            for biased in CALLS:
                assert decide(L, biased, cid, WS_SPLITS, m, n, k)[1] == FORM_SPLITK
                for size, split in ((COUNTER_BYTES + 1024, False), (need, True)):
                    lent = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
                    assert L.hgemm_mi355x_set_workspace(lent.data_ptr(), size) == 0
                    r.run(case, (cid, WS_SPLITS), biased, f"{name}, lent workspace of {size} bytes", [cuts])
                    slabs = lent[COUNTER_BYTES:]
                    if split:
                        words = slabs.view(torch.int32)
                        assert int((words == words.new_tensor(WS_FILL - (1 << 32))).sum()) == 0, (name, biased, "a slab element was not written: the plan did not run split")
                    else:
                        assert bool((slabs == 0xA5).all()), (name, biased, "the plan wrote behind a buffer too small for its slabs")
                    assert L.hgemm_mi355x_set_workspace(None, 0) == 0
    finally:
        assert L.hgemm_mi355x_set_workspace(None, 0) == 0
    r.run(case, (0, WS_SPLITS), True, "after the workspace was taken back", [cuts])
    assert case.operands_intact()
    r.close("lent workspace", len(MEMBERS) * len(CALLS) * 2 + 1)


def test_tn_split_k_on_two_streams_does_not_share_partials(g, L, infos):
    """The same split plan on two streams at once, different operands and different biases: each stream has slabs of its own, and the
    bias combine reads its own stream's.  20 rounds, one synchronize, no graphs."""
    m, n, k = WS_SHAPE
    cases = [BarCase(exact("B", WS_SHAPE, sum(WS_SHAPE) + i)) for i in (0, 1)]
    for biased in CALLS:
        assert not np.array_equal(cases[0].ex.want(biased), cases[1].ex.want(biased))
    assert not np.array_equal(cases[0].ex.bias, cases[1].ex.bias)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cuts = two_pass_cuts(k, WS_SPLITS)
    lines, launches, t0 = [], 0, time.perf_counter()
    torch.cuda.synchronize()
    for name, cid, *_ in infos:
        for biased in CALLS:
            assert decide(L, biased, cid, WS_SPLITS, m, n, k)[1] == FORM_SPLITK
            outs = [case.c_buffer() for case in cases]
            torch.cuda.synchronize()
            for rep in range(20):
                for case, st, buf in zip(cases, streams, outs):
                    case.launch(g, L, buf, (cid, WS_SPLITS), biased, stream=st.cuda_stream)
                    launches += 1
            torch.cuda.synchronize()
            for i, (case, buf) in enumerate(zip(cases, outs)):
                said = case.verdict(buf, biased, f"{name} {'tn_bias' if biased else 'tn'} stream {i}", [cuts])
                if said:
                    lines.append(said)
    print(f"two streams: {launches} launches, {len(lines)} wrong, {time.perf_counter() - t0:.2f} s")
    assert not lines, "\n".join(lines)
    assert launches == len(MEMBERS) * len(CALLS) * 40 and all(case.operands_intact() for case in cases)


# ---- 7. misaligned A or b_col_major --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1], ids=["A", "W"])
def test_a_misaligned_a_or_w_is_answered_exactly_by_the_reference_kernel(g, L, infos, side):
    """A, then b_col_major, starts 4 elements (8 bytes) into a larger tensor, strides unchanged: 8-byte aligned, not 16.  Status 0, exact,
    and the backing tensor unchanged around and inside the operand -- whatever split count is named."""
    m, n, k = MISALIGNED
    ex = exact("B", MISALIGNED)
    case = BarCase(ex)
    rows, cols = [(m, k), (n, k)][side]
    flat = torch.full((rows * cols + 8,), float("nan"), dtype=torch.bfloat16, device="cuda")
    view = flat[4:4 + rows * cols].view(rows, cols)
    view.copy_([case.ad, case.wd][side])
    assert view.data_ptr() % 16 == 8
    before = flat.clone()
    if side == 0:
        case.ad = view
    else:
        case.wd = view
    r = Runs(g, L)
    for name, cid, *_ in infos[::3]:
        for biased in CALLS:
            assert kernel_runs(L, biased, cid, m, n, k, case.ld) == 1 and decide(L, biased, cid, 1, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
            for word in (1, 4):
                r.run(case, (cid, word), biased, f"{name} {word}, {'AW'[side]} 8 bytes off")
    assert torch.equal(ibits(flat), ibits(before)), "the backing tensor changed"
    assert torch.equal(ibits(case.bias_buf), ibits(case.before[2]))
    r.close(f"misaligned {'AW'[side]}", 2 * len(CALLS) * 2)
