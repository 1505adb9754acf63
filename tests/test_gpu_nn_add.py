"""GPU tests of the input gradient with a fused residual add, bgemm_mi355x_nn_add: C = bf16(S + float(r[m][n])), family n's kernels of
hgemm_inst_g22.hip, the combine of the two-pass form and the reference kernel (OutAdd) -- and of one gated layer's whole call sequence,
tn_gated_aux -> tn_bias_add -> nn_dgated -> nn_add at K = 2N, each step against torch on the CPU.

tests/residual_common.py has the operands and the expectation: S is exact in fp32 in any order, so the result is defined bit for bit by one
IEEE fp32 add and one rounding.  Every comparison is on bits.  Outputs start as NaN inside and a sentinel outside their M x N elements; the
sentinel and every input must come back unchanged (residual_common.run)."""
import ctypes

import numpy as np
import pytest
import torch

import residual_common as rc
from residual_common import FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, SHAPES, WORDS, bits
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)

pytestmark = pytest.mark.gpu

KIND = "nn"
MEMBERS = ("n64x64_w2x2", "n128x64_w2x2", "n64x128_w2x2", "n128x128_w2x2")
BIG = (152, 152, 320)


@pytest.fixture(scope="module")
def L(g):
    lib = rc.prototypes(g.lib())
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_nn.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    lib.bgemm_mi355x_launch_tn_gated_aux.argtypes = [i] * 2 + [p] * 8 + [i] * 8 + [p]
    lib.bgemm_mi355x_launch_nn_dgated.argtypes = [i] * 2 + [p] * 6 + [i] * 8 + [p]
    assert [lib.hgemm_mi355x_nn_config_by_name(nm.encode()) for nm in MEMBERS] == [0, 1, 2, 3]
    return lib


@pytest.fixture(scope="module")
def cases():
    return {shape: rc.Ops(*shape) for shape in SHAPES}


def form_of(word, k):
    return FORM_SPLITK if min(word & 0xffff, k // 64) > 1 else FORM_PLAIN


def same(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_and_word_is_the_cpu_result_bit_for_bit(g, L, cases, shape, padded):
    """All four members, the plain launch, the NT store and the two split words; padded strides have ldr != ldc."""
    ops = cases[shape]
    m, n, k = shape
    lds = (k + 8, n + 16, n + 8, n + 24) if padded else None
    expect = rc.want(KIND, ops)
    for cid in range(4):
        for word in WORDS:
            what = f"{MEMBERS[cid]} {hex(word)} {shape} {'padded' if padded else 'contiguous'}"
            got = rc.run(L, KIND, ops, cid, word, lds, want_form=form_of(word, k), stream=g.stream(), what=what)
            assert same(got, expect), f"{what}: {rc.differing(got, expect)} elements differ"


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
def test_in_place_equals_out_of_place_for_every_member_and_word(g, L, cases, padded):
    """r == c, ldr == ldc: each C[m][n] from the old r[m][n]; the pad columns of c stay (residual_common.run checks them)."""
    ops = cases[BIG]
    m, n, k = BIG
    lds = (k, n, n + 8, n + 8) if padded else None
    expect = rc.want(KIND, ops)
    for cid in range(4):
        for word in WORDS:
            what = f"in place {MEMBERS[cid]} {hex(word)}"
            there = rc.run(L, KIND, ops, cid, word, lds, want_form=form_of(word, k), stream=g.stream(), what=what)
            here = rc.run(L, KIND, ops, cid, word, lds, inplace=True, want_form=form_of(word, k), stream=g.stream(), what=what)
            assert same(here, there) and same(here, expect), what


@pytest.mark.parametrize("why", ["r 2 bytes off", "ldr % 8 == 4", "in place with ldc % 8 == 4"])
def test_the_reference_form_gives_the_same_bits(g, L, cases, why):
    for shape in ((136, 72, 128), BIG):
        ops = cases[shape]
        m, n, k = shape
        lds = {"r 2 bytes off": None, "ldr % 8 == 4": (k, n, n, n + 4), "in place with ldc % 8 == 4": (k, n, n + 4, n + 4)}[why]
        for cid, word in ((0, 1), (3, 2)):
            got = rc.run(L, KIND, ops, cid, word, lds, inplace=why.startswith("in place"), off_r=1 if why.startswith("r 2") else 0,
                         want_form=FORM_REFERENCE, stream=g.stream(), what=why)
            assert same(got, rc.want(KIND, ops)), (why, shape, cid, word)


def test_the_planned_entry_point(g, L, cases):
    for shape in SHAPES:
        ops = cases[shape]
        for inplace in (False, True):
            got = rc.run(L, KIND, ops, 0, 0, inplace=inplace, planned=True, stream=g.stream(), what=f"planned {shape}")
            assert same(got, rc.want(KIND, ops)), (shape, inplace)


def test_with_an_r_of_zeros_c_is_the_plain_calls_c_wherever_s_is_not_minus_zero(g, L, cases):
    ops = cases[BIG]
    m, n, k = BIG
    zero = rc.Ops(*BIG)
    zero.r = torch.zeros(m, n, dtype=torch.bfloat16)
    a, b = ops.a.cuda(), ops.b.cuda()
    for cid, word in ((0, 1), (3, 1), (1, 2)):
        c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_launch_nn(cid, word, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, k, n, n, g.stream()) == 0
        torch.cuda.synchronize()
        got = rc.run(L, KIND, zero, cid, word, stream=g.stream(), what="r = 0")
        assert same(got, c.cpu()) and same(got, ops.s.bfloat16()), (cid, word)           # (S is never -0: an exact sum gives +0)


def test_a_split_call_captured_without_a_workspace_runs_unsplit(g, L):
    """On a fresh stream with nothing reserved the split call returns 0 while capturing and replays unsplit, in place.  One stream, one chain:
    no parallel branches."""
    m, n, k = 200, 264, 512
    ops = rc.Ops(m, n, k, seed=61)
    a, b = ops.a.cuda(), ops.b.cuda()
    c = ops.r.cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        ret = L.bgemm_mi355x_launch_nn_add(0, 8, a.data_ptr(), b.data_ptr(), c.data_ptr(), c.data_ptr(), m, n, k, k, n, n, n, st)
    assert ret == 0
    torch.cuda.synchronize()
    assert same(c.cpu(), ops.r), "capturing ran nothing"
    graph.replay()
    torch.cuda.synchronize()
    assert same(c.cpu(), rc.want(KIND, ops))


def test_the_refusals(L):
    """Argument checks: no launch.  ldr < N, r == c with ldr != ldc, NULL r (and the planned call's NULL r), NULL a / b / c, a bad id."""
    m, n, k = 136, 72, 128
    p = ctypes.c_void_p
    a, b, r, c = (p(4096 * (i + 1)) for i in range(4))
    launch = lambda ptrs, lds=(k, n, n, n), cid=0: L.bgemm_mi355x_launch_nn_add(cid, 1, *ptrs, m, n, k, *lds, None)   # noqa: E731
    assert launch((a, b, r, c), (k, n, n, n - 8)) == -1
    assert launch((a, b, c, c), (k, n, n + 8, n)) == -1 and launch((a, b, c, c), (k, n, n, n + 8)) == -1
    for i in range(4):
        ptrs = [a, b, r, c]
        ptrs[i] = None
        assert launch(ptrs) == -1, i
    assert L.bgemm_mi355x_nn_add(a, b, None, c, m, n, k, None) == -1
    assert launch((a, b, r, c), cid=4) == -1 and launch((a, b, r, c), cid=-1) == -1
    assert launch((a, b, r, c), (k - 8, n, n, n)) == -1 and launch((a, b, r, c), (k, n - 8, n, n)) == -1 and launch((a, b, r, c), (k, n, n - 8, n)) == -1
    assert L.bgemm_mi355x_nn_add_runs(0, m, n, k, k, n, n, n - 8) == 0 and L.bgemm_mi355x_nn_add_runs(0, m, n, k, k, n, n, n) == 1


def test_one_gated_layer_forward_and_backward_through_the_residual_stream(g, L):
    """tn_gated_aux -> tn_bias_add (in place on the residual stream) -> nn_dgated -> nn_add at K = 2N (in place on the stream's gradient), ReLU,
    M = 72, model width D = 64, inner width N = 64.  X, the weights and dY hold small integers, so every sum is an integer below 2^24, exact in
    fp32 in any order, and every step is defined bit for bit; torch computes each on the CPU from the previous step's expectation."""
    m, d, n = 72, 64, 64
    rng = np.random.default_rng(5)
    ints = lambda lo, hi, *shape: torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))   # noqa: E731
    x, w_gu, b_gu = ints(-1, 1, m, d), ints(-1, 1, 2 * n, d), ints(-4, 4, 2 * n)        # X [M][D], the fused [Wg;Wu] [2N][D], [bg|bu]
    wd, bd, x_in = ints(-3, 3, d, n), ints(-8, 8, d), ints(-100, 100, m, d)           # Wd [D][N], its bias, the residual stream
    dy, dx_out = ints(-3, 3, m, d), ints(-100, 100, m, d)
    dev = lambda t: t.bfloat16().cuda()                                                # noqa: E731
    X, Wgu, Bgu, Wd, Bd, Xs, dY, dXs = (dev(t) for t in (x, w_gu, b_gu, wd, bd, x_in, dy, dx_out))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.bfloat16, device="cuda")   # noqa: E731
    H, GU, dGU = nan(m, n), nan(m, 2 * n), nan(m, 2 * n)
    s = g.stream()
    # forward: H = relu(g) u, g|u saved
    assert L.bgemm_mi355x_launch_tn_gated_aux(0, 1, X.data_ptr(), Wgu.data_ptr(), Wgu.data_ptr() + 2 * n * d, Bgu.data_ptr(), Bgu.data_ptr() + 2 * n, H.data_ptr(),
                                              GU.data_ptr(), GU.data_ptr() + 2 * n, m, n, d, d, d, n, 2 * n, 1, s) == 0
    gu = x @ w_gu.t() + b_gu
    want_gu = gu.bfloat16()
    want_h = (torch.relu(gu[:, :n]) * gu[:, n:]).bfloat16()
    torch.cuda.synchronize()
    assert same(GU.cpu(), want_gu) and same(H.cpu(), want_h), "tn_gated_aux"
    # the down projection into the residual stream, in place: X_out = X_in + (H Wd^T + bd)
    assert L.bgemm_mi355x_launch_tn_bias_add(0, 1, H.data_ptr(), Wd.data_ptr(), Bd.data_ptr(), Xs.data_ptr(), Xs.data_ptr(), m, d, n, n, n, d, d, s) == 0
    s1 = (want_h.double() @ wd.double().t()).float()
    assert float(s1.abs().max()) < 2.0 ** 24
    torch.cuda.synchronize()
    assert same(Xs.cpu(), rc.want_bias_add(s1, bd.bfloat16(), x_in.bfloat16())), "tn_bias_add"
    # backward: dH = dY Wd through the gate
    assert L.bgemm_mi355x_launch_nn_dgated(0, 1, dY.data_ptr(), Wd.data_ptr(), GU.data_ptr(), GU.data_ptr() + 2 * n, dGU.data_ptr(), dGU.data_ptr() + 2 * n, m, n, d,
                                           d, n, 2 * n, 2 * n, 1, s) == 0
    s2 = (dy.double() @ wd.double()).float()
    gs, us = want_gu.float()[:, :n], want_gu.float()[:, n:]
    want_dgu = torch.cat([torch.where(gs <= 0, torch.zeros_like(s2), s2 * us), torch.relu(gs) * s2], 1).bfloat16()
    torch.cuda.synchronize()
    assert same(dGU.cpu(), want_dgu), "nn_dgated"
    # the gradient that reaches the block's input, in place on the stream's gradient: dX = [dG|dU] [Wg;Wu] + dX_out, K = 2N
    for cid, word in ((0, 1), (0, 2)):
        dXs_run = dXs.clone()
        assert L.bgemm_mi355x_launch_nn_add(cid, word, dGU.data_ptr(), Wgu.data_ptr(), dXs_run.data_ptr(), dXs_run.data_ptr(), m, d, 2 * n, 2 * n, d, d, d, s) == 0
        s3 = (want_dgu.double() @ w_gu.double()).float()
        assert float(s3.abs().max()) < 2.0 ** 24
        torch.cuda.synchronize()
        assert same(dXs_run.cpu(), rc.want_add(s3, dx_out.bfloat16())), ("nn_add", word)
