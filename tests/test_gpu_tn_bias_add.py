"""GPU tests of the forward product with a fused bias and residual add, bgemm_mi355x_tn_bias_add: C = bf16((S + float(bias[n])) + float(r[m][n])),
family f's kernels of hgemm_inst_g21.hip, the combine of the two-pass form and the reference kernel (OutBiasAdd).

tests/residual_common.py has the operands and the expectation: S is exact in fp32 in any order, so the result is defined bit for bit by two
IEEE fp32 adds and one rounding, which torch computes on the CPU.  Every comparison is on bits.  Outputs start as NaN inside and a sentinel
outside their M x N elements; the sentinel and every input must come back unchanged (residual_common.run)."""
import ctypes

import pytest
import torch

import residual_common as rc
from residual_common import FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, SHAPES, WORDS, bits
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)

pytestmark = pytest.mark.gpu

KIND = "tn"
MEMBERS = ("f64x64_w2x2", "f128x64_w2x2", "f64x128_w2x2", "f128x128_w2x2")
BIG = (152, 152, 320)


@pytest.fixture(scope="module")
def L(g):
    lib = rc.prototypes(g.lib())
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    assert [lib.bgemm_mi355x_tn_config_by_name(nm.encode()) for nm in MEMBERS] == [0, 1, 2, 3]
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
    lds = (k + 8, k + 16, n + 8, n + 24) if padded else None
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
    lds = (k, k, n + 8, n + 8) if padded else None
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
        lds = {"r 2 bytes off": None, "ldr % 8 == 4": (k, k, n, n + 4), "in place with ldc % 8 == 4": (k, k, n + 4, n + 4)}[why]
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


def test_a_null_bias_is_a_zero_filled_vector(g, L, cases):
    """Plain, split and reference form: bias == NULL gives the bits of a vector of +0.0, which are the CPU's."""
    ops = cases[(136, 72, 128)]
    m, n, k = ops.m, ops.n, ops.k
    expect = rc.want(KIND, ops, bias="zeros")
    for cid, word, lds, form in ((0, 1, None, FORM_PLAIN), (3, 1, None, FORM_PLAIN), (1, 2, None, FORM_SPLITK), (2, 1 | rc.NT, None, FORM_PLAIN),
                                 (0, 1, (k, k, n, n + 4), FORM_REFERENCE)):
        null = rc.run(L, KIND, ops, cid, word, lds, bias="null", want_form=form, stream=g.stream(), what="NULL bias")
        zeros = rc.run(L, KIND, ops, cid, word, lds, bias="zeros", want_form=form, stream=g.stream(), what="zero bias")
        assert same(null, zeros) and same(null, expect), (cid, word, form)


def test_the_order_of_the_two_adds(g, L):
    """bias = +-2^16 (1 + (n mod 128) / 128), r = -bias: (S + bias) + r loses S's low bits, S + (bias + r) keeps them.  Every member, the plain
    launch and splits = 2."""
    for shape in (SHAPES[0],) + SHAPES[2:]:
        ops = rc.Ops(*shape, data="order")
        expect = rc.want(KIND, ops)
        other = rc.wrong_variants(ops, KIND)["order of the adds"]
        assert rc.differing(other, expect) >= rc.FLOOR["order of the adds"] * ops.m * ops.n
        for cid in range(4):
            for word in (1, 2):
                got = rc.run(L, KIND, ops, cid, word, want_form=form_of(word, ops.k), stream=g.stream(), what="order data")
                assert same(got, expect), f"{MEMBERS[cid]} {word} {shape}: {rc.differing(got, expect)} elements differ"


def test_with_an_r_of_zeros_c_is_the_bias_calls_c_wherever_z_is_not_minus_zero(g, L, cases):
    ops = cases[BIG]
    m, n, k = BIG
    zero = rc.Ops(*BIG)
    zero.r = torch.zeros(m, n, dtype=torch.bfloat16)
    a, bt, bias = ops.a.cuda(), ops.bt.cuda(), ops.bias.cuda()
    z_minus_zero = bits((ops.s + ops.bias.float()).bfloat16()) == -32768
    for cid, word in ((0, 1), (3, 1), (1, 2)):
        c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_launch_tn_bias(cid, word, a.data_ptr(), bt.data_ptr(), bias.data_ptr(), c.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
        torch.cuda.synchronize()
        got = rc.run(L, KIND, zero, cid, word, stream=g.stream(), what="r = 0")
        assert bool((bits(got) == bits(c.cpu()))[~z_minus_zero].all()) and bool((bits(got)[z_minus_zero] == 0).all()), (cid, word)


def test_a_split_call_captured_without_a_workspace_runs_unsplit(g, L):
    """On a fresh stream with nothing reserved the split call returns 0 while capturing and replays unsplit, in place.  One stream, one chain:
    no parallel branches."""
    m, n, k = 200, 264, 512
    ops = rc.Ops(m, n, k, seed=61)
    a, bt, bias = ops.a.cuda(), ops.bt.cuda(), ops.bias.cuda()
    c = ops.r.cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        ret = L.bgemm_mi355x_launch_tn_bias_add(0, 8, a.data_ptr(), bt.data_ptr(), bias.data_ptr(), c.data_ptr(), c.data_ptr(), m, n, k, k, k, n, n, st)
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
    a, b, bias, r, c = (p(4096 * (i + 1)) for i in range(5))
    launch = lambda ptrs, lds=(k, k, n, n), cid=0: L.bgemm_mi355x_launch_tn_bias_add(cid, 1, *ptrs, m, n, k, *lds, None)   # noqa: E731
    assert launch((a, b, bias, r, c), (k, k, n, n - 8)) == -1
    assert launch((a, b, bias, c, c), (k, k, n + 8, n)) == -1 and launch((a, b, bias, c, c), (k, k, n, n + 8)) == -1
    for i in (0, 1, 3, 4):
        ptrs = [a, b, bias, r, c]
        ptrs[i] = None
        assert launch(ptrs) == -1, i
    assert L.bgemm_mi355x_tn_bias_add(a, b, bias, None, c, m, n, k, None) == -1
    assert launch((a, b, bias, r, c), cid=4) == -1 and launch((a, b, bias, r, c), cid=-1) == -1
    assert launch((a, b, bias, r, c), (k - 8, k, n, n)) == -1 and launch((a, b, bias, r, c), (k, k, n - 8, n)) == -1
    assert L.bgemm_mi355x_tn_bias_add_runs(0, m, n, k, k, k, n, n - 8) == 0 and L.bgemm_mi355x_tn_bias_add_runs(0, m, n, k, k, k, n, n) == 1
