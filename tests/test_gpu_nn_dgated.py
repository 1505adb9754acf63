"""GPU tests of the gated MLP's input gradient, bgemm_mi355x_nn_dgated: dU = bf16(act(g) S), dG = bf16(dact_mul(fl32(S u), g)), S = dY Wd.

Operands make S exactly known in fp32 whatever the order of the sum: dY and Wd hold integers of [-15, 15], dY scaled by 2^-9, so S is a
multiple of 2^-9 with |S| <= 225 K 2^-9 < 2^9 (K <= 704; typically 2 to 4: the activations' live range) and every partial sum is exact: an
integer below 2^18.  Most S have more than eight significant bits, so a bf16 dH would show.  The fp64 truth then follows from S and the
saved bf16 g and u.  The bars and their constants are csrc/hgemm_dgated.hpp's, read by tests/test_nn_dgated_host.py:
    |du - act*(g) S|     <= 1/2 ulp_bf16(.) + 2^-19 |g| |S| + 2^-23 |.|
    |dg - S u act'*(g)|  <= 1/2 ulp_bf16(.) + 2^-19 |S u|
ReLU is held bit for bit.  Outputs start as NaN inside and a sentinel outside their M x N elements; the sentinel must come back unchanged,
and so must every input."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gpu_common import FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, OUT_FILL, _bits, _place
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_nn_dgated_host import ACT_EPS, ACTS, DACT_EPS, GELU, GELU_TANH, HOOK, MUL_EPS, RELU, SILU

pytestmark = pytest.mark.gpu

NN_MEMBERS = ("n64x64_w2x2", "n128x64_w2x2", "n64x128_w2x2", "n128x128_w2x2")
ACT_NAME = {RELU: "relu", GELU: "gelu", GELU_TANH: "gelu_tanh", SILU: "silu"}
NT = 0x20000                                                   # HGEMM_PLAN_NT_STORE
WORDS = (1, 1 | NT, 2, 5)                                      # plain, NT store, 2 and 5 two-pass splits (clamped to K / 64)
SHAPES = ((64, 32, 64), (8, 8, 64), (136, 72, 128), (152, 152, 320))
# The share of elements (of those with S != 0 and u != 0) on which each deliberately wrong reference must land outside a bar, on the 152 x 152
# x 320 operands below: g and u swapped and act' in place of act change the value by a factor that is rarely within 2^-8 of 1; dH rounded to
# bf16 first moves the result to a neighbouring bf16 value, more than half an ulp from the truth, where S is not a bf16 value and the first
# rounding pushes the product across a rounding boundary.
MISTAKE_SHARE = {"g and u swapped": 0.5, "act' in place of act": 0.5, "dH rounded to bf16 first": 0.1}


# ---- fp64 truth and the bars ---------------------------------------------------------------------------------------------------------------
def act64(z, act):
    if act == RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == GELU:
        return 0.5 * z * torch.erfc(-z / math.sqrt(2.0))
    x = 2.0 * math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3) if act == GELU_TANH else z
    return z / (1.0 + torch.exp(-x))


def dact64(z, act):
    if act == RELU:
        return (z > 0).double()
    if act == GELU:
        return 0.5 * torch.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if act == SILU:
        s = torch.sigmoid(z)
        return s + z * s * (1.0 - s)
    c = math.sqrt(2.0 / math.pi)
    s = torch.sigmoid(2.0 * c * (z + 0.044715 * z ** 3))
    return s + z * s * (1.0 - s) * 2.0 * c * (1.0 + 3 * 0.044715 * z * z)


def half_ulp_bf16(y):
    """half an ulp of bf16 at |y| (fp64), the subnormal spacing below 2^-126"""
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -126)))
    return 0.5 * torch.pow(2.0, e - 7)


def truths(s, gz, uz, act):
    s, gz, uz = s.double(), gz.double(), uz.double()
    return s * uz * dact64(gz, act), act64(gz, act) * s


def bars(s, gz, uz, act):
    s, gz, uz = s.double(), gz.double(), uz.double()
    dg, du = truths(s, gz, uz, act)
    return half_ulp_bf16(dg) + DACT_EPS * (s * uz).abs(), half_ulp_bf16(du) + ACT_EPS * gz.abs() * s.abs() + MUL_EPS * du.abs()


def relu_want(s, gz, uz):
    """the ReLU call bit for bit: fp32 products, the select, one rounding"""
    s, gz, uz = s.float(), gz.float(), uz.float()
    du = (torch.where((gz > 0) | gz.isnan(), gz, torch.zeros_like(gz)) * s).bfloat16()
    dg = torch.where(gz <= 0, torch.zeros_like(s), s * uz).bfloat16()
    return dg, du


def same_bits(a, b):
    """bit for bit; a NaN for a NaN"""
    a, b = a.cpu(), b.cpu()
    nan = b.float().isnan()
    return bool((_bits(a)[~nan] == _bits(b)[~nan]).all()) and bool(a.float()[nan].isnan().all())


class Ops:
    """dY [M][K], Wd [K][N], g and u [M][N] on the CPU, and S exactly"""

    def __init__(self, m, n, k, seed, g_const=None, u_const=None):
        rng = np.random.default_rng(seed)
        ai, bi = rng.integers(-15, 16, size=(m, k)), rng.integers(-15, 16, size=(k, n))
        self.m, self.n, self.k = m, n, k
        self.a = torch.from_numpy(ai * 2.0 ** -9).bfloat16()
        self.b = torch.from_numpy(bi.astype(np.float64)).bfloat16()
        self.s = torch.from_numpy((ai @ bi) * 2.0 ** -9).float()                  # exact: integers below 2^18
        assert float(self.s.abs().max()) < 2.0 ** 9 and torch.equal(self.s.double(), self.a.double() @ self.b.double())
        self.g = torch.from_numpy(rng.standard_normal((m, n)) * 1.5).bfloat16() if g_const is None else torch.full((m, n), g_const).bfloat16()
        self.u = torch.from_numpy(rng.standard_normal((m, n)) * 1.5).bfloat16() if u_const is None else torch.full((m, n), u_const).bfloat16()


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_nn_dgated.argtypes = [i] * 2 + [p] * 6 + [i] * 8 + [p]
    lib.bgemm_mi355x_nn_dgated.argtypes = [p] * 6 + [i] * 4 + [p]
    lib.bgemm_mi355x_launch_nn_dact.argtypes = [i] * 2 + [p] * 4 + [i] * 8 + [p]
    lib.bgemm_mi355x_launch_nn.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    lib.hgemm_mi355x_nn_reserve_workspace.argtypes = [i] * 3 + [p]
    assert [lib.hgemm_mi355x_nn_config_by_name(nm.encode()) for nm in NN_MEMBERS] == [0, 1, 2, 3]
    return lib


def decision(L, cid, word, act, m, n, k, lda, ldb, ldz, ldc, aligned=True):
    out = (ctypes.c_longlong * 20)()
    st = getattr(L, HOOK)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldz, ldc, 0, act, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def run(g, L, ops, cfg, word, act, lds=None, fused=False, want_form=None, off=None, planned=False, stream=None, what=""):
    """One call.  lds = (lda, ldb, ldz, ldc); fused: g|u in one [M][ldz >= 2N] buffer (u = g + N) and dg|du in one [M][ldc >= 2N] buffer
    (du = dg + N).  off = {"u": elements, "du": elements}: that pointer moved (out of scope).  Everything outside the outputs' M x N elements
    and every input must come back unchanged.  -> (dg, du) on the CPU."""
    m, n, k = ops.m, ops.n, ops.k
    lda, ldb, ldz, ldc = lds or (k, n, 2 * n if fused else n, 2 * n if fused else n)
    off = off or {}
    aligned = not off and not ((lda | ldb | ldz | ldc) & 7)
    if want_form is not None:
        st, form, disp = decision(L, cfg, word, act, m, n, k, lda, ldb, ldz, ldc, aligned)
        assert (st, form) == (0, want_form), (what, st, form, disp)
    nan16 = torch.full((m, n), float("nan"), dtype=torch.bfloat16)
    keep = [_place(ops.a, lda), _place(ops.b, ldb)]
    if fused:
        keep.append(_place(torch.cat([ops.g, ops.u], 1), ldz))
        outs = [_place(torch.cat([nan16, nan16], 1), ldc, fill=OUT_FILL)]
        pg, pu = keep[2][0].data_ptr(), keep[2][0].data_ptr() + 2 * n
        pdg, pdu = outs[0][0].data_ptr(), outs[0][0].data_ptr() + 2 * n
        views = [outs[0][1][:, :n], outs[0][1][:, n:2 * n]]
    else:
        keep += [_place(ops.g, ldz), _place(ops.u, ldz, off.get("u", 0))]
        outs = [_place(nan16, ldc, fill=OUT_FILL), _place(nan16, ldc, off.get("du", 0), fill=OUT_FILL)]
        pg, pu = keep[2][0].data_ptr(), keep[3][0].data_ptr() + 2 * off.get("u", 0)
        pdg, pdu = outs[0][0].data_ptr(), outs[1][0].data_ptr() + 2 * off.get("du", 0)
        views = [outs[0][1][:, :n], outs[1][1][:, :n]]
    before = [flat.clone() for flat, _ in outs]
    inputs = [flat.clone() for flat, _ in keep]
    stream = g.stream() if stream is None else stream
    if planned:
        st = L.bgemm_mi355x_nn_dgated(keep[0][0].data_ptr(), keep[1][0].data_ptr(), pg, pu, pdg, pdu, m, n, k, act, stream)
    else:
        st = L.bgemm_mi355x_launch_nn_dgated(cfg, word, keep[0][0].data_ptr(), keep[1][0].data_ptr(), pg, pu, pdg, pdu, m, n, k, lda, ldb, ldz, ldc, act, stream)
    torch.cuda.synchronize()
    assert st == 0, (what, st)
    got = [v.cpu().clone() for v in views]
    for v in views:
        v.zero_()
    for (flat, view), was in zip(outs, before):
        w = was.clone()
        wv = w[(view.data_ptr() - flat.data_ptr()) // 2:][:view.numel()].view(view.shape)
        wv[:, :2 * n if fused else n] = 0
        assert torch.equal(_bits(flat), _bits(w)), f"{what}: an output was written outside its elements"
    assert all(torch.equal(_bits(flat), _bits(was)) for (flat, _), was in zip(keep, inputs)), f"{what}: an input changed"
    return got[0], got[1]


def check(ops, act, dg, du, what, s=None):
    s = ops.s if s is None else s
    if act == RELU:
        wdg, wdu = relu_want(s, ops.g, ops.u)
        assert same_bits(dg, wdg) and same_bits(du, wdu), f"{what}: ReLU is not bit for bit"
        return 0.0
    fin = s.isfinite()
    tdg, tdu = truths(s, ops.g, ops.u, act)
    bdg, bdu = bars(s, ops.g, ops.u, act)
    rg, ru = ((dg.double() - tdg).abs() / bdg)[fin], ((du.double() - tdu).abs() / bdu)[fin]
    worst = max(float(rg.max()), float(ru.max()))
    print(f"{what}: worst error / bar dg {float(rg.max()):.3f} du {float(ru.max()):.3f}")
    assert worst <= 1.0, f"{what}: outside the bar on {int((rg > 1).sum())} (dg) and {int((ru > 1).sum())} (du) elements"
    return worst


@pytest.fixture(scope="module")
def cases():
    return {shape: Ops(*shape, seed=sum(shape)) for shape in SHAPES}


# ---- the bar itself, on the CPU --------------------------------------------------------------------------------------------------------------
def test_the_bar_tells_the_mistakes_apart(cases):
    """Deliberately wrong references land outside the bars on at least MISTAKE_SHARE of the live elements; the fp32 restatement of the
    call's own formulas is inside on all of them."""
    ops = cases[(152, 152, 320)]
    s, gz, uz = ops.s, ops.g.float(), ops.u.float()
    live = (s != 0) & (uz != 0) & (gz.abs() > 0.25)
    assert int(live.sum()) >= 15000
    for act in (GELU, GELU_TANH, SILU):
        tdg, tdu = truths(s, gz, uz, act)
        bdg, bdu = bars(s, gz, uz, act)
        own_dg, own_du = (s * uz * dact64(gz.double(), act).float()).bfloat16(), (act64(gz.double(), act).float() * s).bfloat16()
        assert bool(((own_dg.double() - tdg).abs() <= bdg).all()) and bool(((own_du.double() - tdu).abs() <= bdu).all())
        sb = s.bfloat16().float()
        wrong = {"g and u swapped": truths(s, uz, gz, act),
                 "act' in place of act": (s.double() * uz.double() * act64(gz.double(), act), dact64(gz.double(), act) * s.double()),
                 "dH rounded to bf16 first": tuple(t.float().bfloat16().double() for t in truths(sb, gz, uz, act))}
        for name, (wdg, wdu) in wrong.items():
            out = ((wdg - tdg).abs() > bdg) | ((wdu - tdu).abs() > bdu)
            share = float(out[live].double().mean())
            print(f"{ACT_NAME[act]}: {name}: outside a bar on {share:.3f} of the live elements (floor {MISTAKE_SHARE[name]})")
            assert share >= MISTAKE_SHARE[name], (act, name, share)


# ---- every member, form, activation, stride set and buffer arrangement -----------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_form_and_activation_meets_its_bar(g, L, cases, shape, padded, fused):
    ops = cases[shape]
    m, n, k = shape
    lds = (k + 8, n + 16, (2 * n if fused else n) + 24, (2 * n if fused else n) + 8) if padded else None
    steps = k // 64
    worst = 0.0
    for cid, word, act in ((c, w, a) for c in range(4) for w in WORDS for a in ACTS):
        splits = min(word & 0xffff, steps)
        want_form = FORM_SPLITK if splits > 1 else FORM_PLAIN
        what = f"{NN_MEMBERS[cid]} {hex(word)} {ACT_NAME[act]} {shape} {'padded' if padded else 'contiguous'} {'fused' if fused else 'separate'}"
        dg, du = run(g, L, ops, cid, word, act, lds, fused, want_form, what=what)
        worst = max(worst, check(ops, act, dg, du, what))
    assert worst <= 1.0


# ---- identities, bit for bit --------------------------------------------------------------------------------------------------------------------
def launch_nn(g, L, ops, cid, word, z=None, act=0):
    """C of bgemm_mi355x_launch_nn, or of bgemm_mi355x_launch_nn_dact at z"""
    a, b = ops.a.cuda(), ops.b.cuda()
    c = torch.full((ops.m, ops.n), float("nan"), dtype=torch.bfloat16, device="cuda")
    if z is None:
        st = L.bgemm_mi355x_launch_nn(cid, word, a.data_ptr(), b.data_ptr(), c.data_ptr(), ops.m, ops.n, ops.k, ops.k, ops.n, ops.n, g.stream())
    else:
        zd = z.cuda()
        st = L.bgemm_mi355x_launch_nn_dact(cid, word, a.data_ptr(), b.data_ptr(), zd.data_ptr(), c.data_ptr(), ops.m, ops.n, ops.k, ops.k, ops.n, ops.n, ops.n, act, g.stream())
    torch.cuda.synchronize()
    assert st == 0
    return c.cpu()


def test_with_u_of_ones_dg_is_the_dact_calls_c(g, L):
    m, n, k = 136, 72, 128
    ops = Ops(m, n, k, 7, u_const=1.0)
    for cid, word, act in ((c, w, a) for c in range(4) for w in (1, 2) for a in (RELU, GELU, GELU_TANH)):
        dg, _ = run(g, L, ops, cid, word, act, what=f"u = 1 {cid} {word} {act}")
        assert same_bits(dg, launch_nn(g, L, ops, cid, word, ops.g, act)), (cid, word, act)


def test_with_a_constant_g_under_relu_du_is_the_plain_c_scaled_exactly(g, L):
    m, n, k = 136, 72, 128
    ops = Ops(m, n, k, 8, g_const=4.0)                                          # relu(4) = 2^2: the product is exact
    for cid, word in ((c, w) for c in range(4) for w in (1, 2)):
        _, du = run(g, L, ops, cid, word, RELU, what=f"g = 4 {cid} {word}")
        plain = launch_nn(g, L, ops, cid, word)
        assert same_bits(du, (plain.float() * 4.0).bfloat16()) and same_bits(plain, ops.s.bfloat16()), (cid, word)


def test_two_runs_are_identical_and_the_planned_call_is_the_explicit_call_of_the_plan(g, L):
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for (m, n, k), want in (((256, 264, 512), 8), ((1024, 1024, 64), 1)):
        assert L.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == want
        ops = Ops(m, n, k, m + n + k)
        for act in ACTS:
            first = run(g, L, ops, cfg.value, splits.value, act, what="explicit")
            again = run(g, L, ops, cfg.value, splits.value, act, what="explicit again")
            planned = run(g, L, ops, 0, 0, act, planned=True, what="planned")
            assert all(same_bits(x, y) and same_bits(x, z) for x, y, z in zip(first, again, planned)), (m, n, k, act)
            check(ops, act, *planned, f"planned {ACT_NAME[act]} {m}x{n}x{k}")


# ---- the helper kernels: the combine and the reference kernel (a local twin of gpu_common.HelperKernelSet's scheme, which knows one second
# matrix and one output) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,splits", [(128, 2), (704, 11)])
def test_the_combine_split_against_unsplit_against_the_reference_call(g, L, k, splits):
    """The 64 x 64 member, M = N = 64 on padded strides: the split call (the combine's remainder loop only / one unrolled block of eight and
    three remainder slabs), the unsplit call and the reference-kernel call (u moved by 2 bytes) agree bit for bit: S is order-exact."""
    ops = Ops(64, 64, k, k)
    lds = (k, 64, 80, 72)
    for act in ACTS:
        plain = run(g, L, ops, 0, 1, act, lds, want_form=FORM_PLAIN, what="unsplit")
        split = run(g, L, ops, 0, splits, act, lds, want_form=FORM_SPLITK, what="split")
        ref = run(g, L, ops, 0, splits, act, lds, want_form=FORM_REFERENCE, off={"u": 1}, what="reference")
        assert all(same_bits(x, y) and same_bits(x, z) for x, y, z in zip(plain, split, ref)), (k, act)
        check(ops, act, *split, f"combine {ACT_NAME[act]} K {k}")


def test_the_reference_kernel_against_the_member_kernel_on_zero_padded_operands(g, L):
    m, n, k = 5, 12, 24
    ops = Ops(m, n, k, 3)
    big = Ops(64, 64, 64, 3)
    for name in ("a", "b", "g", "u"):
        t = torch.zeros_like(getattr(big, name))
        src = getattr(ops, name)
        t[:src.shape[0], :src.shape[1]] = src
        setattr(big, name, t)
    big.s = torch.zeros(64, 64)
    big.s[:m, :n] = ops.s
    for act in ACTS:
        want = run(g, L, big, 0, 1, act, (64, 64, 80, 72), want_form=FORM_PLAIN, what="padded to the member")
        got = run(g, L, ops, 0, 1, act, (k + 3, n + 5, n + 9, n + 7), want_form=FORM_REFERENCE, what="reference")
        assert all(same_bits(x, y[:m, :n]) for x, y in zip(got, want)), act
        check(ops, act, *got, f"reference {ACT_NAME[act]}")


@pytest.mark.parametrize("what", ["N % 8 == 4", "du 8 bytes off", "u 2 bytes off", "ldz % 8 == 4"])
def test_out_of_scope_goes_to_the_reference_kernel_and_meets_the_same_bars(g, L, what):
    m, n, k = 136, 76 if what.startswith("N") else 72, 128
    ops = Ops(m, n, k, 11)
    lds = (k, n + 4 if n % 8 else n, n + 4 if what.startswith(("ldz", "N")) else n, n + 4 if n % 8 else n)
    off = {"du 8 bytes off": {"du": 4}, "u 2 bytes off": {"u": 1}}.get(what)
    for cid, act in ((c, a) for c in (0, 3) for a in ACTS):
        dg, du = run(g, L, ops, cid, 2, act, lds, want_form=FORM_REFERENCE, off=off, what=what)
        check(ops, act, dg, du, f"{what} {NN_MEMBERS[cid]} {ACT_NAME[act]}")


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
def test_a_split_call_captured_without_a_workspace_runs_unsplit_and_split_after_the_reserve(g, L):
    """On a fresh stream with nothing reserved the split call returns 0 while capturing and replays unsplit; after the reserve call on that
    stream it replays split.  One stream, one chain per graph: no parallel branches."""
    m, n, k = 200, 264, 512
    ops = Ops(m, n, k, 61)
    a, b, gz, uz = (x.cuda() for x in (ops.a, ops.b, ops.g, ops.u))
    for reserve in (False, True):
        s = torch.cuda.Stream()
        if reserve:
            assert L.hgemm_mi355x_nn_reserve_workspace(m, n, k, s.cuda_stream) == 0
        for act in (RELU, SILU):
            dg = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            du = dg.clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                st = torch.cuda.current_stream().cuda_stream
                rc = L.bgemm_mi355x_launch_nn_dgated(0, 8, a.data_ptr(), b.data_ptr(), gz.data_ptr(), uz.data_ptr(), dg.data_ptr(), du.data_ptr(), m, n, k, k, n, n, n, act, st)
            assert rc == 0
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            check(ops, act, dg.cpu(), du.cpu(), f"replayed {ACT_NAME[act]} reserve {reserve}")
            eager = run(g, L, ops, 0, 8 if reserve else 1, act, want_form=FORM_SPLITK if reserve else FORM_PLAIN, what="eager")
            assert same_bits(dg, eager[0]) and same_bits(du, eager[1]), (act, reserve)


# ---- non-finite values --------------------------------------------------------------------------------------------------------------------------
def test_non_finite_g_and_an_infinite_s_follow_the_formulas(g, L):
    """Columns of g hold +inf, -inf, NaN, +0, -0 with a finite S; then S = +inf (every product 3e38 x 2 overflows fp32) under g <= 0 for
    ReLU: dg = +0 by the select, du = 0 x inf = NaN as the formula has it."""
    m, n, k = 64, 64, 64
    ops = Ops(m, n, k, 13)
    special = (float("inf"), float("-inf"), float("nan"), 0.0, -0.0)
    for j, v in enumerate(special):
        ops.g[:, 8 * j:8 * j + 8] = v
    for cid, word in ((0, 1), (3, 1), (0, 2)):
        for act in ACTS:
            dg, du = run(g, L, ops, cid, word, act, want_form=FORM_PLAIN, what="special g")   # (K = 64: one stage, the split word runs plain)
            sf, uf = ops.s[:, :40], ops.u[:, :40].float()
            if act == RELU:
                wdg, wdu = relu_want(ops.s, ops.g, ops.u)
                assert same_bits(dg, wdg) and same_bits(du, wdu)
                continue
            live = (sf != 0) & (uf != 0)
            # +inf: act' = 1, act = +inf; -inf: act' = +0, act = NaN (GELUs, SiLU: inf / inf or 0 x inf); NaN: NaN; +-0: act' = 1/2, act = a zero
            assert same_bits(dg[:, 0:8], (sf[:, 0:8] * uf[:, 0:8]).bfloat16()) and bool((du[:, 0:8].float()[sf[:, 0:8] != 0].abs() == float("inf")).all())
            assert bool((dg[:, 8:16].float() == 0).all()) and bool(du[:, 8:16].float().isnan().all())
            assert bool(dg[:, 16:24].float()[live[:, 16:24]].isnan().all()) and bool(du[:, 16:24].float().isnan().all())
            assert same_bits(dg[:, 24:40], ((sf[:, 24:40] * uf[:, 24:40]) * 0.5).bfloat16()) and bool((du[:, 24:40].float() == 0).all())
            rest = Ops(m, n, k, 13)
            tail = slice(40, n)
            rest.s, rest.g, rest.u = ops.s[:, tail], ops.g[:, tail], ops.u[:, tail]
            check(rest, act, dg[:, tail], du[:, tail], f"special g, the finite columns {ACT_NAME[act]}")
    big = Ops(m, n, k, 14)
    big.a = torch.full((m, k), 3.0e38).bfloat16()
    big.b = torch.full((k, n), 2.0).bfloat16()
    big.g = -big.g.abs()
    big.s = torch.full((m, n), float("inf"))
    dg, du = run(g, L, big, 0, 1, RELU, what="S = inf under g <= 0")
    assert bool((_bits(dg) == 0).all()), "dg = +0 whatever S holds"
    wdg, wdu = relu_want(big.s, big.g, big.u)
    assert same_bits(du, wdu) and same_bits(dg, wdg)
