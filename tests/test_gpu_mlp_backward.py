"""GPU tests of the fused MLP backward pair: bgemm_mi355x_tn_bias_act_aux (the forward that also writes the rounded pre-activation z_out)
and bgemm_mi355x_nn_dact (dZ = (dY W) (.) act'(Z), one fp32 multiply on the finished sum and one rounding).

The aux form is held by its two identities, bit for bit, for the same arguments and plan: C is bgemm_mi355x_launch_tn_bias_act's C and
z_out is bgemm_mi355x_launch_tn_bias's C.  The dact form runs on operands whose sum S is exact in fp32 in any order (asserted) and a
seeded bf16 Z over the activations' live range: ReLU bit for bit against where(z <= 0, +0, bf16(S)), both GELUs unmasked inside
|C - S g*(z)| <= 1/2 ulp_bf16(S g*) + eps |S| against fp64, eps the derived value of hgemm_act.hpp (imported from
tests/test_mlp_backward_host.py, which reads it there).  Before any launch the CPU shows, from reference data alone, that the
reference's own result is inside the bar and that each listed mistake is outside it in at least 300 elements at every shape."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, two_pass_cuts
from test_gpu_tn_bf16 import MEMBERS, SHAPES, Case
from test_gpu_tn_bias_act import ACT_NAME, ACTS, GELU, GELU_TANH, RELU, ActCase, a_scale
from test_gpu_tr_bf16 import SENTINEL, ibits, operands, seed_of, to_bf16
from test_mlp_backward_host import DACT_EPS

pytestmark = pytest.mark.gpu

NN_MEMBERS = ("n64x64_w2x2", "n128x64_w2x2", "n64x128_w2x2", "n128x128_w2x2")
MISTAKE_FLOOR = 300
WORST = {}                                                       # (call, act, member, form) -> worst error / bar, printed by the last test


# ---- the derivative in fp64 and the bar ------------------------------------------------------------------------------------------------
def dact64(z, act):
    """act'(z) of a float64 tensor, in fp64 (ReLU: 0 where z <= 0, else 1 -- a NaN z counts as 1)."""
    if act == RELU:
        return torch.where(z <= 0, torch.zeros_like(z), torch.ones_like(z))
    if act == GELU:
        return 0.5 * torch.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    c = math.sqrt(2.0 / math.pi)
    s = torch.sigmoid(2.0 * c * (z + 0.044715 * z * z * z))
    return s + z * s * (1.0 - s) * 2.0 * c * (1.0 + 3 * 0.044715 * z * z)


def bar(y64, s64):
    ay = y64.abs()
    half_ulp = torch.where(ay > 0, torch.exp2(torch.floor(torch.log2(torch.where(ay > 0, ay, torch.ones_like(ay)))) - 8), torch.zeros_like(ay))
    return half_ulp + DACT_EPS * s64.abs()


def outside(c16, y64, s64):
    bound = bar(y64, s64)
    err = (c16.double() - y64).abs()
    bad = (err > bound) | ~torch.isfinite(c16.double())
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)), torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max())


def relu_want(s32, z32):
    return torch.where(z32 <= 0, torch.zeros_like(s32, dtype=torch.bfloat16), to_bf16(s32))


def torch_backward32(s32, z32, act):
    """torch's own fp32 backward of the activation, grad_output = S: the reference whose bf16 result must itself be inside the bar."""
    z = z32.clone().requires_grad_(True)
    y = torch.relu(z) if act == RELU else torch.nn.functional.gelu(z, approximate="none" if act == GELU else "tanh")
    y.backward(s32)
    return z.grad


def forward32(z32, act):
    return torch.relu(z32) if act == RELU else torch.nn.functional.gelu(z32, approximate="none" if act == GELU else "tanh")


def make_z(m, n, ldz, seed):
    """A seeded bf16 Z buffer [M + 1][ldz]: the window dense in [-4, 4] (i.i.d., so no function of m or n alone), every 37th element a
    zero of alternating sign; NaN in the pad columns and in the guard row."""
    rng = np.random.default_rng(7000 + seed)
    z = torch.from_numpy(rng.uniform(-4.0, 4.0, size=(m, n)).astype(np.float32)).to(torch.bfloat16)
    flat = z.view(-1)
    flat[0::74] = 0.0
    flat[37::74] = -0.0
    buf = torch.full((m + 1, ldz), float("nan"), dtype=torch.bfloat16)
    buf[:m, :n] = z
    assert int((z.float() < -0.76).sum()) > m * n // 8 and int((ibits(z) == -32768).sum()) > 0       # derivative < 0 there; -0 present
    return buf


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    lib.bgemm_mi355x_launch_tn_bias_act.argtypes = [i] * 2 + [p] * 4 + [i] * 7 + [p]
    lib.bgemm_mi355x_launch_tn_bias_act_aux.argtypes = [i] * 2 + [p] * 5 + [i] * 8 + [p]
    lib.bgemm_mi355x_tn_bias_act_aux.argtypes = [p] * 5 + [i] * 4 + [p]
    lib.bgemm_mi355x_launch_nn_dact.argtypes = [i] * 2 + [p] * 4 + [i] * 8 + [p]
    lib.bgemm_mi355x_nn_dact.argtypes = [p] * 4 + [i] * 4 + [p]
    lib.bgemm_mi355x_tn_reserve_workspace.argtypes = [i] * 3 + [p]
    lib.hgemm_mi355x_nn_reserve_workspace.argtypes = [i] * 3 + [p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    tn = [(nm, L.bgemm_mi355x_tn_config_by_name(nm.encode())) for nm in MEMBERS]
    nn = [(nm, L.hgemm_mi355x_nn_config_by_name(nm.encode())) for nm in NN_MEMBERS]
    assert [c for _, c in tn] == [0, 1, 2, 3] and [c for _, c in nn] == [0, 1, 2, 3]
    return tn, nn


def decision(L, hook, cid, word, act, m, n, k, ld, ldz, aligned=True):
    out = (ctypes.c_longlong * 20)()
    st = getattr(L, hook)(cid, word, 4 if aligned else 0, m, n, k, *ld, ldz, 0, act, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


AUX_HOOK, DACT_HOOK = "bgemm_mi355x_selfcheck_launch_tn_bias_act_aux", "bgemm_mi355x_selfcheck_launch_nn_dact"


def sentinel_buffer(m, ld):
    return torch.full((m + 1, ld), SENTINEL, dtype=torch.bfloat16, device="cuda")


def pads_hold(buf, m, n):
    sent = ibits(torch.full((1,), SENTINEL, dtype=buf.dtype, device="cuda"))
    return bool((ibits(buf[:m, n:]) == sent).all()) and bool((ibits(buf[m]) == sent).all())


# ---- the aux form ------------------------------------------------------------------------------------------------------------------------
def aux_identities(g, L, case, plan, act, ldz, what, z_off=0):
    """Runs the three calls with the same arguments and plan and holds the two identities; returns (c, z_out) of the aux call."""
    m, n, k = case.m, case.n, case.k
    cid, word = plan
    ptrs = (case.ad.data_ptr(), case.wd.data_ptr(), case.bias_d.data_ptr())
    c_act, c_bias, c_aux = sentinel_buffer(m, case.ld[2]), sentinel_buffer(m, case.ld[2]), sentinel_buffer(m, case.ld[2])
    z_store = torch.full(((m + 1) * ldz + z_off,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    z_aux = z_store[z_off:].view(m + 1, ldz)
    assert L.bgemm_mi355x_launch_tn_bias_act(cid, word, *ptrs, c_act.data_ptr(), m, n, k, *case.ld, act, g.stream()) == 0, what
    assert L.bgemm_mi355x_launch_tn_bias(cid, word, *ptrs, c_bias.data_ptr(), m, n, k, *case.ld, g.stream()) == 0, what
    st = L.bgemm_mi355x_launch_tn_bias_act_aux(cid, word, *ptrs, c_aux.data_ptr(), z_aux.data_ptr(), m, n, k, *case.ld, ldz, act, g.stream())
    assert st == 0, (what, L.hgemm_mi355x_strerror(st))
    torch.cuda.synchronize()
    bad_c = int((ibits(c_aux) != ibits(c_act)).sum())
    assert bad_c == 0, f"{what}: C differs from bgemm_mi355x_launch_tn_bias_act's in {bad_c} elements"
    bad_z = int((ibits(z_aux[:m, :n]) != ibits(c_bias[:m, :n])).sum())
    assert bad_z == 0, f"{what}: z_out differs from bgemm_mi355x_launch_tn_bias's C in {bad_z} elements"
    assert pads_hold(z_aux, m, n) and pads_hold(c_aux, m, n), f"{what}: a pad or a guard row changed"
    assert bool((ibits(z_store[:z_off]) == ibits(torch.full((1,), SENTINEL, dtype=torch.bfloat16, device="cuda"))).all())
    assert not bool(torch.isnan(c_aux[:m, :n].float()).any()) and bool((ibits(c_bias[:m, :n]) == ibits(to_bf16(case.z32.cuda()))).all())
    return c_aux, z_aux


@pytest.fixture(scope="module")
def act_cases():
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            built[(shape, padded)] = ActCase(*shape, seed_of(shape), padded)
        return built[(shape, padded)]

    return get


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_aux_both_outputs_are_the_two_calls_outputs_bit_for_bit(g, L, members, act_cases, shape, padded):
    m, n, k = shape
    case = act_cases(shape, padded)
    ldz = n + 24 if padded else n                                 # padded: ldz != ldc = n + 8
    for name, cid in members[0]:
        assert L.bgemm_mi355x_tn_bias_act_aux_runs(cid, m, n, k, *case.ld, ldz) == 1
        for word in FORMS:
            cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
            for act in ACTS:
                st, form, disp = decision(L, AUX_HOOK, cid, word, act, m, n, k, case.ld, ldz)
                assert (st, form) == (0, FORM_SPLITK if cuts else FORM_PLAIN) and [d[2] for d in disp] == ([1, 8 + act] if cuts else [8 + act])
                aux_identities(g, L, case, (cid, word), act, ldz, f"aux {ACT_NAME[act]} {name} {hex(word)} {shape} ldz={ldz}")
    assert case.operands_intact()


@pytest.mark.parametrize("what", ["z_out 8 bytes off", "ldz % 8 != 0"])
def test_aux_outside_the_kernels_scope_the_reference_kernel_holds_the_identities(g, L, members, act_cases, what):
    shape = SHAPES[2]
    m, n, k = shape
    case = act_cases(shape, False)
    ldz, off = (n + 8, 4) if what.startswith("z_out") else (n + 4, 0)
    for act in ACTS:
        st, form, disp = decision(L, AUX_HOOK, 3, 1, act, m, n, k, case.ld, ldz, aligned=off == 0)
        assert (st, form, len(disp)) == (0, FORM_REFERENCE, 1), what
        assert L.bgemm_mi355x_tn_bias_act_aux_runs(3, m, n, k, *case.ld, ldz) == (1 if off else 0)
        aux_identities(g, L, case, (3, 1), act, ldz, f"aux reference {ACT_NAME[act]} {what}", z_off=off)
    assert case.operands_intact()


def test_aux_refusals(g, L, act_cases):
    case = act_cases(SHAPES[0])
    m, n, k = SHAPES[0]
    c, z = sentinel_buffer(m, n), sentinel_buffer(m, n)
    ptrs = (case.ad.data_ptr(), case.wd.data_ptr(), case.bias_d.data_ptr())
    null = ctypes.c_void_p(0)
    assert L.bgemm_mi355x_launch_tn_bias_act_aux(0, 1, *ptrs, c.data_ptr(), null, m, n, k, k, k, n, n, GELU, g.stream()) == -1
    assert L.bgemm_mi355x_launch_tn_bias_act_aux(0, 1, *ptrs, c.data_ptr(), c.data_ptr(), m, n, k, k, k, n, n, GELU, g.stream()) == -1
    assert L.bgemm_mi355x_launch_tn_bias_act_aux(0, 1, *ptrs, c.data_ptr(), z.data_ptr(), m, n, k, k, k, n, n - 8, GELU, g.stream()) == -1
    assert L.bgemm_mi355x_launch_tn_bias_act_aux(0, 1, *ptrs, c.data_ptr(), z.data_ptr(), m, n, k, k, k, n, n, 0, g.stream()) == -1
    assert L.bgemm_mi355x_tn_bias_act_aux(*ptrs, c.data_ptr(), null, m, n, k, GELU, g.stream()) == -1
    torch.cuda.synchronize()
    assert pads_hold(c, m, 0) and pads_hold(z, m, 0)              # nothing was written


# ---- the dact form ------------------------------------------------------------------------------------------------------------------------
class DactCase(Case):
    """test_gpu_tn_bf16.Case with A scaled as the forward's tests scale it (S exact in fp32 in any order, asserted there), its row-major B
    as bgemm_mi355x_nn's operand and a seeded Z in a padded buffer; per activation the CPU's expectation."""

    def __init__(self, m, n, k, seed, padded=False, z=None):
        super().__init__(m, n, k, seed, False, scale=(a_scale(k), 1.0))
        self.ld = (k + 8, n + 16, n + 8) if padded else (k, n, n)
        self.ldz = n + 24 if padded else n
        self.ad = torch.full((m, self.ld[0]), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.ad[:, :k] = self.before[0][:, :k]
        self.bd = torch.full((k, self.ld[1]), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.bd[:, :n] = self.b_rows
        self.z_host = make_z(m, n, self.ldz, seed) if z is None else z
        self.zd = self.z_host.cuda()
        self.before = [x.clone() for x in (self.ad, self.bd, self.zd)]
        self.s32 = torch.from_numpy(self.prod32_np)
        self.s64 = self.s32.double()
        self.z32 = self.z_host[:m, :n].float()
        self.relu16 = relu_want(self.s32, self.z32)
        self.y64 = {act: self.s64 * dact64(self.z32.double(), act) for act in (GELU, GELU_TANH)}

    def c_buffer(self):
        return sentinel_buffer(self.m, self.ld[2])

    def launch(self, g, L, buf, plan, act):
        m, n, k = self.m, self.n, self.k
        if plan is None:
            assert self.ld == (k, n, n) and self.ldz == n
            st = L.bgemm_mi355x_nn_dact(self.ad.data_ptr(), self.bd.data_ptr(), self.zd.data_ptr(), buf.data_ptr(), m, n, k, act, g.stream())
        else:
            st = L.bgemm_mi355x_launch_nn_dact(plan[0], plan[1], self.ad.data_ptr(), self.bd.data_ptr(), self.zd.data_ptr(), buf.data_ptr(), m, n, k,
                                               *self.ld, self.ldz, act, g.stream())
        assert st == 0, (plan, act, L.hgemm_mi355x_strerror(st))

    def check(self, buf, what, act, key=None):
        torch.cuda.synchronize()
        got = buf[:self.m, :self.n].cpu()
        if act == RELU:
            bad = int((ibits(got) != ibits(self.relu16)).sum())
            assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements differ from where(z <= 0, +0, bf16(S))"
        else:
            bad, worst = outside(got, self.y64[act], self.s64)
            if key is not None:
                WORST[key] = max(WORST.get(key, 0.0), worst)
            print(f"{what}: worst error {worst:.3f} of the bar")
            assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements outside 1/2 ulp_bf16(S g*) + eps |S| (worst {worst:.3f} of it)"
        assert pads_hold(buf, self.m, self.n), f"{what}: the pad or the guard row changed"

    def run(self, g, L, plan, what, act, key=None):
        buf = self.c_buffer()
        self.launch(g, L, buf, plan, act)
        self.check(buf, what, act, key)
        return buf

    def operands_intact(self):
        return all(torch.equal(ibits(x), ibits(was)) for x, was in zip((self.ad, self.bd, self.zd), self.before))


def evidence_of(shape):
    """CPU only, from reference data alone, at the padded strides (ldz = n + 24, ldc = n + 8): torch's own fp32 backward rounded to bf16
    is inside the bar everywhere; each mistake is outside it (ReLU: differs in bits) in at least MISTAKE_FLOOR elements.  One exception,
    asserted: at K = 64 every S of these operands is a bf16 value, so rounding S first is no mistake at (64, 64, 64)."""
    m, n, k = shape
    a, b = operands(m, n, k, seed_of(shape))
    s64 = torch.from_numpy((a.astype(np.int64) @ b.astype(np.int64)).astype(np.float64) * a_scale(k))
    s32 = s64.float()
    assert torch.equal(s32.double(), s64), "S is not exact in fp32"
    ldz, ldc = n + 24, n + 8
    zbuf = make_z(m, n, ldz, seed_of(shape))
    z32 = zbuf[:m, :n].float()
    flat = zbuf.view(-1).float()
    mi, ni = torch.meshgrid(torch.arange(m), torch.arange(n), indexing="ij")
    z_at_ldc = torch.nan_to_num(flat[mi * ldc + ni], nan=1.0)                  # (a NaN from the pad counts as a mistake either way)
    z_transposed = torch.nan_to_num(flat[(ni * ldz + mi) % flat.numel()], nan=1.0)
    row = {"|S| median": float(s64.abs().median())}
    for act in ACTS:
        y64 = s64 * dact64(z32.double(), act)

        def count(c16):
            if act == RELU:
                return int((ibits(c16) != ibits(relu_want(s32, z32))).sum())
            return outside(c16, y64, s64)[0]
        own = to_bf16(torch_backward32(s32, z32, act))
        assert count(own) == 0, (shape, ACT_NAME[act], "the reference's own bf16 result is outside the bar", count(own))
        wrong = {"the forward activation instead of the derivative": to_bf16(s32 * forward32(z32, act)),
                 "Z taken at ldc": to_bf16(torch_backward32(s32, z_at_ldc, act)),
                 "Z of the transposed position": to_bf16(torch_backward32(s32, z_transposed, act)),
                 "no multiply at all": to_bf16(s32)}
        if act != RELU:                                            # ReLU has no other form, and its select commutes with the rounding
            wrong["the other form's derivative"] = to_bf16(torch_backward32(s32, z32, GELU + GELU_TANH - act))
            if torch.equal(to_bf16(s32).float(), s32):             # (64, 64, 64): |S| 16 < 2^8, every S is a bf16 value -- no such mistake there
                assert k == 64
            else:
                wrong["S rounded to bf16 before the multiply"] = to_bf16(torch_backward32(to_bf16(s32).float(), z32, act))
        for what, c16 in wrong.items():
            row[f"{ACT_NAME[act]}: {what}"] = count(c16)
            assert row[f"{ACT_NAME[act]}: {what}"] >= MISTAKE_FLOOR, (shape, ACT_NAME[act], what, row)
    return row


@pytest.fixture(scope="module")
def evidence():
    return {shape: evidence_of(shape) for shape in SHAPES}


def test_dact_the_reference_is_inside_the_bar_and_the_bar_tells_the_mistakes_apart(evidence):
    for shape, row in evidence.items():
        print(shape, row)
    assert len(evidence) == 4


@pytest.fixture(scope="module")
def dact_cases():
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            built[(shape, padded)] = DactCase(*shape, seed_of(shape), padded)
        return built[(shape, padded)]

    return get


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dact_every_member_form_and_activation_meets_its_bar(g, L, members, dact_cases, evidence, shape, padded):
    m, n, k = shape
    case = dact_cases(shape, padded)
    for name, cid in members[1]:
        assert L.bgemm_mi355x_nn_dact_runs(cid, m, n, k, *case.ld, case.ldz) == 1, (name, shape)
        for word in FORMS:
            cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
            for act in ACTS:
                st, form, disp = decision(L, DACT_HOOK, cid, word, act, m, n, k, case.ld, case.ldz)
                assert (st, form) == (0, FORM_SPLITK if cuts else FORM_PLAIN) and [d[2] for d in disp] == ([1, 11 + act] if cuts else [11 + act])
                case.run(g, L, (cid, word), f"dact {ACT_NAME[act]} {name} {hex(word)} {shape} ld={case.ld} ldz={case.ldz}", act,
                         ("dact", ACT_NAME[act], name, hex(word)))
    assert case.operands_intact()


@pytest.mark.parametrize("what", ["z 8 bytes off", "ldz % 8 != 0"])
def test_dact_outside_the_kernels_scope_the_reference_kernel_meets_the_same_bars(g, L, members, evidence, what):
    shape = SHAPES[2]
    m, n, k = shape
    case = DactCase(m, n, k, seed_of(shape))
    if what.startswith("z 8"):
        store = torch.full(((m + 1) * n + 4,), float("nan"), dtype=torch.bfloat16, device="cuda")
        store[4:].view(m + 1, n).copy_(case.zd)
        case.zd = store[4:].view(m + 1, n)
        assert case.zd.data_ptr() % 16 == 8
        aligned = False
    else:
        case.ldz = n + 4
        case.z_host = make_z(m, n, case.ldz, seed_of(shape))
        case.zd = case.z_host.cuda()
        case.z32 = case.z_host[:m, :n].float()
        case.relu16 = relu_want(case.s32, case.z32)
        case.y64 = {act: case.s64 * dact64(case.z32.double(), act) for act in (GELU, GELU_TANH)}
        aligned = True
        assert L.bgemm_mi355x_nn_dact_runs(3, m, n, k, *case.ld, case.ldz) == 0
    case.before[2] = case.zd.clone()
    for act in ACTS:
        st, form, disp = decision(L, DACT_HOOK, 3, 1, act, m, n, k, case.ld, case.ldz, aligned=aligned)
        assert (st, form, len(disp)) == (0, FORM_REFERENCE, 1), what
        case.run(g, L, (3, 1), f"dact reference {ACT_NAME[act]} {what}", act, ("dact", ACT_NAME[act], "reference", what))
    assert case.operands_intact()


def test_dact_special_z_by_column(g, L, members):
    """Column n of Z holds special value n % 12: NaN, +-inf, +-0, +-3e38, +-1e20, +-16 and 20.  As the header states: ReLU passes S under a
    NaN z and gives +0 under every z <= 0; both GELUs give exactly bf16(S) for z >= 16, a zero for z <= -16, NaN for NaN and bf16(S / 2)
    for +-0.  Plain, split and reference forms."""
    m, n, k = 136, 72, 128
    vals = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 3e38, -3e38, 1e20, -1e20, 16.0, -16.0, 20.0]
    zrow = torch.tensor([vals[j % 12] for j in range(n)], dtype=torch.float32).to(torch.bfloat16)
    z = torch.full((m + 1, n), float("nan"), dtype=torch.bfloat16)
    z[:m] = zrow[None, :]
    case = DactCase(m, n, k, 77, z=z)
    zf = z[:m].float()
    s16 = to_bf16(case.s32)
    assert int((case.s32 != 0).sum()) > m * n // 2
    for (cid, word), act in ((p, a) for p in ((1, 1), (0, 2), (3, 5)) for a in ACTS):
        buf = case.c_buffer()
        case.launch(g, L, buf, (cid, word), act)
        torch.cuda.synchronize()
        got = buf[:m, :n].cpu()
        if act == RELU:
            assert torch.equal(ibits(got), ibits(torch.where(zf <= 0, torch.zeros_like(s16), s16))), (cid, word)
            continue
        nan, one, zero, half = torch.isnan(zf), zf >= 16, zf <= -16, zf == 0
        assert bool(torch.isnan(got.float()[nan]).all()) and not bool(torch.isnan(got.float()[~nan]).any()), (cid, word, act)
        assert torch.equal(ibits(got[one]), ibits(s16[one])), (cid, word, act, "z >= 16 gives S")
        assert bool((got.float()[zero] == 0).all()), (cid, word, act, "z <= -16 gives a zero")
        assert torch.equal(ibits(got[half]), ibits(to_bf16(case.s32 * 0.5)[half])), (cid, word, act, "z = +-0 gives S / 2")
    assert case.operands_intact()


# ---- planned calls, capture, end to end ----------------------------------------------------------------------------------------------------
def test_the_planned_calls_agree_with_the_explicit_calls_at_the_plan(g, L, members):
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for (m, n, k), want in (((256, 264, 512), 8), ((1024, 1024, 64), 1)):
        assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == want
        fwd = ActCase(m, n, k, m + n + k)
        ptrs = (fwd.ad.data_ptr(), fwd.wd.data_ptr(), fwd.bias_d.data_ptr())
        for act in ACTS:
            c, z = aux_identities(g, L, fwd, (cfg.value, splits.value), act, n, f"aux at the plan {ACT_NAME[act]}")
            c2, z2 = sentinel_buffer(m, n), sentinel_buffer(m, n)
            assert L.bgemm_mi355x_tn_bias_act_aux(*ptrs, c2.data_ptr(), z2.data_ptr(), m, n, k, act, g.stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(ibits(c2), ibits(c)) and torch.equal(ibits(z2), ibits(z)), ("planned aux", act)
        assert L.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0
        bwd = DactCase(m, n, k, m + n + k)
        for act in ACTS:
            explicit = bwd.run(g, L, (cfg.value, splits.value), f"dact at the plan {ACT_NAME[act]} {m}x{n}x{k}", act)
            planned = bwd.run(g, L, None, f"planned dact {ACT_NAME[act]} {m}x{n}x{k}", act)
            assert torch.equal(ibits(planned), ibits(explicit))
        assert fwd.operands_intact() and bwd.operands_intact()


def test_a_split_call_captured_without_a_workspace_runs_unsplit(g, L, members):
    """On a fresh stream with nothing reserved the split calls return 0 while capturing and replay unsplit; the replay meets the checks of
    the eager call.  One stream, one chain per graph: no parallel branches."""
    m, n, k = 200, 264, 512
    fwd, bwd = ActCase(m, n, k, 61), DactCase(m, n, k, 61)
    for act in ACTS:
        eager_c, eager_z = aux_identities(g, L, fwd, (0, 8), act, n, f"eager aux {ACT_NAME[act]}")
        c, z, dz = sentinel_buffer(m, n), sentinel_buffer(m, n), bwd.c_buffer()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            st = torch.cuda.current_stream().cuda_stream
            rc1 = L.bgemm_mi355x_launch_tn_bias_act_aux(0, 8, fwd.ad.data_ptr(), fwd.wd.data_ptr(), fwd.bias_d.data_ptr(), c.data_ptr(), z.data_ptr(),
                                                        m, n, k, k, k, n, n, act, st)
            rc2 = L.bgemm_mi355x_launch_nn_dact(0, 8, bwd.ad.data_ptr(), bwd.bd.data_ptr(), bwd.zd.data_ptr(), dz.data_ptr(), m, n, k, k, n, n, n, act, st)
        assert (rc1, rc2) == (0, 0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ibits(c), ibits(eager_c)) and torch.equal(ibits(z), ibits(eager_z)), act
        bwd.check(dz, f"replayed dact {ACT_NAME[act]}", act)
    assert fwd.operands_intact() and bwd.operands_intact()


@pytest.mark.parametrize("act", ACTS, ids=[ACT_NAME[a] for a in ACTS])
def test_one_mlp_layer_forward_with_aux_and_back_with_dact(g, L, members, act):
    """X [M][K] W^T + b -> (Y, Z) with the aux call; dY [M][N2] x W2 [N2][N] with the dact call at the saved z_out: dZ is inside the bar of
    the fp64 chain S2 g*(z_out) computed from the saved z_out."""
    m, n, k = 152, 152, 320
    fwd = ActCase(m, n, k, 5)
    c, z = aux_identities(g, L, fwd, (1, 1), act, n, f"layer forward {ACT_NAME[act]}")
    bwd = DactCase(m, n, 128, 6, z=z.cpu())                       # dY [m][128], W2 [128][n]; Z = the saved z_out, guard row included
    assert torch.equal(ibits(bwd.z_host[:m]), ibits(to_bf16(fwd.z32)))
    bwd.run(g, L, (2, 2), f"layer backward {ACT_NAME[act]}", act, ("layer", ACT_NAME[act], NN_MEMBERS[2], "0x2"))


def test_print_the_worst_ratios(evidence):
    for key in sorted(WORST):
        print("worst ratio", *key, f"{WORST[key]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())                  # (each test has asserted its own rows; run alone, the table is empty)


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the three aux sets (C and z_out) and the three dact sets (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72, ldz = 80 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit."""
    def aux(act):
        return g.HelperKernelSet(lambda cfg, word, p, d, acc: L.bgemm_mi355x_launch_tn_bias_act_aux(cfg, word, p["a"], p["b"], p["bias"], p["c"], p["z"], *d, act, g.stream()),
                                 lambda cfg, word, d, aligned, acc: decision(L, AUX_HOOK, cfg, word, act, *d[:3], d[3:6], d[6], aligned), torch.bfloat16,
                                 b_col=True, bias=True, z="out")

    def dact(act):
        return g.HelperKernelSet(lambda cfg, word, p, d, acc: L.bgemm_mi355x_launch_nn_dact(cfg, word, p["a"], p["b"], p["z"], p["c"], *d, act, g.stream()),
                                 lambda cfg, word, d, aligned, acc: decision(L, DACT_HOOK, cfg, word, act, *d[:3], d[3:6], d[6], aligned), torch.bfloat16, z="in")
    sets = [aux(act) for act in ACTS] + [dact(act) for act in ACTS]
    for s in sets:
        s.check_combine(128, 2, 9171)
        s.check_combine(704, 11, 9171 + 1)
        s.check_reference(9171 + 2)
