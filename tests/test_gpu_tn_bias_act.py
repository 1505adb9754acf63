"""GPU tests of the forward product with a fused bias and activation (run with `-m gpu` on an MI355X): bgemm_mi355x_tn_bias_act /
bgemm_mi355x_launch_tn_bias_act -- Y = act(X W^T + b); family f's EPI_C16_BIAS + ACT kernels (hgemm_inst_g14.hip), the activation combine
of the two-pass form and the activation reference kernel, all three on the one activation text of hgemm_act.hpp.

The semantics under test:  z = fl32(S + float(bias[n])),  C = bf16_rne(act32(z)): the activation of the UNROUNDED fp32 sum, never of a
slab, the result rounded ONCE.
  * ReLU (act 1) is an exact function and is held bit for bit against where(z > 0, bf16(z), +0) from the CPU.
  * Both GELUs (act 2: erf form, act 3: tanh form) are held, unmasked, to  |C - y*| <= 1/2 ulp_bf16(y*) + 2^-19 |z|,  y* the activation
    of the exactly known z in fp64.

Inputs with an exact z: tests/test_gpu_tr_bf16.py's integers in -2 .. 2 with A scaled by 2^-(floor(log2 K) - 2) (2^-4 .. 2^-7 for the
four shapes) and a bias of N pairwise distinct multiples of 2^-8 in [-1, 1]: S is a multiple of 2^-7 below 2^6 and z a multiple of 2^-8,
exact in fp32 in any order (asserted).  Before any launch the module shows on the CPU, from reference data alone, that z lies in the
activations' live range, that the reference's own bf16 result is inside the bar everywhere and that each mistake -- the other GELU form,
the activation of bf16(z), no activation, the bias added after the activation, the activation of every slab -- is outside it (for ReLU:
differs in bits) in at least 300 elements at every shape.  Rounding and ReLU commute, so the twice-rounded mistake and the other form
are GELU mistakes only.

C lies in [M + 1][ldc] with a sentinel in the pad and the guard row, NaN sits in the operands' padding, the bias vector is followed by a
NaN guard element, and operands and bias must be bit-unchanged afterwards."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, two_pass_cuts
from test_gpu_tn_bf16 import MEMBERS, SHAPES, Case
from test_gpu_tr_bf16 import SENTINEL, ibits, operands, seed_of, to_bf16

pytestmark = pytest.mark.gpu

EPI_SLAB, EPI_C16_BIAS = 1, 5
RELU, GELU, GELU_TANH = 1, 2, 3
ACTS = (RELU, GELU, GELU_TANH)
ACT_NAME = {RELU: "relu", GELU: "gelu", GELU_TANH: "gelu_tanh"}
MISTAKE_FLOOR = 300
WORST = {}                                                       # (act, member, form) -> worst error / bar, printed by the last test


# ---- the activations in fp64 and the bar -----------------------------------------------------------------------------------------------
def act64(z, act):
    """The activation of a float64 tensor, in fp64.  The erf form through erfc (no cancellation in the negative tail), the tanh form as
    z sigmoid(2u)."""
    if act == RELU:
        return torch.where((z > 0) | torch.isnan(z), z, torch.zeros_like(z))
    if act == GELU:
        return 0.5 * z * torch.erfc(-z / math.sqrt(2.0))
    u = math.sqrt(2.0 / math.pi) * (z + 0.044715 * z * z * z)
    return z / (1.0 + torch.exp(-2.0 * u))


def act32_torch(z32, act):
    """torch's own fp32 activation: the reference whose bf16 result must itself be inside the bar."""
    if act == RELU:
        return torch.relu(z32)
    return torch.nn.functional.gelu(z32, approximate="none" if act == GELU else "tanh")


def bar(y64, z64):
    """1/2 ulp_bf16(y*) + 2^-19 |z| per element (bf16: 8 significand bits; a zero y* has no first term)."""
    ay = y64.abs()
    half_ulp = torch.where(ay > 0, torch.exp2(torch.floor(torch.log2(torch.where(ay > 0, ay, torch.ones_like(ay)))) - 8), torch.zeros_like(ay))
    return half_ulp + 2.0 ** -19 * z64.abs()


def outside(c16, y64, z64, extra=None):
    """Elements of a bf16 result outside the bar (+ `extra`, a per-element widening that only the N(0,1) test passes), and the worst ratio."""
    bound = bar(y64, z64) if extra is None else bar(y64, z64) + extra
    err = (c16.double() - y64).abs()
    finite = torch.isfinite(y64)
    bad = (err > bound) & finite | (finite & ~torch.isfinite(c16.double()))
    ratio = torch.where(finite & (bound > 0), err / torch.where(bound > 0, bound, torch.ones_like(bound)), torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max())


def relu_want(z32):
    return torch.where(z32 > 0, to_bf16(z32), torch.zeros_like(z32, dtype=torch.bfloat16))


def a_scale(k):
    return 2.0 ** -(int(math.floor(math.log2(k))) - 2)


def make_bias(n, seed):
    """N pairwise distinct multiples of 2^-8 in [-1, 1] (all 513 are bf16 values: |q| <= 256 has at most 8 significant bits) in a seeded
    order, the odd multiples first: with one of those z has its 2^-8 bit set and is no bf16 value once |z| >= 1, so a rounding of z in
    front of the activation shows.  A vector longer than the pool repeats it."""
    grid = torch.arange(-256, 257, dtype=torch.float32) / 256
    pool = grid[grid.to(torch.bfloat16).float() == grid].numpy()
    rng = np.random.default_rng(2000 + seed)
    odd = np.round(pool * 256).astype(np.int64) % 2 == 1
    pool = np.concatenate([rng.permutation(pool[odd]), rng.permutation(pool[~odd])])   # the 256 odd multiples first
    distinct = n <= len(pool)
    b = np.ascontiguousarray(np.resize(pool, n))
    t = torch.from_numpy(b).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy(), b) and np.abs(b).max() <= 1 and np.array_equal(b * 256, np.round(b * 256))
    assert not distinct or len(set(b.tolist())) == n
    return t


def exact_z(prod32_np, bias):
    """z = S + bias as fp32, asserted exact (the fp64 sum is an fp32 value)."""
    z64 = torch.from_numpy(prod32_np).double() + bias.double()[None, :]
    z32 = z64.float()
    assert torch.equal(z32.double(), z64), "z = S + b is not exact in fp32"
    assert torch.equal(torch.from_numpy(prod32_np) + bias.float()[None, :], z32)
    return z32


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    lib.bgemm_mi355x_launch_tn_bias_act.argtypes = [i] * 2 + [p] * 4 + [i] * 7 + [p]
    lib.bgemm_mi355x_tn_bias_act.argtypes = [p] * 4 + [i] * 4 + [p]
    lib.bgemm_mi355x_tn_reserve_workspace.argtypes = [i] * 3 + [p]
    lib.bgemm_mi355x_tn_plan_workspace_bytes.restype, lib.bgemm_mi355x_tn_plan_workspace_bytes.argtypes = ctypes.c_size_t, [i] * 5
    return lib


@pytest.fixture(scope="module")
def members(L):
    ids = [(nm, L.bgemm_mi355x_tn_config_by_name(nm.encode())) for nm in MEMBERS]
    assert [cid for _, cid in ids] == [0, 1, 2, 3]
    return ids


def decision(L, cid, word, act, m, n, k, ld=None, aligned=True):
    """What the call decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    st = L.bgemm_mi355x_selfcheck_launch_tn_bias_act(cid, word, 4 if aligned else 0, m, n, k, *(ld or (k, k, n)), 0, act, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


class ActCase(Case):
    """test_gpu_tn_bf16.Case with A scaled to the activations' live range, a bias vector (N bf16 values on the device followed by a NaN
    guard element), the exact z and, per activation, the CPU's expectation: bits for ReLU, y* in fp64 for the GELUs."""

    def __init__(self, m, n, k, seed, padded=False, bias=None):
        super().__init__(m, n, k, seed, padded, scale=(a_scale(k), 1.0))
        self.set_bias(make_bias(n, seed) if bias is None else bias)

    def set_bias(self, bias, offset=0):
        self.bias = bias
        self.bias_buf = torch.full((offset + self.n + 1,), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.bias_buf[offset:offset + self.n] = bias.cuda()
        self.bias_d = self.bias_buf[offset:offset + self.n]
        assert self.bias_d.data_ptr() % 16 == (2 * offset) % 16
        self.bias_before = self.bias_buf.clone()
        self.z32 = exact_z(self.prod32_np, bias)
        self.z64 = self.z32.double()
        self.relu16 = relu_want(self.z32)
        self.y64 = {act: act64(self.z64, act) for act in (GELU, GELU_TANH)}

    def launch(self, g, L, buf, plan, act):
        m, n, k = self.m, self.n, self.k
        if plan is None:
            assert self.ld == (k, k, n)
            st = L.bgemm_mi355x_tn_bias_act(self.ad.data_ptr(), self.wd.data_ptr(), self.bias_d.data_ptr(), buf.data_ptr(), m, n, k, act, g.stream())
        else:
            st = L.bgemm_mi355x_launch_tn_bias_act(plan[0], plan[1], self.ad.data_ptr(), self.wd.data_ptr(), self.bias_d.data_ptr(), buf.data_ptr(), m, n,
                                                   k, *self.ld, act, g.stream())
        assert st == 0, (plan, act, L.hgemm_mi355x_strerror(st))

    def check(self, buf, what, act, key=None):
        torch.cuda.synchronize()
        got = buf[:self.m, :self.n].cpu()
        if act == RELU:
            bad = int((ibits(got) != ibits(self.relu16)).sum())
            assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements differ from where(z > 0, bf16(z), +0)"
        else:
            bad, worst = outside(got, self.y64[act], self.z64)
            if key is not None:
                WORST[key] = max(WORST.get(key, 0.0), worst)
            print(f"{what}: worst error {worst:.3f} of the bar")
            assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements outside 1/2 ulp_bf16(y*) + 2^-19 |z| (worst {worst:.3f} of it)"
        sent = ibits(torch.full((1,), SENTINEL, dtype=buf.dtype, device="cuda"))
        assert bool((ibits(buf[:self.m, self.n:]) == sent).all()) and bool((ibits(buf[self.m]) == sent).all()), f"{what}: the pad or the guard row changed"

    def run(self, g, L, plan, what, act, key=None):
        buf = self.c_buffer()
        self.launch(g, L, buf, plan, act)
        self.check(buf, what, act, key)
        return buf

    def operands_intact(self):
        return super().operands_intact() and torch.equal(ibits(self.bias_buf), ibits(self.bias_before))


@pytest.fixture(scope="module")
def cases():
    """The sweep's operands, biases and expectations, built once per (shape, padded) and shared; nothing writes to them."""
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            built[(shape, padded)] = ActCase(*shape, seed_of(shape), padded)
        return built[(shape, padded)]

    return get


# ---- CPU pre-checks, from reference data alone -----------------------------------------------------------------------------------------
def evidence_of(shape):
    m, n, k = shape
    a, b = operands(m, n, k, seed_of(shape))
    scale = a_scale(k)
    s64 = torch.from_numpy((a.astype(np.int64) @ b.astype(np.int64)).astype(np.float64) * scale)
    bias = make_bias(n, seed_of(shape))
    z32 = exact_z(s64.float().numpy(), bias)
    assert torch.equal(s64.float().double(), s64)
    z64, b32 = z32.double(), bias.float()[None, :]
    az = z64.abs()
    row = {"live": float(((az >= 2.0 ** -6) & (az <= 4)).double().mean()), "negative": float((z64 < 0).double().mean()),
           "in [-4, -2.5]": int(((z64 >= -4) & (z64 <= -2.5)).sum())}
    assert row["live"] >= 0.3 and row["in [-4, -2.5]"] >= 60, (shape, row)

    def slabs(word):
        cuts = [0] + two_pass_cuts(k, word) + [k]
        return [torch.from_numpy(((a[:, lo:hi].astype(np.int64) @ b[lo:hi].astype(np.int64)).astype(np.float64) * scale).astype(np.float32))
                for lo, hi in zip(cuts, cuts[1:])]

    for act in ACTS:
        def count(c16):
            if act == RELU:
                return int((ibits(c16) != ibits(relu_want(z32))).sum())
            return outside(c16, act64(z64, act), z64)[0]
        own = to_bf16(act32_torch(z32, act))
        assert count(own) == 0, (shape, ACT_NAME[act], "the reference's own bf16 result is outside the bar")
        wrong = {"no activation": to_bf16(z32), "bias after the activation": to_bf16(act32_torch(z32 - b32, act) + b32)}
        if act != RELU:                                            # rounding and ReLU commute; ReLU has no other form
            wrong["the other GELU form"] = to_bf16(act32_torch(z32, GELU + GELU_TANH - act))
            wrong["the activation of bf16(z)"] = to_bf16(act32_torch(to_bf16(z32).float(), act))
        for word in (2, 5):
            parts = slabs(word)
            if len(parts) == 1:                                    # K = 64 is one stage: the splits word is clamped to one slab, no such mistake
                assert k == 64
                continue
            wrong[f"the activation of each of {len(parts)} slabs"] = to_bf16(sum(act32_torch(p, act) for p in parts) + b32)
        for what, c16 in wrong.items():
            row[f"{ACT_NAME[act]}: {what}"] = count(c16)
            assert row[f"{ACT_NAME[act]}: {what}"] >= MISTAKE_FLOOR, (shape, ACT_NAME[act], what, row)
    return row


@pytest.fixture(scope="module")
def evidence():
    return {shape: evidence_of(shape) for shape in SHAPES}


def test_the_inputs_are_live_and_the_bar_tells_the_mistakes_apart(evidence):
    for shape, row in evidence.items():
        print(shape, row)
    assert len(evidence) == 4


# ---- every member x form x activation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_form_and_activation_meets_its_bar(g, L, members, cases, evidence, shape, padded):
    m, n, k = shape
    case = cases(shape, padded)
    ran = 0
    for name, cid in members:
        assert L.bgemm_mi355x_tn_bias_act_runs(cid, m, n, k, *case.ld) == 1, (name, shape)
        for word in FORMS:
            cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
            for act in ACTS:
                st, form, disp = decision(L, cid, word, act, m, n, k, case.ld)
                assert (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1), (name, hex(word))
                assert [d[2] for d in disp] == ([EPI_SLAB, EPI_C16_BIAS + act] if cuts else [EPI_C16_BIAS + act])
                case.run(g, L, (cid, word), f"{ACT_NAME[act]} {name} {hex(word)} {m}x{n}x{k} ld={case.ld}", act, (ACT_NAME[act], name, hex(word)))
                ran += 1
    assert ran == 4 * len(FORMS) * 3 and case.operands_intact()


@pytest.mark.parametrize("act", [GELU, GELU_TANH], ids=["gelu", "gelu_tanh"])
def test_the_plain_split_and_reference_forms_agree_bit_for_bit(g, L, members, cases, evidence, act):
    """z is exact in any order and the activation text is one: the kernels' epilogue (plain, non-temporal), the combine (splits 2 and 5) and
    the reference kernel (reached through a bias pointer 2 bytes off) store the same bits."""
    for shape in SHAPES:
        m, n, k = shape
        case = cases(shape)
        off = ActCase(*shape, seed_of(shape))
        off.set_bias(off.bias, offset=1)
        assert decision(L, 0, 1, act, m, n, k, aligned=False)[:2] == (0, FORM_REFERENCE)
        ref = off.run(g, L, (0, 1), f"reference {ACT_NAME[act]} {shape}", act, (ACT_NAME[act], "reference", "0x1"))
        for name, cid in members:
            for word in FORMS:
                got = case.run(g, L, (cid, word), f"{ACT_NAME[act]} {name} {hex(word)} {shape}", act)
                bad = int((ibits(got[:m, :n]) != ibits(ref[:m, :n])).sum())
                assert bad == 0, (ACT_NAME[act], name, hex(word), shape, f"{bad} elements differ from the reference kernel's bits")


def test_m_100_goes_through_the_kernels(g, L, members):
    m, n, k = 100, 136, 128
    case = ActCase(m, n, k, m + n + k)
    for name, cid in members:
        for act in ACTS:
            assert decision(L, cid, 1, act, m, n, k)[:2] == (0, FORM_PLAIN)
            for word in FORMS:
                case.run(g, L, (cid, word), f"M=100 {ACT_NAME[act]} {name} {hex(word)}", act)
    assert case.operands_intact()


# ---- the reference kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["K=72", "N=100", "ldb=K+4", "C 8 bytes off", "bias 2 bytes off"])
def test_what_the_kernels_do_not_take_is_answered_by_the_reference_kernel_on_the_same_bars(g, L, members, what):
    m, n, k = {"K=72": (200, 136, 72), "N=100": (200, 100, 128)}.get(what, (200, 136, 128))
    case = ActCase(m, n, k, m + n + k)
    aligned = what not in ("C 8 bytes off", "bias 2 bytes off")
    if what == "ldb=K+4":
        case.ld = (k, k + 4, n)
        bf = case.wd[:, :k].clone()
        case.wd = torch.full((n, k + 4), float("nan"), dtype=torch.bfloat16, device="cuda")
        case.wd[:, :k] = bf
        case.before = [case.ad.clone(), case.wd.clone()]
    if what == "bias 2 bytes off":
        case.set_bias(case.bias, offset=1)
    for name, cid in members[::3]:
        assert L.bgemm_mi355x_tn_bias_act_runs(cid, m, n, k, *case.ld) == (0 if aligned else 1)
        for act in ACTS:
            assert decision(L, cid, 1, act, m, n, k, case.ld, aligned)[:2] == (0, FORM_REFERENCE)
            for word in (1, 4):
                if what == "C 8 bytes off":
                    flat = torch.full(((m + 1) * n + 16,), SENTINEL, dtype=torch.bfloat16, device="cuda")
                    buf = flat[4:4 + (m + 1) * n].view(m + 1, n)
                    assert buf.data_ptr() % 16 == 8
                    buf[:m] = float("nan")
                    case.launch(g, L, buf, (cid, word), act)
                    case.check(buf, f"{what} {ACT_NAME[act]} {name} {word}", act)
                    assert bool((flat[:4] == SENTINEL).all()) and bool((flat[4 + (m + 1) * n:] == SENTINEL).all()), "the backing tensor changed"
                else:
                    case.run(g, L, (cid, word), f"{what} {ACT_NAME[act]} {name} {word}", act)
    assert case.operands_intact()


# ---- special values --------------------------------------------------------------------------------------------------------------------
def test_special_values_by_column(g, L, members):
    """Bias NaN, +inf, -inf and -0 by column, and a row of S = +0.  ReLU: NaN, +inf, +0, and z = +0 + -0 = +0 gives +0, bits as defined.
    GELU: NaN, +inf, NaN (the formulas' 0 x inf), and z = 0 gives a zero.  Every other element meets its bar."""
    m, n, k = 72, 72, 128
    a, b = operands(m, n, k, 5)
    a[3, :] = 0
    bias = make_bias(n, 5).float().numpy().copy()
    bias[11], bias[30], bias[20], bias[40] = np.nan, np.inf, -np.inf, -0.0
    case = Case(m, n, k, 5, a=a, b=b, scale=(a_scale(k), 1.0))
    with np.errstate(invalid="ignore"):
        z32 = torch.from_numpy(case.prod32_np) + torch.from_numpy(bias)[None, :]
    z64 = z32.double()
    assert bool(torch.isnan(z32[:, 11]).all()) and bool((z32[:, 30] == np.inf).all()) and bool((z32[:, 20] == -np.inf).all())
    assert float(z32[3, 40]) == 0 and not np.signbit(float(z32[3, 40]))
    bd = torch.from_numpy(bias).to(torch.bfloat16).cuda()
    special = torch.zeros(m, n, dtype=torch.bool)
    special[:, [11, 30, 20]] = True
    for name, cid in members:
        for word in FORMS:
            for act in ACTS:
                got = torch.full((m, n), SENTINEL, dtype=torch.bfloat16, device="cuda")
                assert L.bgemm_mi355x_launch_tn_bias_act(cid, word, case.ad.data_ptr(), case.wd.data_ptr(), bd.data_ptr(), got.data_ptr(), m, n, k, k, k, n,
                                                         act, g.stream()) == 0
                torch.cuda.synchronize()
                got = got.cpu()
                what = (ACT_NAME[act], name, hex(word))
                assert bool(torch.isnan(got[:, 11]).all()) and bool((got[:, 30] == np.inf).all()), what
                if act == RELU:
                    assert bool((ibits(got[:, 20]) == 0).all()), what                                   # -inf gives +0
                    clean = torch.where(special, torch.zeros_like(got), got)
                    assert torch.equal(ibits(clean), ibits(torch.where(special, torch.zeros_like(got), relu_want(z32)))), what
                    assert int(ibits(got[3:4, 40])) == 0, what                                          # z = +0 gives +0
                else:
                    assert bool(torch.isnan(got[:, 20]).all()), what                                    # -inf gives NaN
                    assert float(got[3, 40]) == 0.0, what
                    zf = torch.where(special, torch.ones_like(z64), z64)
                    bad, worst = outside(torch.where(special, act64(zf, act).to(torch.bfloat16), got), act64(zf, act), zf)
                    assert bad == 0, (what, bad, worst)


# ---- N(0,1) operands and bias ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def randn():
    m, n, k = 264, 264, 512
    rng = np.random.default_rng(13)
    a16 = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).to(torch.bfloat16)
    w16 = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32)).to(torch.bfloat16)
    b16 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(torch.bfloat16)
    return (m, n, k), a16, w16, b16


def test_relu_equals_relu_of_the_librarys_bias_call_on_randn_operands(g, L, members, randn):
    """Rounding and ReLU commute, so no exact z is needed: the output equals where(Y > 0 or Y is NaN, Y, +0) bit for bit, Y being
    bgemm_mi355x_launch_tn_bias with the same member and splits."""
    (m, n, k), a16, w16, b16 = randn
    ad, wd, bd = a16.cuda(), w16.cuda(), b16.cuda()
    for name, cid in members:
        for word in FORMS:
            y = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            assert L.bgemm_mi355x_launch_tn_bias(cid, word, ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
            assert L.bgemm_mi355x_launch_tn_bias_act(cid, word, ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, k, k, n, RELU,
                                                     g.stream()) == 0
            torch.cuda.synchronize()
            want = torch.where((y > 0) | torch.isnan(y), y, torch.zeros_like(y))
            assert not bool(torch.isnan(y).any()) and int((y > 0).sum()) > m * n // 4 and int((y < 0).sum()) > m * n // 4
            assert torch.equal(ibits(c), ibits(want)), (name, hex(word))


@pytest.mark.parametrize("act", [GELU, GELU_TANH], ids=["gelu", "gelu_tanh"])
def test_gelu_meets_the_bar_widened_by_the_sums_error_on_randn_operands(g, L, members, randn, act):
    """|C - y*| <= 1/2 ulp_bf16(y*) + 2^-19 |z| + 1.13 (K 2^-24 sum |a||b| + 2^-24 |z|) against the fp64 product: 1.13 bounds |gelu'| for
    both forms, the last bracket is the first-order error of the fp32 sum and of the bias add.  No element is skipped."""
    (m, n, k), a16, w16, b16 = randn
    a64, w64, b64 = a16.double(), w16.double(), b16.double()
    z64 = a64 @ w64.T + b64[None, :]
    mag = a64.abs() @ w64.abs().T
    y64 = act64(z64, act)
    extra = 1.13 * (k * 2.0 ** -24 * mag + 2.0 ** -24 * z64.abs())
    ad, wd, bd = a16.cuda(), w16.cuda(), b16.cuda()
    for name, cid in members:
        for word in FORMS:
            c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            assert L.bgemm_mi355x_launch_tn_bias_act(cid, word, ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), c.data_ptr(), m, n, k, k, k, n, act,
                                                     g.stream()) == 0
            torch.cuda.synchronize()
            bad, worst = outside(c.cpu(), y64, z64, extra)
            print(f"randn {ACT_NAME[act]} {name} {hex(word)}: worst error {worst:.3f} of the bound")
            assert bad == 0, (ACT_NAME[act], name, hex(word), bad, worst)


# ---- planned entries and capture ---------------------------------------------------------------------------------------------------------
def test_the_planned_call_through_a_split_plan_and_an_unsplit_one(g, L, evidence):
    """256 x 264 x 512: 20 tiles of 64 x 64, eight two-pass splits.  1024 x 1024 x 64: 256 tiles fill the chip, one stage, unsplit."""
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for (m, n, k), want in (((256, 264, 512), 8), ((1024, 1024, 64), 1)):
        assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and (cfg.value, splits.value) == (0, want)
        case = ActCase(m, n, k, m + n + k)
        for act in ACTS:
            st, form, disp = decision(L, cfg.value, splits.value, act, m, n, k)
            assert (st, form, len(disp), disp[0][3]) == ((0, FORM_SPLITK, 2, 8) if want > 1 else (0, FORM_PLAIN, 1, 1))
            case.run(g, L, None, f"planned {ACT_NAME[act]} {m}x{n}x{k}", act)
        assert case.operands_intact()
    null = ctypes.c_void_p(0)
    buf = case.c_buffer()
    assert L.bgemm_mi355x_tn_bias_act(case.ad.data_ptr(), case.wd.data_ptr(), null, buf.data_ptr(), m, n, k, GELU, g.stream()) == -1
    for act in (0, 4, -1):
        assert L.bgemm_mi355x_tn_bias_act(case.ad.data_ptr(), case.wd.data_ptr(), case.bias_d.data_ptr(), buf.data_ptr(), m, n, k, act, g.stream()) == -1


def test_a_split_call_captured_without_a_workspace_runs_unsplit_and_split_after_the_reserve_call(g, L, evidence):
    """On a fresh stream with nothing reserved the split call returns 0 while capturing and replays unsplit; after
    bgemm_mi355x_tn_reserve_workspace on another fresh stream it replays through its slabs and the activation combine.  Both replays equal
    the eager call bit for bit.  One stream, one chain per graph: no parallel branches."""
    m, n, k = 200, 264, 512
    case = ActCase(m, n, k, 61)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.bgemm_mi355x_tn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == 8
    cid = cfg.value
    assert L.bgemm_mi355x_tn_plan_workspace_bytes(cid, splits.value, m, n, k) == COUNTER_BYTES + 8 * m * n * 4
    for act in ACTS:
        assert decision(L, cid, splits.value, act, m, n, k)[1] == FORM_SPLITK
        eager = case.run(g, L, (cid, splits.value), f"eager {ACT_NAME[act]}", act)
        for reserve in (False, True):
            buf = case.c_buffer()
            s = torch.cuda.Stream()
            if reserve:
                assert L.bgemm_mi355x_tn_reserve_workspace(m, n, k, s.cuda_stream) == 0
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                rc = L.bgemm_mi355x_launch_tn_bias_act(cid, splits.value, case.ad.data_ptr(), case.wd.data_ptr(), case.bias_d.data_ptr(), buf.data_ptr(),
                                                       m, n, k, k, k, n, act, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, reserve
            buf[:m, :n] = float("nan")
            torch.cuda.synchronize()
            graph.replay()
            case.check(buf, f"replay {ACT_NAME[act]}, reserved={reserve}", act)
            assert torch.equal(ibits(buf), ibits(eager))
    assert case.operands_intact()


def test_print_the_worst_ratios(evidence):
    """The worst error / bar per activation, member and form over the sweep above (DESIGN.md 4.28 records them)."""
    for key in sorted(WORST):
        print("worst ratio", *key, f"{WORST[key]:.3f}")
    # two GELUs x (four members x four forms + the reference kernel): an empty or partial table -- this test run alone -- fails
    assert len(WORST) == 2 * (4 * len(FORMS) + 1), f"{len(WORST)} rows: run the whole file, the sweep and the forms test fill the table"
    assert all(v <= 1.0 for v in WORST.values())


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the three bias+activation sets (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit."""
    def one(act):
        return g.HelperKernelSet(lambda cfg, word, p, d, acc: L.bgemm_mi355x_launch_tn_bias_act(cfg, word, p["a"], p["b"], p["bias"], p["c"], *d[:6], act, g.stream()),
                                 lambda cfg, word, d, aligned, acc: decision(L, cfg, word, act, *d[:3], d[3:6], aligned), torch.bfloat16, b_col=True, bias=True)
    sets = [one(act) for act in ACTS]
    for s in sets:
        s.check_combine(128, 2, 9161)
        s.check_combine(704, 11, 9161 + 1)
        s.check_reference(9161 + 2)
