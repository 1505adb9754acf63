"""GPU tests of the gated forward product (run with `-m gpu` on an MI355X): bgemm_mi355x_tn_gated / bgemm_mi355x_launch_tn_gated --
H = act(X Wg^T + bg) (.) (X Wu^T + bu); family f's gated kernels (hgemm_inst_g18.hip), the gated combine of the two-pass form and the gated
reference kernel, all three on the activation text of hgemm_act.hpp and the one product of hgemm_gated.hpp.

The semantics under test:  g = fl32(Sg + float(bias_g[n])),  u = fl32(Su + float(bias_u[n])),  C = bf16_rne(fl32(act32(g) u)): bias,
activation and gate applied once to finished sums, never to a slab, one rounding.
  * ReLU (act 1) is held bit for bit against bf16_rne(fl32(relu(g32) u32)) from the CPU: an IEEE fp32 multiply is the same everywhere.
  * Both GELUs and SiLU (act 2, 3, 4) are held, unmasked, to  |C - y*| <= 1/2 ulp_bf16(y*) + 2^-19 |g| |u| + 2^-23 |y*|,  y* = act*(g) u in
    fp64 on the exactly known g and u; the two constants are read from csrc/hgemm_gated.hpp.

Inputs with exact g and u: Wg and Wu independent integers in -2 .. 2 (tests/test_gpu_tr_bf16.py's operands, two seeds), A scaled by
a_scale(K), two bias vectors of make_bias with different seeds: both sums are multiples of 2^-7 below 2^6 and g, u multiples of 2^-8, exact
in fp32 in any order (asserted).  Before any launch the module shows on the CPU, from reference data alone, at every shape with at least
4096 outputs, that torch's own fp32 evaluation is inside the bar everywhere and that each mistake of MISTAKES is outside it (ReLU: differs in
bits) in at least MISTAKE_FLOOR elements.

C lies in [M + 1][ldc] with a sentinel in the pad and the guard row, NaN sits in the operands' padding, each bias vector is followed by a
NaN guard element, and operands and biases must be bit-unchanged afterwards."""
import contextlib
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from test_gpu_dbias import fresh_stream
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import COUNTER_BYTES, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, two_pass_cuts
from test_gpu_tn_bf16 import MEMBERS, Case
from test_gpu_tn_bias_act import GELU, GELU_TANH, MISTAKE_FLOOR, RELU, a_scale, act32_torch, act64, make_bias
from test_gpu_tr_bf16 import SENTINEL, ibits, operands, seed_of, to_bf16

pytestmark = pytest.mark.gpu

SILU = 4
ACTS = (RELU, GELU, GELU_TANH, SILU)
ACT_NAME = {RELU: "relu", GELU: "gelu", GELU_TANH: "gelu_tanh", SILU: "silu"}
EPI_SLAB, EPI_C16_GATED, EPI_C16_BIAS = 1, 64, 5
NT_STORE = FORMS[1] & ~1
# (M, N output, K): one tile of the smallest member; a sliver; ragged M and N with an 8-column sliver tile and the per-weight row clamp; the
# ring wraps and the cuts are uneven; three tiles each way for f128x128
SHAPES = [(64, 32, 64), (8, 8, 64), (136, 72, 128), (152, 152, 320), (264, 264, 512)]
WORST = {}                                                       # (act, member, form) -> worst error / bar, printed by the last test

_text = (Path(__file__).resolve().parents[1] / "cuda-l2_amd" / "csrc" / "hgemm_gated.hpp").read_text()
ACT_EPS = 2.0 ** int(re.search(r"GATED_ACT_EPS_LOG2 = (-\d+)", _text).group(1))
MUL_EPS = 2.0 ** int(re.search(r"GATED_MUL_EPS_LOG2 = (-\d+)", _text).group(1))
assert (ACT_EPS, MUL_EPS) == (2.0 ** -19, 2.0 ** -23)              # the issue's bar; the header states it once


# ---- the activations, the bar and the expectations -------------------------------------------------------------------------------------
def gact64(z, act):
    return z * torch.sigmoid(z) if act == SILU else act64(z, act)


def gact32(z32, act):
    """torch's own fp32 activation"""
    return torch.nn.functional.silu(z32) if act == SILU else act32_torch(z32, act)


def bar(y64, g64, u64):
    ay = y64.abs()
    half_ulp = torch.where(ay > 0, torch.exp2(torch.floor(torch.log2(torch.where(ay > 0, ay, torch.ones_like(ay)))) - 8), torch.zeros_like(ay))
    return half_ulp + ACT_EPS * g64.abs() * u64.abs() + MUL_EPS * ay


def outside(c16, y64, g64, u64):
    """Elements of a bf16 result outside the bar, and the worst error / bar.  Every element is finite here and none is left out."""
    bound = bar(y64, g64, u64)
    err = (c16.double() - y64).abs()
    bad = ~(err <= bound)                                          # (a NaN or an infinity in the result counts)
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)), torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max())


def relu_want(g32, u32):
    return to_bf16(torch.relu(g32) * u32)


def count_wrong(c16, act, g32, u32):
    if act == RELU:
        return int((ibits(c16) != ibits(relu_want(g32, u32))).sum())
    return outside(c16, gact64(g32.double(), act) * u32.double(), g32.double(), u32.double())[0]


def gated_operands(m, n, k, seed):
    """A [M][K] and the two weights as [K][N] integer matrices: independent draws of tests/test_gpu_tr_bf16.py's operands."""
    a, bg = operands(m, n, k, seed)
    _, bu = operands(m, n, k, seed + 1000)
    return a, bg, bu


def exact(prod64, bias):
    """S + bias as fp32, asserted exact and a multiple of 2^-8"""
    z64 = prod64 + bias.double()[None, :]
    z32 = z64.float()
    assert torch.equal(z32.double(), z64) and torch.equal(prod64.float() + bias.float()[None, :], z32), "S + b is not exact in fp32"
    assert torch.equal(torch.round(z64 * 256), z64 * 256)
    return z32


def biases(n, seed):
    return make_bias(n, seed), make_bias(n, seed + 77)


# ---- CPU proof, from reference data alone -------------------------------------------------------------------------------------------------
def evidence_of(shape):
    m, n, k = shape
    a, wg, wu = gated_operands(m, n, k, seed_of(shape))
    scale = a_scale(k)
    prod = lambda w, lo=0, hi=k: torch.from_numpy((a[:, lo:hi].astype(np.int64) @ w[lo:hi].astype(np.int64)).astype(np.float64) * scale)  # noqa: E731
    bg, bu = biases(n, seed_of(shape))
    g32, u32 = exact(prod(wg), bg), exact(prod(wu), bu)
    bg32, bu32 = bg.float()[None, :], bu.float()[None, :]
    row = {}
    for act in ACTS:
        f = lambda z: gact32(z, act)                               # noqa: E731
        own = to_bf16(f(g32) * u32)
        assert count_wrong(own, act, g32, u32) == 0, (shape, ACT_NAME[act], "torch's own fp32 evaluation is outside the bar")
        wrong = {"gate and up swapped": to_bf16(f(u32) * g32),
                 "the biases swapped": to_bf16(f(g32 - bg32 + bu32) * (u32 - bu32 + bg32)),
                 "act(bf16(g))": to_bf16(f(to_bf16(g32).float()) * u32),
                 "u rounded before the multiply": to_bf16(f(g32) * to_bf16(u32).float()),
                 "act(g) rounded before the multiply": to_bf16(to_bf16(f(g32)).float() * u32),
                 "no activation": to_bf16(g32 * u32),
                 "up from the neighbouring fragment": to_bf16(f(g32) * torch.roll(u32, -16, 1))}
        if act == SILU:
            wrong["gelu_tanh for silu"] = to_bf16(gact32(g32, GELU_TANH) * u32)
        if act == GELU_TANH:
            wrong["silu for gelu_tanh"] = to_bf16(gact32(g32, SILU) * u32)
        for word in (2, 5):
            cuts = [0] + two_pass_cuts(k, word) + [k]
            if len(cuts) > 2:
                parts = [prod(wg, lo, hi).float() for lo, hi in zip(cuts, cuts[1:])]
                wrong[f"the activation of each of {len(parts)} slabs"] = to_bf16((sum(f(p) for p in parts) + bg32) * u32)
        for what, c16 in wrong.items():
            row[f"{ACT_NAME[act]}: {what}"] = count_wrong(c16, act, g32, u32)
            assert row[f"{ACT_NAME[act]}: {what}"] >= MISTAKE_FLOOR, (shape, ACT_NAME[act], what, row)
    return row


@pytest.fixture(scope="module")
def evidence():
    return {shape: evidence_of(shape) for shape in SHAPES if shape[0] * shape[1] >= 4096}


def test_the_bar_tells_the_mistakes_apart(evidence):
    for shape, row in evidence.items():
        print(shape, row)
    assert len(evidence) == 3


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn_gated.argtypes = [i] * 2 + [p] * 6 + [i] * 7 + [p]
    lib.bgemm_mi355x_tn_gated.argtypes = [p] * 6 + [i] * 4 + [p]
    lib.bgemm_mi355x_launch_tn_bias_act.argtypes = [i] * 2 + [p] * 4 + [i] * 7 + [p]
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
    st = L.bgemm_mi355x_selfcheck_launch_tn_gated(cid, word, 4 if aligned else 0, m, n, k, *(ld or (k, k, n)), 0, act, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def guarded(vec, offset=0):
    """A bias vector on the device followed by a NaN guard element; (buffer, view)"""
    buf = torch.full((offset + len(vec) + 1,), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[offset:offset + len(vec)] = vec.cuda()
    return buf, buf[offset:offset + len(vec)]


class GatedCase(Case):
    """test_gpu_tn_bf16.Case over the STACKED weight [Wg; Wu] ([2 N][ldb], NaN in the padding): fused=True passes it as it lies,
    wu = wg + N ldb; otherwise the two halves are copied into buffers of their own.  Two guarded bias vectors, the exact g and u and the
    CPU's expectations."""

    def __init__(self, m, n, k, seed, padded=False, fused=False, wu=None, bu=None):
        a, wg, wu_ = gated_operands(m, n, k, seed)
        wu = wu_ if wu is None else wu
        super().__init__(m, 2 * n, k, seed, padded, a=a, b=np.concatenate([wg, wu], axis=1), scale=(a_scale(k), 1.0))
        self.n = n
        self.ld = (self.ld[0], self.ld[1], (n + 8) if padded else n)
        if fused:
            self.wg_d, self.wu_d = self.wd[:n], self.wd[n:]
            assert self.wu_d.data_ptr() == self.wg_d.data_ptr() + n * self.ld[1] * 2
        else:
            self.wg_d, self.wu_d = self.wd[:n].clone(), self.wd[n:].clone()
        bg, bu_ = biases(n, seed)
        self.bg, self.bu = bg, (bu_ if bu is None else bu)
        (self.bg_buf, self.bg_d), (self.bu_buf, self.bu_d) = guarded(self.bg), guarded(self.bu)
        self.before = [x.clone() for x in (self.ad, self.wd, self.wg_d, self.wu_d, self.bg_buf, self.bu_buf)]
        s64 = torch.from_numpy(self.prod32_np).double()
        self.g32, self.u32 = exact(s64[:, :n], self.bg), exact(s64[:, n:], self.bu)
        self.g64, self.u64 = self.g32.double(), self.u32.double()
        self.relu16 = relu_want(self.g32, self.u32)
        self.y64 = {act: gact64(self.g64, act) * self.u64 for act in ACTS if act != RELU}

    def launch(self, g, L, buf, plan, act, bg="own", bu="own"):
        m, n, k = self.m, self.n, self.k
        bg = self.bg_d.data_ptr() if bg == "own" else bg
        bu = self.bu_d.data_ptr() if bu == "own" else bu
        if plan is None:
            assert self.ld == (k, k, n)
            st = L.bgemm_mi355x_tn_gated(self.ad.data_ptr(), self.wg_d.data_ptr(), self.wu_d.data_ptr(), bg, bu, buf.data_ptr(), m, n, k, act, g.stream())
        else:
            st = L.bgemm_mi355x_launch_tn_gated(plan[0], plan[1], self.ad.data_ptr(), self.wg_d.data_ptr(), self.wu_d.data_ptr(), bg, bu, buf.data_ptr(),
                                                m, n, k, *self.ld, act, g.stream())
        assert st == 0, (plan, act, L.hgemm_mi355x_strerror(st))

    def check(self, buf, what, act, key=None):
        torch.cuda.synchronize()
        got = buf[:self.m, :self.n].cpu()
        if act == RELU:
            bad = int((ibits(got) != ibits(self.relu16)).sum())
            assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements differ from bf16(relu(g) u)"
        else:
            bad, worst = outside(got, self.y64[act], self.g64, self.u64)
            if key is not None:
                WORST[key] = max(WORST.get(key, 0.0), worst)
            print(f"{what}: worst error {worst:.3f} of the bar")
            assert bad == 0, f"{what}: {bad} of {self.m * self.n} elements outside the bar (worst {worst:.3f} of it)"
        sent = ibits(torch.full((1,), SENTINEL, dtype=buf.dtype, device="cuda"))
        assert bool((ibits(buf[:self.m, self.n:]) == sent).all()) and bool((ibits(buf[self.m]) == sent).all()), f"{what}: the pad or the guard row changed"

    def c_buffer(self):
        buf = torch.full((self.m + 1, self.ld[2]), SENTINEL, dtype=torch.bfloat16, device="cuda")
        buf[:self.m, :self.n] = float("nan")
        return buf

    def run(self, g, L, plan, what, act, key=None, **kw):
        buf = self.c_buffer()
        self.launch(g, L, buf, plan, act, **kw)
        self.check(buf, what, act, key)
        return buf

    def operands_intact(self):
        return all(torch.equal(ibits(x), ibits(was)) for x, was in zip((self.ad, self.wd, self.wg_d, self.wu_d, self.bg_buf, self.bu_buf), self.before))


@pytest.fixture(scope="module")
def cases():
    """The sweep's operands and expectations, built once per (shape, padded) and shared; nothing writes to them."""
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            built[(shape, padded)] = GatedCase(*shape, seed_of(shape), padded)
        return built[(shape, padded)]

    return get


# ---- every member x form x activation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_form_and_activation_meets_its_bar(g, L, members, cases, evidence, shape, padded):
    """ReLU to bits, the others to the bar, unmasked; the non-temporal result is the plain one bit for bit."""
    m, n, k = shape
    case = cases(shape, padded)
    ran = 0
    for name, cid in members:
        assert L.bgemm_mi355x_tn_gated_runs(cid, m, n, k, *case.ld) == 1, (name, shape)
        for act in ACTS:
            plain = None
            for word in FORMS:
                cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
                st, form, disp = decision(L, cid, word, act, m, n, k, case.ld)
                assert (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1), (name, hex(word))
                assert [d[2] for d in disp] == ([EPI_SLAB, EPI_C16_GATED + act] if cuts else [EPI_C16_GATED + act])
                got = case.run(g, L, (cid, word), f"{ACT_NAME[act]} {name} {hex(word)} {m}x{n}x{k} ld={case.ld}", act, (ACT_NAME[act], name, hex(word)))
                if word == 1:
                    plain = got
                if word == 1 | NT_STORE:
                    assert torch.equal(ibits(got), ibits(plain)), (name, ACT_NAME[act], "the non-temporal result differs from the plain one")
                ran += 1
    assert ran == 4 * len(FORMS) * len(ACTS) and case.operands_intact()


def test_a_fused_gate_up_weight_is_passed_as_one_buffer(g, L, members):
    """[2 N][ldb] with wu = wg + N ldb, N = 72: the last gate tile's rows past N are Wu's first rows in memory; the per-weight clamp keeps
    the gate's reads in the gate."""
    shape = (136, 72, 128)
    for padded in (False, True):
        case = GatedCase(*shape, seed_of(shape), padded, fused=True)
        for name, cid in members:
            for act in ACTS:
                for word in (1, 2):
                    case.run(g, L, (cid, word), f"fused {ACT_NAME[act]} {name} {word}", act)
        assert case.operands_intact()


def test_wg_equal_to_wu_is_allowed(g, L, members):
    m, n, k = 72, 40, 128
    a, wg, _ = gated_operands(m, n, k, 9)
    case = GatedCase(m, n, k, 9, wu=wg)
    case.wu_d = case.wg_d
    for name, cid in members:
        for act in (RELU, SILU):
            case.run(g, L, (cid, 1), f"wg == wu {ACT_NAME[act]} {name}", act)


# ---- the reference form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["N % 8 == 4", "C 8 bytes off", "bias_u 2 bytes off"])
def test_what_the_kernels_do_not_take_is_answered_by_the_reference_kernel_on_the_same_bars(g, L, members, what):
    m, n, k = (136, 76, 128) if what == "N % 8 == 4" else (136, 72, 128)
    case = GatedCase(m, n, k, m + n + k)
    aligned = what == "N % 8 == 4"
    if what == "bias_u 2 bytes off":
        case.bu_buf, case.bu_d = guarded(case.bu, offset=1)
        assert case.bu_d.data_ptr() % 16 == 2
        case.before[5] = case.bu_buf.clone()
    for name, cid in members[::3]:
        assert L.bgemm_mi355x_tn_gated_runs(cid, m, n, k, *case.ld) == (0 if aligned else 1)
        for act in ACTS:
            assert decision(L, cid, 1, act, m, n, k, case.ld, aligned)[:2] == (0, FORM_REFERENCE)
            for word in (1, 4):
                if what == "C 8 bytes off":
                    flat = torch.full(((m + 1) * n + 16,), SENTINEL, dtype=torch.bfloat16, device="cuda")
                    buf = flat[4:4 + (m + 1) * n].view(m + 1, n)
                    assert buf.data_ptr() % 16 == 8
                    buf[:m] = float("nan")
                    case.launch(g, L, buf, (cid, word), act)
                    case.check(buf, f"{what} {ACT_NAME[act]} {name} {word}", act, (ACT_NAME[act], "reference", "0x1"))
                    assert bool((flat[:4] == SENTINEL).all()) and bool((flat[4 + (m + 1) * n:] == SENTINEL).all()), "the backing tensor changed"
                else:
                    case.run(g, L, (cid, word), f"{what} {ACT_NAME[act]} {name} {word}", act, (ACT_NAME[act], "reference", "0x1"))
    assert case.operands_intact()


# ---- null biases, repeatability, the planned call, the identity ----------------------------------------------------------------------------
def test_a_null_bias_equals_a_vector_of_zeros_bit_for_bit(g, L, members):
    shape = (136, 72, 128)
    case = GatedCase(*shape, seed_of(shape))
    zbuf, zero = guarded(torch.zeros(shape[1], dtype=torch.bfloat16))
    null = ctypes.c_void_p(0)
    ref_case = GatedCase(136, 76, 128, 1)                          # N % 8 == 4: the reference kernel
    zbuf76, zero76 = guarded(torch.zeros(76, dtype=torch.bfloat16))
    for name, cid in members:
        for act in (RELU, GELU, SILU):
            for word in (1, 2):
                for c, z, why in ((case, zero, "kernels"), (ref_case, zero76, "reference")):
                    if why == "reference" and cid:
                        continue
                    for which in ("g", "u", "both"):
                        outs = []
                        for bias_of in (lambda own: null, lambda own: z.data_ptr()):
                            buf = c.c_buffer()
                            c.launch(g, L, buf, (cid, word), act, bg=bias_of(0) if which in ("g", "both") else "own",
                                     bu=bias_of(0) if which in ("u", "both") else "own")
                            outs.append(buf)
                        torch.cuda.synchronize()
                        assert not bool(torch.isnan(outs[0][:c.m, :c.n]).any())
                        assert torch.equal(ibits(outs[0]), ibits(outs[1])), (why, name, ACT_NAME[act], word, which)
    assert case.operands_intact() and bool((zbuf[:-1] == 0).all()) and bool((zbuf76[:-1] == 0).all())


def test_two_runs_of_one_plan_are_bit_identical_and_the_planned_call_is_the_explicit_one(g, L, cases, evidence):
    """256 x 136 x 512: bgemm_mi355x_tn_plan(M, 2 N, K) -- 20 tiles of the 64 x 64 member, eight splits.  1024 x 512 x 64: 256 tiles, unsplit."""
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for (m, n, k), want in (((256, 136, 512), 8), ((1024, 512, 64), 1)):
        assert L.bgemm_mi355x_tn_plan(m, 2 * n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and (cfg.value, splits.value) == (0, want)
        case = GatedCase(m, n, k, m + n + k)
        for act in ACTS:
            st, form, disp = decision(L, cfg.value, splits.value, act, m, n, k)
            assert (st, form, len(disp), disp[0][3]) == ((0, FORM_SPLITK, 2, 8) if want > 1 else (0, FORM_PLAIN, 1, 1))
            planned = case.run(g, L, None, f"planned {ACT_NAME[act]} {m}x{n}x{k}", act)
            first = case.run(g, L, (cfg.value, splits.value), f"explicit {ACT_NAME[act]}", act)
            second = case.run(g, L, (cfg.value, splits.value), f"explicit again {ACT_NAME[act]}", act)
            assert torch.equal(ibits(first), ibits(second)) and torch.equal(ibits(planned), ibits(first)), ACT_NAME[act]
        assert case.operands_intact()


def test_relu_with_u_equal_to_one_is_the_bias_act_call_bit_for_bit(g, L, members):
    """Wu = 0 and bias_u = 1.0: u = 1 exactly, so C = bf16(relu(g)) -- bgemm_mi355x_launch_tn_bias_act's ReLU C with (Wg, bias_g) at width N."""
    for shape in ((136, 72, 128), (264, 264, 512)):
        m, n, k = shape
        case = GatedCase(m, n, k, seed_of(shape), wu=np.zeros((k, n), dtype=np.int64), bu=torch.ones(n, dtype=torch.bfloat16))
        assert bool((case.u32 == 1).all())
        for name, cid in members:
            for word in FORMS:
                got = case.run(g, L, (cid, word), f"u = 1 {name} {hex(word)}", RELU)
                want = case.c_buffer()
                assert L.bgemm_mi355x_launch_tn_bias_act(cid, word, case.ad.data_ptr(), case.wg_d.data_ptr(), case.bg_d.data_ptr(), want.data_ptr(), m, n, k,
                                                         *case.ld, RELU, g.stream()) == 0
                torch.cuda.synchronize()
                assert torch.equal(ibits(got), ibits(want)), (shape, name, hex(word))


def test_bad_arguments_are_refused_on_the_device_too(g, L, cases):
    case = cases((64, 32, 64))
    buf = case.c_buffer()
    m, n, k = 64, 32, 64
    for act in (0, 5, -1):
        assert L.bgemm_mi355x_tn_gated(case.ad.data_ptr(), case.wg_d.data_ptr(), case.wu_d.data_ptr(), None, None, buf.data_ptr(), m, n, k, act, g.stream()) == -1
    assert L.bgemm_mi355x_launch_tn_bias_act(0, 1, case.ad.data_ptr(), case.wg_d.data_ptr(), case.bg_d.data_ptr(), buf.data_ptr(), m, n, k, k, k, n, SILU,
                                             g.stream()) == -1     # SiLU stays the gated calls' alone
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:m, :n]).all())


# ---- capture -------------------------------------------------------------------------------------------------------------------------------
def test_a_split_call_captured_without_a_workspace_runs_unsplit_and_split_after_the_reserve_call(g, L, evidence):
    """On a fresh stream with nothing reserved the split call returns 0 while capturing and replays unsplit; after
    bgemm_mi355x_tn_reserve_workspace(M, 2 N, K) on another fresh stream it replays through its slabs and the gated combine.  Both replays
    equal the eager call bit for bit (g and u are exact in any order).  Streams made with the runtime and destroyed on the way out; one
    stream, one chain per graph."""
    m, n, k = 200, 136, 512
    case = GatedCase(m, n, k, 61)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.bgemm_mi355x_tn_plan(m, 2 * n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == 8
    cid = cfg.value
    assert L.bgemm_mi355x_tn_plan_workspace_bytes(cid, splits.value, m, 2 * n, k) == COUNTER_BYTES + 8 * m * 2 * n * 4
    with contextlib.ExitStack() as streams:
        for act in (RELU, SILU):
            assert decision(L, cid, splits.value, act, m, n, k)[1] == FORM_SPLITK
            eager = case.run(g, L, (cid, splits.value), f"eager {ACT_NAME[act]}", act)
            for reserve in (False, True):
                buf = case.c_buffer()
                s = streams.enter_context(fresh_stream())
                if reserve:
                    assert L.bgemm_mi355x_tn_reserve_workspace(m, 2 * n, k, s.cuda_stream) == 0
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.stream(s):
                    graph.capture_begin()
                    try:
                        rc = L.bgemm_mi355x_launch_tn_gated(cid, splits.value, case.ad.data_ptr(), case.wg_d.data_ptr(), case.wu_d.data_ptr(),
                                                            case.bg_d.data_ptr(), case.bu_d.data_ptr(), buf.data_ptr(), m, n, k, k, k, n, act, s.cuda_stream)
                    finally:
                        graph.capture_end()
                    assert rc == 0, reserve
                    buf[:m, :n] = float("nan")
                    torch.cuda.synchronize()
                    graph.replay()
                torch.cuda.synchronize()
                del graph
                case.check(buf, f"replay {ACT_NAME[act]}, reserved={reserve}", act)
                assert torch.equal(ibits(buf), ibits(eager))
    assert case.operands_intact()


@pytest.fixture(scope="module", autouse=True)
def print_the_worst_ratios():
    """The worst error / bar per activation, member and form over whatever tests of this module ran (DESIGN.md 4.32 records the whole
    file's table).  A record, not a threshold: each run asserts its own bar where it is measured."""
    yield
    for key in sorted(WORST):
        print("worst ratio", *key, f"{WORST[key]:.3f}")
