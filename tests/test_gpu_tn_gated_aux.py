"""GPU tests of the gated forward product's training form (run with `-m gpu` on an MI355X): bgemm_mi355x_tn_gated_aux /
bgemm_mi355x_launch_tn_gated_aux -- H = act(X Wg^T + bg) (.) (X Wu^T + bu) AND the rounded pre-activations g_out = bf16(g), u_out = bf16(u);
family f's gated aux kernels (hgemm_inst_g20.hip), the combine of the two-pass form and the reference kernel (OutGatedAux).

The semantics under test, g and u the fp32 values of tests/test_gpu_tn_gated.py:
    g_out = bf16_rne(g)     u_out = bf16_rne(u)     C = bf16_rne(fl32(act32(g) u))          the activation and the gate on the UNROUNDED g, u
  * C is judged by that module's count_wrong (ReLU bit for bit, the others to its bar); g_out and u_out bit for bit, every activation.
  * Operands, bars, shapes and forms are that module's; g and u are multiples of 2^-8 below 2^6, bf16 keeps 8 bits, so the rounding is live
    (asserted).  Before any launch the module shows on the CPU, from reference data alone, that each mistake of the list differs in at
    least MISTAKE_FLOOR elements.

All three outputs lie in [M + 1][ld] with a sentinel in the pad and the guard row, in two layouts: separate g_out and u_out at ldz = N + 8,
and the fused [M][2N + 8] buffer (u_out = g_out + N) that bgemm_mi355x_launch_nn_dgated takes as it is."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_dbias import fresh_stream
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_nn_dgated import Ops
from test_gpu_nn_dgated import check as dgated_check
from test_gpu_ta import FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, two_pass_cuts
from test_gpu_tn_bf16 import MEMBERS
from test_gpu_tn_bias_act import MISTAKE_FLOOR, RELU, a_scale
from test_gpu_tn_gated import (ACT_NAME, ACTS, EPI_SLAB, NT_STORE, SHAPES, SILU, GatedCase, count_wrong, gact32, guarded)
from test_gpu_tr_bf16 import SENTINEL, ibits, seed_of, to_bf16

pytestmark = pytest.mark.gpu

EPI_C16_GATED, EPI_C16_GATED_AUX, EPI_C16_BIAS = 64, 128, 5
LAYOUTS = ("separate", "fused")
assert SHAPES == [(64, 32, 64), (8, 8, 64), (136, 72, 128), (152, 152, 320), (264, 264, 512)]


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_tn_gated_aux.argtypes = [i] * 2 + [p] * 8 + [i] * 8 + [p]
    lib.bgemm_mi355x_tn_gated_aux.argtypes = [p] * 8 + [i] * 4 + [p]
    lib.bgemm_mi355x_launch_tn_gated.argtypes = [i] * 2 + [p] * 6 + [i] * 7 + [p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    lib.bgemm_mi355x_launch_nn_dgated.argtypes = [i] * 2 + [p] * 6 + [i] * 8 + [p]
    lib.bgemm_mi355x_tn_reserve_workspace.argtypes = [i] * 3 + [p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    ids = [(nm, L.bgemm_mi355x_tn_config_by_name(nm.encode())) for nm in MEMBERS]
    assert [cid for _, cid in ids] == [0, 1, 2, 3]
    return ids


def decision(L, cid, word, act, m, n, k, ld, ldz, aligned=True, hook="bgemm_mi355x_selfcheck_launch_tn_gated_aux"):
    """What the call decides, nothing launched: (status, form, [(thunk, grid, epi, splits, k_chunk)])."""
    out = (ctypes.c_longlong * 20)()
    st = getattr(L, hook)(cid, word, 4 if aligned else 0, m, n, k, *ld, ldz, 0, act, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def sentinel_buffer(rows, ld, m, n):
    buf = torch.full((rows, ld), SENTINEL, dtype=torch.bfloat16, device="cuda")
    buf[:m, :n] = float("nan")
    return buf


class Outs:
    """The three outputs of one call: C in [M + 1][ldc]; g_out and u_out in [M + 1][N + pad] each, or -- fused -- side by side in one
    [M + 1][2 N + pad] buffer, u_out = g_out + N.  pad = 8; pad = 4 gives an ldz the kernels do not take (the reference form)."""

    def __init__(self, case, layout, pad=8):
        m, n = case.m, case.n
        self.m, self.n, self.layout = m, n, layout
        self.c = case.c_buffer()
        if layout == "fused":
            self.ldz = 2 * n + pad
            self.gu = sentinel_buffer(m + 1, self.ldz, m, 2 * n)
            self.bufs = [self.gu]
            self.g_ptr, self.u_ptr = self.gu.data_ptr(), self.gu.data_ptr() + 2 * n
            self.g_view, self.u_view = self.gu[:m, :n], self.gu[:m, n:2 * n]
        else:
            self.ldz = n + pad
            self.gb, self.ub = sentinel_buffer(m + 1, self.ldz, m, n), sentinel_buffer(m + 1, self.ldz, m, n)
            self.bufs = [self.gb, self.ub]
            self.g_ptr, self.u_ptr = self.gb.data_ptr(), self.ub.data_ptr()
            self.g_view, self.u_view = self.gb[:m, :n], self.ub[:m, :n]

    def all_bits(self):
        return [ibits(self.c).clone()] + [ibits(b).clone() for b in self.bufs]

    def pads_intact(self):
        sent = ibits(torch.full((1,), SENTINEL, dtype=torch.bfloat16, device="cuda"))
        width = 2 * self.n if self.layout == "fused" else self.n
        ok = bool((ibits(self.c[:self.m, self.n:]) == sent).all()) and bool((ibits(self.c[self.m]) == sent).all())
        for b in self.bufs:
            ok = ok and bool((ibits(b[:self.m, width:]) == sent).all()) and bool((ibits(b[self.m]) == sent).all())
        return ok


def launch(g, L, case, outs, plan, act, bg="own", bu="own", stream=None):
    m, n, k = case.m, case.n, case.k
    bg = case.bg_d.data_ptr() if bg == "own" else bg
    bu = case.bu_d.data_ptr() if bu == "own" else bu
    return L.bgemm_mi355x_launch_tn_gated_aux(plan[0], plan[1], case.ad.data_ptr(), case.wg_d.data_ptr(), case.wu_d.data_ptr(), bg, bu, outs.c.data_ptr(),
                                              outs.g_ptr, outs.u_ptr, m, n, k, *case.ld, outs.ldz, act, g.stream() if stream is None else stream)


def check(case, outs, act, what):
    torch.cuda.synchronize()
    m, n = case.m, case.n
    bad = count_wrong(outs.c[:m, :n].cpu(), act, case.g32, case.u32)
    assert bad == 0, f"{what}: {bad} of {m * n} elements of C wrong"
    for name, view, want in (("g_out", outs.g_view, case.g16), ("u_out", outs.u_view, case.u16)):
        bad = int((ibits(view.cpu()) != ibits(want)).sum())
        assert bad == 0, f"{what}: {bad} of {m * n} elements of {name} differ from bf16(fp32 value)"
    assert outs.pads_intact(), f"{what}: a pad or a guard row changed"


def run(g, L, case, plan, act, layout, what, pad=8, **kw):
    outs = Outs(case, layout, pad)
    st = launch(g, L, case, outs, plan, act, **kw)
    assert st == 0, (what, st)
    check(case, outs, act, what)
    return outs


@pytest.fixture(scope="module")
def cases():
    """The sweep's operands and expectations, built once per (shape, padded) and shared; nothing writes to them."""
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            c = GatedCase(*shape, seed_of(shape), padded)
            c.g16, c.u16 = to_bf16(c.g32), to_bf16(c.u32)
            built[(shape, padded)] = c
        return built[(shape, padded)]

    return get


# ---- CPU proof, from reference data alone -------------------------------------------------------------------------------------------------
def trunc_bf16(x32):
    return (x32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


@pytest.fixture(scope="module")
def evidence(cases):
    rows = {}
    for shape in SHAPES:
        m, n, k = shape
        if m * n < 4096:
            continue
        case = cases(shape)
        g32, u32, g16, u16 = case.g32, case.u32, case.g16, case.u16
        differ = lambda a, b: int((ibits(a) != ibits(b)).sum())       # noqa: E731
        row = {"bf16(g) != g": int((g16.float() != g32).sum()), "bf16(u) != u": int((u16.float() != u32).sum())}
        sg = torch.from_numpy(case.prod32_np[:, :n].copy()).float()
        row["g_out and u_out swapped"] = differ(u16, g16)
        row["g_out without its bias"] = differ(to_bf16(sg), g16)
        row["g_out truncated"] = differ(trunc_bf16(g32), g16)
        cuts = [0] + two_pass_cuts(k, 2) + [k]
        assert len(cuts) == 3
        part = (case.a[:, :cuts[1]].astype(np.int64) @ case.b[:cuts[1], :n].astype(np.int64)).astype(np.float64) * a_scale(k)
        slab = torch.from_numpy(part).float() + case.bg.float()[None, :]
        row["g_out from one slab of a split"] = differ(to_bf16(slab), g16)
        for act in ACTS:
            row[f"{ACT_NAME[act]}: C from the rounded g"] = count_wrong(to_bf16(gact32(g16.float(), act) * u32), act, g32, u32)
            row[f"{ACT_NAME[act]}: C from the rounded u"] = count_wrong(to_bf16(gact32(g32, act) * u16.float()), act, g32, u32)
        for what, count in row.items():
            assert count >= MISTAKE_FLOOR, (shape, what, row)
        rows[shape] = row
    return rows


def test_the_rounding_is_live_and_the_checks_tell_the_mistakes_apart(evidence):
    for shape, row in evidence.items():
        print(shape, row)
    assert len(evidence) == 3


# ---- every member x form x activation, both layouts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_form_and_activation_writes_the_three_outputs(g, L, members, cases, evidence, shape, layout):
    """plain, NT, splits 2, splits 5 through the kernels; the reference kernel through an ldz the kernels do not take (pad 4)."""
    m, n, k = shape
    case = cases(shape, True)
    assert case.ld[2] == n + 8
    ran = 0
    for name, cid in members:
        for act in ACTS:
            plain = None
            for word in FORMS:
                cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
                ldz = (2 * n if layout == "fused" else n) + 8
                assert L.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, *case.ld, ldz) == 1
                st, form, disp = decision(L, cid, word, act, m, n, k, case.ld, ldz)
                assert (st, form, disp[0][3]) == (0, FORM_SPLITK if cuts else FORM_PLAIN, len(cuts) + 1), (name, hex(word))
                assert [d[2] for d in disp] == ([EPI_SLAB, EPI_C16_GATED_AUX + act] if cuts else [EPI_C16_GATED_AUX + act])
                outs = run(g, L, case, (cid, word), act, layout, f"{layout} {ACT_NAME[act]} {name} {hex(word)} {m}x{n}x{k}")
                if word == 1:
                    plain = outs.all_bits()
                if word == 1 | NT_STORE:
                    assert all(torch.equal(a, b) for a, b in zip(outs.all_bits(), plain)), (name, ACT_NAME[act], "the non-temporal result differs from the plain one")
                ran += 1
            ldz = (2 * n if layout == "fused" else n) + 4
            assert L.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, *case.ld, ldz) == 0
            assert decision(L, cid, 1, act, m, n, k, case.ld, ldz)[:2] == (0, FORM_REFERENCE)
            run(g, L, case, (cid, 1), act, layout, f"reference {layout} {ACT_NAME[act]} {name}", pad=4)
            ran += 1
    assert ran == 4 * (len(FORMS) + 1) * len(ACTS) and case.operands_intact()


# ---- the identities, on operands that are not exact -------------------------------------------------------------------------------------------
class Normal:
    """N(0, 1) bf16 operands on the device: X [M][K], Wg and Wu [N][K], two bias vectors"""

    def __init__(self, m, n, k, seed):
        gen = torch.Generator().manual_seed(seed)
        self.m, self.n, self.k = m, n, k
        mk = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16).cuda()   # noqa: E731
        self.a, self.wg, self.wu, self.bg, self.bu = mk(m, k), mk(n, k), mk(n, k), mk(n), mk(n)
        self.zero = torch.zeros(n, dtype=torch.bfloat16, device="cuda")

    def aux(self, g, L, cid, word, act, bg, bu):
        m, n, k = self.m, self.n, self.k
        c, gu = (torch.full((m, w), float("nan"), dtype=torch.bfloat16, device="cuda") for w in (n, 2 * n))
        st = L.bgemm_mi355x_launch_tn_gated_aux(cid, word, self.a.data_ptr(), self.wg.data_ptr(), self.wu.data_ptr(), bg, bu, c.data_ptr(), gu.data_ptr(),
                                                gu.data_ptr() + 2 * n, m, n, k, k, k, n, 2 * n, act, g.stream())
        assert st == 0
        return c, gu[:, :n], gu[:, n:]

    def gated(self, g, L, cid, word, act, bg, bu):
        m, n, k = self.m, self.n, self.k
        c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_launch_tn_gated(cid, word, self.a.data_ptr(), self.wg.data_ptr(), self.wu.data_ptr(), bg, bu, c.data_ptr(), m, n, k, k, k, n, act,
                                              g.stream()) == 0
        return c

    def bias(self, g, L, cid, word, w, b):
        m, n, k = self.m, self.n, self.k
        c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_launch_tn_bias(cid, word, self.a.data_ptr(), w.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
        return c


def plain_decision(L, hook, cid, word, m, n, k):
    out = (ctypes.c_longlong * 20)()
    assert getattr(L, hook)(cid, word, 4, m, n, k, k, k, n, 0, out) == 0
    return out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


@pytest.mark.parametrize("shape", [(136, 72, 128), (264, 264, 512)], ids=lambda s: "x".join(map(str, s)))
def test_the_three_identities_bit_for_bit_on_normal_operands(g, L, members, shape):
    """C is the gated call's C; g_out is the C of bgemm_mi355x_launch_tn_bias on (wg, bias_g) at (M, N, K) and u_out that on (wu, bias_u):
    plain and NT on every member, and the split forms, whose K cuts the hook shows to coincide (they depend on K and the splits word
    alone).  A NULL bias is compared against the zero-filled vector, in all three outputs."""
    m, n, k = shape
    ops = Normal(m, n, k, seed_of(shape))
    null = ctypes.c_void_p(0)
    split_ran = 0
    for name, cid in members:
        for word in FORMS:
            _, aux_d = decision(L, cid, word, SILU, m, n, k, (k, k, n), 2 * n)[1:]
            form_b, bias_d = plain_decision(L, "bgemm_mi355x_selfcheck_launch_tn_bias", cid, word, m, n, k)
            assert (aux_d[0][3], aux_d[0][4]) == (bias_d[0][3], bias_d[0][4]), (name, hex(word), "the K cuts of the two calls differ")
            split_ran += aux_d[0][3] > 1
            for act in (ACTS if word == 1 else (RELU, SILU)):
                c, go, uo = ops.aux(g, L, cid, word, act, ops.bg.data_ptr(), ops.bu.data_ptr())
                want_c = ops.gated(g, L, cid, word, act, ops.bg.data_ptr(), ops.bu.data_ptr())
                want_g, want_u = ops.bias(g, L, cid, word, ops.wg, ops.bg), ops.bias(g, L, cid, word, ops.wu, ops.bu)
                torch.cuda.synchronize()
                assert not bool(torch.isnan(c).any())
                assert torch.equal(ibits(c), ibits(want_c)), (name, hex(word), ACT_NAME[act], "C differs from the gated call's")
                assert torch.equal(ibits(go), ibits(want_g)), (name, hex(word), ACT_NAME[act], "g_out differs from the tn_bias call's C")
                assert torch.equal(ibits(uo), ibits(want_u)), (name, hex(word), ACT_NAME[act], "u_out differs from the tn_bias call's C")
        for word in (1, 2):
            for which in ("g", "u", "both"):
                got = []
                for absent in (null, ops.zero.data_ptr()):
                    bg = absent if which in ("g", "both") else ops.bg.data_ptr()
                    bu = absent if which in ("u", "both") else ops.bu.data_ptr()
                    got.append(ops.aux(g, L, cid, word, SILU, bg, bu))
                torch.cuda.synchronize()
                want_g = ops.bias(g, L, cid, word, ops.wg, ops.zero if which in ("g", "both") else ops.bg)
                torch.cuda.synchronize()
                for x, y in zip(*got):
                    assert torch.equal(ibits(x), ibits(y)) and not bool(torch.isnan(x).any()), (name, word, which, "a NULL bias is not a vector of zeros")
                assert torch.equal(ibits(got[0][1]), ibits(want_g))
    assert split_ran == 8


def test_a_null_bias_in_the_reference_kernel_equals_a_vector_of_zeros(g, L, cases):
    case = cases((136, 72, 128), True)
    zbuf, zero = guarded(torch.zeros(72, dtype=torch.bfloat16))
    null = ctypes.c_void_p(0)
    for which in ("g", "u", "both"):
        got = []
        for absent in (null, zero.data_ptr()):
            outs = Outs(case, "fused", pad=4)
            assert launch(g, L, case, outs, (0, 1), SILU, bg=absent if which in ("g", "both") else "own", bu=absent if which in ("u", "both") else "own") == 0
            torch.cuda.synchronize()
            assert not bool(torch.isnan(outs.gu[:case.m, :2 * case.n]).any()) and not bool(torch.isnan(outs.c[:case.m, :case.n]).any())
            got.append(outs.all_bits())
        assert all(torch.equal(a, b) for a, b in zip(*got)), which


# ---- refusals, the reference form, capture --------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_all_outputs_untouched(g, L, cases):
    case = cases((64, 32, 64), True)
    m, n, k = 64, 32, 64
    outs = Outs(case, "separate")
    before = outs.all_bits()
    a, wg, wu, c, go, uo = case.ad.data_ptr(), case.wg_d.data_ptr(), case.wu_d.data_ptr(), outs.c.data_ptr(), outs.g_ptr, outs.u_ptr
    ld, ldz, s = case.ld, outs.ldz, g.stream()
    call = L.bgemm_mi355x_launch_tn_gated_aux
    refused = [call(0, 1, a, wg, wu, None, None, c, None, uo, m, n, k, *ld, ldz, SILU, s), call(0, 1, a, wg, wu, None, None, c, go, None, m, n, k, *ld, ldz, SILU, s),
               call(0, 1, a, wg, wu, None, None, c, go, go, m, n, k, *ld, ldz, SILU, s), call(0, 1, a, wg, wu, None, None, c, c, uo, m, n, k, *ld, ldz, SILU, s),
               call(0, 1, a, wg, wu, None, None, c, go, c, m, n, k, *ld, ldz, SILU, s), call(0, 1, a, wg, wu, None, None, c, go, uo, m, n, k, *ld, n - 8, SILU, s),
               call(0, 1, a, wg, wu, None, None, c, go, uo, m, n, k, ld[0], ld[1], n - 8, ldz, SILU, s), call(0, 1, a, None, wu, None, None, c, go, uo, m, n, k, *ld, ldz, SILU, s),
               call(0, 1, a, wg, None, None, None, c, go, uo, m, n, k, *ld, ldz, SILU, s), call(4, 1, a, wg, wu, None, None, c, go, uo, m, n, k, *ld, ldz, SILU, s),
               call(0, 1, a, wg, wu, None, None, c, go, uo, m, n, k, *ld, ldz, 0, s), call(0, 1, a, wg, wu, None, None, c, go, uo, m, n, k, *ld, ldz, 5, s),
               L.bgemm_mi355x_tn_gated_aux(a, wg, wu, None, None, c, go, go, m, n, k, SILU, s), L.bgemm_mi355x_tn_gated_aux(a, wg, wu, None, None, c, go, uo, m, n, k, 7, s)]
    assert refused == [-1] * len(refused), refused
    assert L.bgemm_mi355x_tn_gated_aux_runs(0, m, n, k, *ld, n - 8) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs.all_bits(), before)), "a refused call wrote to an output"


def test_a_misaligned_g_out_is_answered_by_the_reference_kernel(g, L, cases):
    shape = (136, 72, 128)
    case = cases(shape, True)
    m, n, k = shape
    for act in ACTS:
        assert decision(L, 3, 1, act, m, n, k, case.ld, n + 8, aligned=False)[:2] == (0, FORM_REFERENCE)
        outs = Outs(case, "separate")
        flat = torch.full(((m + 1) * (n + 8) + 16,), SENTINEL, dtype=torch.bfloat16, device="cuda")
        outs.gb = flat[4:4 + (m + 1) * (n + 8)].view(m + 1, n + 8)
        outs.gb[:m, :n] = float("nan")
        outs.bufs[0], outs.g_ptr, outs.g_view = outs.gb, outs.gb.data_ptr(), outs.gb[:m, :n]
        assert outs.g_ptr % 16 == 8
        for word in (1, 4):
            assert launch(g, L, case, outs, (3, word), act) == 0
            check(case, outs, act, f"g_out 8 bytes off {ACT_NAME[act]} {word}")
        assert bool((flat[:4] == SENTINEL).all()) and bool((flat[4 + (m + 1) * (n + 8):] == SENTINEL).all()), "the backing tensor changed"
    assert case.operands_intact()


def test_the_planned_call_and_a_captured_split_call_without_a_workspace(g, L):
    """256 x 136 x 512 plans eight splits of the 64 x 64 member (bgemm_mi355x_tn_plan(M, 2 N, K)).  The planned call equals the explicit
    one; captured on a fresh stream with nothing reserved the split call returns 0 and replays unsplit, after the reserve call through its
    slabs and the combine: the same bits (g and u are exact in any order)."""
    m, n, k = 256, 136, 512
    case = GatedCase(m, n, k, 61)
    case.g16, case.u16 = to_bf16(case.g32), to_bf16(case.u32)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.bgemm_mi355x_tn_plan(m, 2 * n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and (cfg.value, splits.value) == (0, 8)
    with contextlib.ExitStack() as streams:
        for act in (RELU, SILU):
            assert decision(L, 0, 8, act, m, n, k, case.ld, 2 * n)[1] == FORM_SPLITK
            eager = run(g, L, case, (0, 8), act, "fused", f"eager {ACT_NAME[act]}", pad=0)
            sep = Outs(case, "separate", pad=0)
            assert L.bgemm_mi355x_tn_gated_aux(case.ad.data_ptr(), case.wg_d.data_ptr(), case.wu_d.data_ptr(), case.bg_d.data_ptr(), case.bu_d.data_ptr(),
                                               sep.c.data_ptr(), sep.g_ptr, sep.u_ptr, m, n, k, act, g.stream()) == 0
            check(case, sep, act, f"planned {ACT_NAME[act]}")
            assert torch.equal(ibits(sep.c), ibits(eager.c)) and torch.equal(ibits(sep.g_view), ibits(eager.g_view)) and torch.equal(ibits(sep.u_view), ibits(eager.u_view))
            for reserve in (False, True):
                outs = Outs(case, "fused", pad=0)
                s = streams.enter_context(fresh_stream())
                if reserve:
                    assert L.bgemm_mi355x_tn_reserve_workspace(m, 2 * n, k, s.cuda_stream) == 0
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.stream(s):
                    graph.capture_begin()
                    try:
                        rc = launch(g, L, case, outs, (0, 8), act, stream=s.cuda_stream)
                    finally:
                        graph.capture_end()
                    assert rc == 0, reserve
                    outs.c[:m, :n] = float("nan")
                    outs.gu[:m, :2 * n] = float("nan")
                    torch.cuda.synchronize()
                    graph.replay()
                torch.cuda.synchronize()
                del graph
                check(case, outs, act, f"replay {ACT_NAME[act]}, reserved={reserve}")
                assert all(torch.equal(x, y) for x, y in zip(outs.all_bits(), eager.all_bits()))
    assert case.operands_intact()


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(136, 72, 128), (264, 264, 512)], ids=lambda s: "x".join(map(str, s)))
def test_the_fused_buffer_is_handed_to_the_input_gradient_as_it_is(g, L, members, cases, shape):
    """bgemm_mi355x_launch_tn_gated_aux writes g|u into one [M][2 N + 8] buffer; bgemm_mi355x_launch_nn_dgated reads it in place (u = g + N,
    its ldz = this call's) with dY [M][64] and Wd [64][N] of tests/test_gpu_nn_dgated.py, whose own check judges dG and dU against
    bf16(g32) and bf16(u32): no copy, no re-layout."""
    m, n, k = shape
    case = cases(shape, True)
    ops = Ops(m, n, 64, seed=sum(shape))
    ops.g, ops.u = case.g16, case.u16
    dy, wd = ops.a.cuda(), ops.b.cuda()
    for (name, cid), word in zip(members, FORMS):
        for act in ACTS:
            outs = run(g, L, case, (cid, word), act, "fused", f"chain forward {ACT_NAME[act]} {name} {hex(word)}")
            dgu = torch.full((m, 2 * n), float("nan"), dtype=torch.bfloat16, device="cuda")
            st = L.bgemm_mi355x_launch_nn_dgated(cid, 1, dy.data_ptr(), wd.data_ptr(), outs.g_ptr, outs.u_ptr, dgu.data_ptr(), dgu.data_ptr() + 2 * n, m, n, 64, 64, n,
                                                 outs.ldz, 2 * n, act, g.stream())
            torch.cuda.synchronize()
            assert st == 0
            dgated_check(ops, act, dgu[:, :n].cpu(), dgu[:, n:].cpu(), f"chain backward {ACT_NAME[act]} {name}")
            check(case, outs, act, "the saved buffer after the backward call")
