"""GPU tests of the grouped gated forward, bgemm_mi355x_tn_grouped_gated (hgemm_inst_g26.hip / g27.hip) and of its reference kernel.
tests/test_gpu_tn_grouped.py's method and exact-sum operands: gv = S_g + bias_g.float() and uv are known exactly, so g_out = gv.bfloat16(), u_out and the
ReLU C = (relu(gv) uv).bfloat16() are the result BIT FOR BIT (torch on the CPU, fp32); for SiLU EVERY element is held to the dense gated call's derived bar
(hgemm_gated.hpp) against fp64 on those gv and uv; all values are finite (|S| < 141).  Outputs start as NaN in owned rows and as a sentinel elsewhere; the
sentinel and every input must come back unchanged; the weight buffer holds NaN wherever no weight lies, so a read past a clamp shows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import residual_common as rc
from residual_common import FORM_PLAIN, FORM_REFERENCE, NT, bits
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_tn_grouped import BOUNDARIES, CAP, MEMBERS

pytestmark = pytest.mark.gpu
RELU, SILU = 1, 4


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.bgemm_mi355x_launch_tn_grouped_gated.argtypes = [i] * 2 + [p] * 9 + [i] * 6 + [ll] + [i] * 4 + [p]
    lib.bgemm_mi355x_tn_grouped_gated.argtypes = [p] * 9 + [i] * 5 + [p]
    lib.bgemm_mi355x_selfcheck_launch_tn_grouped_gated.argtypes = [i] * 9 + [ll] + [i] * 4 + [p]
    lib.bgemm_mi355x_launch_tn_grouped.argtypes = [i] * 2 + [p] * 5 + [i] * 6 + [ll] + [i] * 2 + [p]
    lib.bgemm_mi355x_launch_tn_gated.argtypes = [i] * 2 + [p] * 6 + [i] * 7 + [p]
    lib.bgemm_mi355x_launch_tn_gated_aux.argtypes = [i] * 2 + [p] * 8 + [i] * 8 + [p]
    return lib


class Ops:   # A [M][K], G gate and G up weights [N][K], G bias rows each, on the CPU; pre(off): the exact fp32 gv and uv, NaN in the rows no group owns
    def __init__(self, m, n, k, groups, seed=rc.SEED):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k, self.G, self.memo = m, n, k, groups, {}
        self.a = torch.from_numpy(rng.integers(-15, 16, size=(m, k)) * 2.0 ** -9).bfloat16()
        self.w = [torch.from_numpy(rng.integers(-15, 16, size=(groups, n, k)).astype(np.float64)).bfloat16() for _ in range(2)]
        self.bias = [torch.from_numpy(rng.standard_normal((groups, n))).bfloat16() for _ in range(2)]

    def pre(self, off, bias=True):
        if (tuple(off), bias) not in self.memo:
            gu = self.memo[tuple(off), bias] = [torch.full((self.m, self.n), float("nan")) for _ in range(2)]
            for h, i in ((h, i) for h in range(2) for i in range(self.G)):
                s, e = off[i], off[i + 1]
                gu[h][s:e] = self.a[s:e].float() @ self.w[h][i].float().t() + (self.bias[h][i].float() if bias else torch.zeros(self.n))   # exact sums
        return self.memo[tuple(off), bias]


def run(L, ops, off, cfg, act, word=1, padded=False, fused=False, aux=True, bias="rows", form=FORM_PLAIN, planned=False, ldz=None, stream=0, what=""):
    """-> the owned rows of (C, g_out, u_out) (None without aux); checks the hook's form, the status, the sentinels, the inputs.  fused: wu = wg + N ldb"""
    m, n, k, G = ops.m, ops.n, ops.k, ops.G
    lda, ldb, ldbias, ldc = (k + 8, k + 16, n + 8, n + 24) if padded else (k, k, n, n)
    ldz = ldz or (n + 16 if padded else n)
    gsb = (2 if fused else 1) * n * ldb + (24 if padded else 0)
    out20 = (ctypes.c_longlong * 20)()
    st = L.bgemm_mi355x_selfcheck_launch_tn_grouped_gated(cfg, word, 4 | (8 if bias != "null" else 0) | (16 if aux else 0), G, m, n, k, lda, ldb, gsb, ldbias, ldc, ldz, act, out20)
    assert planned or (st, out20[0]) == (0, form), (what, st, out20[0])
    up0 = n * ldb if fused else G * gsb                       # where Wu_0 starts in the weight buffer
    wflat = torch.full((up0 + G * gsb + 8,), float("nan"), dtype=torch.bfloat16, device="cuda")
    for h, i in ((h, i) for h in range(2) for i in range(G)):
        wflat[h * up0 + i * gsb:h * up0 + i * gsb + n * ldb].view(n, ldb)[:, :k] = ops.w[h][i].cuda()
    rows = [b if bias == "rows" else torch.zeros_like(b) for b in ops.bias]
    keep = [rc.place(ops.a, lda)[0], wflat, rc.place(rows[0], ldbias)[0], rc.place(rows[1], ldbias)[0], torch.tensor(off, dtype=torch.int32, device="cuda")]
    x0 = torch.full((m, n), rc.OUT_FILL, dtype=torch.bfloat16)
    x0[off[0]:off[-1]] = float("nan")
    outs = [rc.place(x0, ld, fill=rc.OUT_FILL) + (ld,) for ld in (ldc, ldz, ldz)[:3 if aux else 1]]
    inputs, befores = [t.clone() for t in keep], [o[0].clone() for o in outs]
    pa, pw, pbg, pbu, po = (None if bias == "null" and j in (2, 3) else t.data_ptr() for j, t in enumerate(keep))
    pc, pg, pu = [o[0].data_ptr() for o in outs] + [None] * (3 - len(outs))
    st = (L.bgemm_mi355x_tn_grouped_gated(pa, pw, pw + 2 * up0, pbg, pbu, pc, pg, pu, po, G, m, n, k, act, stream) if planned else
          L.bgemm_mi355x_launch_tn_grouped_gated(cfg, word, pa, pw, pw + 2 * up0, pbg, pbu, pc, pg, pu, po, G, m, n, k, lda, ldb, gsb, ldbias, ldc, ldz, act, stream))
    torch.cuda.synchronize()
    assert st == 0, (what, st)
    got = []
    for (flat, v, ld), before in zip(outs, befores):
        got.append(v[off[0]:off[-1], :n].cpu().clone())
        v[off[0]:off[-1], :n] = 0
        before[:m * ld].view(m, ld)[off[0]:off[-1], :n] = 0
        assert torch.equal(bits(flat), bits(before)), f"{what}: output {len(got) - 1} was written outside the groups' rows"
    assert all(torch.equal(t.view(torch.uint8), w.view(torch.uint8)) for t, w in zip(keep, inputs)), f"{what}: an input changed"
    return got + [None] * (3 - len(got))


def check(L, ops, off, cfg, act, what, **kw):
    c, gq, uq = run(L, ops, off, cfg, act, what=what, **kw)
    gv, uv = (t[off[0]:off[-1]] for t in ops.pre(off, bias=kw.get("bias", "rows") == "rows"))
    if kw.get("aux", True):
        assert torch.equal(bits(gq), bits(gv.bfloat16())) and torch.equal(bits(uq), bits(uv.bfloat16())), f"{what}: g_out / u_out differ from bf16(gv), bf16(uv)"
    if act == RELU:
        expect = (torch.where(gv > 0, gv, torch.zeros_like(gv)) * uv).bfloat16()
        assert torch.equal(bits(c), bits(expect)), f"{what}: {rc.differing(c, expect)} elements of C differ"
    else:
        g64, u64, y64 = gv.double(), uv.double(), gv.double() * torch.sigmoid(gv.double()) * uv.double()
        bar = torch.where(y64 != 0, torch.exp2(torch.floor(torch.log2(y64.abs().clamp_min(1e-300))) - 8), torch.zeros_like(y64)) + 2.0 ** -19 * g64.abs() * u64.abs() + 2.0 ** -23 * y64.abs()
        excess = ((c.double() - y64).abs() - bar).nan_to_num(nan=float("inf"))
        assert bool((excess <= 0).all()), f"{what}: {int((excess > 0).sum())} elements of C outside the bar, the worst by {float(excess.max()):.3e}"


boundary_ops = functools.lru_cache(None)(lambda k: Ops(300, 72, k, 7))      # the boundaries case's operands, built once per K


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("k", [128, 320])
@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_group_boundaries_inside_fragments_and_tiles(g, L, cfg, k, padded):
    # ends inside a fragment and a 64- / 128-row tile; the sliver tile (N = 72) needs the per-weight clamp in both weight layouts; K = 320 wraps the ring
    for fused in (False, True):
        for word, act in ((1, RELU), (1 | NT, SILU), (1, SILU), (1 | NT, RELU)):
            check(L, boundary_ops(k), BOUNDARIES, cfg, act, f"{MEMBERS[cfg]} K={k} fused={fused} {hex(word)} act={act}", word=word, padded=padded, fused=fused, stream=g.stream())


@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_the_cap_of_groups_mostly_single_rows_and_all_groups_empty(g, L, cfg):
    sizes = [45 if i == 200 else 0 if i in (0, 63, 64, 130, 255) else 1 for i in range(CAP)]
    check(L, Ops(CAP + 44, 8, 64, CAP), [2] + [int(x) for x in 2 + np.cumsum(sizes)], cfg, RELU, "the cap", aux=False, stream=g.stream())
    assert all(t.numel() == 0 for t in run(L, Ops(100, 72, 128, 5), [37] * 6, cfg, SILU, stream=g.stream(), what="all empty"))      # nothing is written


@pytest.mark.parametrize("act", [1, 2, 3, 4], ids=["relu", "gelu", "gelu_tanh", "silu"])
def test_one_group_is_the_dense_gated_call_and_a_null_bias_is_zeros(g, L, act):
    (m, n, k), ops = (136, 72, 128), Ops(136, 72, 128, 1)
    dev = [t.cuda() for t in (ops.a, ops.w[0][0], ops.w[1][0], ops.bias[0][0], ops.bias[1][0])]
    ptrs = [t.data_ptr() for t in dev]
    for cfg in range(4):
        c, c3, gq, uq = (torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(4))
        assert L.bgemm_mi355x_launch_tn_gated(cfg, 1, *ptrs, c.data_ptr(), m, n, k, k, k, n, act, g.stream()) == 0
        assert L.bgemm_mi355x_launch_tn_gated_aux(cfg, 1, *ptrs, c3.data_ptr(), gq.data_ptr(), uq.data_ptr(), m, n, k, k, k, n, n, act, g.stream()) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(bits(x), bits(y.cpu())) for x, y in zip(run(L, ops, [0, m], cfg, act, stream=g.stream(), what="G = 1 aux"), (c3, gq, uq))), MEMBERS[cfg]
        assert torch.equal(bits(run(L, ops, [0, m], cfg, act, aux=False, stream=g.stream(), what="G = 1")[0]), bits(c.cpu())), MEMBERS[cfg]
        null, zeros = (run(L, ops, [0, m], cfg, act, bias=b, stream=g.stream(), what=b) for b in ("null", "zeros"))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(null, zeros)), MEMBERS[cfg]


def test_g_out_and_u_out_are_the_grouped_forward_calls_c_and_the_planned_entry_point(g, L):
    ops, (m, n, k) = boundary_ops(128), (300, 72, 128)
    a, off = ops.a.cuda(), torch.tensor(BOUNDARIES, dtype=torch.int32, device="cuda")
    for cfg, h in ((cfg, h) for cfg in range(4) for h in range(2)):
        w, bias, c = ops.w[h].cuda(), ops.bias[h].cuda(), torch.zeros(m, n, dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_launch_tn_grouped(cfg, 1, a.data_ptr(), w.data_ptr(), bias.data_ptr(), c.data_ptr(), off.data_ptr(), 7, m, n, k, k, k, n * k, n, n, g.stream()) == 0
        torch.cuda.synchronize()
        got = run(L, ops, BOUNDARIES, cfg, SILU, stream=g.stream(), what="aux")[1 + h]
        assert torch.equal(bits(got), bits(c[BOUNDARIES[0]:BOUNDARIES[-1]].cpu())), (MEMBERS[cfg], h)
    check(L, boundary_ops(320), BOUNDARIES, 0, SILU, "the planned entry point", planned=True, stream=g.stream())


@pytest.mark.parametrize("act", [RELU, SILU], ids=["relu", "silu"])
@pytest.mark.parametrize("why", ["K = 72", "ldz % 8 == 4", "G = cap + 1"])
def test_the_reference_form(g, L, why, act):
    big, ldz = why == "G = cap + 1", 76 if why == "ldz % 8 == 4" else None
    ops, off = (Ops(CAP + 1, 8, 64, CAP + 1), list(range(CAP + 2))) if big else (Ops(300, 72, 72 if why == "K = 72" else 128, 7), BOUNDARIES)
    for cfg in (0, 3):
        check(L, ops, off, cfg, act, why, ldz=ldz, form=FORM_REFERENCE, fused=cfg == 3, stream=g.stream())
        check(L, ops, off, cfg, act, why + " NULL bias, no aux", ldz=ldz, bias="null", aux=False, stream=g.stream(),
              form=FORM_PLAIN if ldz else FORM_REFERENCE)                      # (without aux ldz is not read: the member's kernel)


def test_one_capture_follows_the_offsets_of_each_replay(g, L):
    # captured once on a fresh stream with nothing reserved; the offsets buffer is overwritten between two replays; one stream, one chain
    ops, m, n, k = boundary_ops(128), 300, 72, 128
    ins = [t.cuda() for t in (ops.a, ops.w[0], ops.w[1], ops.bias[0], ops.bias[1])]
    off = torch.tensor(BOUNDARIES, dtype=torch.int32, device="cuda")
    outs = [torch.full((m, n), rc.OUT_FILL, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        assert L.bgemm_mi355x_launch_tn_grouped_gated(1, 1, *(t.data_ptr() for t in (*ins, *outs, off)), 7, m, n, k, k, k, n * k, n, n, n, RELU,
                                                      torch.cuda.current_stream().cuda_stream) == 0
    for routing in (BOUNDARIES, [0, 50, 50, 131, 200, 264, 299, 300]):
        off.copy_(torch.tensor(routing, dtype=torch.int32))
        [t.fill_(rc.OUT_FILL) for t in outs]
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        gv, uv = ops.pre(routing)
        for got, expect in zip(outs, ((torch.where(gv > 0, gv, torch.zeros_like(gv)) * uv).bfloat16(), gv.bfloat16(), uv.bfloat16())):
            expect[:routing[0]], expect[routing[-1]:] = rc.OUT_FILL, rc.OUT_FILL
            assert torch.equal(bits(got.cpu()), bits(expect)), routing


def test_the_refusals(L):
    # argument checks through the real entry point, fake aligned pointers (a, wg, wu, bias_g, bias_u, c, g_out, u_out, offsets), nothing launched
    (m, n, k), ptrs = (300, 72, 128), tuple(ctypes.c_void_p(4096 * (i + 1)) for i in range(9))
    good = dict(cfg=0, word=1, ptrs=ptrs, G=7, dims=(m, n, k), lds=(k, k, n * k, n, n, n), act=SILU)
    launch = lambda **kw: (lambda q: L.bgemm_mi355x_launch_tn_grouped_gated(q["cfg"], q["word"], *q["ptrs"], q["G"], *q["dims"], *q["lds"], q["act"], None))({**good, **kw})  # noqa: E731
    swap = lambda i, v: tuple(v if j == i else p for j, p in enumerate(ptrs))  # noqa: E731
    assert all(launch(ptrs=swap(i, None)) == -1 for i in (0, 1, 2, 5, 6, 7, 8))            # a NULL a, wg, wu, c, offsets; exactly one of g_out / u_out
    assert launch(ptrs=swap(7, ptrs[6])) == -1 and launch(ptrs=swap(6, ptrs[5])) == -1 and launch(ptrs=swap(7, ptrs[5])) == -1      # g_out == u_out, either == c
    assert launch(G=0) == -1 and launch(dims=(0, n, k)) == -1 and launch(dims=(m, 0, k)) == -1 and launch(dims=(m, n, 0)) == -1
    assert all(launch(lds=tuple(v - 8 * (j == i) for j, v in enumerate(good["lds"]))) == -1 for i in range(6))
    assert launch(cfg=4) == -1 and launch(cfg=-1) == -1 and launch(word=2) == -1 and launch(word=2 | NT) == -1 and launch(act=0) == -1 and launch(act=5) == -1
