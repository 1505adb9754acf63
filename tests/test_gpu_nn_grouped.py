"""GPU tests of the grouped input gradient, bgemm_mi355x_nn_grouped (hgemm_inst_g25.hip), and of its reference kernel, by tests/test_gpu_tn_grouped.py's
method: integer operands with sums exact in fp32 in any order, so (A_g.float() @ W_g.float() [+ r.float()]).bfloat16() by torch on the CPU per group is
the result bit for bit.  C starts as NaN in the owned rows (in place: as r) and as a sentinel elsewhere; the sentinel and every input must come back
unchanged.  The weight buffer's gaps and pads and the rows of A and r that no group owns are NaN: none may reach a stored value."""
import ctypes

import numpy as np
import pytest
import torch

import residual_common as rc
from residual_common import FORM_PLAIN, FORM_REFERENCE, NT, bits
from test_gpu_nn import MEMBERS, g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_tn_grouped import BOUNDARIES, CAP

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def L(g):
    lib = rc.prototypes(g.lib())
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.bgemm_mi355x_launch_nn_grouped.argtypes = [i] * 2 + [p] * 5 + [i] * 6 + [ll] + [i] * 2 + [p]
    lib.bgemm_mi355x_nn_grouped.argtypes = [p] * 5 + [i] * 4 + [p]
    lib.bgemm_mi355x_nn_grouped_runs.argtypes = [i] * 7 + [ll] + [i] * 2
    lib.bgemm_mi355x_selfcheck_launch_nn_grouped.argtypes = [i] * 9 + [ll] + [i] * 2 + [p]
    lib.bgemm_mi355x_launch_nn.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    return lib


class Ops:   # A [M][K], G matrices [K][N] and r [M][N] on the CPU; want(off, r): the expectation, NaN in the rows no group owns
    def __init__(self, m, n, k, groups, data="int", seed=rc.SEED):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k, self.G = m, n, k, groups
        draw = (lambda s, scale: rng.integers(-15, 16, size=s) * scale) if data == "int" else (lambda s, scale: rng.standard_normal(s))
        self.a, self.w = torch.from_numpy(draw((m, k), 2.0 ** -9)).bfloat16(), torch.from_numpy(draw((groups, k, n), 1.0)).bfloat16()
        self.r = torch.from_numpy(4.0 * rng.standard_normal((m, n))).bfloat16()

    def want(self, off, r):
        c = torch.full((self.m, self.n), NAN, dtype=torch.bfloat16)
        for i, (s, e) in enumerate(zip(off[:-1], off[1:])):
            sums = self.a[s:e].float() @ self.w[i].float()                                # exact sums: any order
            c[s:e] = (sums + self.r[s:e].float() if r != "none" else sums).bfloat16()
        return c


def run(L, ops, off, cfg, word=1, lds=None, r="none", form=FORM_PLAIN, planned=False, stream=0, what=""):
    """One call; lds = (lda, ldb, group_stride_b, ldr, ldc); r: "none" / "separate" / "inplace".  -> C's owned rows (cpu); checks form, status, sentinel, inputs"""
    m, n, k, G = ops.m, ops.n, ops.k, ops.G
    lda, ldb, gsb, ldr, ldc = lds or (k, n, k * n, n, n)
    s, e = off[0], off[-1]
    out20 = (ctypes.c_longlong * 20)()
    st = L.bgemm_mi355x_selfcheck_launch_nn_grouped(cfg, word, 4 | (8 if r != "none" else 0) | (16 if r == "inplace" else 0), G, m, n, k, lda, ldb, gsb, ldr, ldc, out20)
    assert planned or (st, out20[0]) == (0, form), (what, st, out20[0])
    wflat = torch.full((G * gsb + 8,), NAN, dtype=torch.bfloat16, device="cuda")
    for i in range(G):
        wflat[i * gsb:i * gsb + k * ldb].view(k, ldb)[:, :n] = ops.w[i].cuda()
    a_in, r_in = ops.a.clone(), ops.r.clone()
    a_in[:s], a_in[e:], r_in[:s], r_in[e:] = NAN, NAN, NAN, NAN
    keep = [rc.place(a_in, lda), (wflat, None), (torch.tensor(off, dtype=torch.int32, device="cuda"), None)]
    cflat, c = rc.place(torch.zeros(m, n, dtype=torch.bfloat16), ldc, fill=rc.OUT_FILL)
    c[:, :n] = rc.OUT_FILL
    c[s:e, :n] = r_in[s:e].cuda() if r == "inplace" else NAN
    if r == "separate":
        keep.append(rc.place(r_in, ldr))
    pr = cflat.data_ptr() if r == "inplace" else keep[-1][0].data_ptr() if r == "separate" else None
    before, inputs = cflat.clone(), [t.clone() for t, _ in keep]
    pa, pw, po = (t.data_ptr() for t, _ in keep[:3])
    st = (L.bgemm_mi355x_nn_grouped(pa, pw, pr, cflat.data_ptr(), po, G, m, n, k, stream) if planned else
          L.bgemm_mi355x_launch_nn_grouped(cfg, word, pa, pw, pr, cflat.data_ptr(), po, G, m, n, k, lda, ldb, gsb, ldr, ldc, stream))
    torch.cuda.synchronize()
    assert st == 0, (what, st)
    got = c[s:e, :n].cpu().clone()
    c[s:e, :n] = 0
    before[:m * ldc].view(m, ldc)[s:e, :n] = 0
    assert torch.equal(bits(cflat), bits(before)), f"{what}: C was written outside the groups' rows"
    assert all(torch.equal(t.view(torch.uint8), w.view(torch.uint8)) for (t, _), w in zip(keep, inputs)), f"{what}: an input changed"
    return got


def check(L, ops, off, cfg, what, **kw):
    got, expect = run(L, ops, off, cfg, what=what, **kw), ops.want(off, kw.get("r", "none"))[off[0]:off[-1]]
    assert torch.equal(bits(got), bits(expect)), f"{what}: {rc.differing(got, expect)} elements differ"


@pytest.fixture(scope="module")
def boundary_ops():
    return {k: Ops(300, 72, k, 7) for k in (72, 128, 320)}


@pytest.mark.parametrize("r", ["none", "separate", "inplace"])
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("k", [128, 320])
@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_group_boundaries_inside_fragments_and_tiles(g, L, boundary_ops, cfg, k, padded, r):
    lds = (k + 8, 72 + 16, k * (72 + 16) + 24, 72 + (24 if r == "inplace" else 8), 72 + 24) if padded else None
    for word in (1, 1 | NT):
        check(L, boundary_ops[k], BOUNDARIES, cfg, f"{MEMBERS[cfg]} K={k} r={r} {hex(word)}", word=word, lds=lds, r=r, stream=g.stream())


@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_the_cap_of_groups_and_all_groups_empty(g, L, cfg):
    # the forward test's routing: G = the cap, mostly single-row groups, a few empty ones, one of 45 rows; then five empty groups: C untouched
    sizes = [45 if i == 200 else 0 if i in (0, 63, 64, 130, 255) else 1 for i in range(CAP)]
    check(L, Ops(CAP + 44, 8, 64, CAP), [2] + [int(x) for x in 2 + np.cumsum(sizes)], cfg, "the cap", r="separate", stream=g.stream())
    assert run(L, Ops(100, 72, 128, 5), [37] * 6, cfg, r="separate", stream=g.stream(), what="all empty").numel() == 0


@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_one_group_is_the_dense_call_bit_for_bit(g, L, cfg):
    m, n, k = 136, 72, 320
    ops = Ops(m, n, k, 1, data="normal")
    a, w, r = ops.a.cuda(), ops.w[0].cuda(), ops.r.cuda()
    c = torch.full((m, n), NAN, dtype=torch.bfloat16, device="cuda")
    for mode in ("none", "separate"):
        assert (L.bgemm_mi355x_launch_nn(cfg, 1, a.data_ptr(), w.data_ptr(), c.data_ptr(), m, n, k, k, n, n, g.stream()) if mode == "none" else
                L.bgemm_mi355x_launch_nn_add(cfg, 1, a.data_ptr(), w.data_ptr(), r.data_ptr(), c.data_ptr(), m, n, k, k, n, n, n, g.stream())) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(run(L, ops, [0, m], cfg, r=mode, stream=g.stream(), what="G = 1")), bits(c.cpu())), mode


@pytest.mark.parametrize("r", ["none", "separate"])
@pytest.mark.parametrize("why", ["K = 72", "ldc % 8 == 4", "G = cap + 1"])
def test_the_reference_form_gives_the_cpu_bits(g, L, boundary_ops, why, r):
    k = 72 if why == "K = 72" else 128
    ops, off = (Ops(CAP + 1, 8, 64, CAP + 1), list(range(CAP + 2))) if why == "G = cap + 1" else (boundary_ops[k], BOUNDARIES)
    lds = (k, 72, k * 72, 72, 76) if why == "ldc % 8 == 4" else None
    for cfg in (0, 3):
        check(L, ops, off, cfg, why, lds=lds, r=r, form=FORM_REFERENCE, stream=g.stream())


def test_the_planned_call_and_one_capture_under_two_routings(g, L, boundary_ops):
    check(L, boundary_ops[320], BOUNDARIES, 0, "planned", r="inplace", planned=True, stream=g.stream())
    ops, m, n, k = boundary_ops[128], 300, 72, 128
    a, w, r = ops.a.cuda(), ops.w.cuda(), ops.r.cuda()
    off = torch.tensor(BOUNDARIES, dtype=torch.int32, device="cuda")
    c = torch.full((m, n), rc.OUT_FILL, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        ret = L.bgemm_mi355x_launch_nn_grouped(1, 1, a.data_ptr(), w.data_ptr(), r.data_ptr(), c.data_ptr(), off.data_ptr(), 7, m, n, k, k, n, k * n, n, n,
                                               torch.cuda.current_stream().cuda_stream)
    assert ret == 0
    for routing in (BOUNDARIES, [0, 50, 50, 131, 200, 264, 299, 300]):
        off.copy_(torch.tensor(routing, dtype=torch.int32))
        c.fill_(rc.OUT_FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        expect = ops.want(routing, "separate")
        expect[:routing[0]], expect[routing[-1]:] = rc.OUT_FILL, rc.OUT_FILL
        assert torch.equal(bits(c.cpu()), bits(expect)), routing


def test_the_refusals(L):
    m, n, k, G = 300, 72, 128, 7
    a, b, r, c, off = (ctypes.c_void_p(4096 * (i + 1)) for i in range(5))
    good = dict(cfg=0, word=1, ptrs=(a, b, r, c, off), G=G, dims=(m, n, k), lds=(k, n, k * n, n, n))
    launch = lambda **kw: (lambda q: L.bgemm_mi355x_launch_nn_grouped(q["cfg"], q["word"], *q["ptrs"], q["G"], *q["dims"], *q["lds"], None))({**good, **kw})  # noqa: E731
    for i in (0, 1, 3, 4):
        assert launch(ptrs=tuple(None if j == i else p for j, p in enumerate(good["ptrs"]))) == -1, i
    for kw in (dict(G=0), dict(dims=(0, n, k)), dict(dims=(m, 0, k)), dict(dims=(m, n, 0)), dict(cfg=4), dict(cfg=-1), dict(word=2), dict(word=2 | NT),
               dict(ptrs=(a, b, c, c, off), lds=(k, n, k * n, n + 8, n)),                         # in place with ldr != ldc; then each stride 8 short
               *[dict(lds=tuple(v - 8 * (j == i) for j, v in enumerate(good["lds"]))) for i in range(5)]):
        assert launch(**kw) == -1, kw
    runs = lambda G=G, gsb=k * n, ldr=n: L.bgemm_mi355x_nn_grouped_runs(0, G, m, n, k, k, n, gsb, ldr, n)  # noqa: E731
    assert runs() == 1 and runs(gsb=k * n + 4) == 0 and runs(ldr=0) == 1 and runs(ldr=n + 4) == 0 and runs(G=CAP) == 1 and runs(G=CAP + 1) == 0
