"""GPU tests of the grouped forward product, bgemm_mi355x_tn_grouped (hgemm_inst_g23.hip, the tile map read from device offsets) and of its
reference kernel.  residual_common.py's method: A and W hold integers of [-15, 15], A scaled by 2^-9, so every sum is exact in fp32 in any
order and (S_g + bias_g.float()).bfloat16(), computed by torch on the CPU per group, is the result bit for bit.  C starts as NaN in the rows
the call owns and as a sentinel everywhere else; the sentinel and every input must come back unchanged.  Well-formed offsets only: malformed
ones are tests/test_grouped_map_host.py's."""
import ctypes

import numpy as np
import pytest
import torch

import residual_common as rc
from residual_common import FORM_PLAIN, FORM_REFERENCE, NT, bits
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)

pytestmark = pytest.mark.gpu

MEMBERS, CAP = ("f64x64_w2x2", "f128x64_w2x2", "f64x128_w2x2", "f128x128_w2x2"), 256      # CAP: HGEMM_GROUPED_MAX_GROUPS
BOUNDARIES = [3, 3, 4, 68, 68, 197, 290, 290]                    # M = 300: empty first / middle / last group, 1 row, 64 rows, dropped rows at both ends


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.bgemm_mi355x_launch_tn_grouped.argtypes = [i] * 2 + [p] * 5 + [i] * 6 + [ll] + [i] * 2 + [p]
    lib.bgemm_mi355x_tn_grouped.argtypes = [p] * 5 + [i] * 4 + [p]
    lib.bgemm_mi355x_tn_grouped_runs.argtypes = [i] * 7 + [ll] + [i] * 2
    lib.bgemm_mi355x_selfcheck_launch_tn_grouped.argtypes = [i] * 9 + [ll] + [i] * 2 + [p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    lib.bgemm_mi355x_tn_config_by_name.argtypes = [ctypes.c_char_p]
    assert [lib.bgemm_mi355x_tn_config_by_name(nm.encode()) for nm in MEMBERS] == [0, 1, 2, 3]
    return lib


class Ops:   # A [M][K], G weights [N][K] and G bias rows [N] on the CPU; want(off): the expectation, NaN in the rows no group owns
    def __init__(self, m, n, k, groups, seed=rc.SEED):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k, self.G = m, n, k, groups
        self.a = torch.from_numpy(rng.integers(-15, 16, size=(m, k)) * 2.0 ** -9).bfloat16()
        self.w = torch.from_numpy(rng.integers(-15, 16, size=(groups, n, k)).astype(np.float64)).bfloat16()
        self.bias = torch.from_numpy(rng.standard_normal((groups, n))).bfloat16()

    def want(self, off, bias=True):
        c = torch.full((self.m, self.n), float("nan"), dtype=torch.bfloat16)
        for i, (s, e) in enumerate(zip(off[:-1], off[1:])):
            b = self.bias[i].float() if bias else torch.zeros(self.n)
            c[s:e] = (self.a[s:e].float() @ self.w[i].float().t() + b).bfloat16()        # exact sums: any order
        return c


def run(L, ops, off, cfg, word=1, lds=None, bias="rows", form=FORM_PLAIN, planned=False, stream=0, what=""):
    """One call; lds = (lda, ldb, group_stride_b, ldbias, ldc).  -> the owned rows of C (cpu); checks the hook's form, the status, C's sentinel, the inputs"""
    m, n, k, G = ops.m, ops.n, ops.k, ops.G
    lda, ldb, gsb, ldbias, ldc = lds or (k, k, n * k, n, n)
    out20 = (ctypes.c_longlong * 20)()
    st = L.bgemm_mi355x_selfcheck_launch_tn_grouped(cfg, word, 4 | (8 if bias != "null" else 0), G, m, n, k, lda, ldb, gsb, ldbias, ldc, out20)
    assert planned or (st, out20[0]) == (0, form), (what, st, out20[0])
    wflat = torch.full((G * gsb + 8,), float("nan"), dtype=torch.bfloat16, device="cuda")
    for i in range(G):
        wflat[i * gsb:i * gsb + n * ldb].view(n, ldb)[:, :k] = ops.w[i].cuda()
    rows = ops.bias if bias == "rows" else torch.zeros(G, n, dtype=torch.bfloat16)
    keep = [rc.place(ops.a, lda), (wflat, None), rc.place(rows, ldbias), (torch.tensor(off, dtype=torch.int32, device="cuda"), None)]
    cflat, c = rc.place(torch.zeros(m, n, dtype=torch.bfloat16), ldc, fill=rc.OUT_FILL)
    c[:, :n] = rc.OUT_FILL
    c[off[0]:off[-1], :n] = float("nan")
    before, inputs = cflat.clone(), [t.clone() for t, _ in keep]
    pa, pw, pb, po = (t.data_ptr() for t, _ in keep)
    pb = None if bias == "null" else pb
    st = (L.bgemm_mi355x_tn_grouped(pa, pw, pb, cflat.data_ptr(), po, G, m, n, k, stream) if planned else
          L.bgemm_mi355x_launch_tn_grouped(cfg, word, pa, pw, pb, cflat.data_ptr(), po, G, m, n, k, lda, ldb, gsb, ldbias, ldc, stream))
    torch.cuda.synchronize()
    assert st == 0, (what, st)
    got = c[off[0]:off[-1], :n].cpu().clone()
    c[off[0]:off[-1], :n] = 0
    before[:m * ldc].view(m, ldc)[off[0]:off[-1], :n] = 0
    assert torch.equal(bits(cflat), bits(before)), f"{what}: C was written outside the groups' rows"
    assert all(torch.equal(t.view(torch.uint8), w.view(torch.uint8)) for (t, _), w in zip(keep, inputs)), f"{what}: an input changed"
    return got


def check(L, ops, off, cfg, what, **kw):
    got, expect = run(L, ops, off, cfg, what=what, **kw), ops.want(off, bias=kw.get("bias", "rows") == "rows")[off[0]:off[-1]]
    assert torch.equal(bits(got), bits(expect)), f"{what}: {rc.differing(got, expect)} elements differ"


@pytest.fixture(scope="module")
def boundary_ops():
    return {k: Ops(300, 72, k, 7) for k in (128, 320)}


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("k", [128, 320])
@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_group_boundaries_inside_fragments_and_tiles(g, L, boundary_ops, cfg, k, padded):
    # ends inside a 16-row fragment and a 64- and 128-row tile, a sliver column tile (N = 72), K = 320 wraps the ring; plain and NT store
    lds = (k + 8, k + 16, 72 * (k + 16) + 24, 72 + 8, 72 + 24) if padded else None
    for word in (1, 1 | NT):
        check(L, boundary_ops[k], BOUNDARIES, cfg, f"{MEMBERS[cfg]} K={k} {hex(word)}", word=word, lds=lds, stream=g.stream())


@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_the_cap_of_groups_mostly_single_rows(g, L, cfg):
    # G = the cap, M = G + 44: every lane of the map holds groups, the grid is nearly all single-row tiles; a few empty groups, one of 45 rows
    sizes = [45 if i == 200 else 0 if i in (0, 63, 64, 130, 255) else 1 for i in range(CAP)]
    off = [2] + [int(x) for x in 2 + np.cumsum(sizes)]
    assert off[-1] == CAP + 41 and len(off) == CAP + 1                          # 250 single rows + 45, 2 dropped rows in front and 3 behind
    check(L, Ops(CAP + 44, 8, 64, CAP), off, cfg, "the cap", stream=g.stream())


def test_all_groups_empty_leaves_c_untouched(g, L):
    ops = Ops(100, 72, 128, 5)
    for cfg in range(4):
        assert run(L, ops, [37] * 6, cfg, stream=g.stream(), what="all empty").numel() == 0


def test_one_group_is_the_bias_call_and_a_null_bias_is_zeros(g, L):
    m, n, k = 136, 72, 128
    ops = Ops(m, n, k, 1)
    a, w, bias = ops.a.cuda(), ops.w[0].cuda(), ops.bias[0].cuda()
    for cfg in range(4):
        c = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert L.bgemm_mi355x_launch_tn_bias(cfg, 1, a.data_ptr(), w.data_ptr(), bias.data_ptr(), c.data_ptr(), m, n, k, k, k, n, g.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(run(L, ops, [0, m], cfg, stream=g.stream(), what="G = 1")), bits(c.cpu())), MEMBERS[cfg]
        null, zeros = (run(L, ops, [0, m], cfg, bias=b, stream=g.stream(), what=b) for b in ("null", "zeros"))
        assert torch.equal(bits(null), bits(zeros)) and torch.equal(bits(null), bits(ops.want([0, m], bias=False))), MEMBERS[cfg]


@pytest.mark.parametrize("why", ["K = 72", "ldc % 8 == 4", "G = cap + 1"])
def test_the_reference_form_gives_the_cpu_bits(g, L, why):
    if why == "G = cap + 1":
        ops, off, lds = Ops(CAP + 1, 8, 64, CAP + 1), list(range(CAP + 2)), None
    else:
        k = 72 if why == "K = 72" else 128
        ops, off, lds = Ops(300, 72, k, 7), BOUNDARIES, (k, k, 72 * k, 72, 76) if why == "ldc % 8 == 4" else None
    for cfg in (0, 3):
        check(L, ops, off, cfg, why, lds=lds, form=FORM_REFERENCE, stream=g.stream())
        check(L, ops, off, cfg, why + " NULL bias", lds=lds, bias="null", form=FORM_REFERENCE, stream=g.stream())


def test_the_planned_entry_point(g, L, boundary_ops):
    check(L, boundary_ops[320], BOUNDARIES, 0, "planned", planned=True, stream=g.stream())


def test_one_capture_follows_the_offsets_of_each_replay(g, L, boundary_ops):
    # captured once on a fresh stream with nothing reserved; the offsets buffer is overwritten between two replays; one stream, one chain
    ops, m, n, k = boundary_ops[128], 300, 72, 128
    a, w, bias = ops.a.cuda(), ops.w.cuda(), ops.bias.cuda()
    off = torch.tensor(BOUNDARIES, dtype=torch.int32, device="cuda")
    c = torch.full((m, n), rc.OUT_FILL, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        ret = L.bgemm_mi355x_launch_tn_grouped(1, 1, a.data_ptr(), w.data_ptr(), bias.data_ptr(), c.data_ptr(), off.data_ptr(), 7, m, n, k, k, k, n * k, n, n,
                                               torch.cuda.current_stream().cuda_stream)
    assert ret == 0
    for routing in (BOUNDARIES, [0, 50, 50, 131, 200, 264, 299, 300]):
        off.copy_(torch.tensor(routing, dtype=torch.int32))
        c.fill_(rc.OUT_FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        expect = ops.want(routing)
        expect[:routing[0]], expect[routing[-1]:] = rc.OUT_FILL, rc.OUT_FILL
        assert torch.equal(bits(c.cpu()), bits(expect)), routing


def test_the_refusals(L):
    # argument checks, nothing launched; _runs on both sides of a stride condition and of the cap
    m, n, k, G = 300, 72, 128, 7
    a, b, bias, c, off = (ctypes.c_void_p(4096 * (i + 1)) for i in range(5))
    good = dict(cfg=0, word=1, ptrs=(a, b, bias, c, off), G=G, dims=(m, n, k), lds=(k, k, n * k, n, n))
    launch = lambda **kw: (lambda q: L.bgemm_mi355x_launch_tn_grouped(q["cfg"], q["word"], *q["ptrs"], q["G"], *q["dims"], *q["lds"], None))({**good, **kw})  # noqa: E731
    for i in (0, 1, 3, 4):
        assert launch(ptrs=tuple(None if j == i else p for j, p in enumerate(good["ptrs"]))) == -1, i
    assert launch(G=0) == -1 and launch(dims=(0, n, k)) == -1 and launch(dims=(m, 0, k)) == -1 and launch(dims=(m, n, 0)) == -1
    for lds in ((k - 8, k, n * k, n, n), (k, k - 8, n * k, n, n), (k, k, n * k - 8, n, n), (k, k, n * k, n - 8, n), (k, k, n * k, n, n - 8)):
        assert launch(lds=lds) == -1, lds
    assert launch(cfg=4) == -1 and launch(cfg=-1) == -1 and launch(word=2) == -1 and launch(word=2 | NT) == -1
    assert L.bgemm_mi355x_tn_grouped_runs(0, G, m, n, k, k, k, n * k, n, n) == 1 and L.bgemm_mi355x_tn_grouped_runs(0, G, m, n, k, k, k, n * k + 4, n, n) == 0
    assert L.bgemm_mi355x_tn_grouped_runs(0, CAP, m, n, k, k, k, n * k, n, n) == 1 and L.bgemm_mi355x_tn_grouped_runs(0, CAP + 1, m, n, k, k, k, n * k, n, n) == 0
