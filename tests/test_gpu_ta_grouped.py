"""GPU tests of the grouped weight gradient, bgemm_mi355x_ta_grouped / _ta_grouped_c32 (hgemm_inst_g24.hip) and of its reference kernel, by
tests/test_gpu_tn_grouped.py's method: integer operands (A scaled by 2^-9), so every sum is exact in fp32 in any order; torch on the CPU in float64 per
group, cast once, compared on BITS.  C starts as NaN (store forms), small integers (accumulate; NaN / -0.0 in an empty group) and a sentinel in every pad."""
import ctypes

import numpy as np
import pytest
import torch

import residual_common as rc
from residual_common import FORM_PLAIN, FORM_REFERENCE, NT, bits
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)

pytestmark = pytest.mark.gpu

MEMBERS = ("a64x64_w2x2", "a128x64_w2x2", "a64x128_w2x2", "a128x128_w2x2")
FORMS = ("store", "accumulate", "bf16")
K, M, N = 700, 72, 136       # one full tile plus an 8-wide sliver in each direction for every member
ROUTING = [3, 3, 4, 68, 68, 197, 524, 690]   # groups of 0, 1, 64, 0, 129, 327 (wraps both rings, ends 7 rows into a stage), 166 rows; dropped ends


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.bgemm_mi355x_launch_ta_grouped_c32.argtypes = [i] * 2 + [p] * 4 + [i] * 7 + [ll, i, p]
    lib.bgemm_mi355x_launch_ta_grouped.argtypes = [i] * 2 + [p] * 4 + [i] * 7 + [ll, p]
    lib.bgemm_mi355x_ta_grouped_c32.argtypes = [p] * 4 + [i] * 5 + [p]
    lib.bgemm_mi355x_ta_grouped.argtypes = [p] * 4 + [i] * 4 + [p]
    lib.bgemm_mi355x_selfcheck_launch_ta_grouped.argtypes = [i] * 11 + [ll, i, p]
    lib.bgemm_mi355x_launch_ta_c32.argtypes = [i] * 2 + [p] * 3 + [i] * 7 + [p]
    lib.bgemm_mi355x_launch_ta.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    return lib


class Ops:   # a_col_major [K][M] and b [K][N] on the CPU; sums(off): S_g of every group, exact
    def __init__(self, k, m, n, normal=False):
        rng = np.random.default_rng(rc.SEED)
        self.k, self.m, self.n = k, m, n
        a = rng.standard_normal((k, m)) if normal else rng.integers(-15, 16, size=(k, m)) * 2.0 ** -9
        b = rng.standard_normal((k, n)) if normal else rng.integers(-15, 16, size=(k, n)).astype(np.float64)
        self.a, self.b = torch.from_numpy(a).bfloat16(), torch.from_numpy(b).bfloat16()

    def sums(self, off):   # (+ 0.0: the accumulation starts from +0.0, so a one-row group's product -x * 0 is +0.0 and not -0.0)
        return torch.stack([(self.a[s:e].double().t() @ self.b[s:e].double()).float() + 0.0 for s, e in zip(off[:-1], off[1:])])


OPS = Ops(K, M, N)


def run(L, ops, off, cfg, form, word=1, lds=None, want_form=FORM_PLAIN, planned=False, c_off=0, old=None, stream=0, what=""):
    """One call; lds = (lda, ldb, ldc, group_stride_c), c_off: C moved by that many elements.  -> (C [G][M][N], what it held before) on the CPU"""
    k, m, n, G = ops.k, ops.m, ops.n, len(off) - 1
    c32, acc = form != "bf16", int(form == "accumulate")
    lda, ldb, ldc, gsc = lds or (m, n, n, m * n)
    out20 = (ctypes.c_longlong * 20)()
    st = L.bgemm_mi355x_selfcheck_launch_ta_grouped(cfg, word, 0 if c_off else 4, int(c32), G, m, n, k, lda, ldb, ldc, gsc, acc, out20)
    assert planned or (st, out20[0]) == (0, want_form), (what, st, out20[0])
    keep = [rc.place(ops.a, lda), rc.place(ops.b, ldb), (torch.tensor(off, dtype=torch.int32, device="cuda"), None)]
    cflat = torch.full((c_off + G * gsc + 8,), rc.OUT_FILL, dtype=torch.float32 if c32 else torch.bfloat16, device="cuda")
    c = torch.as_strided(cflat, (G, m, n), (gsc, ldc, 1), c_off)
    if old is None and acc:
        old = torch.from_numpy(np.random.default_rng(3).integers(-64, 65, size=(G, m, n))).float()
        old[[e <= s for s, e in zip(off[:-1], off[1:])]] = torch.tensor([float("nan"), -0.0]).repeat(m * n // 2).view(m, n)
    elif old is None:
        old = torch.full((G, m, n), float("nan"), dtype=cflat.dtype)
    c.copy_(old)
    before, inputs = cflat.clone(), [t.clone() for t, _ in keep]
    pa, pb, po, pc = *(t.data_ptr() for t, _ in keep), cflat.data_ptr() + c_off * cflat.element_size()
    if c32:
        st = (L.bgemm_mi355x_ta_grouped_c32(pa, pb, pc, po, G, m, n, k, acc, stream) if planned else
              L.bgemm_mi355x_launch_ta_grouped_c32(cfg, word, pa, pb, pc, po, G, m, n, k, lda, ldb, ldc, gsc, acc, stream))
    else:
        st = (L.bgemm_mi355x_ta_grouped(pa, pb, pc, po, G, m, n, k, stream) if planned else
              L.bgemm_mi355x_launch_ta_grouped(cfg, word, pa, pb, pc, po, G, m, n, k, lda, ldb, ldc, gsc, stream))
    torch.cuda.synchronize()
    assert st == 0, (what, st)
    got = c.cpu().clone()
    c.zero_()
    torch.as_strided(before, (G, m, n), (gsc, ldc, 1), c_off).zero_()
    assert torch.equal(bits(cflat), bits(before)), f"{what}: C was written outside the groups' M x N elements"
    assert all(torch.equal(t.view(torch.uint8), w.view(torch.uint8)) for (t, _), w in zip(keep, inputs)), f"{what}: an input changed"
    return got, old


def check(L, ops, off, cfg, form, what, nan_group=None, **kw):
    got, old = run(L, ops, off, cfg, form, what=what, **kw)
    s = ops.sums(off)
    empty = torch.tensor([e <= s_ for s_, e in zip(off[:-1], off[1:])]).view(-1, 1, 1)
    expect = s if form == "store" else s.bfloat16() if form == "bf16" else torch.where(empty, old, old + s)
    if nan_group is not None:   # a group whose own rows are poison: all NaN, whatever the payload
        assert bool(got[nan_group].isnan().all()), f"{what}: the poisoned group's C is not all NaN"
        got[nan_group], expect[nan_group] = 0, 0
    assert torch.equal(bits(got), bits(expect)), f"{what}: {int((got != expect).sum())} elements differ"


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_every_walk_length_and_start(g, L, cfg, form, padded):
    ldc = N + (12 if form != "bf16" else 16)
    lds = (M + 8, N + 16, ldc, M * ldc + 16) if padded else None
    for word in (1, 1 | NT):
        check(L, OPS, ROUTING, cfg, form, f"{MEMBERS[cfg]} {form} {hex(word)}", word=word, lds=lds, planned=cfg == 0 and not padded and word == 1, stream=g.stream())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cfg", range(4), ids=MEMBERS)
def test_rows_outside_a_group_contribute_nothing(g, L, cfg, form):
    # the K edge at both ends of a walk: the rows no group owns and every row of group 5 hold NaN / +-Inf in BOTH operands
    bad = torch.ones(K, dtype=torch.bool)
    bad[ROUTING[0]:ROUTING[5]], bad[ROUTING[6]:ROUTING[7]] = False, False
    p = Ops(K, M, N)   # (the same seed: OPS's operands once more)
    values = torch.tensor([float("nan"), float("inf"), float("-inf")]).bfloat16()
    for x in (p.a, p.b):
        x[bad] = values[(torch.arange(K)[:, None] + torch.arange(x.shape[1])[None, :]) % 3][bad]
    check(L, p, ROUTING, cfg, form, f"{MEMBERS[cfg]} {form} poison", nan_group=5, stream=g.stream())


def test_one_group_is_the_dense_call_bit_for_bit(g, L):
    k = 192   # random normal operands: inexact sums, so this pins the K order
    dense, old = Ops(k, M, N, normal=True), torch.from_numpy(np.random.default_rng(5).standard_normal((1, M, N))).float()
    a, b = dense.a.cuda(), dense.b.cuda()
    for cfg in range(4):
        for form in FORMS:
            c = (old[0].clone() if form == "accumulate" else torch.full((M, N), float("nan"), dtype=torch.float32 if form != "bf16" else torch.bfloat16)).cuda()
            st = (L.bgemm_mi355x_launch_ta(cfg, 1, a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, k, M, N, N, g.stream()) if form == "bf16" else
                  L.bgemm_mi355x_launch_ta_c32(cfg, 1, a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, k, M, N, N, int(form == "accumulate"), g.stream()))
            torch.cuda.synchronize()
            got, _ = run(L, dense, [0, k], cfg, form, old=old if form == "accumulate" else None, stream=g.stream(), what="G = 1")
            assert st == 0 and torch.equal(bits(got[0]), bits(c.cpu())), (MEMBERS[cfg], form)


@pytest.mark.parametrize("form", FORMS)
def test_all_groups_empty_and_three_hundred_single_rows(g, L, form):
    for cfg in range(4):
        check(L, OPS, [5] * 8, cfg, form, "all empty", stream=g.stream())
        check(L, Ops(304, 8, 8), list(range(2, 303)), cfg, form, "G = 300", stream=g.stream())       # no cap on G


@pytest.mark.parametrize("why", ["M = 20", "misaligned c", "ldc % 4 == 2"])
def test_the_reference_form_gives_the_cpu_bits(g, L, why):
    o = Ops(K, 20, N) if why == "M = 20" else OPS
    for cfg in (0, 3):
        for form in FORMS:
            check(L, o, ROUTING, cfg, form, f"{why} {form}", want_form=FORM_REFERENCE, c_off=2 if why == "misaligned c" else 0,
                  lds=(M, N, N + 2, M * (N + 2)) if why == "ldc % 4 == 2" else None, stream=g.stream())


def test_one_capture_follows_the_offsets_of_each_replay(g, L):
    a, b = OPS.a.cuda(), OPS.b.cuda()
    off = torch.tensor(ROUTING, dtype=torch.int32, device="cuda")
    c = torch.full((7, M, N), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        ret = L.bgemm_mi355x_launch_ta_grouped_c32(1, 1, a.data_ptr(), b.data_ptr(), c.data_ptr(), off.data_ptr(), 7, M, N, K, M, N, N, M * N, 0,
                                                   torch.cuda.current_stream().cuda_stream)
    assert ret == 0
    for routing in (ROUTING, [0, 50, 50, 131, 200, 264, 699, 700]):
        off.copy_(torch.tensor(routing, dtype=torch.int32))
        c.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(c.cpu()), bits(OPS.sums(routing))), routing


def test_the_refusals_leave_c_untouched(g, L):
    G, a, b, off = 7, OPS.a.cuda(), OPS.b.cuda(), torch.tensor(ROUTING, dtype=torch.int32, device="cuda")
    c = torch.full((G, M, N), rc.OUT_FILL, dtype=torch.float32, device="cuda")
    good = dict(cfg=0, word=1, ptrs=(a.data_ptr(), b.data_ptr(), c.data_ptr(), off.data_ptr()), G=G, dims=(M, N, K), lds=(M, N, N, M * N), acc=1)

    def launch(bf16_too=True, **kw):
        q = {**good, **kw}
        st = L.bgemm_mi355x_launch_ta_grouped_c32(q["cfg"], q["word"], *q["ptrs"], q["G"], *q["dims"], *q["lds"], q["acc"], g.stream())
        return (st, L.bgemm_mi355x_launch_ta_grouped(q["cfg"], q["word"], *q["ptrs"], q["G"], *q["dims"], *q["lds"], g.stream()) if bf16_too else None)

    bad = [dict(ptrs=tuple(None if j == i else p for j, p in enumerate(good["ptrs"]))) for i in range(4)]
    bad += [dict(G=0), dict(dims=(0, N, K)), dict(dims=(M, 0, K)), dict(dims=(M, N, 0)), dict(cfg=4), dict(cfg=-1), dict(word=2), dict(word=2 | NT)]
    bad += [dict(lds=lds) for lds in ((M - 8, N, N, M * N), (M, N - 8, N, M * N), (M, N, N - 8, M * N), (M, N, N, M * N - 8))]
    for kw in bad:
        assert launch(**kw) == (-1, -1), kw
    assert launch(False, acc=2)[0] == -1 and launch(False, acc=-1)[0] == -1        # (the bf16 form has no accumulate argument)
    torch.cuda.synchronize()
    assert bool((c == rc.OUT_FILL).all())
