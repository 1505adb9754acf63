"""GPU tests of the address arithmetic (run with `-m gpu` on an MI355X): operands at padded row strides, the 32-bit reach edges of
the LDS-DMA kernels executed at the largest stride each geometry still takes, contiguous operands past 2^31 bytes / elements, and
the stride check of hgemm_mi355x_launch.

Every other GPU test calls the kernels at (lda, ldb, ldc) = (K, K, N).  Here the padding of A and b_col_major holds NaN
(0 x NaN = NaN: a read of it shows in C), C's padding a value no 0/1 product takes, and both must come back bit-unchanged.  On
N(0,1) inputs a stride must not change the summation order: the padded C is bit-identical to the same kernel's contiguous C."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_common import resolve

pytestmark = pytest.mark.gpu

RAGGED, GENERIC = -2, -1                        # HGEMM_CONFIG_RAGGED, HGEMM_CONFIG_GENERIC
FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000
XCD_STAGGER, RS_NT_LOADS = 0x80000, 0x100000
GIB = 1 << 30


@pytest.fixture(scope="module")
def g():
    import gpu_common

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return gpu_common


@pytest.fixture(scope="module")
def oracle():
    from oracle import hgemm_oracle

    return hgemm_oracle


def bits(x):
    return x.view(np.uint16) if isinstance(x, np.ndarray) else x.view(torch.int16)


# ---- a. every geometry at padded strides ----------------------------------------------------------------------------------------
M, N = 300, 456                # no tile height or width (16 ... 256, 96, 192) divides either; N % 8 == 0 (wide epilogue possible)
STRIDES = [(64, 64, 64),       # + (K, K, N): LDS-DMA loads, wide epilogue
           (8, 16, 4),         # ldc % 8 = 4: narrow epilogue
           (4, 0, 0)]          # lda % 8 != 0: the ragged kernel


def plan_forms(g, cid, name):
    forms = [1, 3, 3 | FUSED, 1 | NT_STORE]
    if cid >= 0 and g.lib().hgemm_mi355x_config_streamk(cid) > 0:
        forms.append(STREAMK | 37)
    if name == "r128x128_k128":
        forms.append(1 | XCD_STAGGER | RS_NT_LOADS)
    if name == "q256x256_w2x2":
        forms.append(1 | XCD_STAGGER)
    return forms


@pytest.mark.parametrize("k", [1024, 1064])
def test_every_geometry_is_exact_and_stride_blind_at_padded_strides(g, oracle, k):
    """Every geometry (and the ragged / reference kernels) in every form at three stride sets.  K = 1024 every geometry takes
    whole; K = 1064 = 8 x 128 + 40 runs the K tails of families q / r / t.  Each case: the form the launch resolves to (a padded
    stride must not silently turn an LDS-DMA case into a ragged one; lda % 8 != 0 must), 0/1 inputs bit-exact against the
    oracle, padding bit-unchanged (gpu_common.gemm), and N(0,1) inputs bit-identical to the contiguous run of the same kernel."""
    L = g.lib()
    m, n = M, N
    rng = np.random.default_rng(k)
    a, b = oracle.zero_one_inputs(m, n, k, rng)
    truth = oracle.truth_numpy(a, b)
    ar = rng.standard_normal((m, k), dtype=np.float32).astype(np.float16)
    br = rng.standard_normal((k, n), dtype=np.float32).astype(np.float16)
    contiguous = (k, k, n)
    ragged_ref = g.gemm(ar, br, plan=(RAGGED, 1, 2))
    assert not np.isnan(ragged_ref).any()
    names = g.config_names()
    cases = [(RAGGED, "ragged"), (GENERIC, "generic")]
    cases += [(cid, name) for cid, name in enumerate(names)
              if k % 64 == 0 or (name[0] in "tqr" and L.hgemm_mi355x_config_accepts_k(cid, k))]
    assert len(cases) > 20
    ran = 0
    for cid, name in cases:
        for splits in plan_forms(g, cid, name):
            plan = (cid, splits, 2)
            base = resolve(cid, splits, m, n, k, contiguous)
            assert base[0] == 0 and base[1] == {RAGGED: "ragged", GENERIC: "reference"}.get(cid, base[1]), (name, hex(splits), base)
            if cid >= 0:
                assert base[1] != "ragged", (name, hex(splits), base)
            ref = g.gemm(ar, br, plan=plan)
            for pad in STRIDES:
                lds = tuple(x + p for x, p in zip(contiguous, pad))
                got = resolve(cid, splits, m, n, k, lds)
                if pad[0] % 8 and cid != GENERIC:
                    assert got[:2] == (0, "ragged"), (name, hex(splits), lds, got)
                    want = ragged_ref
                else:
                    assert got == base, (name, hex(splits), lds, got, base)
                    want = ref
                out = g.gemm(a, b, plan=plan, ld=lds)
                assert np.array_equal(bits(out), bits(truth)), (name, hex(splits), lds, got[1])
                out = g.gemm(ar, br, plan=plan, ld=lds)
                assert np.array_equal(bits(out), bits(want)), (name, hex(splits), lds, got[1], "N(0,1): differs from the contiguous run")
                ran += 1
    assert ran >= len(cases) * 4 * len(STRIDES)


# ---- b. the 32-bit reach edges, executed ----------------------------------------------------------------------------------------
def largest_fast_stride(g, cid, m, n, k, side):
    """The largest stride (a multiple of 8) of operand `side` (0: A, 1: b_col_major, 2: C) at which the geometry's own kernel still
    runs, the others contiguous -- found through the launch's decision (bisection: it is monotone in the stride)."""
    def fast(s):
        lds = [k, k, n]
        lds[side] = s
        st, form, _ = resolve(cid, 1, m, n, k, tuple(lds))
        assert st == 0
        return form != "ragged"

    lo, hi = (k if side < 2 else n) // 8, 1 << 27          # 8 x 2^27 = 2^30 elements: beyond every reach for tiles of >= 4 rows
    assert fast(8 * lo) and not fast(8 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fast(8 * mid) else (lo, mid)
    return 8 * lo


REACH_CASES = [  # (geometry, M, N, K, operand (0: A, 1: b_col_major, 2: C), the rule's limit in bytes)
    ("t64x64_w2x2_m16_s4", 64 + 8, 64, 256, 0, 2 * GIB),    # classic family: descriptors end at 2 GiB (bit 31 marks out of range)
    ("q256x256_w2x2", 256 + 8, 64, 256, 0, 4 * GIB),        # family q, whole stages: 4 GiB
    ("q256x256_w2x2", 256 + 8, 64, 264, 0, 2 * GIB),        # ... with a direct K tail: bit 31 marks out of range again
    ("r128x128_k128", 64, 128 + 8, 256, 1, 4 * GIB),        # family r, the B side (bn x ldb)
    ("s256x256_w2x2", 256 + 8, 72, 256, 2, 2 * GIB),        # the LDS-staged epilogue's C descriptor (bm x ldc)
]


def all_bits_equal(flat, value):
    want = bits(torch.full((1,), value, dtype=torch.half, device="cuda")).item()
    step = 1 << 28
    return all(bool((bits(flat[i:i + step]) == want).all()) for i in range(0, flat.numel(), step))


@pytest.mark.parametrize("case", REACH_CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1:4]))}-{'ABC'[c[4]]}")
def test_reach_edges_run_exact_on_both_sides(g, oracle, case):
    """The largest stride at which the geometry's LDS-DMA kernel still runs (its 32-bit offsets reach to the end of a tile band)
    and the next multiple of 8 (the ragged kernel, 64-bit addressing), both executed.  M (N on the B side) spans a second tile
    band that ends in a ragged edge: a band base just below the limit and the last band's clamped range.  The operand lives in a
    buffer filled with NaN (C: with -3.0) that must come back unchanged outside the operand's window."""
    name, m, n, k, side, limit = case
    L = g.lib()
    cid = g.config_names().index(name)
    info = (ctypes.c_int * 8)()
    assert L.hgemm_mi355x_config_info(cid, info) == 0
    rows_per_tile = info[1] if side == 1 else info[0]
    s = largest_fast_stride(g, cid, m, n, k, side)
    tail = 2 * (n if side == 2 else k)
    assert rows_per_tile * s * 2 + tail < limit <= rows_per_tile * (s + 8) * 2 + tail, (s, limit)   # the rule the launch applies
    rng = np.random.default_rng(s)
    a_np, b_np = oracle.zero_one_inputs(m, n, k, rng)
    truth = torch.from_numpy(oracle.truth_numpy(a_np, b_np))
    rows, cols = [(m, k), (n, k), (m, n)][side]
    pad_value = -3.0 if side == 2 else float("nan")
    flat = torch.full((rows * (s + 8),), pad_value, dtype=torch.half, device="cuda")
    a = torch.from_numpy(a_np).cuda()
    b = torch.from_numpy(b_np).cuda()
    bt = b.t().contiguous()
    for stride, form in ((s, "plain"), (s + 8, "ragged")):
        lds = [k, k, n]
        lds[side] = stride
        assert resolve(cid, 1, m, n, k, tuple(lds))[:2] == (0, form), (stride, form)
        window = flat.as_strided((rows, cols), (stride, 1))
        c = torch.full((m, n), float("nan"), dtype=torch.half, device="cuda")
        if side == 2:
            window.fill_(float("nan"))
            c = window
        else:
            window.copy_([a, bt][side])
        ops = [a, bt, c]
        ops[side] = flat
        st = L.hgemm_mi355x_launch(cid, 1, 2, ops[0].data_ptr(), b.data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), m, n, k, *lds,
                                   g.stream())
        assert st == 0, L.hgemm_mi355x_strerror(st)
        torch.cuda.synchronize()
        got = c.contiguous().cpu()
        assert torch.equal(bits(got), bits(truth)), (name, stride, form)
        window.fill_(pad_value)
        assert all_bits_equal(flat, pad_value), (name, stride, form, "the padding changed")
    del flat, window, c
    torch.cuda.empty_cache()


# ---- c. large contiguous operands through the entry points ----------------------------------------------------------------------
def zero_one_on_device(rows, cols, gen):
    """0/1 fp16 [rows, cols] with P(1) = 1/4, generated on the device in slices (a K = 16384 sum stays far below 2048: exact)."""
    x = torch.empty((rows, cols), dtype=torch.half, device="cuda")
    step = max(1, (1 << 27) // cols)
    for r in range(0, rows, step):
        x[r:r + step] = torch.rand((min(step, rows - r), cols), generator=gen, device="cuda") < 0.25
    return x


def probe_indices(count, row_elems, seed):
    """First and last row, the rows either side of where a row's byte offset reaches 2^31 and 2^32 and its element offset 2^31,
    and random ones: 64 in all."""
    idx = {0, count - 1}
    for edge in ((1 << 31) // (2 * row_elems), (1 << 32) // (2 * row_elems), (1 << 31) // row_elems):
        idx |= {i for i in (edge - 1, edge, edge + 1) if 0 <= i < count}
    rng = np.random.default_rng(seed)
    while len(idx) < 64:
        idx.add(int(rng.integers(0, count)))
    return sorted(idx)


LARGE_CASES = [  # (M, N, K, entry, the large operand)
    (139264, 256, 16384, "fp32", "A"),      # A: 2^31 + 2^27 elements (4.25 GiB)
    (256, 139264, 16384, "fp16", "B"),      # b_col_major (and b): 4.25 GiB
    (139264, 16384, 64, "fp32", "C"),       # C: 4.25 GiB
]


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: f"{c[4]}-{c[0]}x{c[1]}x{c[2]}")
def test_operands_past_2_gib_and_2_31_elements_through_the_entry_points(g, case):
    """Contiguous operands whose offsets pass 2^31 bytes, 2^32 bytes and 2^31 elements, through hgemm_mi355x_fp32 / _fp16 at the
    plan the library picks: 64 rows of C (columns in the b_col_major case) bit-exact against the CPU product of those rows."""
    m, n, k, entry, big = case
    L = g.lib()
    cfg, splits, group = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.hgemm_mi355x_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    plan = (L.hgemm_mi355x_config_name(cfg.value) if cfg.value >= 0 else cfg.value, hex(splits.value), group.value)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(m + 3 * n + 7 * k)
    a = zero_one_on_device(m, k, gen)
    if big == "B":
        bt = zero_one_on_device(n, k, gen)
        b = bt.t().contiguous()
    else:
        b = zero_one_on_device(k, n, gen)
        bt = b.t().contiguous()
    c = torch.full((m, n), float("nan"), dtype=torch.half, device="cuda")
    fn = L.hgemm_mi355x_fp16 if entry == "fp16" else L.hgemm_mi355x_fp32
    st = fn(a.data_ptr(), b.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, g.stream())
    assert st == 0, (L.hgemm_mi355x_strerror(st), plan)
    torch.cuda.synchronize()
    if big == "B":
        idx = probe_indices(n, k, n)
        sel = torch.tensor(idx, device="cuda")
        got = c.index_select(1, sel).cpu()
        want = a.float().cpu() @ bt.index_select(0, sel).float().cpu().t()
    else:
        idx = probe_indices(m, k if big == "A" else n, m)
        sel = torch.tensor(idx, device="cuda")
        got = c.index_select(0, sel).cpu()
        want = a.index_select(0, sel).float().cpu() @ b.float().cpu()
    assert len(idx) == 64 and float(want.max()) <= 2047
    bad = (bits(got) != bits(want.half())).any(dim=0 if big == "B" else 1).nonzero().flatten().tolist()
    assert not bad, (plan, big, "wrong " + ("columns" if big == "B" else "rows"), [idx[i] for i in bad][:16])
    del a, b, bt, c
    torch.cuda.empty_cache()


# ---- d. strides below the row length -------------------------------------------------------------------------------------------
def test_strides_below_the_row_length_are_rejected_and_c_is_untouched(g):
    """lda < K, ldb < K (b_col_major given) and ldc < N return HGEMM_ERR_BAD_ARG before anything is launched.  (The buffers are
    sized so that an unchecked launch would still stay inside them.)"""
    L = g.lib()
    m, n, k = 320, 256, 512
    a = torch.ones((m, k), dtype=torch.half, device="cuda")
    b = torch.ones((k, n), dtype=torch.half, device="cuda")
    bt = b.t().contiguous()
    c = torch.full((m, n), -3.0, dtype=torch.half, device="cuda")
    names = g.config_names()
    for cid in (RAGGED, GENERIC, names.index("q256x256_w2x2"), names.index("t128x128_w2x2_m16_s3"), names.index("r64x64_k256")):
        for lds in ((k - 8, k, n), (k, k - 8, n), (k, k, n - 4)):
            for splits in (1, 2):
                st = L.hgemm_mi355x_launch(cid, splits, 1, a.data_ptr(), b.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, *lds,
                                           g.stream())
                assert st == -1, (cid, lds, splits, st)
    torch.cuda.synchronize()
    assert bool((c == -3.0).all())
