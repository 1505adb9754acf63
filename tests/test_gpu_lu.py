"""GPU tests of family "u" (run with `-m gpu` on an MI355X): the K walk of one output tile split over four K-groups of waves
inside the workgroup, partial accumulators reduced through LDS (hgemm_kernel_lu.hpp), through the C ABI against the CPU oracle.

Bar: 0/1 inputs BIT-EXACT AND UNMASKED -- every partial sum is an integer <= K <= 8192 < 2**24, exact in fp32 in any order,
followed by one round-to-nearest-even to fp16, so no element is left out (at K = 8192 about half the sums exceed 2047: the
reference's `> 2047` mask would hide half of that case).  The expected value is oracle.truth_f32acc (the C restatement: fp32
accumulate in k order, one RNE); its scalar loop runs at ~0.06 GMAC/s, so above 2**24 multiply-adds (minutes to hours: 512 x 4096 x
4096 would take 40 h) the same value comes from oracle.truth_numpy -- fp32 BLAS, which for 0/1 inputs is the same exact integer
before the same single rounding whatever its summation order; tests/test_oracle.py pins the two together.
N(0,1) inputs: oracle.relative_error <= 1e-3, the project's REL_TOL."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3
MEMBERS = ("u64x64_w2x2_k4", "u128x64_w2x2_k4", "u64x128_w2x2_k4", "u128x128_w2x2_k4")
FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000
# plain, non-temporal stores, external splits 2 / 5 / 16 (two-pass: slab epilogue + combine kernel), the single-launch and the
# stream-K plan words (the family has neither kernel: they run as two-pass / as the plain launch)
FORMS = (1, 1 | NT_STORE, 2, 5, 16, 4 | FUSED, 2 | NT_STORE, STREAMK, STREAMK | 37)


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


@pytest.fixture(scope="module")
def members(g):
    names = g.config_names()
    missing = [nm for nm in MEMBERS if nm not in names]
    assert not missing, f"family u members missing from the library: {missing}"
    L = g.lib()
    return [(nm, names.index(nm), L.hgemm_mi355x_config_k_granularity(names.index(nm))) for nm in MEMBERS]


def bits(x):
    return x.view(np.uint16)


def truth_of(oracle, a, b):
    m, k = a.shape
    return oracle.truth_f32acc(a, b) if m * b.shape[1] * k <= 2 ** 24 else oracle.truth_numpy(a, b)


def check_exact(g, oracle, members, m, n, k, seed, forms=FORMS, ld=None, group=2):
    rng = np.random.default_rng(seed)
    a, b = oracle.zero_one_inputs(m, n, k, rng)
    truth = truth_of(oracle, a, b)
    assert not np.isnan(truth).any()
    L = g.lib()
    ran = 0
    for name, cid, stage in members:
        if k % stage:
            continue
        assert L.hgemm_mi355x_config_accepts_k(cid, k) == 1
        for splits in forms:
            got = g.gemm(a, b, plan=(cid, splits, group), ld=ld)   # (NaN-prefilled C, padding compared bit for bit: gpu_common.gemm)
            bad = int((bits(got) != bits(truth)).sum())
            assert bad == 0, f"{name} splits {hex(splits)} {m}x{n}x{k} ld={ld}: {bad} of {m * n} elements differ from the oracle"
            ran += 1
    return ran, truth


@pytest.mark.parametrize("shape", [(64, 64, 256), (128, 128, 256), (328, 456, 1024), (1000, 520, 768), (72, 200, 128), (200, 68, 384)])
def test_one_tile_and_ragged_edges_are_exact(g, oracle, members, shape):
    """One tile of the smallest and of the largest member, M and N ragged against every tile size (N % 4 == 0 is all the LDS-DMA
    path asks), tiles that are mostly past the edge."""
    m, n, k = shape
    assert check_exact(g, oracle, members, m, n, k, seed=m + 3 * n + 5 * k)[0] == len(MEMBERS) * len(FORMS)


@pytest.mark.parametrize("stages", [1, 2, 3, 7])
def test_k_of_one_two_three_and_seven_stages_is_exact(g, oracle, members, stages):
    """The ring's prologue with fewer stages than buffers, an odd stage count, a count no split divides: per member, K = its
    stage depth x 1 / 2 / 3 / 7 (a split count above the stage count is clamped to one stage per split)."""
    for name, cid, stage in members:
        assert check_exact(g, oracle, [(name, cid, stage)], 200, 136, stage * stages, seed=stages * 1000 + stage)[0] == len(FORMS)


@pytest.mark.parametrize("shape", [(1024, 256, 2048), (512, 512, 2048), (2048, 128, 2048), (64, 64, 8192), (512, 4096, 4096)])
def test_the_class_shapes_are_exact(g, oracle, members, shape):
    """The tiny-output / long-K class the family is for, and 512 x 4096 x 4096.  At K = 8192 about half the sums exceed 2047
    and are compared like every other element."""
    m, n, k = shape
    ran, truth = check_exact(g, oracle, members, m, n, k, seed=7 * m + n + k)
    assert ran == len(MEMBERS) * len(FORMS)
    if k == 8192:
        assert 0.25 < float((truth.astype(np.float32) > 2047).mean()) < 0.75          # the unmasked half is really there


def test_padded_strides_never_read_nan_padding_and_leave_c_padding_alone(g, oracle, members):
    """ld = (K + 8, K + 24, N + 16): A's and b_col_major's padding columns hold NaN (a read of them shows in C), C's hold gpu_common.C_PAD
    and must come back bit-unchanged (gpu_common.gemm compares every padding element); ragged M and N, every form."""
    for m, n, k in ((328, 456, 1024), (136, 72, 384)):
        assert check_exact(g, oracle, members, m, n, k, seed=m + k, ld=(k + 8, k + 24, n + 16))[0] == len(MEMBERS) * len(FORMS)


def test_the_k_groups_are_told_apart(g, oracle, members):
    """A is zero outside ONE K = 32 slice per case (B is dense 0/1), so the expected C is the product of that slice alone: a
    K-group that reads another group's slice, reads its own twice, or is left out of the LDS reduce gives a wrong sum, not merely
    a reordered one.  Every slice of a three-stage walk, i.e. every (stage, K-group) of every member, unsplit and with an external
    split on top; then all slices at once with a different slice live in every row."""
    m, n = 136, 200
    for name, cid, stage in members:
        k = 3 * stage
        a_full, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(stage + cid))
        for s0 in range(0, k, 32):
            a = np.zeros_like(a_full)
            a[:, s0:s0 + 32] = 1.0                       # all ones in the slice: C[m][n] = number of ones of b[s0:s0+32, n]
            truth = oracle.truth_f32acc(a, b)
            assert np.array_equal(truth[0], b[s0:s0 + 32].astype(np.float32).sum(axis=0).astype(np.float16))
            for splits in (1, 2):
                got = g.gemm(a, b, plan=(cid, splits, 1))
                assert np.array_equal(bits(got), bits(truth)), (name, s0, splits)
        a = np.zeros_like(a_full)
        for row in range(m):
            j = row % (k // 32)
            a[row, 32 * j:32 * j + 32] = a_full[row, 32 * j:32 * j + 32]
        truth = oracle.truth_f32acc(a, b)
        for splits in (1, 3):
            assert np.array_equal(bits(g.gemm(a, b, plan=(cid, splits, 1))), bits(truth)), (name, "rows", splits)


def test_randn_tolerance_and_ten_runs_are_bit_identical(g, oracle, members):
    """N(0,1) inputs: max|C - ref| / max|ref| <= 1e-3 against the fp32 product, and ten runs of one plan give the same bits (the
    LDS reduce adds the groups in the fixed order 0, 1, 2, 3; the two-pass combine adds the slabs in split order)."""
    for m, n, k in ((328, 456, 1024), (1024, 256, 2048)):
        rng = np.random.default_rng(12 + m)
        a = rng.standard_normal((m, k), dtype=np.float32).astype(np.float16)
        b = rng.standard_normal((k, n), dtype=np.float32).astype(np.float16)
        ref = a.astype(np.float32) @ b.astype(np.float32)
        for name, cid, stage in members:
            for splits in (1, 1 | NT_STORE, 4, 4 | FUSED):
                first = g.gemm(a, b, plan=(cid, splits, 2))
                err = oracle.relative_error(first, ref)
                print(f"{name} splits {hex(splits)} {m}x{n}x{k}: relative error {err:.3e}")
                assert err <= REL_TOL, (name, hex(splits), err)
                for _ in range(9):
                    assert np.array_equal(bits(g.gemm(a, b, plan=(cid, splits, 2))), bits(first)), (name, hex(splits))
            # the raster group and non-temporal stores cannot change a bit either
            base = g.gemm(a, b, plan=(cid, 1, 1))
            assert np.array_equal(bits(g.gemm(a, b, plan=(cid, 1 | NT_STORE, 8))), bits(base)), name


@pytest.mark.parametrize("k", [200, 1064, 192, 72])
def test_a_k_that_is_not_whole_stages_is_still_answered_exactly(g, oracle, members, k):
    """No K tail in the family: K % stage != 0 (a multiple of 8, or of 64 but not of the stage) is served by the any-shape
    kernel -- status 0 (gpu_common.gemm asserts it), exact, whatever split count the plan names."""
    L = g.lib()
    m, n = 200, 136
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(k))
    truth = oracle.truth_f32acc(a, b)
    ran = 0
    for name, cid, stage in members:
        if k % stage == 0:
            continue
        assert L.hgemm_mi355x_config_accepts_k(cid, k) == 0
        for splits in (1, 4, 4 | FUSED, STREAMK):
            assert np.array_equal(bits(g.gemm(a, b, plan=(cid, splits, 1))), bits(truth)), (name, k, hex(splits))
            ran += 1
    assert ran == 4 * len(MEMBERS)


def test_hipgraph_capture_and_replay_without_workspace(g, oracle, members):
    """A splits = 1 launch of the family needs no workspace: it is captured on a fresh stream with nothing reserved and the graph,
    replayed on NEW operand values written into the captured buffers, computes exactly."""
    L = g.lib()
    L.hgemm_mi355x_plan_workspace_bytes.restype = ctypes.c_size_t
    L.hgemm_mi355x_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    m, n, k = 328, 456, 1024
    s = torch.cuda.Stream()
    bufs = []
    for name, cid, stage in members:
        assert L.hgemm_mi355x_plan_workspace_bytes(cid, 1, m, n, k) == 0
        bufs.append((torch.empty((m, k), dtype=torch.half, device="cuda"), torch.empty((k, n), dtype=torch.half, device="cuda"),
                     torch.empty((n, k), dtype=torch.half, device="cuda"), torch.empty((m, n), dtype=torch.half, device="cuda")))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        for (name, cid, stage), (a, b, bt, c) in zip(members, bufs):
            rc = L.hgemm_mi355x_launch(cid, 1, 2, a.data_ptr(), b.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, k, k, n, st)
            assert rc == 0, L.hgemm_mi355x_strerror(rc)
    for seed in (1, 2):
        truths = []
        for i, (a, b, bt, c) in enumerate(bufs):
            a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(100 * seed + i))
            a.copy_(torch.from_numpy(a_np)); b.copy_(torch.from_numpy(b_np)); bt.copy_(torch.from_numpy(np.ascontiguousarray(b_np.T)))
            c.fill_(float("nan"))
            truths.append(oracle.truth_numpy(a_np, b_np))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for (name, _, _), (_, _, _, c), truth in zip(members, bufs, truths):
            assert np.array_equal(bits(c.cpu().numpy()), bits(truth)), (name, seed)
