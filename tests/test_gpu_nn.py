"""GPU tests of family "n" (run with `-m gpu` on an MI355X): the NN layout -- B row-major, staged row-major into LDS and read through
ds_read_b64_tr_b16 (hgemm_kernel_nn.hpp) -- through the C ABI against the CPU oracle.

Bar: 0/1 inputs BIT-EXACT AND UNMASKED, as tests/test_gpu_lu.py: every partial sum is an integer <= K <= 8192 < 2**24, exact in fp32
in any order, then one round-to-nearest-even to fp16.  The expected value is oracle.truth_f32acc, above 2**24 multiply-adds
oracle.truth_numpy (the same exact integer before the same rounding; tests/test_oracle.py pins the two together).
N(0,1) inputs: oracle.relative_error <= 1e-3 against the CPU fp32 product, the project's REL_TOL.
tests/test_gpu_nn_bars.py holds the family to the other families' bars with these fixtures and helpers: rounding on dyadic operands,
special values, the reach edges executed, rasters of more than eight tile rows, the launch's workspace behaviour, misaligned pointers."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3
MEMBERS = ("n64x64_w2x2", "n128x64_w2x2", "n64x128_w2x2", "n128x128_w2x2")
NT_STORE = 0x20000
FORMS = (1, 1 | NT_STORE, 2, 5)   # plain, non-temporal stores, two-pass splits 2 / 5 (clamped to one split per K stage)


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
def L(g):
    lib = g.lib()
    lib.hgemm_mi355x_nn_config_name.restype = ctypes.c_char_p
    lib.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.hgemm_mi355x_launch_nn.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    lib.hgemm_mi355x_nn_fp32.argtypes = lib.hgemm_mi355x_nn_fp16.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.hgemm_mi355x_nn_plan_workspace_bytes.restype = ctypes.c_size_t
    lib.hgemm_mi355x_nn_plan_workspace_bytes.argtypes = [ctypes.c_int] * 5
    lib.hgemm_mi355x_reserve_workspace.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    ids = [L.hgemm_mi355x_nn_config_by_name(nm.encode()) for nm in MEMBERS]
    assert all(i >= 0 for i in ids), f"family n members missing from the library: {list(zip(MEMBERS, ids))}"
    return list(zip(MEMBERS, ids))


def bits(x):
    return x.view(np.uint16)


def truth_of(oracle, a, b):
    m, k = a.shape
    return oracle.truth_f32acc(a, b) if m * b.shape[1] * k <= 2 ** 24 else oracle.truth_numpy(a, b)


def gemm_nn(g, L, a_np, b_np, plan=None, entry="fp32", ld=None):
    """C = A.B through the NN entry points; plan = (nn_config, splits) for the explicit call.  ld = (lda, ldb, ldc) places A, the
    ROW-MAJOR B and C in wider buffers: A's and B's padding columns hold NaN (a read of them shows in C), C's hold gpu_common.C_PAD,
    and every padding element must come back bit-unchanged."""
    m, k = a_np.shape
    n = b_np.shape[1]
    assert ld is None or plan is not None, "the planned entry points take contiguous operands"
    lda, ldb, ldc = ld or (k, n, n)
    a = torch.full((m, lda), float("nan"), dtype=torch.half, device="cuda")
    a[:, :k] = torch.from_numpy(np.ascontiguousarray(a_np)).cuda()
    b = torch.full((k, ldb), float("nan"), dtype=torch.half, device="cuda")
    b[:, :n] = torch.from_numpy(np.ascontiguousarray(b_np)).cuda()
    c = torch.full((m, ldc), g.C_PAD, dtype=torch.half, device="cuda")
    c[:, :n] = float("nan")  # unwritten outputs stay NaN
    pads = [(x[:, w:], x[:, w:].clone()) for x, w in ((a, k), (b, n), (c, n))]
    if plan is None:
        fn = L.hgemm_mi355x_nn_fp16 if entry == "fp16" else L.hgemm_mi355x_nn_fp32
        st = fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, g.stream())
    else:
        st = L.hgemm_mi355x_launch_nn(plan[0], plan[1], a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, lda, ldb, ldc, g.stream())
    assert st == 0, L.hgemm_mi355x_strerror(st)
    torch.cuda.synchronize()
    for pad, before in pads:
        assert torch.equal(pad.view(torch.int16), before.view(torch.int16)), f"padding changed (lda, ldb, ldc = {lda}, {ldb}, {ldc})"
    return c[:, :n].contiguous().cpu().numpy()


def check_exact(g, L, oracle, members, m, n, k, seed, forms=FORMS, ld=None, runs=1):
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(seed))
    truth = truth_of(oracle, a, b)
    assert not np.isnan(truth).any()
    lds = ld or (k, n, n)
    ran = 0
    for name, cid in members:
        assert L.hgemm_mi355x_nn_runs(cid, m, n, k, *lds) == runs, (name, m, n, k, lds)
        for splits in forms:
            got = gemm_nn(g, L, a, b, plan=(cid, splits), ld=ld)
            bad = int((bits(got) != bits(truth)).sum())
            assert bad == 0, f"{name} splits {hex(splits)} {m}x{n}x{k} ld={ld}: {bad} of {m * n} elements differ from the oracle"
            ran += 1
    return ran, truth


def test_a_transposed_b_is_told_apart(g, L, oracle, members):
    """A = identity (M = K): C must be B itself, an asymmetric 0/1 matrix -- a kernel that reads B transposed, swaps two k-rows or two
    16-byte chunks of a row, or hands a lane another lane's column gives another matrix.  Then A = a row permutation of the identity:
    C = the permuted rows of B."""
    m = k = 128
    n = 136
    rng = np.random.default_rng(5)
    b = (rng.random((k, n)) < 0.5).astype(np.float16)
    assert not np.array_equal(b[:, :128], b[:, :128].T)
    perm = rng.permutation(m)
    for a, want in ((np.eye(m, dtype=np.float16), b), (np.eye(m, dtype=np.float16)[perm], b[perm])):
        for name, cid in members:
            for splits in FORMS:
                got = gemm_nn(g, L, a, b, plan=(cid, splits))
                assert np.array_equal(bits(got), bits(want)), (name, hex(splits), int((bits(got) != bits(want)).sum()))


@pytest.mark.parametrize("shape", [(64, 64, 64), (1, 8, 64), (65, 72, 128), (200, 264, 192), (130, 8, 64)])
def test_one_tile_and_ragged_edges_are_exact(g, L, oracle, members, shape):
    """One tile of the smallest member, one row, one 8-column sliver (every other column of the tile reads past N), M and N ragged
    against every tile size, more than one tile per dimension."""
    m, n, k = shape
    assert check_exact(g, L, oracle, members, m, n, k, seed=m + 3 * n + 5 * k)[0] == len(MEMBERS) * len(FORMS)


@pytest.mark.parametrize("stages", ["1", "2", "3", "NBUF", "NBUF+1", "7"])
def test_k_of_few_and_odd_stage_counts_is_exact(g, L, oracle, members, stages):
    """The ring's prologue with fewer stages than buffers, exactly as many, one more, an odd count no split divides."""
    for name, cid in members:
        info = (ctypes.c_int * 8)()
        assert L.hgemm_mi355x_nn_config_info(cid, info) == 0
        nst = {"NBUF": info[5], "NBUF+1": info[5] + 1}.get(stages) or int(stages)
        assert check_exact(g, L, oracle, [(name, cid)], 96, 136, 64 * nst, seed=nst * 1000 + cid)[0] == len(FORMS)


def test_k_8192_sums_are_compared_unmasked(g, L, oracle, members):
    """64 x 64 x 8192: about half the sums exceed 2047 and are compared like every other element."""
    ran, truth = check_exact(g, L, oracle, members, 64, 64, 8192, seed=8192)
    assert ran == len(MEMBERS) * len(FORMS)
    assert 0.25 < float((truth.astype(np.float32) > 2047).mean()) < 0.75


def test_padded_strides_never_read_nan_padding_and_leave_c_padding_alone(g, L, oracle, members):
    """ld = (K + 8, N + 24, N + 16): A's and B's padding columns hold NaN, C's hold gpu_common.C_PAD and come back bit-unchanged
    (gemm_nn compares every padding element).  B's NaN columns N .. N + 23 DO enter the LDS image of an edge tile: they must only
    meet accumulators of columns >= N, which are never stored."""
    for m, n, k in ((200, 264, 192), (130, 72, 128)):
        assert check_exact(g, L, oracle, members, m, n, k, seed=m + k, ld=(k + 8, n + 24, n + 16))[0] == len(MEMBERS) * len(FORMS)


@pytest.mark.parametrize("case", ["K=72", "N=100", "ldb=N+4"])
def test_what_the_kernel_does_not_take_is_still_answered_exactly(g, L, oracle, members, case):
    """Outside the kernel's scope the reference kernel answers: status 0 (gemm_nn asserts it), exact, whatever split count is named."""
    m, n, k, ld = {"K=72": (200, 136, 72, None), "N=100": (200, 100, 128, None), "ldb=N+4": (200, 136, 128, (128, 140, 136))}[case]
    assert check_exact(g, L, oracle, members, m, n, k, seed=k + n, forms=(1, 4), ld=ld, runs=0)[0] == 2 * len(MEMBERS)


def test_randn_tolerance_and_ten_runs_are_bit_identical(g, L, oracle, members):
    """N(0,1) inputs: max|C - ref| / max|ref| <= 1e-3 against the CPU fp32 product, and ten runs of one plan give the same bits
    (the two-pass combine adds the slabs in split order)."""
    for m, n, k in ((256, 264, 1024), (512, 512, 2048)):
        rng = np.random.default_rng(12 + m)
        a = rng.standard_normal((m, k), dtype=np.float32).astype(np.float16)
        b = rng.standard_normal((k, n), dtype=np.float32).astype(np.float16)
        ref = a.astype(np.float32) @ b.astype(np.float32)
        for name, cid in members:
            for splits in FORMS:
                first = gemm_nn(g, L, a, b, plan=(cid, splits))
                err = oracle.relative_error(first, ref)
                print(f"{name} splits {hex(splits)} {m}x{n}x{k}: relative error {err:.3e}")
                assert err <= REL_TOL, (name, hex(splits), err)
                for _ in range(9):
                    assert np.array_equal(bits(gemm_nn(g, L, a, b, plan=(cid, splits))), bits(first)), (name, hex(splits))
            # non-temporal stores cannot change a bit
            assert np.array_equal(bits(gemm_nn(g, L, a, b, plan=(cid, 1 | NT_STORE))), bits(gemm_nn(g, L, a, b, plan=(cid, 1)))), name


@pytest.mark.parametrize("shape", [(64, 4096, 64), (512, 4096, 4096), (4096, 4096, 4096)])
def test_the_planned_entries_on_the_baseline_shapes_are_exact(g, L, oracle, shape):
    m, n, k = shape
    a, b = oracle.zero_one_inputs(m, n, k, np.random.default_rng(m + n + k))
    truth = truth_of(oracle, a, b)
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    assert L.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0
    assert 0 <= cfg.value < len(MEMBERS) and L.hgemm_mi355x_nn_runs(cfg.value, m, n, k, k, n, n) == 1
    for entry in ("fp32", "fp16"):
        got = gemm_nn(g, L, a, b, entry=entry)
        assert np.array_equal(bits(got), bits(truth)), (shape, entry, int((bits(got) != bits(truth)).sum()))


def test_hipgraph_capture_and_replay(g, L, oracle, members):
    """A splits = 1 call needs no workspace: captured on a fresh stream with nothing reserved.  A split call is captured after
    hgemm_mi355x_reserve_workspace on that stream.  Both graphs, replayed on NEW operand values written into the captured buffers,
    compute exactly."""
    m, n, k = 200, 264, 512
    for splits, reserve in ((1, False), (4, True)):
        s = torch.cuda.Stream()
        bufs = []
        for name, cid in members:
            ws = L.hgemm_mi355x_nn_plan_workspace_bytes(cid, splits, m, n, k)
            assert (ws == 0) == (splits == 1) and ws <= 64 << 20            # (what reserve_workspace guarantees at least)
            bufs.append((torch.empty((m, k), dtype=torch.half, device="cuda"), torch.empty((k, n), dtype=torch.half, device="cuda"),
                         torch.empty((m, n), dtype=torch.half, device="cuda")))
        if reserve:
            assert L.hgemm_mi355x_reserve_workspace(m, n, k, s.cuda_stream) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            st = torch.cuda.current_stream().cuda_stream
            for (name, cid), (a, b, c) in zip(members, bufs):
                rc = L.hgemm_mi355x_launch_nn(cid, splits, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, k, n, n, st)
                assert rc == 0, L.hgemm_mi355x_strerror(rc)
        for seed in (1, 2):
            truths = []
            for i, (a, b, c) in enumerate(bufs):
                a_np, b_np = oracle.zero_one_inputs(m, n, k, np.random.default_rng(100 * seed + i))
                a.copy_(torch.from_numpy(a_np)); b.copy_(torch.from_numpy(b_np))
                c.fill_(float("nan"))
                truths.append(oracle.truth_numpy(a_np, b_np))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            for (name, _), (_, _, c), truth in zip(members, bufs, truths):
                assert np.array_equal(bits(c.cpu().numpy()), bits(truth)), (name, splits, seed)
