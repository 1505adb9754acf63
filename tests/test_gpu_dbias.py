"""GPU tests of the bias gradient: bgemm_mi355x_nn_dact_dbias (the dact call with a fused, deterministic column sum of dZ) and
bgemm_mi355x_colsum_c32 (the column sum on its own).

C is held to bgemm_mi355x_launch_nn_dact's C bit for bit in every run.  db32 is held to the column sum of the C READ BACK, taken in fp64:
with ReLU on tests/test_gpu_mlp_backward.py's operands every stored C is a multiple of one power of two and every column sum is exact in
fp32 in any order (asserted), so the bar is equality of bits; with both GELUs the bar is |db32[n] - sum C| <= gamma_{M-1} sum |C|,
gamma_k = k u / (1 - k u), u read from csrc/hgemm_dbias.hpp -- the bound of an M-term fp32 sum in any order, every column checked.  Before
any launch the CPU shows from reference data alone that the sum of the unrounded S is another vector (K >= 128) and that a GELU kernel
without the row mask is outside the bar (M off the tile)."""
import contextlib
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_mlp_backward import NN_MEMBERS, DactCase, dact64
from test_gpu_ta import FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, FORMS, NT_STORE, two_pass_cuts
from test_gpu_tn_bf16 import SHAPES as BASE_SHAPES
from test_gpu_tn_bias_act import ACT_NAME, ACTS, GELU, GELU_TANH, RELU
from test_gpu_tr_bf16 import ibits, seed_of, to_bf16
from test_ta_host import CSRC

pytestmark = pytest.mark.gpu

SHAPES = list(BASE_SHAPES) + [(1000, 64, 64)]                    # sixteen tile rows of 64 in the finish kernel
TILES = dict(zip(NN_MEMBERS, ((64, 64), (128, 64), (64, 128), (128, 128))))
HOOK = "bgemm_mi355x_selfcheck_launch_nn_dact_dbias"
EPI_SLAB, EPI_DACT, EPI_DBIAS = 1, 11, 32
THUNK_ENTRY, THUNK_SPLITK_REDUCE, THUNK_GENERIC, THUNK_COLSUM_BLOCKED, THUNK_COLSUM_FINISH, THUNK_COLSUM_DIRECT = 0, 1, 4, 5, 6, 7
DB_SENTINEL = -12345.625
GUARD = 8                                                        # floats behind db32[N - 1]


def _u():
    m = re.search(r"constexpr int COLSUM_U_LOG2 = (-\d+);", (CSRC / "hgemm_dbias.hpp").read_text())
    assert m, "hgemm_dbias.hpp does not state the unit roundoff of the column sum's bar"
    return 2.0 ** int(m.group(1))


U = _u()


def gamma(terms):
    return (terms - 1) * U / (1.0 - (terms - 1) * U)


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    lib.bgemm_mi355x_launch_nn_dact.argtypes = [i] * 2 + [p] * 4 + [i] * 8 + [p]
    lib.bgemm_mi355x_launch_nn_dact_dbias.argtypes = [i] * 2 + [p] * 5 + [i] * 9 + [p]
    lib.bgemm_mi355x_nn_dact_dbias.argtypes = [p] * 5 + [i] * 5 + [p]
    lib.bgemm_mi355x_nn_dact_dbias_reserve_workspace.argtypes = [i] * 3 + [p]
    lib.bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes.restype = ctypes.c_size_t
    lib.bgemm_mi355x_colsum_c32.argtypes = [p] * 2 + [i] * 4 + [p]
    lib.bgemm_mi355x_tn_bias_act_aux.argtypes = [p] * 5 + [i] * 4 + [p]
    lib.bgemm_mi355x_ta_c32.argtypes = [p] * 3 + [i] * 4 + [p]
    return lib


@pytest.fixture(scope="module")
def members(L):
    nn = [(nm, L.hgemm_mi355x_nn_config_by_name(nm.encode())) for nm in NN_MEMBERS]
    assert [c for _, c in nn] == [0, 1, 2, 3]
    return nn


def decision(L, cid, word, act, m, n, k, ld, ldz, aligned=True, ruled_out=0):
    out = (ctypes.c_longlong * 44)()
    st = getattr(L, HOOK)(cid, word, 4 if aligned else 0, m, n, k, *ld, ldz, ruled_out, act, out)
    return st, out[0], [tuple(out[4 + 8 * i:10 + 8 * i]) for i in range(out[1])]


def db_buffer(n, fill=float("nan")):
    buf = torch.full((n + GUARD,), DB_SENTINEL, dtype=torch.float32, device="cuda")
    buf[:n] = fill
    return buf


def launch(g, L, case, plan, act, c, db, accumulate=0, stream=None):
    m, n, k = case.m, case.n, case.k
    st = L.bgemm_mi355x_launch_nn_dact_dbias(plan[0], plan[1], case.ad.data_ptr(), case.bd.data_ptr(), case.zd.data_ptr(), c.data_ptr(), db.data_ptr(),
                                             m, n, k, *case.ld, case.ldz, act, accumulate, g.stream() if stream is None else stream)
    assert st == 0, (plan, act, L.hgemm_mi355x_strerror(st))


def check_db(case, c, db, act, what):
    """db32 against the column sum of the C read back, in fp64; the guard behind db32[N - 1]."""
    torch.cuda.synchronize()
    m, n = case.m, case.n
    c64 = c[:m, :n].cpu().double()
    want, mag = c64.sum(0), c64.abs().sum(0)
    got = db[:n].cpu()
    assert bool((db[n:].cpu() == DB_SENTINEL).all()), f"{what}: something was written behind db32[N - 1]"
    assert bool(torch.isfinite(got).all()), f"{what}: db32 is not finite"
    if act == RELU:
        assert torch.equal(want.float().double(), want), f"{what}: the reference sum is not an fp32 value"
        bad = int((ibits(got) != ibits(want.float())).sum())
        assert bad == 0, f"{what}: {bad} of {n} columns differ from the exact sum of the stored C"
    else:
        err, bound = (got.double() - want).abs(), gamma(m) * mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{what}: worst error {worst:.3f} of gamma_(M-1) sum |C|")
        assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {n} columns outside the bar (worst {worst:.3f} of it)"


def run(g, L, case, plan, act, what, reference_c=None):
    """The dbias call next to the dact call at the same plan: C bit for bit, db32 inside its bar from a NaN prefill.  Returns (c, db)."""
    c, db = case.c_buffer(), db_buffer(case.n)
    launch(g, L, case, plan, act, c, db)
    if reference_c is None:
        reference_c = case.c_buffer()
        case.launch(g, L, reference_c, plan, act)
    torch.cuda.synchronize()
    bad = int((ibits(c) != ibits(reference_c)).sum())
    assert bad == 0, f"{what}: C (pads and guard row included) differs from bgemm_mi355x_launch_nn_dact's in {bad} elements"
    check_db(case, c, db, act, what)
    return c, db


@pytest.fixture(scope="module")
def cases():
    built = {}

    def get(shape, padded=False):
        if (shape, padded) not in built:
            built[(shape, padded)] = DactCase(*shape, seed_of(shape), padded)
        return built[(shape, padded)]

    return get


# ---- what the bars can tell apart, from reference data alone ---------------------------------------------------------------------------------
def test_the_bars_tell_the_unrounded_sum_and_the_missing_row_mask_apart(cases):
    for shape in SHAPES:
        m, n, k = shape
        case = cases(shape)
        relu = case.relu16.double()
        assert torch.equal(relu.sum(0).float().double(), relu.sum(0)), (shape, "a column sum of the expected ReLU C is no fp32 value")
        unrounded = torch.where(case.z32 <= 0, torch.zeros_like(case.s64), case.s64).sum(0)
        differ = int((unrounded != relu.sum(0)).sum())
        print(shape, "columns where the sum of the unrounded S differs:", differ)
        assert differ >= 1 or k < 128, shape
        for act in (GELU, GELU_TANH):
            c64 = to_bf16(case.y64[act].float()).double()        # the expected C, up to the bar of the dact call
            bound = gamma(m) * c64.abs().sum(0)
            for name, (bm, _) in TILES.items():
                pad = -m % bm
                if pad:
                    unmasked = (pad * 0.5 * case.s64[m - 1]).abs()
                    assert int((unmasked > 2 * bound).sum()) >= 1, (shape, name, ACT_NAME[act], "rows past M added unmasked would pass")


# ---- every member, form and activation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_member_form_and_activation_c_is_dacts_and_db_meets_its_bar(g, L, members, cases, shape, padded):
    m, n, k = shape
    case = cases(shape, padded)
    for name, cid in members:
        bm = TILES[name][0]
        assert L.bgemm_mi355x_nn_dact_dbias_runs(cid, m, n, k, *case.ld, case.ldz) == 1, (name, shape)
        for act in ACTS:
            plain_db = None
            for word in FORMS:
                cuts = two_pass_cuts(k, word) if (word & 0xFFFF) > 1 else []
                st, form, disp = decision(L, cid, word, act, m, n, k, case.ld, case.ldz)
                if cuts:
                    tail = [(THUNK_COLSUM_BLOCKED, EPI_DBIAS), (THUNK_COLSUM_FINISH, EPI_DBIAS)] if m > 256 else [(THUNK_COLSUM_DIRECT, EPI_DBIAS)]
                    want = [(THUNK_ENTRY, EPI_SLAB), (THUNK_SPLITK_REDUCE, EPI_DACT + act)] + tail
                else:
                    want = [(THUNK_ENTRY, EPI_DBIAS + act), (THUNK_COLSUM_FINISH, EPI_DBIAS)]
                    assert disp[1][5] == -(-m // bm), "the finish kernel adds one row of partials per tile row"
                assert (st, form) == (0, FORM_SPLITK if cuts else FORM_PLAIN) and [(d[0], d[2]) for d in disp] == want, (name, hex(word), disp)
                what = f"dbias {ACT_NAME[act]} {name} {hex(word)} {shape} ld={case.ld} ldz={case.ldz}"
                _, db = run(g, L, case, (cid, word), act, what)
                if word == 1:
                    plain_db = db
                elif word == 1 | NT_STORE:
                    assert torch.equal(ibits(db), ibits(plain_db)), f"{what}: HGEMM_PLAN_NT_STORE changed db32's bits"
    assert case.operands_intact()


def test_accumulate_modes_determinism_and_refusals(g, L, members, cases):
    shape = SHAPES[3]
    m, n, k = shape
    case = cases(shape, True)
    rng = np.random.default_rng(5)
    old_host = torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 64)
    for (cid, word), act in (((3, 1), GELU), ((0, 1), RELU), ((1, 5), GELU_TANH), ((2, 2), GELU)):
        what = f"accumulate {ACT_NAME[act]} member {cid} {hex(word)}"
        c0, s = run(g, L, case, (cid, word), act, what)          # accumulate = 0 from a NaN prefill: finite and inside the bar
        c1, s1 = case.c_buffer(), db_buffer(n)
        launch(g, L, case, (cid, word), act, c1, s1)
        torch.cuda.synchronize()
        assert torch.equal(ibits(s1), ibits(s)) and torch.equal(ibits(c1), ibits(c0)), f"{what}: the same call twice gives other bits"
        acc = db_buffer(n)
        acc[:n] = old_host.cuda()
        launch(g, L, case, (cid, word), act, case.c_buffer(), acc, accumulate=1)
        torch.cuda.synchronize()
        assert torch.equal(ibits(acc[:n].cpu()), ibits(old_host + s[:n].cpu())), f"{what}: accumulate = 1 is not fl32(old + s)"
        assert bool((acc[n:].cpu() == DB_SENTINEL).all())
    c, db = case.c_buffer(), db_buffer(n, DB_SENTINEL)
    args = (case.ad.data_ptr(), case.bd.data_ptr(), case.zd.data_ptr(), c.data_ptr())
    tail = (m, n, k, *case.ld, case.ldz)
    null = ctypes.c_void_p(0)
    for accumulate in (2, -1):
        assert L.bgemm_mi355x_launch_nn_dact_dbias(0, 1, *args, db.data_ptr(), *tail, GELU, accumulate, g.stream()) == -1
    assert L.bgemm_mi355x_launch_nn_dact_dbias(0, 1, *args, null, *tail, GELU, 0, g.stream()) == -1
    assert L.bgemm_mi355x_launch_nn_dact_dbias(0, 1, *args, db.data_ptr(), *tail, 0, 0, g.stream()) == -1
    assert L.bgemm_mi355x_launch_nn_dact_dbias(0, 1, *args[:2], null, c.data_ptr(), db.data_ptr(), *tail, GELU, 0, g.stream()) == -1
    assert L.bgemm_mi355x_launch_nn_dact_dbias(0, 1, *args, db.data_ptr(), m, n, k, *case.ld, n - 8, GELU, 0, g.stream()) == -1
    torch.cuda.synchronize()
    assert bool((db.cpu() == DB_SENTINEL).all()) and bool((c.cpu().float() == case.c_buffer().cpu().float()).all()), "a refused call wrote"
    assert case.operands_intact()


@pytest.mark.parametrize("what", ["z 8 bytes off", "ldz % 8 != 0"])
def test_outside_the_kernels_scope_the_reference_form_meets_the_same_bars(g, L, members, what):
    shape = SHAPES[2]
    m, n, k = shape
    case = DactCase(m, n, k, seed_of(shape))
    if what.startswith("z 8"):
        store = torch.full(((m + 1) * n + 4,), float("nan"), dtype=torch.bfloat16, device="cuda")
        store[4:].view(m + 1, n).copy_(case.zd)
        case.zd = store[4:].view(m + 1, n)
        assert case.zd.data_ptr() % 16 == 8
        aligned = False
    else:
        from test_gpu_mlp_backward import make_z
        case.ldz = n + 4
        case.z_host = make_z(m, n, case.ldz, seed_of(shape))
        case.zd = case.z_host.cuda()
        case.z32 = case.z_host[:m, :n].float()
        aligned = True
        assert L.bgemm_mi355x_nn_dact_dbias_runs(3, m, n, k, *case.ld, case.ldz) == 0
    case.before[2] = case.zd.clone()
    for act in ACTS:
        st, form, disp = decision(L, 3, 1, act, m, n, k, case.ld, case.ldz, aligned=aligned)
        assert (st, form) == (0, FORM_REFERENCE) and [(d[0], d[2]) for d in disp] == [(THUNK_GENERIC, EPI_DACT + act), (THUNK_COLSUM_DIRECT, EPI_DBIAS)]
        run(g, L, case, (3, 1), act, f"dbias reference {ACT_NAME[act]} {what}")
    assert case.operands_intact()


def test_the_planned_call_is_the_explicit_call_at_the_plan(g, L, members):
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    for (m, n, k), want in (((256, 264, 512), 8), ((1024, 1024, 64), 1)):
        assert L.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0 and splits.value == want
        case = DactCase(m, n, k, m + n + k)
        assert L.bgemm_mi355x_nn_dact_dbias_reserve_workspace(m, n, k, g.stream()) == 0
        for act in ACTS:
            c, db = run(g, L, case, (cfg.value, splits.value), act, f"dbias at the plan {ACT_NAME[act]} {m}x{n}x{k}")
            c2, db2 = case.c_buffer(), db_buffer(n)
            st = L.bgemm_mi355x_nn_dact_dbias(case.ad.data_ptr(), case.bd.data_ptr(), case.zd.data_ptr(), c2.data_ptr(), db2.data_ptr(), m, n, k, act, 0,
                                              g.stream())
            assert st == 0
            torch.cuda.synchronize()
            assert torch.equal(ibits(c2), ibits(c)) and torch.equal(ibits(db2), ibits(db)), ("planned dbias", act)
        assert case.operands_intact()


@contextlib.contextmanager
def fresh_stream():
    """A stream of this test's own, made with the runtime torch has loaded and destroyed on the way out.  No stream of torch's pool: those
    live as long as the process, and every one that has run work keeps its share of the process's few hardware queues -- a stream a later
    test module takes from the pool would then be placed next to other work than it is today (tests/test_gpu_harness.py times one)."""
    path = next(ln.split()[-1] for ln in Path("/proc/self/maps").read_text().splitlines() if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamDestroy.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], [ctypes.c_void_p]
    handle = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(handle), 1) == 0 and handle.value        # 1: hipStreamNonBlocking, as torch's are
    try:
        yield torch.cuda.ExternalStream(handle.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(handle) == 0


def test_a_captured_call_without_a_workspace_returns_0_and_with_a_reserve_runs_the_fused_form(g, L, members):
    """A fresh stream, nothing reserved: the call returns 0 while capturing and replays the dact kernel and the direct column sum -- the
    replay meets the bars and C is the eager call's.  Behind a reserve on a second fresh stream the capture takes the workspace: its db is
    the eager fused call's, bit for bit (the direct form adds in another order).  One stream, one chain per graph; the graph is replayed
    on the test's own stream and gone before that stream is."""
    m, n, k = 328, 264, 512
    case = DactCase(m, n, k, 61)
    with contextlib.ExitStack() as streams:                        # all six alive to the end: no address, and so no workspace entry, comes back
        for act, (cid, word) in ((GELU, (3, 1)), (RELU, (0, 8)), (GELU_TANH, (1, 1))):
            eager_c, eager_db = run(g, L, case, (cid, word), act, f"eager dbias {ACT_NAME[act]}")
            for reserve in (False, True):
                c, db = case.c_buffer(), db_buffer(n)
                s = streams.enter_context(fresh_stream())
                if reserve:
                    assert L.bgemm_mi355x_nn_dact_dbias_reserve_workspace(4096, 4096, 512, s.cuda_stream) == 0    # (more than this call's plan needs)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.stream(s):
                    graph.capture_begin()
                    try:
                        rc = L.bgemm_mi355x_launch_nn_dact_dbias(cid, word, case.ad.data_ptr(), case.bd.data_ptr(), case.zd.data_ptr(), c.data_ptr(),
                                                                 db.data_ptr(), m, n, k, *case.ld, case.ldz, act, 0, s.cuda_stream)
                    finally:
                        graph.capture_end()
                    assert rc == 0
                    torch.cuda.synchronize()
                    graph.replay()
                torch.cuda.synchronize()
                del graph
                if (word & 0xFFFF) == 1 or reserve:
                    assert torch.equal(ibits(c), ibits(eager_c)), (act, reserve)
                check_db(case, c, db, act, f"replayed dbias {ACT_NAME[act]} reserve={reserve}")
                if reserve:
                    assert torch.equal(ibits(db), ibits(eager_db)), (act, "with a reserve the capture runs the eager call's form")
    assert case.operands_intact()


# ---- the column sum on its own -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 72, 1001])
@pytest.mark.parametrize("m", [1, 255, 257, 4099])
def test_colsum_integer_data_bit_for_bit_and_normal_data_inside_the_bar(g, L, m, n):
    rng = np.random.default_rng(m * 7 + n)
    for ldx, off in ((n, 0), (n + 8 if n % 8 == 0 else n + 7, 0), (n + 3, 0), (n + 8 - n % 8, 4)):     # contiguous, padded, odd, 8 bytes off
        for kind in ("integers", "normal"):
            host = torch.from_numpy(rng.integers(-2, 3, (m, n)).astype(np.float32) if kind == "integers" else rng.standard_normal((m, n)).astype(np.float32))
            store = torch.full((m * ldx + off + 8,), float("nan"), dtype=torch.bfloat16, device="cuda")
            x = store[off:off + m * ldx].view(m, ldx)
            x[:, :n] = host.to(torch.bfloat16).cuda()
            x64 = host.to(torch.bfloat16).double()
            want, mag = x64.sum(0), x64.abs().sum(0)
            out = db_buffer(n)
            assert L.bgemm_mi355x_colsum_c32(x.data_ptr(), out.data_ptr(), m, n, ldx, 0, g.stream()) == 0
            out2 = db_buffer(n, 3.0)
            assert L.bgemm_mi355x_colsum_c32(x.data_ptr(), out2.data_ptr(), m, n, ldx, 1, g.stream()) == 0
            torch.cuda.synchronize()
            got = out[:n].cpu()
            what = f"colsum {m}x{n} ldx={ldx} off={off} {kind}"
            assert bool((out[n:].cpu() == DB_SENTINEL).all()) and bool((out2[n:].cpu() == DB_SENTINEL).all()), what
            if kind == "integers":
                assert torch.equal(got.double(), want), what
            else:
                assert bool(((got.double() - want).abs() <= gamma(m) * mag).all()), what
            assert torch.equal(ibits(out2[:n].cpu()), ibits(torch.full((n,), 3.0) + got)), f"{what}: accumulate = 1 is not fl32(old + s)"


def test_colsum_refusals(g, L):
    x = torch.zeros((4, 16), dtype=torch.bfloat16, device="cuda")
    out = db_buffer(16, DB_SENTINEL)
    null = ctypes.c_void_p(0)
    assert L.bgemm_mi355x_colsum_c32(x.data_ptr(), out.data_ptr(), 4, 16, 8, 0, g.stream()) == -1            # ldx < N
    assert L.bgemm_mi355x_colsum_c32(null, out.data_ptr(), 4, 16, 16, 0, g.stream()) == -1
    assert L.bgemm_mi355x_colsum_c32(x.data_ptr(), null, 4, 16, 16, 0, g.stream()) == -1
    assert L.bgemm_mi355x_colsum_c32(x.data_ptr(), out.data_ptr(), 4, 16, 16, 2, g.stream()) == -1
    assert L.bgemm_mi355x_colsum_c32(x.data_ptr(), out.data_ptr(), 0, 16, 16, 0, g.stream()) == -1
    assert L.bgemm_mi355x_colsum_c32(x.data_ptr(), out.data_ptr(), 4, 0, 16, 0, g.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out.cpu() == DB_SENTINEL).all())


# ---- one layer, end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS, ids=[ACT_NAME[a] for a in ACTS])
def test_one_layer_aux_forward_dact_dbias_and_the_weight_gradient(g, L, members, act):
    """aux forward -> dact_dbias at the saved z_out -> bgemm_mi355x_ta_c32 (dW = X^T dZ): db is the column sum of the dZ the dW call read --
    with an X of ones, dW's every row is that column sum too, exactly where the sums are exact (ReLU) and inside the bar otherwise."""
    from test_gpu_tn_bias_act import ActCase
    m, n, k = 152, 152, 320
    fwd = ActCase(m, n, k, 5)
    y = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
    z = torch.full((m + 1, n), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert L.bgemm_mi355x_tn_bias_act_aux(fwd.ad.data_ptr(), fwd.wd.data_ptr(), fwd.bias_d.data_ptr(), y.data_ptr(), z.data_ptr(), m, n, k, act, g.stream()) == 0
    torch.cuda.synchronize()
    bwd = DactCase(m, n, 128, 6, z=z.cpu())
    dz, db = run(g, L, bwd, (2, 1), act, f"layer backward {ACT_NAME[act]}")
    ones = torch.ones((m, 8), dtype=torch.bfloat16, device="cuda")                                        # X [M][8]: a_col_major of dW = X^T dZ
    dw = torch.zeros((8, n), dtype=torch.float32, device="cuda")
    assert L.bgemm_mi355x_ta_c32(ones.data_ptr(), dz.data_ptr(), dw.data_ptr(), 8, n, m, 0, g.stream()) == 0
    torch.cuda.synchronize()
    col = dz[:m, :n].cpu().double()
    for r in range(8):
        err = (dw[r].cpu().double() - db[:n].cpu().double()).abs()
        assert bool((err <= 2 * gamma(m) * col.abs().sum(0)).all()), (act, r)
        if act == RELU:
            assert torch.equal(dw[r].cpu(), db[:n].cpu())
    assert bwd.operands_intact()


def test_the_combine_and_the_reference_kernel_on_dyadic_operands(g, L):
    """The two helper kernels of the three dact + dbias sets (C and db32) (hgemm_registry.hip), on order-exact dyadic operands (gpu_common.HelperKernelSet): the 64 x 64 member,
    M = N = 64, ldc = 72, ldz = 80 -- K = 128 in 2 splits runs the combine's remainder loop only, K = 704 in 11 splits one unrolled block of eight and
    two remainder slabs --, the split call against the unsplit and the reference-kernel call bit for bit; then M = 5, N = 12, K = 24 on padded
    strides, which only the reference kernel takes, against the member kernel on the zero-padded operands bit for bit.  db32 bit for bit where its sums are exact (ReLU, and split against reference: one kernel on one C), otherwise inside (M - 1) 2^-24 sum |C|."""
    def one(act):
        return g.HelperKernelSet(lambda cfg, word, p, d, acc: L.bgemm_mi355x_launch_nn_dact_dbias(cfg, word, p["a"], p["b"], p["z"], p["c"], p["db"], *d, act, 0, g.stream()),
                                 lambda cfg, word, d, aligned, acc: decision(L, cfg, word, act, *d[:3], d[3:6], d[6], aligned), torch.bfloat16, z="in",
                                 db=True, db_exact=act == RELU)
    sets = [one(act) for act in ACTS]
    for s in sets:
        s.check_combine(128, 2, 9181)
        s.check_combine(704, 11, 9181 + 1)
        s.check_reference(9181 + 2)
