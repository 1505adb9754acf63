"""q256x256_w2x2's one-tile-per-workgroup kernel (hgemm_kernel_sq_one.hpp) against the general kernel of the same plan, both run from
one library through the switch hgemm_mi355x_set_one_item_kernel:

  * N(0,1) operands: C is BIT-IDENTICAL with the switch on and off (same summation order per element, same epilogue);
  * 0/1 operands: C is exact against the CPU oracle;
  * every operand and C lie inside a guard band (and C's row padding, where ldc > N) that must come back bit-unchanged;
  * the launch counter shows which kernel ran: the new one exactly for the launches the selection rule names.

Shapes (KMIN = 3 K-steps, the depth of the kernel's A stream): one tile at KMIN and KMIN + 1 steps (odd / even step count: the even
count runs the extra head step), a 2 x 3 tile grid, ragged M and N edges inside one tile, and all 256 workgroups.  One step below
KMIN and a launch with more tiles than workgroups (4352^2: 289) stay with the general kernel.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KMIN = 3
NT_STORE = 0x20000
GUARD = 4096          # fp16 elements in front of and behind every buffer (a multiple of 8: the buffers stay 16-byte aligned)
SHAPES = [(256, 256, 64 * KMIN), (256, 256, 64 * (KMIN + 1)), (512, 768, 1024), (200, 248, 640), (4096, 4096, 512)]
OLD_KERNEL_SHAPES = [(256, 256, 64 * (KMIN - 1)), (4352, 4352, 512)]


@pytest.fixture(scope="module")
def g():
    import gpu_common
    import torch

    L = gpu_common.lib()
    L.hgemm_mi355x_one_item_kernel_launches.restype = ctypes.c_ulonglong
    L.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    cfg = L.hgemm_mi355x_config_by_name(b"q256x256_w2x2")
    assert cfg >= 0

    class G:
        pass

    G.L, G.cfg, G.torch, G.stream = L, cfg, torch, staticmethod(gpu_common.stream)
    yield G
    L.hgemm_mi355x_set_one_item_kernel(1)


@pytest.fixture(scope="module")
def oracle():
    from oracle import hgemm_oracle

    return hgemm_oracle


def guarded(g, rows, cols, ld, fill):
    """A [rows][ld] fp16 matrix inside a flat buffer with GUARD elements on both sides; everything but [:, :cols] is `fill`."""
    flat = g.torch.full((2 * GUARD + rows * ld,), fill, dtype=g.torch.half, device="cuda")
    return flat, flat[GUARD:GUARD + rows * ld].view(rows, ld)


def run(g, a, bt, on, flags=1, ldc=None):
    """One launch of plan (q256x256_w2x2, flags, group 2) on device operands a [M][K], bt [N][K]; returns (C bits, new-kernel launches)."""
    (m, k), n = a.shape, bt.shape[0]
    ldc = ldc or n
    bufs = []
    for src, rows, cols, ld in ((a, m, k, k), (bt, n, k, k)):
        flat, view = guarded(g, rows, cols, ld, float("nan"))     # a NaN read from the guard band shows in C
        view[:, :cols] = src
        bufs.append((flat, view))
    cflat, c = guarded(g, m, n, ldc, -3.0 * 2.0 ** -12)
    c[:, :n] = float("nan")
    before_c = cflat.clone()
    before_ops = [flat.clone() for flat, _ in bufs]
    g.L.hgemm_mi355x_set_one_item_kernel(1 if on else 0)
    count = g.L.hgemm_mi355x_one_item_kernel_launches()
    st = g.L.hgemm_mi355x_launch(g.cfg, flags, 2, bufs[0][1].data_ptr(), None, bufs[1][1].data_ptr(), c.data_ptr(), m, n, k, k, k, ldc, g.stream())
    assert st == 0, st
    g.torch.cuda.synchronize()
    count = g.L.hgemm_mi355x_one_item_kernel_launches() - count
    for (flat, _), before in zip(bufs, before_ops):
        assert g.torch.equal(flat.view(g.torch.int16), before.view(g.torch.int16)), "an operand buffer changed"
    out = c[:, :n].clone()
    c[:, :n] = float("nan")      # (back to the prefill: what is left to compare is the guard band and the row padding)
    assert g.torch.equal(cflat.view(g.torch.int16), before_c.view(g.torch.int16)), "C's guard band or row padding changed"
    return out.cpu().numpy().view(np.uint16), count


_inputs = {}


def inputs(g, oracle, shape):
    """Per shape, made once: N(0,1) operands (device) and 0/1 operands (device) with their exact product (host)."""
    if shape not in _inputs:
        m, n, k = shape
        gen = g.torch.Generator(device="cuda").manual_seed(1000 + m + 3 * n + 7 * k)
        a = g.torch.randn((m, k), generator=gen, device="cuda", dtype=g.torch.float32).half()
        bt = g.torch.randn((n, k), generator=gen, device="cuda", dtype=g.torch.float32).half()
        a01, b01 = oracle.zero_one_inputs(m, n, k, np.random.default_rng(m + n + k))
        truth = oracle.truth_numpy(a01, b01).view(np.uint16)
        _inputs[shape] = (a, bt, g.torch.from_numpy(a01).cuda(), g.torch.from_numpy(np.ascontiguousarray(b01.T)).cuda(), truth)
    return _inputs[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_identical_to_the_general_kernel_on_normal_inputs(g, oracle, shape):
    a, bt, *_ = inputs(g, oracle, shape)
    new, n_new = run(g, a, bt, True)
    old, n_old = run(g, a, bt, False)
    assert (n_new, n_old) == (1, 0), "the switch did not select the kernels"
    assert not np.isnan(new.view(np.float16)).any()
    assert np.array_equal(new, old), f"{int((new != old).sum())} elements differ"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_on_zero_one_inputs(g, oracle, shape):
    _, _, a01, bt01, truth = inputs(g, oracle, shape)
    got, n_new = run(g, a01, bt01, True)
    assert n_new == 1
    assert np.array_equal(got, truth), f"{int((got != truth).sum())} elements differ from the exact result"


@pytest.mark.parametrize("shape", OLD_KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_short_k_and_more_tiles_than_workgroups_stay_with_the_general_kernel(g, oracle, shape):
    _, _, a01, bt01, truth = inputs(g, oracle, shape)
    got, n_new = run(g, a01, bt01, True)
    assert n_new == 0, "the one-item kernel took a launch outside its rule"
    assert np.array_equal(got, truth)


@pytest.mark.parametrize("flags", [1, 1 | NT_STORE], ids=["plain-stores", "nt-stores"])
def test_nt_store_flag_and_padded_ldc(g, oracle, flags):
    """Both store forms, each with a C whose rows are 40 elements apart from dense (ldc % 8 == 0: still the wide epilogue)."""
    shape = (512, 768, 1024)
    a, bt, a01, bt01, truth = inputs(g, oracle, shape)
    got, n_new = run(g, a01, bt01, True, flags=flags, ldc=768 + 40)
    assert n_new == 1
    assert np.array_equal(got, truth)
    new, _ = run(g, a, bt, True, flags=flags, ldc=768 + 40)
    old, n_old = run(g, a, bt, False, flags=flags, ldc=768 + 40)
    assert n_old == 0 and np.array_equal(new, old)


def test_narrow_epilogue_and_split_plans_stay_with_the_general_kernel(g, oracle):
    shape = (512, 768, 1024)
    _, _, a01, bt01, truth = inputs(g, oracle, shape)
    got, n_new = run(g, a01, bt01, True, ldc=768 + 4)            # ldc % 8 != 0: narrow epilogue
    assert n_new == 0 and np.array_equal(got, truth)
    got, n_new = run(g, a01, bt01, True, flags=2)                # two-pass split-K
    assert n_new == 0 and np.array_equal(got, truth)
