"""Helpers for the GPU parity tests: the C ABI through ctypes, torch only for device memory."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "cuda-l2_amd"
for p in (str(REPO), str(PKG)):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402  (bench.load_library: the product's only way in, fails loudly if the .so is missing)

FORMS = ["reference", "ragged", "stream-K", "split-K", "fused", "hybrid", "plain"]   # enum Form of hgemm_api.hip

C_PAD = -3.0 * 2.0 ** -12   # prefill of C's padding: negative (no 0/1 sum is) and no multiple of 2^-10 (every dyadic sum is one)

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = bench.load_library()
        _lib.hgemm_mi355x_launch.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def gemm(a_np: np.ndarray, b_np: np.ndarray, entry: str = "fp32", plan=None, ld=None) -> np.ndarray:
    """C = A.B on the GPU through the C ABI; plan = (config_id, splits, group_m) for an explicit launch.  ld = (lda, ldb, ldc)
    (explicit plans only) places A, b_col_major and C in wider buffers: A's columns K..lda-1 and b_col_major's K..ldb-1 hold NaN
    (0 x NaN = NaN: a read of them shows in C), C's columns N..ldc-1 hold C_PAD (no result of 0/1 or dyadic operands), and every
    padding element must come back bit-unchanged.  The row-major b stays contiguous (the library reads it at stride N)."""
    L = lib()
    m, k = a_np.shape
    n = b_np.shape[1]
    assert ld is None or plan is not None, "the entry points take contiguous operands"
    lda, ldb, ldc = ld or (k, k, n)
    b = torch.from_numpy(np.ascontiguousarray(b_np)).cuda()
    a = torch.full((m, lda), float("nan"), dtype=torch.half, device="cuda")
    a[:, :k] = torch.from_numpy(np.ascontiguousarray(a_np)).cuda()
    bt = torch.full((n, ldb), float("nan"), dtype=torch.half, device="cuda")
    bt[:, :k] = b.t()
    c = torch.full((m, ldc), C_PAD, dtype=torch.half, device="cuda")
    c[:, :n] = float("nan")  # unwritten outputs stay NaN
    pads = [(x[:, w:], x[:, w:].clone()) for x, w in ((a, k), (bt, k), (c, n))]
    if plan is None:
        fn = L.hgemm_mi355x_fp16 if entry == "fp16" else L.hgemm_mi355x_fp32
        st = fn(a.data_ptr(), b.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, stream())
    else:
        st = L.hgemm_mi355x_launch(plan[0], plan[1], plan[2], a.data_ptr(), b.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n,
                                   k, lda, ldb, ldc, stream())
    assert st == 0, L.hgemm_mi355x_strerror(st)
    torch.cuda.synchronize()
    for pad, before in pads:
        assert torch.equal(pad.view(torch.int16), before.view(torch.int16)), f"padding changed (lda, ldb, ldc = {lda}, {ldb}, {ldc})"
    return c[:, :n].contiguous().cpu().numpy()


def config_names():
    L = lib()
    return [L.hgemm_mi355x_config_name(i).decode() for i in range(L.hgemm_mi355x_num_configs())]


def resolve(cfg, splits, m, n, k, lds, group=2):
    """hgemm_mi355x_launch's decision for a call with b, b_col_major and 16-byte aligned operands, nothing launched
    (hgemm_mi355x_selfcheck_launch): (status, form, [(thunk, grid, epi, splits, k_chunk, items) per dispatch])."""
    out = (ctypes.c_longlong * 28)()
    st = lib().hgemm_mi355x_selfcheck_launch(cfg, splits, group, 7, m, n, k, *lds, 0, out)
    return st, FORMS[out[0]], [tuple(out[4 + 8 * i:10 + 8 * i]) for i in range(out[1])]
