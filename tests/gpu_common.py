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


FORM_REFERENCE, FORM_SPLITK, FORM_PLAIN = 0, 3, 6            # hgemm_api.hip: enum Form
OUT_FILL = -3.0 * 2.0 ** -12                                  # prefill of everything an output buffer holds besides its M x N elements


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _place(x, ld, off=0, fill=float("nan")):
    """x [rows][cols] (cpu) at row stride ld in a device buffer of `fill`, `off` elements behind the buffer's aligned start: (flat, view)"""
    rows, cols = x.shape
    flat = torch.full((rows * ld + 8,), fill, dtype=x.dtype, device="cuda")
    view = flat[off:off + rows * ld].view(rows, ld)
    view[:, :cols] = x.cuda()
    return flat, view


class HelperKernelSet:
    """One (layout, elem, kind) kernel set of the transposed-read host path, as the checks of its two helper kernels -- the split-K
    combine and the reference kernel (hgemm_registry.hip) -- see it.  call(cfg, word, p, d, acc) launches the set's entry point with the
    device pointers p = {a, b, bias, z, c, db} and d = (m, n, k, lda, ldb, ldc, ldz) and returns its status; decide(cfg, word, d, aligned,
    acc) is the file's own `decision` -> (status, form, dispatches).  dtype: what the operands and a 16-bit C hold; a_col / b_col: A given as
    [K][M] / B given as [N][K]; c32: an fp32 C, run with every accumulate of `accs`; bias: a bf16 vector; z: "" / "in" (dact's z) / "out"
    (aux's z_out); db: dact_dbias's db32, and db_exact whether its column sums are exact in fp32 (ReLU: C is S or +0, S a multiple of 2^-7
    below 2^10, so any order of 64 adds gives the same bits) or not (the GELUs: held to (M - 1) 2^-24 sum |C| of the C read back)."""

    def __init__(self, call, decide, dtype, a_col=False, b_col=False, c32=False, bias=False, z="", db=False, db_exact=True, accs=(0,)):
        self.call, self.decide, self.dtype = call, decide, dtype
        self.a_col, self.b_col, self.c32, self.bias, self.z, self.db, self.db_exact, self.accs = a_col, b_col, c32, bias, z, db, db_exact, accs

    def operands(self, m, n, k, seed):
        """order-exact dyadic operands (oracle.bf16_dyadic_inputs, class B: every fp32 sum of products is exact in any order and grouping),
        a bias of multiples of 2^-4, a z with both signs, a non-zero old C32"""
        from oracle import hgemm_oracle as oracle
        rng = np.random.default_rng(seed)
        a, b = oracle.bf16_dyadic_inputs(m, n, k, rng, "B")
        oracle.assert_bf16_dyadic(a, b, "B")
        ops = {"a": torch.from_numpy(a).to(self.dtype), "b": torch.from_numpy(b).to(self.dtype)}
        assert np.array_equal(ops["a"].float().numpy(), a) and np.array_equal(ops["b"].float().numpy(), b)
        ops["bias"] = torch.from_numpy(rng.integers(-64, 65, size=n) / 16.0).to(torch.bfloat16)
        ops["z"] = torch.from_numpy(rng.standard_normal((m, n)) * 2.0).to(torch.bfloat16)
        ops["old"] = torch.from_numpy((2 * rng.integers(-256, 256, size=(m, n)) + 1) / 16.0).float()
        return ops

    def run(self, ops, cfg, word, want_form, lds, acc=0, misalign=False, what=""):
        """one call on `ops`; the form asserted; everything outside the outputs' M x N (and db32's N) elements must come back unchanged.
        -> {"c": bits, "z": bits, "db": fp32}"""
        a, b = ops["a"], ops["b"]
        m, k = a.shape
        n = b.shape[1]
        lda, ldb, ldc, ldz = lds
        d = (m, n, k, lda, ldb, ldc, ldz)
        st, form, disp = self.decide(cfg, word, d, not misalign, acc)
        assert (st, form) == (0, want_form), (what, st, form, disp)
        if want_form == FORM_SPLITK:
            assert disp[0][3] == word, (what, disp)
        keep = [_place(a.t() if self.a_col else a, lda, 1 if misalign else 0), _place(b.t() if self.b_col else b, ldb)]
        p = {"a": keep[0][0].data_ptr() + (2 if misalign else 0), "b": keep[1][0].data_ptr(), "bias": 0, "z": 0, "db": 0}
        c_dtype = torch.float32 if self.c32 else self.dtype
        outs = {"c": _place(ops["old"] if self.c32 else torch.full((m, n), float("nan"), dtype=c_dtype), ldc, fill=OUT_FILL)}
        p["c"] = outs["c"][0].data_ptr()
        if self.bias:
            keep.append(_place(ops["bias"][None, :], n))
            p["bias"] = keep[-1][0].data_ptr()
        if self.z == "in":
            keep.append(_place(ops["z"], ldz))
            p["z"] = keep[-1][0].data_ptr()
        elif self.z == "out":
            outs["z"] = _place(torch.full((m, n), float("nan"), dtype=torch.bfloat16), ldz, fill=OUT_FILL)
            p["z"] = outs["z"][0].data_ptr()
        if self.db:
            outs["db"] = _place(torch.full((1, n), float("nan"), dtype=torch.float32), n, fill=OUT_FILL)
            p["db"] = outs["db"][0].data_ptr()
        before = {key: flat.clone() for key, (flat, _) in outs.items()}
        inputs = [flat.clone() for flat, _ in keep]
        st = self.call(cfg, word, p, d, acc)
        torch.cuda.synchronize()
        assert st == 0, (what, st)
        got = {}
        for key, (flat, view) in outs.items():
            cols = view.shape[1] if key == "db" else n
            got[key] = view[:, :cols].cpu().clone()
            view[:, :cols] = 0
            was = before[key][:flat.numel() - 8].view(view.shape)
            was[:, :cols] = 0
            assert torch.equal(_bits(flat), _bits(before[key])), f"{what}: {key} was written outside its elements"
        assert all(torch.equal(_bits(flat), _bits(was)) for (flat, _), was in zip(keep, inputs)), f"{what}: an input changed"
        return got

    def same(self, got, want, what, db_against=None):
        for key in want:
            if key == "db" and not self.db_exact and db_against is not None:
                c = got["c"].double()
                bound = (c.shape[0] - 1) * 2.0 ** -24 * c.abs().sum(0)
                assert bool(((got["db"][0].double() - c.sum(0)).abs() <= bound).all()), f"{what}: db32 outside (M - 1) u sum |C|"
                continue
            diff = _bits(got[key]) != _bits(want[key])
            assert not bool(diff.any()), f"{what}: {key} differs in {int(diff.sum())} of {diff.numel()} elements, first at {tuple(diff.nonzero()[0].tolist())}"

    def check_combine(self, k, splits, seed):
        """The 64 x 64 member (config 0), M = N = 64, ldc = 72, ldz = 80, `splits` two-pass splits of one K stage each: C (and z_out, db32)
        of the split call equals the unsplit call and the reference-kernel call (a 2-byte aligned A) bit for bit.  K = 128 / 2 splits runs
        the combine's remainder loop only, K = 704 / 11 splits one unrolled block of eight and two remainder slabs."""
        m = n = 64
        assert k == 64 * splits
        ops = self.operands(m, n, k, seed)
        lds = (m if self.a_col else k, k if self.b_col else n, 72, 80)
        for acc in self.accs:
            what = f"{m}x{n}x{k} acc {acc}"
            plain = self.run(ops, 0, 1, FORM_PLAIN, lds, acc, what=what + " unsplit")
            split = self.run(ops, 0, splits, FORM_SPLITK, lds, acc, what=what + f" {splits} splits")
            ref = self.run(ops, 0, splits, FORM_REFERENCE, lds, acc, misalign=True, what=what + " reference")
            self.same(split, ref, what + ": split against reference")         # (db32: both are the direct column sum of the same C)
            self.same(plain, split, what + ": unsplit against split", db_against=True)
            assert not bool(torch.isnan(split["c"].float()).any())

    def check_reference(self, seed):
        """M = 5, N = 12, K = 24 on padded strides: outside every kernel's scope, so the reference kernel answers.  Expected: the same
        operands zero-padded to 64 x 64 x 64 (exact: zeros add nothing) through the 64 x 64 member's unsplit kernel, whose top-left
        5 x 12 the reference kernel must give bit for bit; an fp32 C once with accumulate = 1 on a non-zero C."""
        m, n, k = 5, 12, 24
        ops = self.operands(m, n, k, seed)
        big = {"a": torch.zeros(64, 64, dtype=self.dtype), "b": torch.zeros(64, 64, dtype=self.dtype), "bias": torch.zeros(64, dtype=torch.bfloat16),
               "z": torch.zeros(64, 64, dtype=torch.bfloat16), "old": torch.full((64, 64), 0.5)}
        big["a"][:m, :k], big["b"][:k, :n], big["bias"][:n], big["z"][:m, :n], big["old"][:m, :n] = ops["a"], ops["b"], ops["bias"], ops["z"], ops["old"]
        for acc in self.accs:
            what = f"{m}x{n}x{k} acc {acc}"
            want = self.run(big, 0, 1, FORM_PLAIN, (64, 64, 72, 80), acc, what=what + " padded to the member")
            want = {key: v[:m if key != "db" else 1, :n] for key, v in want.items()}
            got = self.run(ops, 0, 1, FORM_REFERENCE, ((m if self.a_col else k) + 3, (k if self.b_col else n) + 5, n + 7, n + 9), acc, what=what + " reference")
            self.same(got, want, what + ": reference against the member kernel", db_against=True)


def config_names():
    L = lib()
    return [L.hgemm_mi355x_config_name(i).decode() for i in range(L.hgemm_mi355x_num_configs())]


def resolve(cfg, splits, m, n, k, lds, group=2):
    """hgemm_mi355x_launch's decision for a call with b, b_col_major and 16-byte aligned operands, nothing launched
    (hgemm_mi355x_selfcheck_launch): (status, form, [(thunk, grid, epi, splits, k_chunk, items) per dispatch])."""
    out = (ctypes.c_longlong * 28)()
    st = lib().hgemm_mi355x_selfcheck_launch(cfg, splits, group, 7, m, n, k, *lds, 0, out)
    return st, FORMS[out[0]], [tuple(out[4 + 8 * i:10 + 8 * i]) for i in range(out[1])]
