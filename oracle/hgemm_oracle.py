"""TEST INFRASTRUCTURE ONLY -- CPU oracle of the CUDA-L2 HGEMM hot path (numpy + ctypes over
hgemm_oracle.c).  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this module; the product (cuda-l2_amd/) never does.

Restated rules (reference file:line):
  truth_f32acc          zero_one_correctness_check.py:85-90   (a.float() @ b.float()).half()
  zero_one_values       zero_one_correctness_check.py:65-73   {0,1} / {0,0,1} beyond 8192
  mask / max diff       zero_one_correctness_check.py:92,167-172
  guard bars            zero_one_correctness_check.py:98-150  (16384 elements either side)
  pass rule             zero_one_correctness_check.py:263-268 (average max-diff == 0.0 exactly)
  as_col_major          tools/utils.py:110-115
  padding               tools/utils.py:8-36, benchmarking_offline.py:102-113
  TFLOPS                benchmarking_utils.py:66              2*m*n*k*1e-12*1000/ms (unpadded sizes)
  -max row              summarize_result.py:43-53             lower cuda_l2 speedup of tn/nn
Parity pinning: see hgemm_oracle.c header and tests/golden/make_golden.py.
Of this project, not restated: dyadic_inputs / truth_exact and the three wrong-rounding mutants (the rounding tests).
Likewise bf16_dyadic_inputs / bf16_exact_product and their mutants (the bf16 rounding bars of tests/test_gpu_tn_bars.py).
"""
from __future__ import annotations

import ctypes
import math
import re
import subprocess
from pathlib import Path

import numpy as np

ORACLE_DIR = Path(__file__).resolve().parent
BAR_SIZE = 16384
MAX_EXACT_FP16_INT = 2047.0

_lib = None


def build(force: bool = False) -> Path:
    """Compile hgemm_oracle.c with gcc (seconds); returns the .so path."""
    so = ORACLE_DIR / "libhgemm_oracle.so"
    src = ORACLE_DIR / "hgemm_oracle.c"
    if force or not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
        subprocess.run(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return so


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(str(build()))
        u16p = ctypes.POINTER(ctypes.c_uint16)
        for name in ("hgemm_oracle_f32acc", "hgemm_oracle_f32acc_tn", "hgemm_oracle_f16acc"):
            getattr(_lib, name).argtypes = [u16p, u16p, u16p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
            getattr(_lib, name).restype = None
        _lib.hgemm_oracle_as_col_major.argtypes = [u16p, u16p, ctypes.c_int, ctypes.c_int]
        _lib.hgemm_oracle_masked_max_diff.argtypes = [u16p, u16p, ctypes.c_size_t]
        _lib.hgemm_oracle_masked_max_diff.restype = ctypes.c_float
        _lib.hgemm_oracle_half_to_float.argtypes = [ctypes.c_uint16]
        _lib.hgemm_oracle_half_to_float.restype = ctypes.c_float
        _lib.hgemm_oracle_float_to_half.argtypes = [ctypes.c_float]
        _lib.hgemm_oracle_float_to_half.restype = ctypes.c_uint16
    return _lib


def _u16(x: np.ndarray):
    assert x.dtype == np.float16 and x.flags["C_CONTIGUOUS"]
    return x.view(np.uint16).ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))


def _gemm(name: str, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float16)
    b = np.ascontiguousarray(b, dtype=np.float16)
    m, k = a.shape
    k2, n = b.shape
    assert k == k2
    c = np.empty((m, n), dtype=np.float16)
    getattr(lib(), name)(_u16(a), _u16(b), _u16(c), m, n, k)
    return c


def truth_f32acc(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """C restatement: fp32 accumulate in k order, one RNE rounding to fp16."""
    return _gemm("hgemm_oracle_f32acc", a, b)


def truth_f32acc_tn(a: np.ndarray, bt: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float16)
    bt = np.ascontiguousarray(bt, dtype=np.float16)
    m, k = a.shape
    n, k2 = bt.shape
    assert k == k2
    c = np.empty((m, n), dtype=np.float16)
    lib().hgemm_oracle_f32acc_tn(_u16(a), _u16(bt), _u16(c), m, n, k)
    return c


def truth_f16acc(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return _gemm("hgemm_oracle_f16acc", a, b)


def truth_numpy(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """numpy restatement (BLAS summation order): the fast oracle for large sizes."""
    return (a.astype(np.float32) @ b.astype(np.float32)).astype(np.float16)


def truth_prefix_k(a: np.ndarray, b: np.ndarray, ks):
    """Truths of ALL K-prefixes of one {0,1} problem, for sweeping many (M,N,K) shapes with one pair of
    operands: yields (K, truth_K) for K in ascending `ks`, truth_K = (a[:, :K].float() @ b[:K, :].float()).half()
    (zero_one_correctness_check.py:85-90), and the truth of the sub-problem (M, N, K) is truth_K[:M, :N].
    Only valid for 0/1 operands: every partial sum is an integer <= K < 2**24, exact in fp32 whatever the
    summation order, so accumulating the K-slices incrementally is bit-identical to the one-shot product
    (pinned in tests/test_oracle.py); total work 2*M*N*max(ks) instead of 2*M*N*sum(ks)."""
    assert a.dtype == np.float16 and b.dtype == np.float16
    ks = sorted(set(int(k) for k in ks))
    assert ks and ks[-1] <= a.shape[1] == b.shape[0] and ks[-1] < 2 ** 24
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    k0 = 0
    for k in ks:
        if k > k0:
            sa, sb = a[:, k0:k] , b[k0:k, :]
            assert ((sa == 0) | (sa == 1)).all() and ((sb == 0) | (sb == 1)).all(), "truth_prefix_k is exact for {0,1} inputs only"
            acc += sa.astype(np.float32) @ sb.astype(np.float32)
            k0 = k
        yield k, acc.astype(np.float16)


def as_col_major(b: np.ndarray) -> np.ndarray:
    """[K,N] array -> array of the SAME shape whose memory is b^T (= reference as_col_major)."""
    return np.ascontiguousarray(b.T).reshape(b.shape)


def zero_one_values(m: int, n: int, k: int) -> np.ndarray:
    return np.array([0.0, 1.0] if max(m, n, k) <= 8192 else [0.0, 0.0, 1.0], dtype=np.float16)


def zero_one_inputs(m: int, n: int, k: int, rng: np.random.Generator, force_sparse: bool | None = None):
    vals = zero_one_values(m, n, k) if force_sparse is None else np.array(
        [0.0, 0.0, 1.0] if force_sparse else [0.0, 1.0], dtype=np.float16)
    a = vals[rng.integers(0, len(vals), size=(m, k))]
    b = vals[rng.integers(0, len(vals), size=(k, n))]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


DYADIC_MAX_K = 8160   # K x (1 + 3 x 2^-10) < 2^13: every partial sum is a multiple of 2^-10 below 2^13, at most 23 significant bits


def dyadic_inputs(m: int, n: int, k: int, rng: np.random.Generator):
    """Operands whose sums are exact in fp32 in ANY order and grouping, yet need a real rounding to fp16 (0/1 sums never do):
    A in {-1, 0, 1}, B = z x (1 + e x 2^-10) with z in {0, 1}, e in {0, 1, 2, 3}, all uniform.  Every product is 0 or
    +-(1 + e / 1024); a sum of any subset of K <= 8160 of them is a multiple of 2^-10 below 2^13.  Results are ~sqrt(K / 3) in
    size, where fp16 spacing is 2^-9 ... 2^-4: most need rounding, many are exact ties, about half are negative."""
    assert k <= DYADIC_MAX_K
    a = rng.integers(-1, 2, size=(m, k)).astype(np.float16)
    z = rng.integers(0, 2, size=(k, n))
    e = rng.integers(0, 4, size=(k, n))
    b = (z * (1024 + e) / 1024.0).astype(np.float16)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def assert_dyadic(a: np.ndarray, b: np.ndarray) -> None:
    """The class of dyadic_inputs, on which truth_exact's claim (and that of any fp32 accumulation order) rests."""
    assert a.dtype == np.float16 and b.dtype == np.float16 and a.shape[1] == b.shape[0]
    assert a.shape[1] <= DYADIC_MAX_K, f"K = {a.shape[1]} > {DYADIC_MAX_K}: a partial sum may need more than 24 bits"
    assert np.isin(a, (-1.0, 0.0, 1.0)).all(), "A must hold -1 / 0 / 1 only"
    b1024 = b.astype(np.float64) * 1024.0
    assert (b1024 == np.floor(b1024)).all() and ((b1024 == 0) | ((b1024 >= 1024) & (b1024 <= 1027))).all(), \
        "B must hold 0 or 1 + e / 1024, e in 0 ... 3, only"


def exact_product(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    assert_dyadic(a, b)
    return a.astype(np.float64) @ b.astype(np.float64)   # 23-bit sums: exact in fp64 whatever the BLAS order


def truth_exact(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The one right answer for dyadic operands: the exact product, rounded to fp16 once (astype: round-to-nearest-even)."""
    return exact_product(a, b).astype(np.float16)


def round_toward_zero(x: np.ndarray) -> np.ndarray:
    """MUTANT: fp64 -> fp16 by truncation (finite values inside the fp16 range)."""
    x = np.asarray(x, dtype=np.float64)
    h = x.astype(np.float16)
    return np.where(np.abs(h.astype(np.float64)) > np.abs(x), np.nextafter(h, np.float16(0)), h)


def round_half_away(x: np.ndarray) -> np.ndarray:
    """MUTANT: fp64 -> fp16 to nearest, ties away from zero (finite values inside the fp16 range; the distances to the two
    fp16 neighbours must be exact in fp64, as they are for dyadic sums)."""
    x = np.asarray(x, dtype=np.float64)
    lo = round_toward_zero(x)
    hi = np.nextafter(lo, np.where(x < 0, -np.inf, np.inf).astype(np.float16))
    up = (x != lo) & (np.abs(hi.astype(np.float64) - x) <= np.abs(x - lo.astype(np.float64)))
    return np.where(up, hi, lo)


def fp16_partials(a: np.ndarray, b: np.ndarray, cuts) -> np.ndarray:
    """MUTANT: a split-K whose partials are held in fp16 -- the exact sum of every K chunk [0, cuts[0]), [cuts[0], cuts[1]), ...
    rounded to fp16, the chunks added in fp32, the total rounded once more."""
    assert_dyadic(a, b)
    edges = [0] + [int(c) for c in cuts] + [a.shape[1]]
    assert all(lo < hi for lo, hi in zip(edges, edges[1:])), edges
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for lo, hi in zip(edges, edges[1:]):
        acc += truth_exact(a[:, lo:hi], b[lo:hi]).astype(np.float32)
    return acc.astype(np.float16)


# ---- order-exact bfloat16 operands with live mantissa bits (the bf16 rounding bars: tests/test_gpu_tn_bars.py) ------------------
# numpy has no bfloat16: a bf16 operand is an fp32 array whose low 16 bits are clear, a bf16 result a uint16 array of bit patterns.
BF16_DYADIC_GRANULARITY = {"A": 2.0 ** -7, "B": 2.0 ** -7, "AB": 2.0 ** -14}


def bf16_dyadic_inputs(m: int, n: int, k: int, rng: np.random.Generator, side: str):
    """dyadic_inputs for bfloat16, whose significand has 7 stored bits: the two lowest of them live in B ("B"), in A ("A") or in both
    ("AB").  "B": A in {-1, 0, 1}, B = z x (1 + e x 2^-7), z in {0, 1}, e in 0 .. 3.  "A": the mirror, A = s x (1 + f x 2^-7) with
    the signs kept in A, B in {0, 1}.  "AB": A = s x (1 + f x 2^-7), B = z x (1 + e x 2^-7), products multiples of 2^-14.  All draws
    uniform.  The sums are exact in fp32 in any order and grouping while sum |a| |b| stays below 2^23 granules: assert_bf16_dyadic
    asserts that on the operands it is given; no K is promised here.  Returns fp32 arrays of bf16 values."""
    assert side in BF16_DYADIC_GRANULARITY, side
    s = rng.integers(-1, 2, size=(m, k)).astype(np.float64)
    f = rng.integers(0, 4, size=(m, k)) if side in ("A", "AB") else 0
    z = rng.integers(0, 2, size=(k, n)).astype(np.float64)
    e = rng.integers(0, 4, size=(k, n)) if side in ("B", "AB") else 0
    a = (s * (128 + f) / 128.0).astype(np.float32)
    b = (z * (128 + e) / 128.0).astype(np.float32)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def is_bf16(x: np.ndarray) -> bool:
    return x.dtype == np.float32 and not (np.ascontiguousarray(x).view(np.uint32) & 0xFFFF).any()


def bf16_dyadic_bits(a: np.ndarray, b: np.ndarray, side: str) -> float:
    """log2 of the largest sum |a| |b| of an element of C, in granules of the class: the significant bits its partial sums may need."""
    return float(np.log2((np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))).max() / BF16_DYADIC_GRANULARITY[side]))


def assert_bf16_dyadic(a: np.ndarray, b: np.ndarray, side: str) -> None:
    """The class of bf16_dyadic_inputs and the exactness rule DYADIC_MAX_K rests on, asserted on the actual operands: every product is a
    whole number of granules, so every partial sum of every order is one, of magnitude <= sum |a| |b| < 2^23 granules: 23 significant bits."""
    assert is_bf16(a) and is_bf16(b) and a.shape[1] == b.shape[0], "operands must be fp32 arrays of bf16 values"
    a128, b128 = np.abs(a.astype(np.float64)) * 128.0, b.astype(np.float64) * 128.0
    top_a, top_b = (131 if side in ("A", "AB") else 128), (131 if side in ("B", "AB") else 128)
    assert (a128 == np.floor(a128)).all() and ((a128 == 0) | ((a128 >= 128) & (a128 <= top_a))).all(), f"class {side}: A must hold 0 or +-(1 + f / 128), f <= {top_a - 128}"
    assert (b128 == np.floor(b128)).all() and ((b128 == 0) | ((b128 >= 128) & (b128 <= top_b))).all(), f"class {side}: B must hold 0 or 1 + e / 128, e <= {top_b - 128}"
    worst = (np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))).max() / BF16_DYADIC_GRANULARITY[side]
    assert worst < 2.0 ** 23, f"class {side}, K = {a.shape[1]}: a partial sum may need {np.log2(worst):.1f} > 23 significant bits"


def bf16_exact_product(a: np.ndarray, b: np.ndarray, side: str) -> np.ndarray:
    """The exact product as fp32 (the fp64 BLAS product of 23-bit sums is exact in any order; the cast is asserted exact)."""
    assert_bf16_dyadic(a, b, side)
    x = a.astype(np.float64) @ b.astype(np.float64)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x), "the exact product is no fp32 matrix"
    return x32


def bf16_roundings(x32: np.ndarray):
    """An fp32 matrix (finite, inside the bf16 range) as bf16 bit patterns under three roundings: (nearest even, truncation, nearest
    with ties away from zero).  The first is the right one; the other two are MUTANTS."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    keep = u >> 16
    return ((u + 0x7FFF + (keep & 1)) >> 16).astype(np.uint16), keep.astype(np.uint16), ((u + 0x8000) >> 16).astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_partials(a: np.ndarray, b: np.ndarray, side: str, cuts, bias=None) -> np.ndarray:
    """MUTANT: a split-K whose slabs are held in bf16 -- the exact sum of every K chunk rounded to bf16, the chunks added in fp32 in
    split order, the bias (if any) added last, the total rounded once more.  Bit patterns."""
    edges = [0] + [int(c) for c in cuts] + [a.shape[1]]
    assert all(lo < hi for lo, hi in zip(edges, edges[1:])), edges
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for lo, hi in zip(edges, edges[1:]):
        acc += bf16_to_f32(bf16_roundings(bf16_exact_product(a[:, lo:hi], b[lo:hi], side))[0])
    return bf16_roundings(acc if bias is None else acc + bias[None, :].astype(np.float32))[0]


def masked_max_diff(out: np.ndarray, truth: np.ndarray) -> float:
    diff = np.abs(out.astype(np.float32) - truth.astype(np.float32))
    diff[np.abs(truth.astype(np.float32)) > MAX_EXACT_FP16_INT] = 0.0
    return float(diff.max()) if diff.size else 0.0


def check_passes(max_diffs) -> bool:
    """Pass rule of the reference: the AVERAGE of the per-iteration max diffs is exactly 0.0."""
    return len(max_diffs) > 0 and (sum(max_diffs) / len(max_diffs)) == 0.0


def relative_error(out: np.ndarray, ref_f32: np.ndarray) -> float:
    """max|out - ref| / max|ref| : the tolerance metric for N(0,1) inputs (BASELINE.json: 1e-3 rel with
    fp32 accumulate, 1e-2 rel with fp16 accumulate)."""
    ref = ref_f32.astype(np.float64)
    return float(np.max(np.abs(out.astype(np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-30))


def extract_bm_bk_bn(text: str):
    found = {"BM": -1, "BN": -1, "BK": -1}
    for raw in text.split("\n"):
        m = re.search(r"(BM|BN|BK)\s*=\s*Int<(\d+)>", raw.strip().replace(" ", ""))
        if m:
            found[m.group(1)] = int(m.group(2))
    if min(found.values()) > 0:
        return found["BM"], found["BK"], found["BN"]
    return -1, -1, -1


def paddings(m: int, n: int, k: int, text: str):
    bm, bk, bn = extract_bm_bk_bn(text)
    if bm > 0:
        return (math.ceil(m / bm) * bm - m, math.ceil(k / bk) * bk - k, math.ceil(n / bn) * bn - n)
    return 0, 0, 0


def tflops(m: int, n: int, k: int, ms: float) -> float:
    return (2 * m * n * k) * 1e-12 * 1000 / ms


def max_row(tn: dict, nn: dict) -> dict:
    """summarize_result.py:43-53: the variant with the LOWER cuda_l2 speedup."""
    return tn if tn["Speedup"] < nn["Speedup"] else nn
