"""Pins the CPU oracle (oracle/) against the fixtures generated from the reference
(tests/golden/make_golden.py) and checks the product's host-side helpers against the same fixtures."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import hgemm_oracle as oracle

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "hgemm_golden.npz"), json.loads((GOLDEN / "harness_golden.json").read_text())


def _cases(prefix):
    meta = json.loads((GOLDEN / "harness_golden.json").read_text())
    return [c for c in meta["cases"] if c.startswith(prefix)]


@pytest.mark.parametrize("case", _cases("zo_"))
def test_zero_one_truth_is_bit_exact(gold, case):
    npz, _ = gold
    a, b, truth = npz[case + "_a"], npz[case + "_b"], npz[case + "_truth"]
    # integer partial sums: any summation order gives the same bits wherever |truth| <= 2047 ...
    for got in (oracle.truth_f32acc(a, b), oracle.truth_numpy(a, b), oracle.truth_f32acc_tn(a, np.ascontiguousarray(b.T))):
        assert oracle.masked_max_diff(got, truth) == 0.0
    # ... and here even beyond (fp32 holds integers up to 2^24 exactly, the fp16 rounding is shared)
    assert np.array_equal(oracle.truth_f32acc(a, b).view(np.uint16), truth.view(np.uint16))


def test_mask_rule_hides_values_above_2047(gold):
    npz, _ = gold
    truth = npz["zo_masked_4_8_4096_truth"]
    assert float(truth.min()) == 4096.0
    wrong = np.zeros_like(truth)                      # maximally wrong output
    assert oracle.masked_max_diff(wrong, truth) == 0.0  # ... is invisible: every entry is masked
    assert oracle.lib().hgemm_oracle_masked_max_diff(oracle._u16(wrong), oracle._u16(np.ascontiguousarray(truth)),
                                                     truth.size) == 0.0
    half = truth.copy()
    half[:] = 2047.0
    assert oracle.masked_max_diff(np.zeros_like(half), half) == 2047.0  # 2047 itself is NOT masked


@pytest.mark.parametrize("case", _cases("randn_"))
def test_randn_truth_within_one_ulp_and_tolerances(gold, case):
    npz, _ = gold
    a, b, truth, f32 = npz[case + "_a"], npz[case + "_b"], npz[case + "_truth"], npz[case + "_f32"]
    got = oracle.truth_f32acc(a, b)
    # fp32 summation order differs between the C loop and torch's BLAS, so a few results land on the
    # neighbouring fp16 value (more than one ulp only where the dot product cancels to ~0)
    assert (got.view(np.uint16) == truth.view(np.uint16)).mean() > 0.97
    assert oracle.relative_error(got, truth.astype(np.float32)) <= 2.0 ** -10
    # the tolerance contract of BASELINE.json: 1e-3 rel (fp32 accumulate), 1e-2 rel (fp16 accumulate)
    assert oracle.relative_error(got, f32) <= 1e-3
    assert oracle.relative_error(oracle.truth_f16acc(a, b), f32) <= 1e-2
    assert oracle.relative_error(oracle.truth_f16acc(a, b), f32) > oracle.relative_error(got, f32)


@pytest.mark.parametrize("name", ["acm_3_5", "acm_64_16", "acm_1_7"])
def test_as_col_major_matches_reference(gold, name):
    npz, _ = gold
    x, y = npz[name + "_x"], npz[name + "_y"]
    assert np.array_equal(oracle.as_col_major(x), y)
    from tools.utils import as_col_major  # the product's torch implementation

    got = as_col_major(torch.from_numpy(x))
    assert got.is_contiguous() and tuple(got.shape) == x.shape
    assert np.array_equal(got.numpy(), y)
    k, n = x.shape  # the memory of the result is x^T
    assert np.array_equal(got.numpy().reshape(-1), np.ascontiguousarray(x.T).reshape(-1))
    bt = np.empty((n, k), dtype=np.float16)
    oracle.lib().hgemm_oracle_as_col_major(oracle._u16(np.ascontiguousarray(x)), oracle._u16(bt), k, n)
    assert np.array_equal(bt.reshape(-1), y.reshape(-1))


def test_tile_regex_and_padding_match_reference(gold):
    _, meta = gold
    from tools.utils import compute_padding, extract_bm_bk_bn

    for name, text in meta["snippets"].items():
        want = tuple(meta["extract_bm_bk_bn"][name])
        assert oracle.extract_bm_bk_bn(text) == want, name
        assert extract_bm_bk_bn(text) == want, name
    text = meta["snippets"]["cute_style"]  # BM=128, BK=32, BN=160
    assert oracle.paddings(4096, 4096, 4096, text) == (0, 0, 64)
    assert compute_padding(4096, 4096, 4096, text) == (0, 0, 64)
    assert compute_padding(64, 4096, 64, text) == (64, 0, 64)
    assert compute_padding(64, 4096, 64, meta["snippets"]["mi355x_shape_file"]) == (0, 0, 0)


def test_pass_rule_and_generator():
    assert oracle.check_passes([0.0, 0.0]) and not oracle.check_passes([0.0, 1.0]) and not oracle.check_passes([])
    assert list(oracle.zero_one_values(64, 4096, 8192)) == [0.0, 1.0]
    assert list(oracle.zero_one_values(64, 12288, 64)) == [0.0, 0.0, 1.0]
    rng = np.random.default_rng(3)
    a, b = oracle.zero_one_inputs(16, 16, 512, rng, force_sparse=True)
    assert set(np.unique(a)) <= {0.0, 1.0} and 0.2 < a.mean() < 0.45
    assert oracle.tflops(4096, 4096, 4096, 0.1) == pytest.approx(1374.39, rel=1e-4)


def test_half_conversions_are_exact():
    L = oracle.lib()
    for h in range(0, 65536, 13):
        f = L.hgemm_oracle_half_to_float(h)
        e = float(np.array([h], dtype=np.uint16).view(np.float16)[0])
        assert f == e or (f != f and e != e)
    rng = np.random.default_rng(0)
    vals = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 5, 4000)).astype(np.float32)
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    got = np.array([L.hgemm_oracle_float_to_half(float(v)) for v in vals], dtype=np.uint16)
    assert np.array_equal(got, want)


def test_prefix_k_truths_are_bit_identical_to_the_one_shot_oracle():
    """tests/tools/verify_plans.py sweeps the 1000-shape grid with one operand pair per input class and the
    incremental K-prefix truths; for 0/1 inputs they must equal the C restatement bit for bit."""
    rng = np.random.default_rng(3)
    for sparse in (False, True):
        a, b = oracle.zero_one_inputs(96, 80, 640, rng, force_sparse=sparse)
        ks = [64, 128, 320, 640]
        seen = []
        for k, t in oracle.truth_prefix_k(a, b, ks):
            seen.append(k)
            for (m, n) in [(96, 80), (33, 17), (64, 64)]:
                ref = oracle.truth_f32acc(np.ascontiguousarray(a[:m, :k]), np.ascontiguousarray(b[:k, :n]))
                assert np.array_equal(t[:m, :n].view(np.uint16), ref.view(np.uint16))
        assert seen == ks
    with pytest.raises(AssertionError):
        list(oracle.truth_prefix_k(np.full((4, 64), 0.5, np.float16), np.ones((64, 4), np.float16), [64]))


# ---- dyadic operands: the inputs of tests/test_gpu_rounding.py, proved on the CPU ----------------------------------------------
@pytest.fixture(scope="module")
def rounding_cases():
    """The very operands of the GPU rounding tests (same seed, shape and K list, from the same table reader) at every K
    they run, each with every K cut a kernel makes there: the host's 2-way and 3-way stage cuts of the geometries that run
    that K, and the stream-K cuts.  The table is read through the C ABI and the launch-decision hook, no GPU."""
    import build

    build.build_library()
    import gpu_common
    import test_gpu_rounding as R

    geos = R.read_table(gpu_common)
    sk = R.table_cuts(geos)
    m, n, ks = R.table_extent(geos, sk)
    ops = R.DyadicOperands(oracle, m, n, ks, R.SEED)
    cases = []
    for k in ks:
        cuts = {tuple(R.stage_cuts(k, geo.stage, ways)) for geo in geos if k in R.rounding_ks(geo) for ways in (2, 3)}
        cuts |= {tuple(at) for kk, at in sk.values() if kk == k}
        assert cuts and all(cuts), (k, cuts)
        cases.append((*ops.sub(m, n, k), sorted(cuts)))
    return cases


def test_dyadic_truth_is_the_same_in_every_fp32_summation_order(rounding_cases):
    """truth_exact (fp64, exact) equals the C oracle's k-order fp32 accumulation, numpy's BLAS order, and an fp32 accumulation
    over a random permutation of K cut into uneven chunks: whatever order a kernel sums in, there is one right answer."""
    rng = np.random.default_rng(9)
    for a, b, truth, _ in rounding_cases:
        k = a.shape[1]
        assert np.array_equal(oracle.truth_exact(a, b).view(np.uint16), truth.view(np.uint16))
        assert np.array_equal(oracle.truth_f32acc(a, b).view(np.uint16), truth.view(np.uint16))
        assert np.array_equal(oracle.truth_numpy(a, b).view(np.uint16), truth.view(np.uint16))
        perm = rng.permutation(k)
        edges = [0] + sorted(rng.choice(np.arange(1, k), size=6, replace=False).tolist()) + [k]
        acc = np.zeros(truth.shape, dtype=np.float32)
        for lo, hi in reversed(list(zip(edges, edges[1:]))):
            part = np.zeros(truth.shape, dtype=np.float32)
            for kk in perm[lo:hi]:
                part += np.outer(a[:, kk].astype(np.float32), b[kk].astype(np.float32))   # one fp32 add per product, this order
            acc += part
        assert np.array_equal(acc.astype(np.float64), oracle.exact_product(a, b))       # no fp32 add ever rounded
        assert np.array_equal(acc.astype(np.float16).view(np.uint16), truth.view(np.uint16))


def test_dyadic_operands_discriminate_in_every_16x16_block(rounding_cases):
    """Conditions on the inputs, not measurements of a kernel: every whole 16x16 block of C (the footprint of one MFMA tile: all
    lanes, all accumulator registers) holds an element that a truncating convert gets wrong, one that round-half-away gets
    wrong, and one that fp16-held partials of each host cut get wrong; a tenth of C and more is negative and inexact."""
    def every_block(differs):
        mm, nn = differs.shape[0] // 16 * 16, differs.shape[1] // 16 * 16
        return differs[:mm, :nn].reshape(mm // 16, 16, nn // 16, 16).any(axis=(1, 3)).all()

    for a, b, truth, cut_sets in rounding_cases:
        x = oracle.exact_product(a, b)
        assert every_block(oracle.round_toward_zero(x) != truth), "RTZ"
        assert every_block(oracle.round_half_away(x) != truth), "half-away"
        for cuts in cut_sets:
            assert every_block(oracle.fp16_partials(a, b, cuts) != truth), cuts
        assert ((x < 0) & (truth.astype(np.float64) != x)).mean() >= 0.10


def test_dyadic_mutants_round_as_they_say():
    """The three wrong roundings on hand-made values: ties, both signs, exact values, the first integer fp16 cannot hold."""
    x = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2049.0, -2049.0, 1.0, 0.0, 1 + 2.0 ** -12, 1 + 2.0 ** -11 + 2.0 ** -20,
                  -(1 + 2.0 ** -10 - 2.0 ** -20)])
    e = 2.0 ** -10
    assert x.astype(np.float16).tolist() == [1.0, 1 + 2 * e, -1.0, 2048.0, -2048.0, 1.0, 0.0, 1.0, 1 + e, -(1 + e)]
    assert oracle.round_half_away(x).tolist() == [1 + e, 1 + 2 * e, -(1 + e), 2050.0, -2050.0, 1.0, 0.0, 1.0, 1 + e, -(1 + e)]
    assert oracle.round_toward_zero(x).tolist() == [1.0, 1 + e, -1.0, 2048.0, -2048.0, 1.0, 0.0, 1.0, 1.0, -1.0]
    assert oracle.round_toward_zero(x).dtype == oracle.round_half_away(x).dtype == np.float16
    # 1 + (1 + e) = 2 + e is a tie and rounds to 2; (1 + e) + (1 + e) is exact: the fp16-held halves give 4 + 2e -> 4, the truth is 4 + 3e -> 4 + 4e
    a = np.ones((1, 4), np.float16)
    b = np.array([[1.0], [1 + e], [1 + e], [1 + e]], np.float16)
    assert oracle.truth_exact(a, b)[0, 0] == 4 + 4 * e and oracle.fp16_partials(a, b, [2])[0, 0] == 4.0
    assert oracle.fp16_partials(a, b, [])[0, 0] == 4 + 4 * e


def test_dyadic_class_assertion_rejects_what_would_break_exactness():
    rng = np.random.default_rng(5)
    a, b = oracle.dyadic_inputs(8, 8, 64, rng)
    oracle.truth_exact(a, b)
    bad = b.copy()
    bad[3, 3] = 1 + 4 / 1024                    # e = 4
    for wrong_b in (bad, np.where(b == 0, np.float16(0.5), b), np.where(b == 0, np.float16("nan"), b)):
        with pytest.raises(AssertionError):
            oracle.truth_exact(a, wrong_b)
    with pytest.raises(AssertionError):
        oracle.truth_exact(np.where(a == 0, np.float16(2), a), b)
    a1 = np.ones((1, 8161), np.float16)
    b1 = np.ones((8161, 1), np.float16)
    oracle.truth_exact(a1[:, :8160], b1[:8160])
    with pytest.raises(AssertionError):
        oracle.truth_exact(a1, b1)               # K = 8161
    with pytest.raises(AssertionError):
        oracle.dyadic_inputs(1, 1, 8161, rng)


# ---- dyadic operands of the NN layout's rounding tests (tests/test_gpu_nn_bars.py), proved on the CPU ---------------------------
@pytest.fixture(scope="module")
def nn_rounding_cases():
    """The very operands of tests/test_gpu_nn_bars.py's rounding tests (same seeds, shapes and K, the members read through the C
    ABI, no GPU): per case the sub-block the GPU test runs, its truth, and the K cuts of every two-pass form run there."""
    import ctypes

    import build

    lib = ctypes.CDLL(str(build.build_library()))
    import test_gpu_nn_bars as B

    infos = B.nn_infos(lib)
    assert B.member_extent(infos) == (152, 152, [192, 256, 320, 8128]) and B.SEED == 601
    sets = [(B.DyadicOperands(oracle, *B.member_extent(infos), B.SEED), B.member_cases(infos)),
            (B.DyadicOperands(oracle, *B.planned_extent(), B.PLANNED_SEED), B.planned_cases())]
    cases = [(*ops.sub(m, n, k), cuts) for ops, plan in sets for (m, n, k), cuts in sorted(plan.items())]
    assert len(cases) == len(B.member_cases(infos)) + len(B.PLANNED) and any(cuts for *_, cuts in cases)
    return cases


def test_nn_dyadic_truth_is_the_same_in_every_fp32_summation_order(nn_rounding_cases):
    """As test_dyadic_truth_is_the_same_in_every_fp32_summation_order, on the NN tests' operands: the exact truth equals the C
    oracle's k-order fp32 accumulation, numpy's BLAS order, and the two-pass form's own order -- fp32 chunk sums added in split
    order -- at every cut used, with no fp32 add ever rounding."""
    for a, b, truth, cut_sets in nn_rounding_cases:
        k = a.shape[1]
        x = oracle.exact_product(a, b)
        assert np.array_equal(oracle.truth_exact(a, b).view(np.uint16), truth.view(np.uint16))
        assert np.array_equal(oracle.truth_numpy(a, b).view(np.uint16), truth.view(np.uint16))
        if k <= 512:
            assert np.array_equal(oracle.truth_f32acc(a, b).view(np.uint16), truth.view(np.uint16))
        for cuts in cut_sets + [()]:
            edges = [0, *cuts, k]
            acc = np.zeros(truth.shape, dtype=np.float32)
            for lo, hi in zip(edges, edges[1:]):
                part = a[:, lo:hi].astype(np.float32) @ b[lo:hi].astype(np.float32)
                assert np.array_equal(part.astype(np.float64), oracle.exact_product(a[:, lo:hi], b[lo:hi]))
                acc += part
            assert np.array_equal(acc.astype(np.float64), x) and np.array_equal(acc.astype(np.float16).view(np.uint16), truth.view(np.uint16))


def test_nn_dyadic_operands_discriminate_in_every_16x16_block(nn_rounding_cases):
    """Conditions on the inputs: in every case, every 16 x 16 block of C -- the partial blocks at the right and bottom edges
    included -- holds an element that a truncating convert gets wrong, one that round-half-away gets wrong, and one that
    fp16-held partials get wrong at each cut the two-pass forms make there."""
    def every_block(differs):
        mm, nn = -(-differs.shape[0] // 16) * 16, -(-differs.shape[1] // 16) * 16
        padded = np.zeros((mm, nn), dtype=bool)
        padded[:differs.shape[0], :differs.shape[1]] = differs
        return padded.reshape(mm // 16, 16, nn // 16, 16).any(axis=(1, 3)).all()

    for a, b, truth, cut_sets in nn_rounding_cases:
        shape = (a.shape[0], b.shape[1], a.shape[1])
        x = oracle.exact_product(a, b)
        assert every_block(oracle.round_toward_zero(x) != truth), ("RTZ", shape)
        assert every_block(oracle.round_half_away(x) != truth), ("half-away", shape)
        for cuts in cut_sets:
            assert every_block(oracle.fp16_partials(a, b, cuts) != truth), (cuts, shape)
