"""CPU proof of the operands of tests/test_gpu_tn_bars.py (oracle.bf16_dyadic_inputs), in the manner of tests/test_oracle.py's dyadic
section: for exactly the operand pairs, shapes and K cuts the GPU tests draw (test_gpu_tn_bars.operand_sets), before any GPU is involved --
the operands are bf16 values with live mantissa bits, the exact product is the same in every fp32 summation order, the expected matrices
hold every rounding case, each mistake a kernel could make gives another matrix, and the GPU file's own comparison code rejects each of
those matrices and names it.  No kernel is launched here; every figure below comes from the reference alone."""
import numpy as np
import pytest
import torch

import test_gpu_tn_bars as B
from oracle import hgemm_oracle as oracle
from test_gpu_tr_bf16 import rounding_classes

# Elements in which bf16(bf16(S) + bias) -- the bias added after the rounding -- must differ from the expected bf16(S + bias), per operand
# pair (class, shape, seed): HALF the count measured on the reference when this file was written (152, 410, 1786, 6754, ... for class B).
# (64, 64, 64) included: with live mantissa bits S needs a rounding already at one K stage, which the integer operands of
# test_gpu_tn_bias.TWICE_ROUNDED_FLOOR cannot show.
TWICE_ROUNDED_FLOOR = {
    ("A", (64, 64, 64), 192): 65, ("A", (136, 72, 128), 336): 207, ("A", (152, 152, 320), 624): 856, ("A", (264, 264, 512), 1040): 3461,
    ("B", (64, 64, 64), 192): 76, ("B", (136, 72, 128), 336): 205, ("B", (152, 152, 320), 624): 893, ("B", (264, 264, 512), 1040): 3377,
    ("AB", (64, 64, 64), 192): 120, ("AB", (136, 72, 128), 336): 299, ("AB", (152, 152, 256), 560): 1101,
    ("A", (256, 264, 512), 1032): 3258, ("B", (256, 264, 512), 1032): 3286, ("B", (64, 64, 8128), 8256): 404,
    ("B", (136, 64, 128), 328): 227, ("B", (64, 136, 128), 328): 260, ("B", (72, 136, 128), 336): 262,
    ("B", (1160, 136, 128), 1424): 4381, ("B", (520, 1096, 64), 1680): 31517,
    ("B", (200, 264, 512), 976): 2636, ("B", (200, 264, 512), 977): 2812, ("B", (200, 136, 128), 464): 909,
}
BITS_AT_MOST = {"A": 18.6, "B": 18.6, "AB": 21.0}          # 18.50 (K = 8128) and 20.87 (K = 256) measured on these operands; 23 is the rule


@pytest.fixture(scope="module")
def sets():
    """[(Exact, cut sets, section)]: the very objects the GPU tests take from test_gpu_tn_bars.exact."""
    out = [(B.exact(side, shape, seed), cuts, section) for side, shape, seed, cuts, section in B.operand_sets()]
    assert len(out) == len(TWICE_ROUNDED_FLOOR) == 22
    shapes = {(ex.side, ex.shape) for ex, _, _ in out}
    for side, want in (("A", B.SHAPES), ("B", B.SHAPES + [B.LONG]), ("AB", [(64, 64, 64), (136, 72, 128), (152, 152, 256)])):
        assert all((side, s) in shapes for s in want)
    assert all(ex.shape[2] <= 256 for ex, _, _ in out if ex.side == "AB")
    return out


def every_block(differs):
    """every whole 16 x 16 block of C -- the footprint of one MFMA tile: all lanes, all accumulator registers -- holds a differing element"""
    mm, nn = differs.shape[0] // 16 * 16, differs.shape[1] // 16 * 16
    return bool(differs[:mm, :nn].reshape(mm // 16, 16, nn // 16, 16).any(axis=(1, 3)).all())


def test_every_operand_is_a_bf16_value_with_live_mantissa_bits(sets):
    for ex, _, _ in sets:
        oracle.assert_bf16_dyadic(ex.a, ex.b, ex.side)
        for x, live in ((ex.a, ex.side in ("A", "AB")), (ex.b, ex.side in ("B", "AB"))):
            t = torch.from_numpy(x).to(torch.bfloat16)
            assert np.array_equal(t.float().numpy().view(np.uint32), x.view(np.uint32)), "an operand is no bf16 value"
            pattern = t.view(torch.int16).numpy().view(np.uint16)
            bit0, bit1, higher = int((pattern & 1 != 0).sum()), int((pattern & 2 != 0).sum()), int((pattern & 0x7C != 0).sum())
            assert higher == 0 and ((bit0 > x.size // 8 and bit1 > x.size // 8) if live else (bit0 == 0 and bit1 == 0)), (ex.side, ex.shape, bit0, bit1)
        bits = oracle.bf16_dyadic_bits(ex.a, ex.b, ex.side)
        assert bits <= BITS_AT_MOST[ex.side] < 23, (ex.side, ex.shape, bits)
        assert (ex.a < 0).any() and (ex.a > 0).any() and (ex.b >= 0).all()


def test_the_exact_product_is_the_same_in_every_fp32_summation_order(sets):
    """The exact product (fp64) equals an fp32 accumulation of the products one by one in forward order, in reverse order, and in blocks
    of 32 (an MFMA's K) added in fp32; and the two-pass forms' own order -- fp32 chunk sums added in split order -- at every cut used:
    no fp32 add ever rounded, so whatever order a kernel sums in, there is one right answer."""
    for ex, cut_sets, _ in sets:
        m, n, k = ex.shape
        x = ex.a.astype(np.float64) @ ex.b.astype(np.float64)
        assert np.array_equal(ex.s32.astype(np.float64), x)
        for order in (range(k), range(k - 1, -1, -1)):
            acc = np.zeros((m, n), dtype=np.float32)
            for kk in order:
                acc += ex.a[:, kk, None] * ex.b[kk][None, :]           # an exact fp32 product, then one fp32 add
            assert np.array_equal(acc.astype(np.float64), x), (ex.side, ex.shape)
        acc = np.zeros((m, n), dtype=np.float32)
        for lo in range(0, k, 32):
            acc += (ex.a[:, lo:lo + 32].astype(np.float64) @ ex.b[lo:lo + 32].astype(np.float64)).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), x), (ex.side, ex.shape)
        for cuts in cut_sets:
            acc = np.zeros((m, n), dtype=np.float32)
            for part in ex.slab_sums(cuts):
                acc += part
            assert np.array_equal(acc.astype(np.float64), x), (ex.side, ex.shape, cuts)


def test_the_expected_matrices_hold_every_rounding_case_and_tell_the_mistakes_apart(sets):
    """Conditions on the inputs, not measurements of a kernel.  Classes A and B, the plain expected matrix of every pair: ties whose even
    neighbour is below, ties whose even neighbour is above and plain round-ups occur, and truncation and round-half-away each differ
    from round-to-nearest-even in every whole 16 x 16 block.  Class AB (products of 2^-14: ties are rare) and every expected matrix with
    the bias: ties to both sides and round-ups occur, truncation differs in every block, half-away differs somewhere.  Slabs held in
    bf16 give another matrix at every cut of every split case (all have K >= 128)."""
    for ex, cut_sets, section in sets:
        row = {"bits": round(oracle.bf16_dyadic_bits(ex.a, ex.b, ex.side), 1)}
        for biased in (False, True):
            want = ex.want(biased)
            down, up, ups, trunc, away, rne = rounding_classes(ex.value32(biased))
            assert np.array_equal(rne.astype(np.uint16), want)
            mutants = ex.mutants(biased, cut_sets)
            assert np.array_equal(mutants["truncation"], trunc.astype(np.uint16)) and np.array_equal(mutants["round-half-away"], away.astype(np.uint16))
            assert min(down, up, ups) > 0, (ex.side, ex.shape, biased, down, up, ups)
            assert every_block(mutants["truncation"] != want), (ex.side, ex.shape, biased, "truncation")
            if ex.side != "AB" and not biased:
                assert every_block(mutants["round-half-away"] != want), (ex.side, ex.shape, "half-away")
            assert (mutants["round-half-away"] != want).any()
            assert all(cuts and ex.shape[2] >= 128 for cuts in cut_sets)
            slabs = {name: int((mu != want).sum()) for name, mu in mutants.items() if name.startswith("bf16 slabs")}
            assert len(slabs) == len(cut_sets) and all(d > 0 for d in slabs.values()), (ex.side, ex.shape, biased, slabs)
            row["bias" if biased else "plain"] = {"ties down": down, "ties up": up, "round-ups": ups,
                                                  **{name: int((mu != want).sum()) for name, mu in mutants.items()}}
        print(f"class {ex.side} {ex.shape} seed {ex.seed} ({section}): {row}")


def test_the_bias_add_is_exact_and_the_twice_rounded_matrix_differs_at_every_shape(sets):
    """test_gpu_tn_bias.make_bias's biases (multiples of 2^-8, |b| <= 256, pairwise distinct) on these sums: S + b is exact in fp32 -- shown
    here, so the expected matrix of the bias form owes nothing to the order of anything -- and rounding S first gives another matrix at
    every shape, the one-stage shape (64, 64, 64) included, in at least TWICE_ROUNDED_FLOOR elements; no bias at all differs in more than a
    quarter of the elements."""
    for ex, _, _ in sets:
        m, n, _ = ex.shape
        assert len(set(ex.bias.tolist())) == n and np.abs(ex.bias).max() <= 256 and np.array_equal(ex.bias * 256, np.round(ex.bias * 256))
        assert oracle.is_bf16(ex.bias) and ex.bias_add_exact, (ex.side, ex.shape)
        want, mutants = ex.want(True), ex.mutants(True)
        twice = int((mutants["twice-rounded bias"] != want).sum())
        assert twice >= TWICE_ROUNDED_FLOOR[ex.side, ex.shape, ex.seed] > 0, (ex.side, ex.shape, twice)
        assert twice < 2 * TWICE_ROUNDED_FLOOR[ex.side, ex.shape, ex.seed] + 2            # the table states the measured count
        assert int((mutants["no bias"] != want).sum()) > m * n // 4
    assert TWICE_ROUNDED_FLOOR["B", (64, 64, 64), 192] == 76


def test_no_partial_sum_of_the_workspace_case_has_the_fill_pattern(sets):
    fill = np.array([B.WS_FILL], dtype=np.uint32).view(np.float32)[0]
    assert -1e-15 < fill < 0
    for ex, cut_sets, section in sets:
        if section == "workspace":
            assert cut_sets == [tuple(B.two_pass_cuts(B.WS_SHAPE[2], B.WS_SPLITS))] and len(cut_sets[0]) == B.WS_SPLITS - 1
            for part in ex.slab_sums(cut_sets[0]):
                assert not (part.view(np.uint32) == B.WS_FILL).any() and np.array_equal(part * 128, np.round(part * 128))


def test_the_gpu_files_comparison_rejects_every_mutant_and_names_it(sets):
    """The mutation check of the tests themselves: each mutant matrix, fed to test_gpu_tn_bars.compare in place of a GPU result, is
    rejected and named; the expected matrix passes; a single flipped element is reported with its position."""
    checked = 0
    for ex, cut_sets, _ in sets:
        for biased in (False, True):
            want = ex.want(biased)
            assert B.compare(ex, biased, want.copy(), cut_sets, "expected") is None
            for name, mu in ex.mutants(biased, cut_sets).items():
                said = B.compare(ex, biased, mu, cut_sets, "mutant")
                assert said is not None and f"the whole result equals the {name} mutant" in said, (ex.side, ex.shape, biased, name, said)
                assert f"{int((mu != want).sum())} of {want.size} elements differ" in said
                checked += 1
            one = want.copy()
            one[3, 5] ^= 1
            said = B.compare(ex, biased, one, cut_sets, "one element")
            assert said is not None and "1 of" in said and "first at (3, 5)" in said and "the whole result" not in said
    print(f"{checked} mutant matrices rejected and named")
    assert checked >= 22 * 5


def test_the_mutants_round_as_they_say():
    """The wrong roundings on hand-made values: ties to both sides, both signs, exact values, the first integer bf16 cannot hold."""
    e = 2.0 ** -7
    x = np.array([1 + e / 2, 1 + 3 * e / 2, -(1 + e / 2), 257.0, -257.0, 259.0, 1.0, 0.0, 1 + e / 4, 1 + e / 2 + 2.0 ** -20, -(1 + e - 2.0 ** -20)], dtype=np.float32)
    rne, trunc, away = (oracle.bf16_to_f32(r).tolist() for r in oracle.bf16_roundings(x))
    assert rne == [1.0, 1 + 2 * e, -1.0, 256.0, -256.0, 260.0, 1.0, 0.0, 1.0, 1 + e, -(1 + e)]
    assert away == [1 + e, 1 + 2 * e, -(1 + e), 258.0, -258.0, 260.0, 1.0, 0.0, 1.0, 1 + e, -(1 + e)]
    assert trunc == [1.0, 1 + e, -1.0, 256.0, -256.0, 258.0, 1.0, 0.0, 1.0, 1.0, -1.0]
    assert torch.from_numpy(x).to(torch.bfloat16).float().tolist() == rne
    # 1 + (1 + e) = 2 + e is a tie and rounds to 2; (1 + e) + (1 + e) is exact: bf16-held halves give 4 + 2 e -> 4, the truth is 4 + 3 e -> 4 + 4 e
    a = np.ones((1, 4), np.float32)
    b = np.array([[1.0], [1 + e], [1 + e], [1 + e]], np.float32)
    assert oracle.bf16_to_f32(oracle.bf16_roundings(oracle.bf16_exact_product(a, b, "B"))[0])[0, 0] == 4 + 4 * e
    assert oracle.bf16_to_f32(oracle.bf16_partials(a, b, "B", [2]))[0, 0] == 4.0 and oracle.bf16_to_f32(oracle.bf16_partials(a, b, "B", []))[0, 0] == 4 + 4 * e


def test_the_class_assertion_rejects_what_would_break_exactness():
    rng = np.random.default_rng(5)
    for side in ("A", "B", "AB"):
        a, b = oracle.bf16_dyadic_inputs(8, 8, 64, rng, side)
        oracle.bf16_exact_product(a, b, side)
        bad = b.copy()
        bad[3, 3] = 1 + 4 / 128                                      # e = 4
        for wrong_b in (bad, np.where(b == 0, np.float32(0.5), b), np.where(b == 0, np.float32("nan"), b), b + np.float32(2.0 ** -9), b.astype(np.float64)):
            with pytest.raises(AssertionError):
                oracle.bf16_exact_product(a, wrong_b, side)
        with pytest.raises(AssertionError):
            oracle.bf16_exact_product(np.where(a == 0, np.float32(2), a), b, side)
    a, b = oracle.bf16_dyadic_inputs(8, 8, 64, rng, "AB")
    for side in ("A", "B"):                                          # a live mantissa on the side the class keeps clear
        with pytest.raises(AssertionError):
            oracle.assert_bf16_dyadic(a, b, side)
    with pytest.raises(AssertionError):
        oracle.bf16_dyadic_inputs(8, 8, 64, rng, "C")
    # the rule is asserted on the operands, not on K: in class B ones x (1 + 3/128) pass up to 2^23 / 131 = 64035 terms ...
    ones = np.ones((1, 1 << 16), np.float32)
    oracle.assert_bf16_dyadic(ones[:, :64000], np.full((64000, 1), 1 + 3 / 128, np.float32), "B")           # 64000 x 131 < 2^23
    with pytest.raises(AssertionError):
        oracle.assert_bf16_dyadic(ones[:, :64100], np.full((64100, 1), 1 + 3 / 128, np.float32), "B")       # 64100 x 131 > 2^23
    # ... and class AB stops 2^7 earlier: 512 x 131 x 131 > 2^23
    with pytest.raises(AssertionError):
        oracle.assert_bf16_dyadic(np.full((1, 512), 1 + 3 / 128, np.float32), np.full((512, 1), 1 + 3 / 128, np.float32), "AB")
    oracle.assert_bf16_dyadic(np.full((1, 488), 1 + 3 / 128, np.float32), np.full((488, 1), 1 + 3 / 128, np.float32), "AB")   # 488 x 131^2 < 2^23
