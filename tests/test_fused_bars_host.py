"""CPU companion of tests/test_gpu_fused_bars.py: from the reference data alone, for every operand set the GPU file draws (operand_sets),
that the sums are exact in any order, that a displaced or cut-short second matrix gives another result in every 64 x 64 tile it can
reach, and that the GPU file's comparison names the mistake; and, through the built library's host logic, that the edge strides of its
reach cases obey the written rules.  DESIGN.md 4.36 records the shares printed here."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_fused_bars as fb
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the built library with the prototypes)

SETS = sorted({(shape, seed) for shape, seed, _ in fb.operand_sets()})
IDS = ["x".join(map(str, shape)) for shape, _ in SETS]


def test_the_operand_sets_cover_every_section():
    sections = {section for _, _, section in fb.operand_sets()}
    assert sections == {"reach", "clamp", "raster", "ladder", "long K"}
    assert {shape for shape, _ in SETS} >= {fb.RASTER, fb.LONG, fb.CLAMP, *fb.LADDER}
    assert sorted(shape[2] // fb.BK for shape in fb.LADDER) == list(range(1, 8))
    stages = [shape[2] // fb.BK for shape in fb.LADDER]
    assert {s % 3 for s in stages} == {0, 1, 2} and {s % 4 for s in stages} == {0, 1, 2, 3}
    # every member and every tile height and width appears among the reach cases of each family
    for family in ("tn", "nn"):
        assert {c[1] for c in fb.REACH_CASES if fb.CALLS[c[0]].family == family} == {0, 1, 2, 3}, family
    roles = {(c[0], c[2]) for c in fb.REACH_CASES}
    assert roles == {("tn_bias_act_aux", "z_out"), ("nn_dact", "z"), ("nn_dact_dbias", "z"), ("nn_dgated", "g|u"), ("nn_dgated", "dg|du"), ("tn_gated_aux", "g_out|u_out"),
                     ("tn_gated", "wg|wu"), ("tn_bias_add", "r"), ("nn_add", "r"), ("tn_bias_add", "r=c"), ("nn_add", "r=c")}
    # the table's second matrices ride on the strides the launch takes
    for name, call in fb.CALLS.items():
        assert all(m in call.args and fb.STRIDE_OF[m] == s and s in call.strides and rw == ("w" if m in fb.WRITTEN else "r") for m, s, rw in call.second), name


@pytest.mark.parametrize("shape,seed", SETS, ids=IDS)
def test_the_sums_are_exact_in_any_order_and_grouping(shape, seed):
    """Every product is an integer of [-225, 225] (times 2^-9) and K x 225 < 2^24: every partial sum over any subset of K, in any order and
    grouping, is an integer below 2^24 and exact in fp32.  Checked besides: the operands are bf16 values, S is the fp64 product, and fp32
    sums over K slabs in both orders and over a permuted K give S's bits."""
    m, n, k = shape
    ops = fb.ops_of(shape)
    assert seed == fb.seed_of(shape)
    ai, bi, b2i = ops.ints
    assert all(int(np.abs(x).max()) <= 15 for x in ops.ints) and k * 225 < 2 ** 24
    assert np.array_equal(ops.a.double().numpy() * 2.0 ** 9, ai) and np.array_equal(ops.b.double().numpy(), bi) and np.array_equal(ops.b2.double().numpy(), b2i)
    perm = np.random.default_rng(seed).permutation(k)
    for s, w, wt in ((ops.s, ops.b, ops.bt), (ops.s2, ops.b2, ops.b2t)):
        assert torch.equal(s.double(), ops.a.double() @ w.double()) and torch.equal(wt, w.t())
        a32, w32 = ops.a.float(), w.float()
        for cut in sorted({64 * ((k // 64 + 1) // 2), 64} - {k}):
            lo, hi = a32[:, :cut] @ w32[:cut], a32[:, cut:] @ w32[cut:]
            assert torch.equal(lo + hi, s) and torch.equal(hi + lo, s), cut
        assert torch.equal(a32[:, perm] @ w32[perm], s)
    for x in (ops.z, ops.u):
        assert bool((x != 0).all()) and 0.4 < float((x > 0).float().mean()) < 0.6
        assert len(set(x.view(torch.int16).flatten().tolist())) > min(x.numel(), 4096) // 8, "the second matrices are position-dependent"


@pytest.mark.parametrize("shape,seed", SETS, ids=IDS)
def test_the_bias_gradients_column_sums_are_exact(shape, seed):
    """expect() asserts it: every stored C is a multiple of 2^-9 and every column's sum of |C| is below 2^15, so db32 is defined bit for bit."""
    out = fb.expect("nn_dact_dbias", fb.ops_of(shape))
    assert out["db32"].dtype == torch.float32 and out["db32"].shape == (shape[1],) and bool((out["db32"] != 0).any())


@pytest.mark.parametrize("shape,seed", SETS, ids=IDS)
def test_a_displaced_or_cut_short_second_matrix_shows_in_every_tile(shape, seed):
    """For every call that reads a second matrix: the expectation with the matrix read one row, one 4-column group, one tile row or one tile
    column further on (and at the previous column tile, where there is one), or with zeros from row 7 / 64 on, differs from the true one in
    EVERY 64 x 64 tile of every output that the mistake can reach.  Prints each variant's share of differing elements."""
    ops = fb.ops_of(shape)
    for call in fb.READS_SECOND:
        want = fb.expect(call, ops)
        for name, (outs, (tile_row, tile_col)) in fb.wrong_expectations(call, ops).items():
            for out in want:
                if out == "db32":
                    continue
                tiles = fb.tiles_differing(outs[out], want[out])
                reach = tiles[tile_row:, tile_col:]
                share = float((fb.bits(outs[out]) != fb.bits(want[out])).float().mean())
                print(f"{'x'.join(map(str, shape))} {call} {out}, second matrix {name}: {100 * share:.1f} % of the elements differ, {int(tiles.sum())} of {tiles.numel()} tiles")
                if reach.numel():
                    assert bool(reach.all()), (call, out, name, tiles)
                assert not bool(tiles[:tile_row].any()) and not bool(tiles[:, :tile_col].any()), (call, out, name, "differs where the mistake cannot reach")


def test_the_comparison_names_the_mistake():
    """verdict() on the true expectation, on every wrong one and on a result that is none of them"""
    ops = fb.ops_of((136, 72, 128))
    for call in fb.CALLS:
        want = fb.expect(call, ops)
        assert fb.verdict(call, ops, {k: v.clone() for k, v in want.items()}) is None
        first = next(k for k in want if k != "db32")
        broken = {k: v.clone() for k, v in want.items()}
        broken[first][5, 9] = 1234.0
        said = fb.verdict(call, ops, broken, "x")
        assert f"{first} differs in 1 of" in said and "first at (5, 9)" in said and "1 of its 64 x 64 tiles differ" in said
        assert ("none of the known mistakes" in said) == (call in fb.READS_SECOND)
        if call not in fb.READS_SECOND:
            continue
        for name, (outs, _) in fb.wrong_expectations(call, ops).items():
            got = {k: outs.get(k, want[k]).clone() for k in want}
            said = fb.verdict(call, ops, got, "x")
            assert said is not None and f"second matrix {name}" in said, (call, name, said)
    if "db32" in fb.expect("nn_dact_dbias", ops):
        broken = {k: v.clone() for k, v in fb.expect("nn_dact_dbias", ops).items()}
        broken["db32"][70] += 1.0
        assert "db32 differs in 1 of 72 elements, first at (70,)" in fb.verdict("nn_dact_dbias", ops, broken, "x")


def test_displaced_and_cut_short_read_what_they_say():
    x = torch.arange(1, 13, dtype=torch.float32).view(3, 4)
    assert fb.displaced(x, 1, 0).tolist() == [[5, 6, 7, 8], [9, 10, 11, 12], [0, 0, 0, 0]]
    wide = torch.arange(72, dtype=torch.float32).view(1, 72)
    assert fb.previous_tile_column(wide)[0].tolist() == list(range(64)) + list(range(8))
    assert fb.displaced(x, 0, 64).tolist() == [[0] * 4] * 3 and fb.cut_short(x, 1).tolist() == [[1, 2, 3, 4], [0] * 4, [0] * 4]


@pytest.mark.parametrize("case", fb.REACH_CASES, ids=lambda c: f"{c[0]}-{c[2]}-{'x'.join(map(str, fb.TILES[c[1]]))}")
def test_the_edge_strides_of_the_reach_cases_obey_the_written_rules(lib, case):
    """The host logic alone (no launch): the bisected edge stride against (rows ld + tail / 2) 2 < 2^31 <= (rows (ld + 8) + tail / 2) 2, the
    hook's forms on both sides, and the sizes of the buffers the GPU test lays out."""
    call, cid, what, edge, fuse, inplace, m, n = case
    shape = (m, n, fb.REACH_K)
    s = fb.edge_stride(lib, call, cid, shape, edge, fuse)
    rows, tail = fb.reach_rule(call, cid, what, shape)
    assert rows * s * 2 + tail < 2 ** 31 <= rows * (s + 8) * 2 + tail
    base = fb.contiguous(call, shape)
    if fuse and fuse[0] != "wg":
        base[fb.STRIDE_OF[fuse[0]]] = 2 * n
    for stride, forms in ((s, (FORM_PLAIN, FORM_SPLITK)), (s + 8, (FORM_REFERENCE, FORM_REFERENCE))):
        lds = dict(base, **{e: stride for e in edge})
        assert fb.kernel_runs(lib, call, cid, shape, lds) == (stride == s)
        assert [fb.decision(lib, call, cid, word, shape, lds)[:2] for word in (1, 2)] == [(0, f) for f in forms]
    elements = (2 * n if what == "wg|wu" else m) * (s + 8) + 8
    print(f"{call} {what} {fb.member(call, cid)}: edge stride {s}, buffer {elements * 2 / 1e9:.2f} GB")
    assert 2.2e9 < elements * 2 < 5.0e9


def test_the_clamp_cases_have_a_clamped_an_unclamped_and_an_exact_range(lib):
    lib.bgemm_mi355x_selfcheck_dact_z_range.restype = ctypes.c_uint
    m, n, k = fb.CLAMP
    for call in fb.CLAMP_CASES:
        ldz = fb.edge_stride(lib, call, 0, fb.CLAMP, "z", ())
        got = [lib.bgemm_mi355x_selfcheck_dact_z_range(m, n, ldz, m0) for m0 in (0, 64, 128)]
        assert got == [0xFFFFFFFF, (71 * ldz + n) * 2, (7 * ldz + n) * 2] and (135 * ldz + n) * 2 > 2 ** 32 > got[1]
        wrapped = ((135 * ldz + n) * 2) % 2 ** 32
        assert -(-wrapped // (2 * ldz)) in fb.SHORT_RANGES, "a wrapped range would cut the first tile short at a row the data are shown to tell"
        print(f"{call}: ldz {ldz}, z of {(m * ldz + 8) * 2 / 1e9:.2f} GB, a wrapped range would read zeros from row {-(-wrapped // (2 * ldz))} on")
