"""CPU tests of the grouped weight gradient's host side (bgemm_mi355x_ta_grouped / _ta_grouped_c32): what a launch decides over the scope and the
refusal rules (bgemm_mi355x_selfcheck_launch_ta_grouped: nothing is launched), and hgemm_grouped.hpp's map arithmetic against a restatement in Python."""
import ctypes

import pytest

from residual_common import FORM_PLAIN, FORM_REFERENCE, NT

BM, BN = (64, 128, 64, 128), (64, 64, 128, 128)
G, M, N, K = 7, 72, 136, 700


@pytest.fixture(scope="module")
def lib():
    import build
    L = ctypes.CDLL(str(build.build_library()))
    i, ll, p = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    L.bgemm_mi355x_selfcheck_launch_ta_grouped.argtypes = [i] * 11 + [ll, i, p]
    L.bgemm_mi355x_ta_grouped_runs.argtypes = L.bgemm_mi355x_ta_grouped_c32_runs.argtypes = [i] * 8 + [ll]
    return L


def decide(lib, cfg=0, word=1, aligned=True, c32=1, g=G, dims=(M, N, K), lds=(M, N, N, M * N), acc=0):
    out = (ctypes.c_longlong * 20)()
    st = lib.bgemm_mi355x_selfcheck_launch_ta_grouped(cfg, word, 4 if aligned else 0, c32, g, *dims, *lds, acc, out)
    return st, out[0], out[5]


def test_scope_grid_and_refusals(lib):
    for cfg in range(4):
        grid = G * -(-M // BM[cfg]) * -(-N // BN[cfg])
        for c32, acc in ((1, 0), (1, 1), (0, 0)):
            assert decide(lib, cfg, c32=c32, acc=acc) == (0, FORM_PLAIN, grid) == decide(lib, cfg, 1 | NT, c32=c32, acc=acc)
            assert decide(lib, cfg, c32=c32, acc=acc, dims=(M, N, 1)) == (0, FORM_PLAIN, grid)                  # K is unrestricted
            assert decide(lib, cfg, c32=c32, acc=acc, g=100000, dims=(8, 8, 3)) == (0, FORM_PLAIN, 100000)      # no cap on G
    for kw in (dict(aligned=False), dict(dims=(M + 4, N, K), lds=(M + 4, N, N, (M + 4) * N)), dict(dims=(M, N + 4, K), lds=(M, N + 4, N + 4, M * (N + 4))),
               dict(lds=(M + 4, N, N, M * N)), dict(lds=(M, N + 4, N + 4, M * (N + 4))), dict(lds=(M, N, N + 2, M * (N + 2))), dict(lds=(M, N, N, M * N + 2)),
               dict(c32=0, lds=(M, N, N + 4, M * (N + 4))), dict(c32=0, lds=(M, N, N, M * N + 4)),
               dict(dims=(M, N, (1 << 20) + 1), lds=(1024, N, N, M * N)),                            # A's reach: (K' - 1) lda 2 bytes above 2 GiB
               dict(g=1 << 30)):                                                                     # a grid that does not fit an int
        assert decide(lib, **kw)[:2] == (0, FORM_REFERENCE), kw         # outside the kernels' scope: the reference kernel answers
    assert decide(lib, lds=(M, N, N + 4, M * (N + 4)))[1] == FORM_PLAIN and decide(lib, dims=(M, N, (1 << 20) - 64), lds=(1024, N, N, M * N))[1] == FORM_PLAIN
    assert lib.bgemm_mi355x_ta_grouped_c32_runs(0, G, M, N, K, M, N, N + 4, M * (N + 4)) == 1 and lib.bgemm_mi355x_ta_grouped_runs(0, G, M, N, K, M, N, N + 4, M * (N + 4)) == 0
    for kw in (dict(g=0), dict(dims=(0, N, K)), dict(dims=(M, 0, K)), dict(dims=(M, N, 0)), dict(lds=(M - 8, N, N, M * N)), dict(lds=(M, N - 8, N, M * N)),
               dict(lds=(M, N, N - 8, M * N)), dict(lds=(M, N, N, M * N - 1)), dict(cfg=4), dict(cfg=-1), dict(acc=2), dict(acc=-1), dict(c32=0, acc=1),
               dict(word=2), dict(word=3 | NT)):
        assert decide(lib, **kw)[0] == -1, kw                            # refused, nothing launched


@pytest.mark.parametrize("groups, tiles_m, tiles_n", [(1, 1, 1), (7, 2, 3), (3, 19, 2), (300, 1, 1), (5, 9, 4)])
def test_the_map_against_its_restatement(lib, groups, tiles_m, tiles_n):
    grid, out, seen = groups * tiles_m * tiles_n, (ctypes.c_int * 4)(), set()
    for bid in range(grid):
        assert lib.bgemm_mi355x_selfcheck_ta_grouped_tile(bid, grid, tiles_m, tiles_n, -5 + bid, 60 + 3 * bid, 700, out) == 0
        q, r = divmod(grid, 8)                                       # the XCD remap: XCD bid % 8 owns one contiguous run of logical ids
        logical = (bid % 8) * q + min(bid % 8, r) + bid // 8
        grp, local = divmod(logical, tiles_m * tiles_n)              # a group's tiles are one run; inside it bands of 8 tile rows, the row fastest
        first = local // (8 * tiles_n) * 8
        tn, tm = divmod(local % (8 * tiles_n), min(8, tiles_m - first))
        rows = max(min(60 + 3 * bid, 700) - max(-5 + bid, 0), 0)
        assert tuple(out) == (grp, first + tm, tn, -(-rows // 64)), bid
        seen.add(tuple(out)[:3])
    assert len(seen) == grid                                         # every tile of every group exactly once
