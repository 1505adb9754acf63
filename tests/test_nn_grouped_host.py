"""CPU tests of the grouped input gradient's host side (bgemm_mi355x_nn_grouped): what a launch decides over the scope, the reach and the refusal
rules and which form it takes (bgemm_mi355x_selfcheck_launch_nn_grouped: nothing is launched).  The tile map is tests/test_grouped_map_host.py's."""
import ctypes

import pytest

from residual_common import EPI_C16_ADD, FORM_PLAIN, FORM_REFERENCE, NT

BM, BN = (64, 128, 64, 128), (64, 64, 128, 128)
G, M, N, K, CAP = 7, 300, 72, 128, 256
LDS = (K, N, K * N, N, N)            # lda, ldb, group_stride_b, ldr, ldc
bump = lambda i, d: tuple(v + d * (j == i) for j, v in enumerate((K, N, K * (N + 8), N, N)))  # noqa: E731  (LDS with slack and stride i moved by d)
WIDE = (1 << 23) - (1 << 16)         # 130048 column tiles within C's reach: x 16513 row tiles = 2^31 - 1024, a grid that fits an int; x 16514 does not


@pytest.fixture(scope="module")
def lib():
    import build
    L = ctypes.CDLL(str(build.build_library()))
    i, ll, p = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    L.bgemm_mi355x_selfcheck_launch_nn_grouped.argtypes = [i] * 9 + [ll] + [i] * 2 + [p]
    return L


def decide(lib, cfg=0, word=1, ops=4 | 8, g=G, dims=(M, N, K), lds=LDS):   # ops: 4 aligned, 8 an r, 16 r is c  -> (status, form, grid bound, epilogue)
    out = (ctypes.c_longlong * 20)()
    st = lib.bgemm_mi355x_selfcheck_launch_nn_grouped(cfg, word, ops, g, *dims, *lds, out)
    return st, out[0], out[5], out[6]


def test_forms_and_the_grid_bound(lib):
    for cfg in range(4):
        grid = (M + G * (BM[cfg] - 1)) // BM[cfg] * -(-N // BN[cfg])                  # grouped_tiles_m_max x tiles_n
        assert decide(lib, cfg, ops=4) == (0, FORM_PLAIN, grid, 0) == decide(lib, cfg, 1 | NT, ops=4)          # EPI_C16
        assert decide(lib, cfg) == (0, FORM_PLAIN, grid, EPI_C16_ADD) == decide(lib, cfg, ops=4 | 8 | 16)
        assert decide(lib, cfg, ops=8)[:3] == (0, FORM_REFERENCE, 0) == decide(lib, cfg, dims=(M, N, 72), lds=(72, N, 72 * N, N, N))[:3]


@pytest.mark.parametrize("inside, outside", [
    (dict(g=CAP), dict(g=CAP + 1)),                                                                                # the cap
    *[(dict(lds=bump(i, 8)), dict(lds=bump(i, 4))) for i in range(5)],                                             # each of the five strides a multiple of 8
    (dict(dims=(M, 80, K), lds=(K, 80, K * 80, 80, 80)), dict(dims=(M, 76, K), lds=(K, 76, K * 76, 76, 76))),      # N % 8
    (dict(dims=(M, N, 64)), dict(dims=(M, N, 1), lds=(8, N, N, N, N))),                                            # K % 64
    (dict(lds=((1 << 23) - 8, N, K * N, N, N)), dict(lds=(1 << 23, N, K * N, N, N))),                              # A's reach, BM = 128: (BM lda + K) 2 < 2 GiB
    (dict(dims=(M, N, 1 << 10), lds=(1 << 10, (1 << 20) - 8, 1 << 30, N, N)), dict(dims=(M, N, 1 << 10), lds=(1 << 10, 1 << 20 | 1 << 11, 1 << 31, N, N))),  # B's
    (dict(lds=(K, N, K * N, (1 << 23) - 8, N)), dict(lds=(K, N, K * N, 1 << 23, N))),                              # r's reach
    (dict(lds=(K, N, K * N, N, (1 << 23) - 8)), dict(lds=(K, N, K * N, N, 1 << 23))),                              # C's reach
    (dict(g=1, dims=(16513 * 128, WIDE, 64), lds=(64, WIDE, 64 * WIDE, WIDE, WIDE)), dict(g=1, dims=(16513 * 128 + 1, WIDE, 64), lds=(64, WIDE, 64 * WIDE, WIDE, WIDE))),
])
def test_scope_and_reach_on_both_sides(lib, inside, outside):
    assert decide(lib, 1, **inside)[:2] == (0, FORM_PLAIN), inside
    assert decide(lib, 1, **outside)[:2] == (0, FORM_REFERENCE), outside


def test_the_refusals(lib):
    for kw in (dict(g=0), dict(dims=(0, N, K)), dict(dims=(M, 0, K)), dict(dims=(M, N, 0)), dict(lds=(K - 8, N, K * N, N, N)), dict(lds=(K, N - 8, K * N, N, N)),
               dict(lds=(K, N, (K - 1) * N + N - 1, N, N)), dict(lds=(K, N, K * N, N - 8, N)), dict(lds=(K, N, K * N, N, N - 8)),
               dict(ops=4 | 8 | 16, lds=(K, N, K * N, N + 8, N)), dict(cfg=4), dict(cfg=-1), dict(word=2), dict(word=3 | NT)):
        assert decide(lib, **kw)[0] == -1, kw                            # refused, nothing launched
    assert decide(lib, ops=4, lds=(K, N, K * N, 0, N))[0] == 0 and decide(lib, lds=(K, N, (K - 1) * N + N, N, N))[0] == 0      # no r: ldr is not read
