"""CPU tests of the grouped gated forward's host side (bgemm_mi355x_tn_grouped_gated): the scope, reach and refusal rules and the form a launch takes, through
bgemm_mi355x_selfcheck_launch_tn_grouped_gated (nothing is launched).  The tile map is tests/test_grouped_map_host.py's; a tile is BM rows by BN / 2 outputs."""
import ctypes

import pytest

from residual_common import FORM_PLAIN, FORM_REFERENCE, NT

BM, WN = (64, 128, 64, 128), (32, 32, 64, 64)            # a member's rows and OUTPUT columns (BN / 2)
G, M, N, K, CAP, SILU = 7, 300, 72, 128, 256, 4
LDS = (K, K, N * K, N, N, N)                              # lda, ldb, group_stride_b, ldbias, ldc, ldz
bump = lambda i, d: tuple(v + d * (j == i) for j, v in enumerate((K, K, (N + 8) * K, N, N, N)))  # noqa: E731  (LDS with slack and stride i moved by d)
WIDE = (1 << 23) - (1 << 16)     # 260096 output tiles of 32 columns within C's reach: x 8256 row tiles = 2^31 - 2^17, a grid that fits an int; x 8257 does not
WIDE_LDS = (64, 64, 64 * WIDE, WIDE, WIDE, WIDE)


@pytest.fixture(scope="module")
def lib():
    import build
    L = ctypes.CDLL(str(build.build_library()))
    L.bgemm_mi355x_selfcheck_launch_tn_grouped_gated.argtypes = [ctypes.c_int] * 9 + [ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    L.bgemm_mi355x_tn_grouped_gated_runs.argtypes = [ctypes.c_int] * 7 + [ctypes.c_longlong] + [ctypes.c_int] * 3
    return L


def decide(lib, cfg=0, word=1, ops=4 | 8 | 16, g=G, dims=(M, N, K), lds=LDS, act=SILU):   # ops: 4 aligned, 8 a bias, 16 g_out / u_out  -> (status, form, grid)
    out = (ctypes.c_longlong * 20)()
    st = lib.bgemm_mi355x_selfcheck_launch_tn_grouped_gated(cfg, word, ops, g, *dims, *lds, act, out)
    return st, out[0], out[5]


def test_forms_and_the_grid_bound(lib):
    for cfg in range(4):
        grid = (M + G * (BM[cfg] - 1)) // BM[cfg] * -(-N // WN[cfg])                   # grouped_tiles_m_max x ceil(N / (BN / 2))
        assert all(decide(lib, cfg, act=act) == (0, FORM_PLAIN, grid) == decide(lib, cfg, 1 | NT, ops=4, act=act) for act in (1, 2, 3, 4))
        assert decide(lib, cfg, ops=8 | 16) == (0, FORM_REFERENCE, 0) == decide(lib, cfg, dims=(M, N, 72), lds=(72, 72, 72 * N, N, N, N))


@pytest.mark.parametrize("inside, outside", [
    (dict(g=CAP), dict(g=CAP + 1)),                                                                                     # the cap
    *[(dict(lds=bump(i, 8)), dict(lds=bump(i, 4))) for i in range(6)],                                                  # each of the six strides a multiple of 8
    (dict(dims=(M, 80, K), lds=(K, K, 80 * K, 80, 80, 80)), dict(dims=(M, 76, K), lds=(K, K, 76 * K, 76, 76, 76))),     # N % 8
    (dict(dims=(M, N, 64), lds=(64, 64, 64 * N, N, N, N)), dict(dims=(M, N, 1), lds=(8, 8, 8 * N, N, N, N))),           # K % 64
    (dict(lds=((1 << 23) - 8, K, N * K, N, N, N)), dict(lds=(1 << 23, K, N * K, N, N, N))),                             # A's reach, BM = 128: (BM lda + K) 2 < 2 GiB
    (dict(lds=(K, (1 << 25) - 8, N << 25, N, N, N)), dict(lds=(K, 1 << 25, N << 25, N, N, N))),                         # each weight's, BN / 2 = 32 rows
    (dict(lds=(K, K, N * K, N, (1 << 23) - 8, N)), dict(lds=(K, K, N * K, N, 1 << 23, N))),                             # C's reach
    (dict(lds=(K, K, N * K, N, N, (1 << 23) - 8)), dict(lds=(K, K, N * K, N, N, 1 << 23))),                             # g_out / u_out's reach
    (dict(g=1, dims=(8256 * 128, WIDE, 64), lds=WIDE_LDS), dict(g=1, dims=(8257 * 128, WIDE, 64), lds=WIDE_LDS)),       # the grid bound fits an int
])
def test_scope_and_reach_on_both_sides(lib, inside, outside):
    assert decide(lib, 1, **inside)[:2] == (0, FORM_PLAIN), inside
    assert decide(lib, 1, **outside)[:2] == (0, FORM_REFERENCE), outside


def test_the_refusals_and_runs(lib):
    for kw in (dict(g=0), dict(dims=(0, N, K)), dict(dims=(M, 0, K)), dict(dims=(M, N, 0)), dict(lds=(K, K, (N - 1) * K + K - 1, N, N, N)),
               *[dict(lds=bump(i, -8)) for i in (0, 1, 3, 4, 5)], dict(cfg=4), dict(cfg=-1), dict(word=2), dict(word=3 | NT), dict(act=0), dict(act=5)):
        assert decide(lib, **kw)[0] == -1, kw                                           # refused, nothing launched
    assert decide(lib, ops=4 | 16, lds=(K, K, N * K, 0, N, N))[0] == 0 and decide(lib, ops=4 | 8, lds=(K, K, N * K, N, N, 0))[:2] == (0, FORM_PLAIN)      # ldbias / ldz not read
    runs = lambda ldz, g=G: lib.bgemm_mi355x_tn_grouped_gated_runs(0, g, M, N, K, K, K, N * K, N, N, ldz)  # noqa: E731
    assert runs(N) == 1 == runs(0) and runs(N + 4) == 0 == runs(N - 8) and runs(N, CAP) == 1 and runs(N, CAP + 1) == 0       # ldz = 0: no g_out / u_out
