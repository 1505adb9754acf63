"""The host path of the two transposed-read layouts (family n: NN, family a: TA) against a recording of the library as it was BEFORE
the two paths were folded into one: tests/golden/tr_resolve_golden.json holds, per family, what hgemm_mi355x_selfcheck_launch_{nn,ta}
answered over a fixed grid (status and out[0 .. 4 + 8 n)), and over the grid's shapes the planner, `runs` and
`plan_workspace_bytes`.  The expected values are the earlier library's, never the one under test;
tests/tools/make_tr_resolve_golden.py wrote the file (run by hand; this test does not call it)."""
import ctypes
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "tr_resolve_golden.json"
FAMILIES = ("nn", "ta")


def prepare(lib):
    for fam in FAMILIES:
        fn = getattr(lib, f"hgemm_mi355x_{fam}_plan_workspace_bytes")
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
    return lib


# each function: the call's arguments (a row's head) -> what the library answers (the row's tail)
def resolve(lib, fam, cfg, splits, operands, m, n, k, lda, ldb, ldc, ruled_out):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, f"hgemm_mi355x_selfcheck_launch_{fam}")(cfg, splits, operands, m, n, k, lda, ldb, ldc, ruled_out, out)
    return [st] + list(out[:4 + 8 * out[1]])


def plan(lib, fam, m, n, k):
    cfg, splits = ctypes.c_int(-7), ctypes.c_int(-7)
    st = getattr(lib, f"hgemm_mi355x_{fam}_plan")(m, n, k, ctypes.byref(cfg), ctypes.byref(splits))
    return [st, cfg.value, splits.value]


def runs(lib, fam, cfg, m, n, k, lda, ldb, ldc):
    return [getattr(lib, f"hgemm_mi355x_{fam}_runs")(cfg, m, n, k, lda, ldb, ldc)]


def workspace(lib, fam, cfg, splits, m, n, k):
    return [getattr(lib, f"hgemm_mi355x_{fam}_plan_workspace_bytes")(cfg, splits, m, n, k)]


CALLS = {"resolve": (resolve, 10), "plan": (plan, 3), "runs": (runs, 7), "workspace": (workspace, 5)}   # (call, number of arguments)


@pytest.fixture(scope="module")
def lib():
    import build

    return prepare(ctypes.CDLL(str(build.build_library())))


def test_the_library_reproduces_every_recorded_row(lib):
    golden = json.loads(GOLDEN.read_text())
    assert set(golden) == set(FAMILIES)
    for fam in FAMILIES:
        assert set(golden[fam]) == set(CALLS)
        assert 300 <= len(golden[fam]["resolve"]) <= 2500 and all(len(golden[fam][what]) >= 100 for what in CALLS)
        for what, (call, nargs) in CALLS.items():
            for i, row in enumerate(golden[fam][what]):
                got = call(lib, fam, *row[:nargs])
                assert got == row[nargs:], f"{fam} {what} row {i}: arguments {row[:nargs]}: recorded {row[nargs:]}, the library answers {got}"
