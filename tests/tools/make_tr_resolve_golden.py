"""Writes tests/golden/tr_resolve_golden.json: what the host path of the two transposed-read layouts (family n / NN, family a / TA)
answers over a fixed grid -- hgemm_mi355x_selfcheck_launch_{nn,ta} (status and out[0 .. 4 + 8 n)), and over the grid's shapes
hgemm_mi355x_{nn,ta}_plan, _runs and _plan_workspace_bytes.  tests/test_tr_resolve_golden.py compares the built library with the file.

Run by hand, against the library whose answers are to be the reference (the one from before a change to that host path):

    python tests/tools/make_tr_resolve_golden.py [--lib path/to/libhgemm_mi355x.so]      (default: the tree's library, built if need be)

Rows are [arguments ..., answers ...] in the argument order of test_tr_resolve_golden.CALLS."""
import argparse
import ctypes
import itertools
import json
import sys
from pathlib import Path

TESTS = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(TESTS), str(TESTS.parent / "cuda-l2_amd")]

import test_tr_resolve_golden as t  # noqa: E402

FUSED, NT_STORE, STREAMK = 0x10000, 0x20000, 0x40000
FORM_SPLITK = 3
SPLITS = (1, 2, 3, 8, 33)
WORDS = SPLITS + tuple(s | NT_STORE for s in SPLITS) + tuple(s | STREAMK for s in SPLITS)
SHAPES = list(itertools.product((8, 64, 72, 200, 264), (8, 64, 136), (64, 128, 192, 72)))
GIB = 1 << 30
TOP = (1 << 31) - 8


def reach_limit(rows, tail):
    """The largest stride (a multiple of 8) with rows x ld x 2 + tail < 2 GiB (tests/test_nn_host.py, tests/test_ta_host.py)."""
    return (2 * GIB - tail - 1) // (2 * rows) // 8 * 8


def grid(fam, members):
    """-> (resolve argument rows, shapes-with-strides rows): `members` = [(bm, bn)] in id order."""
    def contiguous(m, n, k):
        return (k if fam == "nn" else m, n, n)

    def padded(m, n, k):
        return tuple(s + 8 for s in contiguous(m, n, k))

    rows = []
    for cid, (bm, bn) in enumerate(members):
        # every plan word x aligned / misaligned x ruled_out on one shape, every plan word on a padded second one
        for word, operands, ruled in itertools.product(WORDS, (4, 0), (0, 1 << FORM_SPLITK)):
            rows.append((cid, word, operands, 200, 136, 192, *contiguous(200, 136, 192), ruled))
        rows += [(cid, word, 4, 264, 64, 128, *padded(264, 64, 128), 0) for word in WORDS]
        # every shape, contiguous and padded by 8, three splits asked for (K = 72 is outside the kernels' scope)
        for (m, n, k), ld in itertools.product(SHAPES, (contiguous, padded)):
            rows.append((cid, 3, 4, m, n, k, *ld(m, n, k), 0))
        # one stride below the minimum (a bad argument); M = 100 and N = 100 (outside scope)
        m, n, k = 200, 136, 128
        for side, operands in itertools.product(range(3), (4, 0)):
            ld = list(contiguous(m, n, k))
            ld[side] -= 8
            rows.append((cid, 1, operands, m, n, k, *ld, 0))
        for (m, n, k), word in itertools.product(((100, 136, 128), (200, 100, 128)), (1, 3)):
            rows.append((cid, word, 4, m, n, k, *contiguous(m, n, k), 0))
        # the reach rule on both sides of its bound, per operand: A from a tile's first row (n) / from row 0 to the end of the matrix
        # (a), B from row 0 to the end of the matrix, C from a tile's first row
        m, n, k = bm + 8, bn + 8, 128
        rules = ((bm, 2 * k) if fam == "nn" else (k - 1, 2 * m), (k - 1, 2 * n), (bm, 2 * n))
        for side, (rws, tail) in enumerate(rules):
            edge = reach_limit(rws, tail)
            for ld_side, splits in itertools.product((edge - 8, edge, edge + 8, edge + 16), (1, 2)):
                ld = list(contiguous(m, n, k))
                ld[side] = ld_side
                rows.append((cid, splits, 4, m, n, k, *ld, 0))
        # products that a 32-bit (or 64-bit) multiply would wrap, and the stride just below each
        for wrap in ((1 << 31) // bm - 8, (1 << 31) // bm):
            rows.append((cid, 1, 4, bm + 8, bn, 128, wrap if fam == "nn" else bm + 8, bn, bn, 0))
            rows.append((cid, 1, 4, bm + 8, bn, 128, *contiguous(bm + 8, bn, 128)[:2], wrap, 0))
        for wrap in ((1 << 31) // 128 - 8, (1 << 31) // 128):
            rows.append((cid, 1, 4, 64, bn, 128, contiguous(64, bn, 128)[0], wrap, bn, 0))
            if fam == "ta":
                rows.append((cid, 1, 4, 64, bn, 128, wrap, bn, bn, 0))
        for ld in ((TOP, 136, 136), (contiguous(200, 136, 128)[0], TOP, 136), (contiguous(200, 136, 128)[0], 136, TOP), (TOP, TOP, TOP)):
            rows.append((cid, 4, 4, 200, 136, 128, *ld, 0))
        rows.append((cid, 1, 4, TOP, 8, 64, *contiguous(TOP, 8, 64), 0))
    strided = [(m, n, k, *ld(m, n, k)) for (m, n, k), ld in itertools.product(SHAPES + [(100, 136, 128), (200, 100, 128)], (contiguous, padded))]
    return rows, strided


def record(lib, fam):
    out = (ctypes.c_int * 8)()
    count = getattr(lib, f"hgemm_mi355x_{fam}_num_configs")()
    members = []
    for cid in range(count):
        assert getattr(lib, f"hgemm_mi355x_{fam}_config_info")(cid, out) == 0
        members.append((out[0], out[1]))
    rows, strided = grid(fam, members)
    shapes = sorted({s[:3] for s in strided} | {(m, n, k) for m, n, k in itertools.product((64, 1024, 4096, 16384), repeat=3)})
    ids = (-1, *range(count), count)   # (an id on either side of the table as well)
    return {
        "resolve": [list(r) + t.resolve(lib, fam, *r) for r in rows],
        "plan": [list(s) + t.plan(lib, fam, *s) for s in shapes],
        "runs": [[cid, *s] + t.runs(lib, fam, cid, *s) for cid in ids for s in strided],
        "workspace": [[cid, word, *s] + t.workspace(lib, fam, cid, word, *s) for cid in ids for word in (3, 33 | NT_STORE, 8 | STREAMK)
                      for s in sorted({s[:3] for s in strided})],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the library to record (default: the tree's, built if need be)")
    a = ap.parse_args()
    if a.lib:
        path = a.lib
    else:
        import build

        path = str(build.build_library())
    lib = t.prepare(ctypes.CDLL(path))
    golden = {fam: record(lib, fam) for fam in t.FAMILIES}
    lines = ["{"]
    for fam in t.FAMILIES:
        lines.append(f' "{fam}": {{')
        for what in t.CALLS:
            lines.append(f'  "{what}": [')
            lines += ["   " + json.dumps(r, separators=(",", ":")) + "," for r in golden[fam][what]]
            lines[-1] = lines[-1][:-1]
            lines.append("  ]," if what != list(t.CALLS)[-1] else "  ]")
        lines.append(" }," if fam != t.FAMILIES[-1] else " }")
    lines.append("}")
    t.GOLDEN.write_text("\n".join(lines) + "\n")
    print(f"{t.GOLDEN}: {sum(len(v) for f in golden.values() for v in f.values())} rows, {t.GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
