"""GPU test of hgemm_tune's dgated row (`check|bench --layout nn --bf16 --dgated A`, bgemm_mi355x_nn_dgated): the check on one tile with one
stage, ragged tiles over two stages, and a shape outside the kernels' scope (the reference kernel) with 0 failures -- every member x {plain,
non-temporal, splits 2, 5}, ReLU to bits, the others to the two bars, from NaN-filled outputs with sentinels behind them --, and for SiLU a
bench of one small shape whose record carries its keys.  No time is compared with anything."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

PKG = Path(__file__).resolve().parent.parent / "cuda-l2_amd"
SHAPES = ["64_64_64", "65_72_128", "33_17_40"]


@pytest.fixture(scope="module")
def tool():
    import build

    (exe,) = build.build_tools()
    return exe, ctypes.CDLL(str(build.build_library()))


@pytest.mark.parametrize("act", ["relu", "gelu", "gelu_tanh", "silu"])
def test_the_dgated_check_and_for_silu_the_bench(tool, tmp_path, act):
    exe, lib = tool
    flags = ["--layout", "nn", "--bf16", "--dgated", act]
    members = lib.hgemm_mi355x_nn_num_configs()
    res = subprocess.run([str(exe), "check", *flags, "--shapes", ",".join(SHAPES)], capture_output=True, text=True, timeout=120)
    lines = res.stdout.splitlines()
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and not [ln for ln in lines if ln.startswith("FAIL")]
    runs, failures = map(int, re.fullmatch(r"check nn-bf16-dgated-%s: (\d+) runs, (\d+) failures \(.*\)" % act, lines[-1]).groups())
    assert (runs, failures) == (3 * members * 4, 0)
    checked = [ln for ln in lines if ln.startswith("checked ")]
    for ln, mnk, why in zip(checked, SHAPES, ("the NN kernels", "the NN kernels", "outside their scope: the reference kernel")):
        assert ln.endswith(f" {mnk} ({why})"), ln
    assert len(checked) == 3
    if act != "silu":
        return
    out = tmp_path / "bench.jsonl"
    res = subprocess.run([str(exe), "bench", *flags, "--shape", "128_128_128", "--out", str(out)], capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr)
    assert res.returncode == 0
    (record,) = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert record["output"] == "c16_dgated" and record["act"] == "silu" and record["layout"] == "nn" and record["mnk"] == "128_128_128"
    assert all(record[k] > 0 for k in ("dgated_us", "unfused_us", "nn_us")) and record["unfused_spread_us"] >= 0
    assert isinstance(record["dgated_le_unfused"], bool) and {"config", "splits", "runs", "rounds", "protocol"} <= set(record)
