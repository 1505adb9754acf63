"""GPU test of hgemm_tune's gated row (`check|bench --layout tn --bf16 --gated A`, bgemm_mi355x_tn_gated): the check on one tile with one
stage, ragged tiles over two stages with a sliver N, and a shape outside the kernels' alignment rule (the reference kernel) with 0 failures
-- every member x {plain, non-temporal, splits 2, 5}, ReLU to bits, the others to the bar, from a NaN-filled C with sentinels behind it --,
and for SiLU a bench of one small shape whose record carries the keys of the committed records.  No time is compared with anything."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

PKG = Path(__file__).resolve().parent.parent / "cuda-l2_amd"
SHAPES = ["64_32_64", "65_72_128", "33_20_40"]


@pytest.fixture(scope="module")
def tool():
    import build

    (exe,) = build.build_tools()
    return exe, ctypes.CDLL(str(build.build_library()))


@pytest.mark.parametrize("act", ["relu", "gelu", "gelu_tanh", "silu"])
def test_the_gated_check_and_for_silu_the_bench(tool, tmp_path, act):
    exe, lib = tool
    flags = ["--layout", "tn", "--bf16", "--gated", act]
    members = lib.bgemm_mi355x_tn_num_configs()
    res = subprocess.run([str(exe), "check", *flags, "--shapes", ",".join(SHAPES)], capture_output=True, text=True, timeout=120)
    lines = res.stdout.splitlines()
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and not [ln for ln in lines if ln.startswith("FAIL")]
    runs, failures = map(int, re.fullmatch(r"check tn-bf16-gated-%s: (\d+) runs, (\d+) failures \(.*\)" % act, lines[-1]).groups())
    assert (runs, failures) == (3 * members * 4, 0)
    checked = [ln for ln in lines if ln.startswith("checked ")]
    for ln, mnk, why in zip(checked, SHAPES, ("the TN kernels", "the TN kernels", "outside their scope: the reference kernel")):
        assert ln.endswith(f" {mnk} ({why})"), ln
    assert len(checked) == 3
    if act != "silu":
        return
    out = tmp_path / "bench.jsonl"
    res = subprocess.run([str(exe), "bench", *flags, "--shape", "128_128_128", "--out", str(out)], capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr)
    assert res.returncode == 0
    (record,) = [json.loads(ln) for ln in out.read_text().splitlines()]
    committed = [json.loads(ln) for ln in (PKG / "tuning" / "gated_tune_bench_mi355x.jsonl").read_text().splitlines()]
    assert {tuple(r) for r in committed} == {tuple(record)} and record["output"] == "c16_gated" and record["act"] == "silu"
    assert all(record[k] > 0 for k in ("gated_us", "unfused_us", "product_2n_us")) and record["unfused_spread_us"] >= 0
    assert isinstance(record["gated_le_unfused"], bool)
