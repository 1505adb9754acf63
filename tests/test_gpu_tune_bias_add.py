"""GPU test of hgemm_tune's two residual rows (`check|bench --layout tn --bf16 --bias-add`, bgemm_mi355x_tn_bias_add, and `--layout nn --bf16
--nn-add`, bgemm_mi355x_nn_add): the check on one tile with one stage, ragged tiles over two stages, and a shape outside the kernels' scope
(the reference kernel) with 0 failures -- every member x {plain, non-temporal, splits 2, 5}, each run out of place from a NaN-filled output
and once more in place, to bits --, and a bench of one small shape whose record carries its keys.  No time is compared with anything."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

PKG = Path(__file__).resolve().parent.parent / "cuda-l2_amd"
SHAPES = ["64_64_64", "65_72_128", "33_17_40"]
KINDS = {"bias-add": (["--layout", "tn", "--bf16", "--bias-add"], "tn-bf16-bias-add", "the TN kernels", "c16_bias_add", ("bias_add_us", "unfused_us", "bias_us"),
                      "bias_add_le_unfused"),
         "nn-add": (["--layout", "nn", "--bf16", "--nn-add"], "nn-bf16-add", "the NN kernels", "c16_add", ("nn_add_us", "unfused_us", "nn_us"), "nn_add_le_unfused")}


@pytest.fixture(scope="module")
def tool():
    import build

    (exe,) = build.build_tools()
    return exe, ctypes.CDLL(str(build.build_library()))


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_residual_check_and_the_bench(tool, tmp_path, kind):
    exe, lib = tool
    flags, label, kernels, output, times, verdict = KINDS[kind]
    members = lib.bgemm_mi355x_tn_num_configs() if kind == "bias-add" else lib.hgemm_mi355x_nn_num_configs()
    res = subprocess.run([str(exe), "check", *flags, "--shapes", ",".join(SHAPES)], capture_output=True, text=True, timeout=120)
    lines = res.stdout.splitlines()
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and not [ln for ln in lines if ln.startswith("FAIL")]
    runs, failures = map(int, re.fullmatch(r"check %s: (\d+) runs, (\d+) failures \(.*\)" % label, lines[-1]).groups())
    assert (runs, failures) == (3 * members * 4, 0)
    checked = [ln for ln in lines if ln.startswith("checked ")]
    for ln, mnk, why in zip(checked, SHAPES, (kernels, kernels, "outside their scope: the reference kernel")):
        assert ln.endswith(f" {mnk} ({why})"), ln
    assert len(checked) == 3
    out = tmp_path / "bench.jsonl"
    res = subprocess.run([str(exe), "bench", *flags, "--shape", "128_128_128", "--out", str(out)], capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr)
    assert res.returncode == 0
    (record,) = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert record["output"] == output and record["layout"] == flags[1] and record["mnk"] == "128_128_128"
    assert all(record[k] > 0 for k in times) and record["unfused_spread_us"] >= 0
    assert isinstance(record[verdict], bool) and {"config", "splits", "runs", "rounds", "protocol"} <= set(record)
