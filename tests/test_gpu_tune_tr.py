"""GPU tests of hgemm_tune's one check and one bench driver for the twelve transposed-read call kinds (the four activation kinds with
each of their three activations): the check on one tile with one stage, ragged tiles over two stages and a shape outside the kernels'
alignment rule (the reference kernel), and a bench of one small shape whose record must carry the keys, in order, of the variant's
committed records.  No time is compared with anything."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

PKG = Path(__file__).resolve().parent.parent / "cuda-l2_amd"
# flags -> (the library's member count, the words of the "checked" line, the committed record file under tuning/ -- None: no bench --,
# what picks the variant's records in it)
VARIANTS = {
    "--layout nn": ("hgemm_mi355x_nn_num_configs", "the NN kernels", "nn_first_look", {}),
    "--layout ta": ("hgemm_mi355x_ta_num_configs", "the TA kernels", "ta_first_look", {}),
    "--layout ta --c32": ("hgemm_mi355x_ta_num_configs", "the TA kernels", "ta_c32_first_look", {}),
    "--layout nn --bf16": ("hgemm_mi355x_nn_num_configs", "the NN kernels", "tr_bf16_first_look", {"layout": "nn", "output": "c16"}),
    "--layout ta --bf16": ("hgemm_mi355x_ta_num_configs", "the TA kernels", "tr_bf16_first_look", {"layout": "ta", "output": "c16"}),
    "--layout ta --c32 --bf16": ("hgemm_mi355x_ta_num_configs", "the TA kernels", "tr_bf16_first_look", {"layout": "ta", "output": "c32_accumulate"}),
    "--layout tn --bf16": ("bgemm_mi355x_tn_num_configs", "the TN kernels", "tn_bf16_first_look", {}),
    "--layout tn --bf16 --bias": ("bgemm_mi355x_tn_num_configs", "the TN kernels", "tn_bias_first_look", {}),
}
# The activation kinds, each with its three activations.  One activation per kind also runs the bench (a bench repeats the whole
# default-shape check first), a different one per kind so that each activation is benched somewhere.
for _flags, _count, _kernels, _record, _output, _benched in (
        ("--layout tn --bf16 --bias --act {}", "bgemm_mi355x_tn_num_configs", "the TN kernels", "tn_bias_act_first_look", "c16_bias_act", "gelu"),
        ("--layout tn --bf16 --bias --act {} --aux", "bgemm_mi355x_tn_num_configs", "the TN kernels", "mlp_backward_first_look", "c16_bias_act_aux", "relu"),
        ("--layout nn --bf16 --dact {}", "hgemm_mi355x_nn_num_configs", "the NN kernels", "mlp_backward_first_look", "c16_dact", "gelu_tanh"),
        ("--layout nn --bf16 --dact {} --dbias", "hgemm_mi355x_nn_num_configs", "the NN kernels", "dbias_tune_bench", "c16_dact_dbias", "relu")):
    for _act in ("relu", "gelu", "gelu_tanh"):
        VARIANTS[_flags.format(_act)] = (_count, _kernels, _record if _act == _benched else None, {"output": _output})


@pytest.fixture(scope="module")
def tool():
    import build

    (exe,) = build.build_tools()
    return exe, ctypes.CDLL(str(build.build_library()))


@pytest.mark.parametrize("flags", VARIANTS)
def test_variant_check_and_bench(tool, tmp_path, flags):
    exe, lib = tool
    count_fn, kernels, record_file, pick = VARIANTS[flags]
    members = getattr(lib, count_fn)()
    c32 = "--c32" in flags
    # M % 8 is the TA layout's rule, so its ragged shape is ragged in tiles only
    shapes = ["64_64_64", "72_72_128" if "ta" in flags else "65_72_128", "33_17_40"]
    res = subprocess.run([str(exe), "check", *flags.split(), "--shapes", ",".join(shapes)], capture_output=True, text=True, timeout=120)
    lines = res.stdout.splitlines()
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and not [ln for ln in lines if ln.startswith("FAIL")]
    runs, failures = map(int, re.fullmatch(r"check \S+: (\d+) runs, (\d+) failures \(.*\)", lines[-1]).groups())
    assert (runs, failures) == (3 * members * 4 * (2 if c32 else 1), 0)
    checked = [ln for ln in lines if ln.startswith("checked ")]
    assert len(checked) == 3
    for ln, mnk, why in zip(checked, shapes, (kernels, kernels, "outside their scope: the reference kernel")):
        assert ln.endswith(f" {mnk} ({why})"), ln
    if record_file is None:
        return

    out = tmp_path / "bench.jsonl"
    res = subprocess.run([str(exe), "bench", *flags.split(), "--shape", "128_128_128", "--out", str(out)], capture_output=True, text=True,
                         timeout=120)
    print(res.stdout[-2000:], res.stderr)
    assert res.returncode == 0
    (record,) = [json.loads(ln) for ln in out.read_text().splitlines()]
    committed = [json.loads(ln) for ln in (PKG / "tuning" / f"{record_file}_mi355x.jsonl").read_text().splitlines()]
    key_lists = {tuple(k for k in r if k not in ("auto_nn_us", "auto_nn_tflops")) for r in committed if all(r[k] == v for k, v in pick.items())}
    assert key_lists == {tuple(record)}
    # the contenders' times (every "<key>_us" beside a "<key>_tflops"); a spread, the slowest round minus the median, may be zero
    times = [k for k in record if k.endswith("_us") and k[:-3] + "_tflops" in record]
    assert times and all(record[k] > 0 for k in times), record
    assert all(record[k] >= 0 for k in record if k.endswith("_spread_us")), record
