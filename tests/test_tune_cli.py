"""CPU tests of hgemm_tune's command line for the transposed-read variants (--layout nn|ta|tn with --bf16, --c32, --bias, --act A,
--aux, --dact A, --dbias): which
variant the flags resolve to is decided before a device is asked for, so every refusal -- its exact stderr line, exit status 2 -- shows
on a machine without a GPU, where a command line the tool accepts ends with "no HIP device visible" and status 3 instead."""
import subprocess

import pytest
import torch

BIAS = "--bias goes with --layout tn --bf16 (bgemm_mi355x_tn_bias)"
NO_SHAPE = "bench needs --shape"
REFUSED = [
    ("check --layout xx", "--layout takes nn, ta or tn"),
    ("check --layout nn --bias", BIAS),
    ("check --layout nn --bf16 --bias", BIAS),
    ("check --layout nn --c32", "--c32 goes with --layout ta"),
    ("check --bf16", "--bf16 goes with --layout nn, ta or tn (the fp16 b_col_major families have no bf16 form)"),
    ("tune --layout nn --shapes 64_64_64", "--layout nn goes with check or bench"),
    ("tune --layout ta --shapes 64_64_64", "--layout ta goes with check or bench"),
    ("tune --layout tn --bf16 --shapes 64_64_64", "--layout tn --bf16 goes with check or bench"),
    ("bench --layout nn", NO_SHAPE),
    ("bench --layout ta --c32", NO_SHAPE),
    ("bench --layout tn --bf16 --bias", NO_SHAPE),
    ("check --layout tn --bf16 --act relu", "--act goes with --layout tn --bf16 --bias (bgemm_mi355x_tn_bias_act)"),
    ("check --layout tn --bf16 --bias --aux", "--aux goes with --layout tn --bf16 --bias --act A (bgemm_mi355x_tn_bias_act_aux)"),
    ("check --layout ta --bf16 --dact gelu", "--dact goes with --layout nn --bf16 (bgemm_mi355x_nn_dact)"),
    ("check --layout nn --bf16 --dbias", "--dbias goes with --layout nn --bf16 --dact A (bgemm_mi355x_nn_dact_dbias)"),
    ("bench --layout nn --bf16 --dact relu", NO_SHAPE),
]
ACTS = ("relu", "gelu", "gelu_tanh")
# the activation kinds: four call kinds, the activation a value of the call
ACT_VARIANTS = [flags.format(a) for flags in ("--layout tn --bf16 --bias --act {}", "--layout tn --bf16 --bias --act {} --aux",
                                              "--layout nn --bf16 --dact {}", "--layout nn --bf16 --dact {} --dbias") for a in ACTS]
VARIANTS = ["--layout nn", "--layout ta", "--layout ta --c32", "--layout nn --bf16", "--layout ta --bf16", "--layout ta --c32 --bf16",
            "--layout tn --bf16", "--layout tn --bf16 --bias", *ACT_VARIANTS]


@pytest.fixture(scope="module")
def tune():
    import build

    (exe,) = build.build_tools()
    return lambda line: subprocess.run([str(exe), *line.split()], capture_output=True, text=True, timeout=30)


@pytest.mark.parametrize("line,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_command_line(tune, line, message):
    res = tune(line)
    assert res.returncode == 2 and res.stderr == message + "\n" and res.stdout == "", (res.returncode, res.stdout, res.stderr)


@pytest.mark.skipif(torch.cuda.is_available(), reason="an accepted command line starts its check where a GPU is visible: tests/test_gpu_tune_tr.py")
@pytest.mark.parametrize("flags", VARIANTS)
def test_accepted_command_line_reaches_the_device_query(tune, flags):
    res = tune(f"check {flags} --shapes 64_64_64")
    assert res.returncode == 3 and res.stderr.endswith("hgemm_tune: no HIP device visible\n"), (res.returncode, res.stderr)
