"""GPU test of hgemm_tune's gated aux row (`check --layout tn --bf16 --gated-aux A`, bgemm_mi355x_launch_tn_gated_aux): the check on the
tool's default shapes -- one tile, ragged M / N, a sliver, 1 .. 7 K stages, a long K, and three shapes outside the kernels' scope (the
reference kernel) -- for one activation with 0 failures: every member x {plain, non-temporal, splits 2, 5}, C to the gated bar, g_out and
u_out bit for bit, from NaN-filled outputs with sentinel bytes behind each of the three.  No time is compared with anything."""
import ctypes
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    import build

    (exe,) = build.build_tools()
    return exe, ctypes.CDLL(str(build.build_library()))


def test_the_gated_aux_check_on_the_default_shapes(tool):
    exe, lib = tool
    act = "silu"
    members = lib.bgemm_mi355x_tn_num_configs()
    res = subprocess.run([str(exe), "check", "--layout", "tn", "--bf16", "--gated-aux", act], capture_output=True, text=True, timeout=300)
    lines = res.stdout.splitlines()
    print(res.stdout[-3000:], res.stderr)
    assert res.returncode == 0 and not [ln for ln in lines if ln.startswith("FAIL")]
    checked = [ln for ln in lines if ln.startswith("checked ")]
    assert len(checked) == 13 and sum(ln.endswith("(the TN kernels)") for ln in checked) == 10
    runs, failures = map(int, re.fullmatch(r"check tn-bf16-gated-aux-%s: (\d+) runs, (\d+) failures \(.*\)" % act, lines[-2]).groups())
    assert (runs, failures) == (13 * members * 4, 0)
    assert lines[-1] == f"check tn-bf16-gated-aux-{act}: g_out and u_out bit-exact against bf16(g) and bf16(u) in every run"
