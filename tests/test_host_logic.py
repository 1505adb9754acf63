"""CPU tests of the host side: C-ABI library loads and exports everything include/hgemm_mi355x.h
declares, planner / geometry table / error paths (no compute calls without a GPU), harness plumbing
(BASELINE.json config 1: torch.matmul on the host through benchmarking_offline.py), summary rule,
shape-file generator, sweep merge."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "cuda-l2_amd"


@pytest.fixture(scope="module")
def lib():
    import build

    so = build.build_library()
    L = ctypes.CDLL(str(so))
    L.hgemm_mi355x_config_name.restype = ctypes.c_char_p
    L.hgemm_mi355x_strerror.restype = ctypes.c_char_p
    L.hgemm_mi355x_version.restype = ctypes.c_char_p
    L.hgemm_mi355x_model_us.restype = ctypes.c_double
    L.hgemm_mi355x_model_us.argtypes = [ctypes.c_int] * 5
    L.hgemm_mi355x_workspace_bytes.restype = ctypes.c_size_t
    return L


def header_functions():
    text = (REPO / "include" / "hgemm_mi355x.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hgemm_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(lib):
    names = header_functions()
    assert len(names) >= 30
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/hgemm_mi355x.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "lib" / "libhgemm_mi355x.so")], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (hgemm_[a-z0-9_]+)", nm))
    assert set(names) <= exported
    # nothing from the oracle may be linked into the product
    assert "hgemm_oracle" not in nm
    assert b"gfx950" in lib.hgemm_mi355x_version()


def test_geometry_table(lib):
    n = lib.hgemm_mi355x_num_configs()
    assert n >= 24
    seen = set()
    for i in range(n):
        name = lib.hgemm_mi355x_config_name(i).decode()
        assert name not in seen
        seen.add(name)
        info = (ctypes.c_int * 8)()
        assert lib.hgemm_mi355x_config_info(i, info) == 0
        bm, bn, wm, wn, mi, nbuf, threads, lds = list(info)
        # 64-wide waves; the "_k4" members of family w put four waves on ONE wave tile (they split its K walk)
        assert threads == wm * wn * 64 * (4 if name.endswith("_k4") else 1) and threads % 64 == 0
        assert lds <= 160 * 1024                                   # MI355X LDS per CU
        assert bm % (wm * mi) == 0 and bn % (wn * mi) == 0
        assert lib.hgemm_mi355x_config_by_name(name.encode()) == i
    assert lib.hgemm_mi355x_config_name(n) is None
    assert lib.hgemm_mi355x_config_by_name(b"no_such_geometry") == -1
    assert lib.hgemm_mi355x_config_info(-1, (ctypes.c_int * 8)()) == -1


@pytest.mark.parametrize("mnk", [(64, 4096, 64), (512, 4096, 4096), (4096, 4096, 4096), (64, 64, 16384),
                                 (16384, 16384, 16384), (200, 136, 128)])
def test_planner_returns_a_valid_plan(lib, mnk):
    cfg, splits, group = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.hgemm_mi355x_plan(*mnk, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    assert 0 <= cfg.value < lib.hgemm_mi355x_num_configs()
    count = splits.value & 0xFFFF          # | 0x10000 = HGEMM_SPLITK_FUSED (single-launch form), | 0x20000 = HGEMM_PLAN_NT_STORE,
    assert splits.value & ~0x1FFFFF == 0   # | 0x40000 = HGEMM_PLAN_STREAMK (the count is then the number of persistent workgroups), | 0x80000 / 0x100000: family r
    if splits.value & 0x40000:
        assert lib.hgemm_mi355x_config_streamk(cfg.value) > 0 and count <= 4096 and group.value >= 1
    else:
        assert 1 <= count <= max(1, mnk[2] // 64) and group.value >= 1
    assert lib.hgemm_mi355x_model_us(cfg.value, splits.value, *mnk) > 0
    info = (ctypes.c_int * 8)()
    lib.hgemm_mi355x_config_info(cfg.value, info)
    assert info[0] <= 2 * max(mnk[0], 32) and info[1] <= 2 * max(mnk[1], 32)  # no tile that is mostly padding


def test_planner_routes_ragged_shapes_to_the_register_staged_mfma_kernel(lib):
    cfg, splits, group = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.hgemm_mi355x_plan(100, 30, 50, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    assert cfg.value == -2 and splits.value == 1      # HGEMM_CONFIG_RAGGED (K % 64 != 0, N % 4 != 0)
    assert lib.hgemm_mi355x_plan(65, 30, 100, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    assert cfg.value == -2
    # K % 64 != 0 but K % 8 == 0: a classic ("t") geometry, which zero-fills its partial last K-step by itself
    assert lib.hgemm_mi355x_plan(1000, 520, 200, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    assert cfg.value >= 0 and lib.hgemm_mi355x_config_name(cfg.value).decode().startswith("t")
    assert lib.hgemm_mi355x_config_k_granularity(cfg.value) == 8
    # ... round 4: or a member of family q / r, whose "ktail" kernel variants accumulate the remainder from directly loaded fragments
    assert lib.hgemm_mi355x_plan(4000, 4000, 4000, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    assert cfg.value >= 0 and lib.hgemm_mi355x_config_name(cfg.value).decode() == "q256x256_w2x2"
    assert lib.hgemm_mi355x_config_k_granularity(cfg.value) == 8 and lib.hgemm_mi355x_config_accepts_k(cfg.value, 4000) == 1
    # (at least one whole stage must exist: K = 40 is not for them, and the 32x32x16 members have no tail)
    assert lib.hgemm_mi355x_config_accepts_k(cfg.value, 40) == 0 and lib.hgemm_mi355x_config_accepts_k(cfg.value, 64) == 1
    assert lib.hgemm_mi355x_config_accepts_k(cfg.value, 4004) == 0
    m32 = lib.hgemm_mi355x_config_by_name(b"q256x256_w2x2_m32")
    assert m32 >= 0 and lib.hgemm_mi355x_config_accepts_k(m32, 4000) == 0 and lib.hgemm_mi355x_config_accepts_k(m32, 4032) == 1
    r256 = lib.hgemm_mi355x_config_by_name(b"r64x64_k256")
    assert [lib.hgemm_mi355x_config_accepts_k(r256, k) for k in (200, 256, 264, 512, 9160, 9164)] == [0, 1, 1, 1, 1, 0]
    t = lib.hgemm_mi355x_config_by_name(b"t64x64_w2x2_m16_s4")
    assert [lib.hgemm_mi355x_config_accepts_k(t, k) for k in (8, 40, 64, 200, 204)] == [1, 1, 1, 1, 0]
    assert lib.hgemm_mi355x_config_accepts_k(-2, 7) == 1
    assert lib.hgemm_mi355x_plan(1000, 520, 192, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    assert cfg.value >= 0                              # aligned: an LDS-DMA geometry
    assert lib.hgemm_mi355x_plan(0, 4, 4, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == -1


def test_error_paths_do_not_touch_the_gpu(lib):
    assert lib.hgemm_mi355x_fp32(None, None, None, None, 64, 64, 64, None) == -1
    assert lib.hgemm_mi355x_launch(0, 1, 1, None, None, None, None, 64, 64, 64, 64, 64, 64, None) == -1
    assert lib.hgemm_mi355x_launch(10 ** 6, 1, 1, ctypes.c_void_p(16), None, ctypes.c_void_p(16), ctypes.c_void_p(16),
                                   64, 64, 64, 64, 64, 64, None) == -1
    assert lib.hgemm_rocblas_nn(None, None, None, 64, 64, 64, 0, None) == -1
    assert lib.hgemm_hipblaslt_autotune_nn(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 64, 64, 64, 0,
                                           None) == -5  # NOT_READY: no find_best call yet
    assert lib.hgemm_mi355x_strerror(-5).decode().startswith("baseline not")
    # counters (256 KiB) + tile-padded slabs: a sufficient size for either split-K form
    assert lib.hgemm_mi355x_workspace_bytes(64, 128, 4) == (256 << 10) + 4 * 256 * 256 * 4
    assert lib.hgemm_mi355x_workspace_bytes(64, 128, 4 | 0x10000) == (256 << 10) + 4 * 256 * 256 * 4
    assert lib.hgemm_mi355x_workspace_bytes(64, 128, 1) == 0
    # a bad special config id is rejected before any device work
    assert lib.hgemm_mi355x_launch(-3, 1, 1, ctypes.c_void_p(16), None, ctypes.c_void_p(16), ctypes.c_void_p(16),
                                   64, 64, 64, 64, 64, 64, None) == -1


def test_shipping_library_has_no_ablation_switch():
    """The tuner's ablation flags (results garbage by construction) exist only in the -DHGEMM_ABLATION build."""
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "lib" / "libhgemm_mi355x.so")], capture_output=True,
                        text=True, check=True).stdout
    assert "hgemm_mi355x_set_debug" not in nm
    assert "set_debug" not in (REPO / "include" / "hgemm_mi355x.h").read_text()


def test_cpu_plumbing_config_writes_the_reference_json_schema(tmp_path):
    """BASELINE.json config 1: M=64 N=4096 K=64 via torch.matmul on the CPU (no GPU, no extension)."""
    cmd = [sys.executable, "benchmarking_offline.py", "--mnk", "64_4096_64", "--acc_precise", "fp32", "--device_type",
           "mi355x", "--warmup_seconds", "0.05", "--benchmark_seconds", "0.3", "--base_dir", str(tmp_path),
           "--gpu_device_id", "0", "--perf_func", "matmul", "--device", "cpu", "--seed", "0"]
    res = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    data = json.loads((tmp_path / "benchmark_result_matmul.json").read_text())
    assert data["records"]["version"] == "202511261845" and data["records"]["matmul"] > 0
    assert data["device"] == "cpu" and data["cpu"]["os_cpu_count"] >= 1
    lat = data["latency_ms"]["matmul"]
    assert lat["p50"] <= lat["p99"]
    # a GPU perf_func cannot run on the host path, and the extension refuses to load without a GPU
    bad = subprocess.run(cmd[:-5] + ["--perf_func", "hgemm_cublas_tn", "--device", "cpu"], cwd=PKG, capture_output=True, text=True)
    assert bad.returncode != 0


def test_extension_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tools.utils import build_from_sources

    with pytest.raises(RuntimeError, match="needs a visible MI355X"):
        build_from_sources("64_4096_64", "fp32", "mi355x", "/tmp/never", False)


def test_server_mode_sleep_and_tflops_formula(monkeypatch, tmp_path):
    import benchmarking_server
    import benchmarking_utils
    import torch

    slept = []
    monkeypatch.setattr(benchmarking_server.time, "sleep", lambda s: slept.append(s))
    args = benchmarking_server.build_arg_parser().parse_args(
        ["--mnk", "32_48_64", "--acc_precise", "fp32", "--device_type", "mi355x", "--warmup_seconds", "0.02",
         "--benchmark_seconds", "0.1", "--base_dir", str(tmp_path), "--gpu_device_id", "0", "--perf_func", "matmul",
         "--device", "cpu", "--target_qps", "1000", "--seed", "1"])
    result = benchmarking_server.offline.run(args, extra={"target_qps": args.target_qps})
    assert result["mode"] == "server" and result["target_qps"] == 1000 and len(slept) >= result["iterations"]
    assert all(s >= 0 for s in slept)
    rec = benchmarking_utils.run_all_perf_funcs_once(perf_func_list=[torch.matmul], m=32, n=48, k=64, acc_precise="fp32",
                                                     device_type="mi355x", padding_m=0, padding_k=0, padding_n=0, device="cpu")
    assert rec["matmul"] == pytest.approx(2 * 32 * 48 * 64 * 1e-12 * 1000 / rec["matmul_ms"])


def test_summary_max_row_is_the_stronger_baseline(tmp_path):
    import summarize_result

    def put(name, base, ours):
        (tmp_path / f"benchmark_result_{name}.json").write_text(json.dumps(
            {"records": {name: base, "cuda_l2_mi355x_fp32": ours, "version": "x"}}))

    put("hgemm_cublas_tn", 100.0, 120.0)              # speedup 1.2
    put("hgemm_cublas_nn", 80.0, 118.0)               # speedup 1.475 -> -max must pick tn (lower speedup)
    put("hgemm_cublaslt_heuristic_tn", 100.0, 90.0)
    put("hgemm_cublaslt_heuristic_nn", 110.0, 91.0)   # 0.827 -> -max picks nn
    put("hgemm_cublaslt_auto_tuning_tn", 50.0, 100.0)
    put("hgemm_cublaslt_auto_tuning_nn", 50.0, 99.0)
    put("matmul", 60.0, 120.0)
    rows = {r["Baseline Method Name"]: r for r in summarize_result.summarize(tmp_path, "cuda_l2_mi355x_fp32")}
    assert list(rows) == summarize_result.NAME_ORDER
    assert rows["rocBLAS-max"]["Baseline TFLOPS"] == 100.0 and rows["rocBLAS-max"]["Speedup"] == pytest.approx(1.2)
    assert rows["hipBLASLt-heuristic-max"]["Baseline TFLOPS"] == 110.0
    assert rows["hipBLASLt-auto-tuning-max"]["Speedup"] == pytest.approx(1.98)
    assert rows["torch.matmul"]["Speedup"] == pytest.approx(2.0)


def test_shape_file_generator_and_sources(tmp_path):
    from tools import gen_shape_kernels as gen
    from tools.utils import compute_padding, get_build_sources, kernel_source_path

    shapes = gen.grid_shapes()
    assert len(shapes) == 1000 and shapes[0] == "64_64_64" and "12288_16384_64" in shapes
    for mnk in ["64_4096_64", "512_4096_4096", "4096_4096_4096"]:       # the BASELINE.json shapes are committed
        for acc in ("fp16", "fp32"):
            text = kernel_source_path(mnk, acc, "mi355x").read_text()
            assert "HGEMM_MI355X_SHAPE_ENTRY(" + ", ".join(mnk.split("_")) in text
            assert compute_padding(*map(int, mnk.split("_")), text) == (0, 0, 0)
    srcs = get_build_sources("64_4096_64", "fp16", "mi355x")
    assert srcs[-1] == "pybind/hgemm_mi355x_fp16.cc" and "F16F16F16F16" in srcs[-2]
    for s in srcs:
        assert (PKG / s).exists()
    with pytest.raises(ValueError):
        get_build_sources("64_4096_64", "bf16", "mi355x")
    name, splits, group = gen.model_plan(4096, 4096, 4096)
    assert splits >= 1 and group >= 1 and name


def test_sweep_shard_and_merge(tmp_path):
    from tools import sweep

    shapes = [f"{64 * (i + 1)}_64_64" for i in range(11)]
    parts = [sweep.shard(shapes, r, 4) for r in range(4)]
    assert sorted(sum(parts, [])) == sorted(shapes) and max(map(len, parts)) - min(map(len, parts)) <= 1
    with pytest.raises(ValueError):
        sweep.shard(shapes, 4, 4)
    for mnk, sp in [(shapes[0], 1.5), (shapes[1], 0.5)]:
        d = sweep.shape_dir(tmp_path, "fp32", "offline", mnk)
        d.mkdir(parents=True)
        rows = [{"Baseline Method Name": c, "Baseline TFLOPS": 10.0, "CUDA-L2 TFLOPS": 10.0 * sp, "Speedup": sp}
                for c in sweep.CSV_COLUMNS]
        (d / "summary.json").write_text(json.dumps(rows))
    assert sweep.is_done(tmp_path, "fp32", "offline", shapes[0]) and not sweep.is_done(tmp_path, "fp32", "offline", shapes[2])
    rep = sweep.merge(tmp_path, "fp32", "offline", shapes)
    assert rep["shapes"] == 2
    assert rep["geomean_speedup_vs_hipBLASLt-auto-tuning-max"] == pytest.approx((1.5 * 0.5) ** 0.5)
    assert rep["mean_speedup_vs_torch.matmul"] == pytest.approx(1.0)
    csv = Path(rep["csv"]).read_text().splitlines()
    assert csv[0].startswith("mnk,torch.matmul,rocBLAS-tn") and csv[1].startswith(shapes[0] + ",1.500")


def _tuned_rows():
    import re

    rows = []
    for ln in (PKG / "csrc" / "hgemm_tuned_table.inc").read_text().splitlines():
        mm = re.match(r'\s*\{(\d+), (\d+), (\d+), "([^"]+)", (\d+), (\d+)\}', ln)
        if mm:
            rows.append((int(mm[1]), int(mm[2]), int(mm[3]), mm[4], int(mm[5]), int(mm[6])))
    return rows


def test_tuned_table_rows_are_what_the_planner_returns(lib):
    """Every committed tuned plan is served verbatim by hgemm_mi355x_plan (names resolve, no stale rows)."""
    rows = _tuned_rows()
    assert len(rows) == 1000
    for (m, n, k, name, splits, group) in rows:
        cfg, sp, gm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.hgemm_mi355x_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(sp), ctypes.byref(gm)) == 0
        assert lib.hgemm_mi355x_config_name(cfg.value).decode() == name, (m, n, k)
        assert (sp.value, gm.value) == (splits, group), (m, n, k)
        assert k % lib.hgemm_mi355x_config_k_granularity(cfg.value) == 0


def test_every_shipped_plan_has_an_exact_oracle_record():
    """994 of 1000 shipped plans had never been compared with the oracle.  Now the table generator only
    adopts plans with a passing record of tests/tools/verify_plans.py (the reference's 0/1 rule, bit-exact against
    the CPU oracle, measured on an MI355X); the records are committed and this test ties the table to them."""
    ok = set()
    # (round 3's table + the two passes of the round-4 re-tune, tools/update_tuned_table.py --verified)
    # + the four passes of the round-5 re-tune
    for name in ("r03_candidate_parity.jsonl", "r04_candidate_parity_pass1.jsonl", "r04_candidate_parity_pass2.jsonl",
                 "r04_candidate_parity_family_r_flags.jsonl", "r04_candidate_parity_family_r_flags_pass2.jsonl",
                 "r04_candidate_parity_worst_rows.jsonl", "r05_candidate_parity_pass1.jsonl", "r05_candidate_parity_pass2.jsonl",
                 "r05_candidate_parity_pass3.jsonl", "r05_candidate_parity_pass4.jsonl",
                 # round 6: the "fused" re-tune (three passes on three boxes)
                 "r06_candidate_parity_fused_pass1.jsonl", "r06_candidate_parity_fused_pass2.jsonl", "r06_candidate_parity_fused_pass3.jsonl",
                 # ... and the wide re-tune (the model's candidates on the whole grid, three boxes)
                 "r06_candidate_parity_wide_pass1.jsonl", "r06_candidate_parity_wide_pass2.jsonl", "r06_candidate_parity_wide_pass3.jsonl",
                 # ... and the flag pass (K stagger / NT stores / phase offset / raster group toggles, three boxes)
                 "r06_candidate_parity_flags_pass1.jsonl", "r06_candidate_parity_flags_pass2.jsonl", "r06_candidate_parity_flags_pass3.jsonl"):
        for ln in (PKG / "tuning" / name).read_text().splitlines():
            r = json.loads(ln)
            if r["pass"] and r["bitwise_equal_unmasked"] and r["guard_bars_intact"] and r["max_diff_masked"] == 0.0:
                ok.add((r["mnk"], r["plan"]["config"], r["plan"]["splits"], r["plan"]["group_m"]))
    missing = [(m, n, k, c) for (m, n, k, c, s, g) in _tuned_rows() if (f"{m}_{n}_{k}", c, s, g) not in ok]
    assert not missing, missing[:5]
    # ... and the whole-grid run of the SHIPPED table through both entry points (2 x 1000 records, all exact)
    # (the closing run of the round writes r06_parity_1000.jsonl / r06_randn_1000.jsonl for the table as it ships; until they exist the
    # round-5 records stand for the rows round 6 did not change)
    rnd = "r06" if (PKG / "tuning" / "r06_parity_1000.jsonl").exists() else "r05"
    changed6 = set() if rnd == "r06" else {json.loads(ln)["mnk"] for f in (PKG / "tuning").glob("r06_*_changes.jsonl") for ln in f.read_text().splitlines()}
    recs = [json.loads(ln) for ln in (PKG / "tuning" / f"{rnd}_parity_1000.jsonl").read_text().splitlines()]
    assert len(recs) == 2000 and all(r["pass"] and r["bitwise_equal_unmasked"] for r in recs)
    assert {r["run"] for r in recs} == {"fp32", "fp16"} and len({r["mnk"] for r in recs}) == 1000
    shipped = {(f"{m}_{n}_{k}", c, s & 0xFFFF, bool(s & 0x10000), bool(s & 0x20000), bool(s & 0x40000), s >> 19, g) for (m, n, k, c, s, g) in _tuned_rows()}
    for r in recs:
        assert r["mnk"] in changed6 or (r["mnk"], r["plan"]["config"], r["plan"]["splits"], r["plan"]["fused"], r["plan"]["nt_store"], r["plan"]["streamk"],
                                        r["plan"]["plan_flags"], r["plan"]["group_m"]) in shipped, r["mnk"]
    # ... and the N(0,1) tolerance of the same table on the whole grid (BASELINE.json: 1e-3 / 1e-2 relative; 1e-3 for both here)
    rn = [json.loads(ln) for ln in (PKG / "tuning" / f"{rnd}_randn_1000.jsonl").read_text().splitlines()]
    assert len(rn) == 2000 and all(r["pass"] and r["relative_error"] <= 1e-3 and r["rows_checked"] >= 64 for r in rn)
    for r in rn:
        assert r["mnk"] in changed6 or (r["mnk"], r["plan"]["config"], r["plan"]["splits"], r["plan"]["fused"], r["plan"]["nt_store"], r["plan"]["streamk"],
                                        r["plan"]["plan_flags"], r["plan"]["group_m"]) in shipped, r["mnk"]


def test_analytic_model_picks_near_optimal_plans_on_the_measured_candidates(lib):
    """Off-grid shapes are planned by the analytic model.  Its constants are fitted to the measured
    candidates of the tuning run; this pins the fit: the model's pick among the measured (config, splits)
    pairs of every grid shape must stay within a few percent of the measured best (geomean regret)."""
    import math

    lib.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    regrets = []
    for line in (PKG / "tuning" / "r01_grid_tune_run2_mi355x.jsonl").read_text().splitlines():
        r = json.loads(line)
        m, n, k = (int(x) for x in r["mnk"].split("_"))
        measured = {}
        for c in r["candidates"]:
            if c["config"].startswith("p"):   # staggered family of round 1: removed from the library
                continue
            key = (c["config"], c["splits"])
            measured[key] = min(measured.get(key, 1e30), c["us"])
        ids = {key: lib.hgemm_mi355x_config_by_name(key[0].encode()) for key in measured}
        assert min(ids.values()) >= 0
        pick = min(measured, key=lambda key: lib.hgemm_mi355x_model_us(ids[key], key[1], m, n, k))
        regrets.append(measured[pick] / min(measured.values()))
    geomean = math.exp(sum(map(math.log, regrets)) / len(regrets))
    assert len(regrets) == 1000
    assert geomean < 1.04, geomean          # 1.02 on the run the constants were fitted to
    assert sorted(regrets)[int(0.9 * len(regrets))] < 1.15


def test_report_tools_on_synthetic_inputs(tmp_path):
    """tools/plot_speedups.py, tools/tune_report.py and tools/pmc_summary.py parse what the GPU runs write."""
    sys.path.insert(0, str(PKG))
    from tools import plot_speedups, tune_report

    cols = ["torch.matmul", "rocBLAS-tn", "rocBLAS-nn", "rocBLAS-max", "hipBLASLt-heuristic-tn", "hipBLASLt-heuristic-nn",
            "hipBLASLt-heuristic-max", "hipBLASLt-auto-tuning-tn", "hipBLASLt-auto-tuning-nn", "hipBLASLt-auto-tuning-max"]
    csv_path = tmp_path / "s.csv"
    csv_path.write_text("mnk," + ",".join(cols) + "\n64_64_64," + ",".join(["1.5"] * 10) + "\n128_128_128," + ",".join(["1.1"] * 10) + "\n")
    means, n = plot_speedups.mean_speedups(str(csv_path))
    assert n == 2 and all(abs(m - 1.3) < 1e-9 for m in means)
    rows = [{"mnk": "64_64_64", "best": {"config": "t32x32_w1x1_m16_s4", "splits": 1, "group_m": 1, "us": 5.0},
             "rocblas_nn_us": 10.0, "rocblas_tn_us": 9.0, "hipblaslt_heur_nn_us": 8.0, "hipblaslt_heur_tn_us": 7.5, "candidates": []},
            {"mnk": "128_128_128", "best": {"config": "t32x32_w1x1_m16_s4", "splits": 1, "group_m": 1, "us": 6.0},
             "rocblas_nn_us": 6.0, "rocblas_tn_us": 6.0, "hipblaslt_heur_nn_us": 3.0, "hipblaslt_heur_tn_us": 12.0, "candidates": [],
             "hipblaslt_auto_nn_us": 2.0, "hipblaslt_auto_tn_us": 4.0}]
    jl = tmp_path / "t.jsonl"
    jl.write_text("".join(json.dumps(r) + "\n" for r in rows))
    xs, ys = plot_speedups.grid_points(str(jl))
    assert xs == [2.0 * 64 ** 3, 2.0 * 128 ** 3] and ys == [1.5, 0.5]
    rep = tune_report.main(str(jl), 1)
    assert abs(rep["geomean_speedup_vs_hipblaslt_heuristic_max"] - (1.5 * 0.5) ** 0.5) < 1e-9
    assert rep["autotune_shapes"] == 1 and abs(rep["geomean_speedup_vs_hipblaslt_autotune_max"] - 2.0 / 6.0) < 1e-9
    plot_speedups.main(["--csv", str(csv_path), "--grid", str(jl), "--out", str(tmp_path / "f.png")])
    assert (tmp_path / "f.png").stat().st_size > 1000

    # rocprofv3 pass directories as tools/pmc_sweep.sh writes them
    d = tmp_path / "pmc" / "pass0" / "box"
    d.mkdir(parents=True)
    (d / "1_counter_collection.csv").write_text(
        "Dispatch_Id,Kernel_Name,Counter_Name,Counter_Value\n"
        "1,k_sp_kernel,GRBM_GUI_ACTIVE,1600000\n1,k_sp_kernel,SQ_VALU_MFMA_BUSY_CYCLES,102400000\n1,k_sp_kernel,SQ_BUSY_CYCLES,1\n"
        "1,k_sp_kernel,FETCH_SIZE,1000\n1,k_sp_kernel,WRITE_SIZE,500\n2,other,FETCH_SIZE,7\n")
    (d / "1_kernel_trace.csv").write_text("Dispatch_Id,Kernel_Name,Start_Timestamp,End_Timestamp\n1,k_sp_kernel,0,100000\n2,other,0,5\n")
    out = subprocess.run([sys.executable, str(PKG / "tools" / "pmc_summary.py"), str(tmp_path / "pmc"), "--kernel", "sp_kernel",
                          "--mnk", "4096_4096_4096"], check=True, capture_output=True, text=True).stdout
    summ = json.loads(out)
    assert summ["derived"]["avg_kernel_us_profiled"] == 100.0
    assert abs(summ["derived"]["effective_clock_ghz"] - 2.0) < 1e-9            # 1.6e6 cycles / 8 XCDs / 100 us
    assert abs(summ["derived"]["mfma_pipe_busy_frac"] - 0.5) < 1e-9            # 1.024e8 / (1024 SIMDs * 2e5 cycles)
    assert summ["dominant_kernel"]["hbm_bytes_per_launch"] == (2 * 1000 + 500) * 1024


def test_fast_division_is_exact(lib):
    """hgemm_kernel.hpp fast_div / make_fast_div (the multipliers a launch passes to the kernels' raster map):
    exact for every 32-bit dividend, checked on edge values and a random sample."""
    import random

    f = lib.hgemm_mi355x_selfcheck_fastdiv
    f.argtypes = [ctypes.c_uint, ctypes.c_uint]
    f.restype = ctypes.c_uint
    rnd = random.Random(5)
    divisors = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257, 1000, 1023, 1024, 1025,
                4095, 4096, 4097, 65535, 65536, 65537, 262144, (1 << 24) - 1, 1 << 24, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    divisors += [rnd.randrange(1, 1 << rnd.randrange(1, 33)) for _ in range(200)]
    for d in divisors:
        ns = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, ((1 << 32) - 1) // d * d, ((1 << 32) - 1) // d * d - 1}
        ns |= {rnd.randrange(0, 1 << 32) for _ in range(40)} | {rnd.randrange(0, 1 << 16) for _ in range(10)}
        for n in ns:
            if 0 <= n < (1 << 32):
                assert f(n, d) == n // d, (n, d)


def test_raster_map_fast_equals_reference_and_is_a_bijection(lib):
    """The kernels' id -> (split, tile) map (hgemm_kernel.hpp raster_ref = map_logical) against its multiply-shift
    form, on the host, for every id of many launch shapes (plain, split-K, hybrid tail), and the map itself: every
    (split, tile row, tile column) is produced exactly once."""
    f = lib.hgemm_mi355x_selfcheck_raster
    f.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int * 4)]
    out_r, out_f = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    cases = []
    for tm, tn in [(1, 1), (1, 64), (64, 1), (2, 3), (7, 5), (16, 16), (17, 17), (33, 9), (9, 33), (64, 48), (3, 128), (128, 2)]:
        for g in (1, 2, 3, 4, 5, 8, 16, 32, 64, 1000):
            if g > tm and g != 1000:
                continue
            for splits in (1, 2, 5):
                cases.append((tm, tn, min(g, tm), 0, 0, splits))
    cases += [(17, 17, 4, 256, 33, 7), (28, 28, 8, 768, 16, 16), (5, 9, 2, 40, 5, 3), (64, 64, 4, 4095, 1, 31)]   # hybrid tail passes
    for tm, tn, g, tail_first, tail_tiles, splits in cases:
        per = tail_tiles if tail_tiles else tm * tn
        seen = set()
        for bid in range(per * splits):
            assert f(tm, tn, g, tail_first, tail_tiles, bid, 0, ctypes.byref(out_r)) == 0
            assert f(tm, tn, g, tail_first, tail_tiles, bid, 1, ctypes.byref(out_f)) == 0
            assert list(out_r) == list(out_f), (tm, tn, g, tail_first, tail_tiles, bid, list(out_r), list(out_f))
            split, tile, im, jn = out_r
            assert 0 <= split < splits and 0 <= im < tm and 0 <= jn < tn
            assert tail_first <= tile < tail_first + per if tail_tiles else 0 <= tile < per
            seen.add((split, im, jn))
        assert len(seen) == per * splits


def test_off_grid_shapes_are_planned_from_the_surrounding_grid_plans(lib):
    """A shape outside the tuned table takes one of the tuned plans of the lattice corners around it (ranked by the
    analytic model), falls back to the model when no corner plan fits (K % 64 != 0: only the K-tail family), is
    remembered per thread (same answer on every call and from another thread), and never disturbs grid shapes."""
    import threading

    def plan(m, n, k):
        c, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.hgemm_mi355x_plan(m, n, k, ctypes.byref(c), ctypes.byref(s), ctypes.byref(g)) == 0
        return c.value, s.value, g.value

    lattice = [64, 128, 256, 512, 1024, 2048, 4096, 8192, 12288, 16384]

    def bracket(x):
        lo = max([v for v in lattice if v <= x] or [lattice[0]])
        hi = min([v for v in lattice if v >= x] or [lattice[-1]])
        return lo, hi

    for m, n, k in [(5000, 3000, 7040), (6144, 6144, 6144), (4096, 11008, 4096), (8192, 28672, 4096), (100, 200, 320), (20000, 20000, 512),
                    (48, 4096, 64), (3000, 4096, 128)]:
        cfg, splits, group = plan(m, n, k)
        corners = {plan(a, b, c)[0] for a in bracket(m) for b in bracket(n) for c in bracket(k)}
        # (round 3: a dimension that is a multiple of 192 also admits the 192-wide persistent tile of that side)
        if m % 192 == 0:
            corners.add(lib.hgemm_mi355x_config_by_name(b"q192x256_w2x2"))
        if n % 192 == 0:
            corners.add(lib.hgemm_mi355x_config_by_name(b"q256x192_w2x2"))
        assert cfg in corners, (m, n, k, lib.hgemm_mi355x_config_name(cfg))
        assert k % lib.hgemm_mi355x_config_k_granularity(cfg) == 0
        # (a stream-K corner plan keeps its form: the low bits are then a workgroup count)
        assert ((splits & 0x40000) and lib.hgemm_mi355x_config_streamk(cfg) > 0) or 1 <= (splits & 0xFFFF) <= max(1, k // 64)
        assert group >= 1 and plan(m, n, k) == (cfg, splits, group)
        other = []
        t = threading.Thread(target=lambda: other.append(plan(m, n, k)))
        t.start(); t.join()
        assert other == [(cfg, splits, group)]
    # K % 64 != 0: whatever is chosen must accept the K tail (round 4: the corner plans of families q and r do)
    for (m, n, k) in [(4000, 4000, 4000), (1332, 3108, 4440), (64, 16384, 9160), (12032, 2048, 7152), (1000, 520, 200), (72, 4096, 72)]:
        cfg, splits, _ = plan(m, n, k)
        assert lib.hgemm_mi355x_config_k_granularity(cfg) == 8 and lib.hgemm_mi355x_config_accepts_k(cfg, k) == 1, (m, n, k)
        assert not (splits & 0x40000) or lib.hgemm_mi355x_config_name(cfg).decode()[0] == "t"   # no stream-K kernel with a direct tail
    assert lib.hgemm_mi355x_config_name(plan(4000, 4000, 4000)[0]).decode() == "q256x256_w2x2"
    assert lib.hgemm_mi355x_config_name(plan(64, 16384, 9160)[0]).decode()[0] == "r"
    # 33 distinct off-grid shapes map onto 32 memo slots: evictions must not change any answer
    shapes = [(1000 + 8 * i, 520, 704) for i in range(33)]
    first = [plan(*s) for s in shapes]
    assert [plan(*s) for s in shapes] == first
    assert plan(4096, 4096, 4096)[0] == lib.hgemm_mi355x_config_by_name(b"q256x256_w2x2")
    # 3072 = 12 x 256 = 16 x 192: 144 tiles of 256 x 256 leave 112 CUs idle, 192 tiles of 192 x 256 leave 64
    assert plan(3072, 3072, 3072)[0] == lib.hgemm_mi355x_config_by_name(b"q192x256_w2x2")


def test_off_grid_rules_of_round_4(lib):
    """Three rules the first K-tail measurements of families q and r suggested (tuning/r04_ktail_candidates_mi355x.jsonl, DESIGN.md
    section 4.13): (1) family r's load flags travel with a corner plan only while the rows stay 128-byte aligned (K % 64 == 0); (2) a
    single, under-filled round of a q corner plan lets the family's siblings in at one / two / four splits; (3) the model charges
    the LDS-DMA families for rows that are not 128-byte aligned, in proportion to their pieces per MFMA cycle."""
    lib.hgemm_mi355x_model_us.restype = ctypes.c_double

    def plan(m, n, k):
        c, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.hgemm_mi355x_plan(m, n, k, ctypes.byref(c), ctypes.byref(s), ctypes.byref(g)) == 0
        return lib.hgemm_mi355x_config_name(c.value).decode(), s.value

    # (1) rows of 18432 B (K = 9216) keep the corner plan's flags, rows of 18320 B (K = 9160) drop them (geometry and split form stay)
    # (round 5 moved most skinny rows to the two-resident q128x128: the r corners that remain are the N = 64 / M = 64 rows with K >= 12288)
    assert plan(64, 16384, 14336) == ("r64x128_k128", 0x190002) and plan(64, 16384, 14328) == ("r64x128_k128", 0x10002)
    served_by_r = 0
    for (m, n, k) in [(16000, 64, 16000), (64, 16000, 16000), (64, 12000, 16384), (64, 16384, 14328), (64, 12000, 16008), (16000, 128, 16000), (128, 8192, 9616)]:
        name, s = plan(m, n, k)
        if name[0] == "r":
            served_by_r += 1
            assert bool(s & 0x180000) == (k % 64 == 0), (m, n, k, name, hex(s))
        else:
            assert not (s & 0x100000), (m, n, k, name, hex(s))          # NT loads of the streamed operand: family r only
    assert served_by_r >= 4
    # (2) 143 tiles of 128 x 256 on 256 workgroups (the corner plan of 2048 x 4096 x 4096) -> 156 items of 256 x 256 at two splits
    assert plan(1332, 3108, 4440) == ("q256x256_w2x2", 2)
    assert plan(2048, 4096, 4096)[0] == "q128x256_w2x2"                      # the corner itself: a tuned row, untouched
    assert plan(4352, 4352, 4096) == ("q256x256_w2x2", 1)                    # more than one round: the hybrid tail's case, not this rule's
    # (4) a "_k4" member of family w beyond one workgroup per CU, and a family-r workgroup count between 1 and 1.75 rounds of the
    # chip, are not taken from a corner (256 x 1600 x 1024: 400 workgroups of w32x32_k4 measured 12.2 us against 9.0 for a classic
    # tile; 64 x 14928 x 10624: 312 workgroups of r64x96 83.4 us against 63.8 for 234 of r64x128)
    assert plan(256, 1600, 1024)[0][0] == "t" and plan(640, 640, 640)[0][0] == "t" and plan(256, 1024, 1024)[0] == "w32x32_k4"
    # (64 x 14928 x 10624 itself is served by the two-resident q128x128 since round 5 -- its corners' rows moved there; the guard
    # is still what keeps 312 workgroups of a 96-wide r tile away from shapes between the remaining r corners)
    assert plan(64, 14928, 10624)[0] in ("q128x128_w2x2", "q128x128_w2x2_k128", "r64x128_k128", "r64x128_k128_d")   # (round 6: a corner moved to the K = 128 stages)
    # (3) K = 4440 against K = 4416 (69 whole steps): 128 x 256 tiles +50 %, 256 x 256 tiles +10.6 %, family r not charged
    q128, q256, r = (lib.hgemm_mi355x_config_by_name(x) for x in (b"q128x256_w2x2", b"q256x256_w2x2", b"r64x128_k128"))
    def ratio(c, m, n, k0, k1):
        return lib.hgemm_mi355x_model_us(c, 1, m, n, k1) / lib.hgemm_mi355x_model_us(c, 1, m, n, k0)
    assert 1.45 < ratio(q128, 1332, 3108, 4416, 4440) < 1.55 and 1.09 < ratio(q256, 1332, 3108, 4416, 4440) < 1.14
    assert ratio(r, 64, 16384, 9216, 9160) == 1.0 and ratio(q128, 1332, 3108, 4416, 4480) < 1.03


def test_k_is_cut_into_splits_that_cover_it_exactly_once(lib):
    """How hgemm_mi355x_launch cuts K (hgemm_plan.hpp: split_k; the kernels' side: map_logical / sq_k_items): for every geometry, a
    sweep of K (tails included) and every requested split count, the splits are non-empty, all but the last are whole stages, the
    last one ends at K, a direct tail (families q and r) sits behind at least one whole stage of the last split and is shorter than
    a stage, and the classic family's partial step is the last step of the last split."""
    n_cfg = lib.hgemm_mi355x_num_configs()
    out = (ctypes.c_int * 4)()
    seen_direct = seen_classic_tail = 0
    for cid in range(n_cfg):
        name = lib.hgemm_mi355x_config_name(cid).decode()
        info = (ctypes.c_int * 8)()
        lib.hgemm_mi355x_config_info(cid, info)
        for k in list(range(8, 1100, 8)) + [2104, 4440, 7152, 9160, 16384, 16392]:
            if not lib.hgemm_mi355x_config_accepts_k(cid, k):
                assert lib.hgemm_mi355x_selfcheck_ksplit(cid, k, 1, out) != 0
                continue
            for want in (1, 2, 3, 5, 8, 16, 64, 1000):
                assert lib.hgemm_mi355x_selfcheck_ksplit(cid, k, want, out) == 0, (name, k, want)
                steps, splits, chunk, direct = out[0], out[1], out[2], out[3]
                stage = chunk // ((steps + splits - 1) // splits)
                assert 1 <= splits <= min(want, steps) and chunk % stage == 0 and stage in (64, 128, 256), (name, k, want, list(out))
                assert direct == (1 if (name[0] in "qr" and k % stage) else 0)
                ranges = [(i * chunk, k if i == splits - 1 else (i + 1) * chunk) for i in range(splits)]
                assert ranges[0][0] == 0 and ranges[-1][1] == k and all(a < b for a, b in ranges)
                assert all(ranges[i][1] == ranges[i + 1][0] for i in range(splits - 1))
                assert all((b - a) % stage == 0 for a, b in ranges[:-1])
                last = ranges[-1][1] - ranges[-1][0]
                if direct:
                    assert last // stage >= 1 and 0 < last % stage < stage and steps == k // stage
                    seen_direct += 1
                elif k % stage:
                    assert name[0] == "t" and steps == -(-k // stage) and last > 0
                    seen_classic_tail += 1
    assert seen_direct > 1000 and seen_classic_tail > 1000


def test_planner_fuzz_every_answer_is_launchable(lib):
    """Random shapes (aligned and not): the planner always answers with a geometry whose K granularity divides K (or
    a special id), a split count a launch would accept, and a raster group >= 1."""
    import random

    rnd = random.Random(11)
    n_cfg = lib.hgemm_mi355x_num_configs()
    c, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for _ in range(600):
        m = rnd.choice([1, 7, 48, 64, 100, 333, 1000, 4096, 5000, 12288, 20000, 70000])
        n = rnd.choice([4, 12, 64, 136, 200, 520, 4096, 11008, 28672, 16384]) + rnd.choice([0, 0, 0, 1, 2])
        k = rnd.choice([8, 40, 64, 72, 128, 200, 320, 1024, 4000, 4096, 7040, 16384, 20480]) + rnd.choice([0, 0, 0, 4, 1])
        assert lib.hgemm_mi355x_plan(m, n, k, ctypes.byref(c), ctypes.byref(s), ctypes.byref(g)) == 0
        if k % 8 or n % 4:
            assert c.value == -2 and s.value == 1          # HGEMM_CONFIG_RAGGED
            continue
        assert 0 <= c.value < n_cfg, (m, n, k, c.value)
        gran = lib.hgemm_mi355x_config_k_granularity(c.value)
        assert k % gran == 0, (m, n, k, lib.hgemm_mi355x_config_name(c.value), gran)
        assert lib.hgemm_mi355x_config_accepts_k(c.value, k) == 1, (m, n, k, lib.hgemm_mi355x_config_name(c.value))
        name = lib.hgemm_mi355x_config_name(c.value).decode()
        assert not (s.value & 0x40000) or k % 64 == 0 or name[0] == "t", (m, n, k, name)   # stream-K + K tail: classic family only
        assert (s.value & ~0xBFFFFF) == 0 and g.value >= 1              # (0x400000, wave priority: explicit plans only)
        assert not (s.value & 0x100000) or name[0] == "r"               # NT loads of the streamed operand: family r only
        assert not (s.value & 0x080000) or name[0] in "rq"              # K stagger per XCD: families r and q
        assert not (s.value & 0xA00000) or name[0] == "q"               # phase offset of the persistent walk: family q only
        assert ((s.value & 0x40000) and lib.hgemm_mi355x_config_streamk(c.value) > 0 and (s.value & 0xFFFF) <= 4096) or \
            (not (s.value & 0x40000) and 1 <= (s.value & 0xFFFF) <= max(1, k // 64)), (m, n, k, hex(s.value))
        assert not lib.hgemm_mi355x_config_name(c.value).decode().endswith("_m32") or lib.hgemm_mi355x_config_name(c.value).decode().startswith("t")


def test_planner_keeps_the_late_geometries_inside_their_measured_domains(lib):
    """Round 3, DESIGN.md section 4.8 / 6.5: the first version of the off-grid rules took an 8-wave mid tile for 525 tiles, 24
    tiles of 256 x 192, and a 192-wide sibling whenever it saved a fraction of a round -- all three measured slower than the
    corner plans they displaced.  The rules now hold them to <= 512 workgroups, >= 128 tiles, and the 0.87 tile-cost term."""
    def cfg_of(m, n, k):
        c, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.hgemm_mi355x_plan(m, n, k, ctypes.byref(c), ctypes.byref(s), ctypes.byref(g)) == 0
        return lib.hgemm_mi355x_config_name(c.value).decode(), s.value & 0xFFFF

    assert "w2x4_m16_s4" not in cfg_of(1332, 3108, 4440)[0] and "w4x2_m16_s4" not in cfg_of(1332, 3108, 4440)[0]
    assert not cfg_of(1968, 576, 4096)[0].startswith("q256x192")
    for shape in [(8192, 13824, 5120), (4384, 12288, 3840), (10904, 12288, 2048), (9216, 9216, 4096)]:
        assert cfg_of(*shape)[0] == "q256x256_w2x2", shape            # the sibling would save < 8 % of a round: not worth its 0.87
    for shape in [(3072, 3072, 3072), (1536, 6144, 6144), (6144, 6144, 6144), (12288, 1000, 4096)]:
        assert cfg_of(*shape)[0] == "q192x256_w2x2", shape
    for shape in [(8192, 1536, 8192), (2048, 6144, 2048)]:
        assert cfg_of(*shape)[0] == "q256x192_w2x2", shape
    # 4 x 63 = 252 tiles of 128 x 64 were the 8-wave tile's home ground until round 5; the corner row (BASELINE config 4) now ships the
    # two-resident q128x128 at two splits, and the off-grid neighbour follows it
    # (round 6: at K = 128 per stage, single-launch split-K)
    assert cfg_of(512, 4096, 4096)[0].startswith("q128x128_w2x2") and cfg_of(500, 4000, 4096)[0].startswith("q128x128_w2x2") and cfg_of(500, 4000, 4096)[1] == cfg_of(512, 4096, 4096)[1]


def test_tuned_table_overrides_apply_in_order(tmp_path):
    """tools/make_tuned_table.py --override A --override B: B replaces A (and the main runs) for the shapes it contains; a shape
    only in A keeps A's measurements."""
    import json as _json
    import sys as _sys

    _sys.path.insert(0, str(PKG / "tools"))
    import make_tuned_table as mtt

    def rec(mnk, plans):
        return _json.dumps({"mnk": mnk, "best": {}, "candidates": [{"config": c, "splits": s, "group_m": g, "us": us} for (c, s, g, us) in plans]})

    main, a, b = tmp_path / "main.jsonl", tmp_path / "a.jsonl", tmp_path / "b.jsonl"
    main.write_text(rec("64_64_64", [("t32x32_w1x1_m16_s4", 1, 1, 5.0)]) + "\n" + rec("128_128_128", [("t64x64_w2x2_m16_s4", 1, 1, 6.0)]) + "\n")
    a.write_text(rec("64_64_64", [("t64x32_w2x1_m16_s4", 1, 1, 9.0)]) + "\n" + rec("128_128_128", [("t32x64_w1x2_m16_s4", 1, 1, 9.0)]) + "\n")
    b.write_text(rec("64_64_64", [("t32x64_w1x2_m16_s4", 1, 2, 11.0)]) + "\n")
    per = mtt.merge_runs([str(main)])
    for ov in (str(a), str(b)):
        per.update(mtt.merge_runs([ov]))
    assert list(per["64_64_64"]) == [("t32x64_w1x2_m16_s4", 1, 2)]        # the later override wins although it is the slowest
    assert list(per["128_128_128"]) == [("t32x64_w1x2_m16_s4", 1, 1)]     # only the first override knows this shape



def test_stream_k_partition_in_the_library_is_the_model(lib):
    """hgemm_kernel.hpp sk_start / sk_owner (what every producer and the combiner evaluate on the device, compiled for the host
    here) against tests/kernel_layout_model.py: every run start and the owner of every tile's first stage."""
    sys.path.insert(0, str(REPO / "tests"))
    import kernel_layout_model as klm

    f = lib.hgemm_mi355x_selfcheck_streamk
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 2)()
    for tiles, ksteps, G, mn in [(144, 48, 256, 4), (96, 64, 256, 3), (97, 33, 206, 3), (2304, 192, 512, 4), (255, 7, 256, 4),
                                 (1, 256, 256, 2), (128, 128, 256, 3), (1000, 9, 768, 4), (4, 1000, 1024, 4), (65536, 16, 4096, 4)]:
        for w in list(range(0, G + 1, max(1, G // 97))) + [G - 1, G]:
            assert f(tiles, ksteps, G, mn, w, 0, out) == 0
            assert out[0] == klm.streamk_start(tiles, ksteps, G, mn, w), (tiles, ksteps, G, mn, w)
        for tile in range(0, tiles, max(1, tiles // 61)):
            x = tile * ksteps
            assert f(tiles, ksteps, G, mn, 0, x, out) == 0
            assert out[1] == klm.streamk_owner(tiles, ksteps, G, mn, x)
            b = klm.streamk_start(tiles, ksteps, G, mn, out[1])
            e = klm.streamk_start(tiles, ksteps, G, mn, out[1] + 1)
            assert b <= x < e
    assert f(1 << 20, 1 << 12, 256, 4, 0, 0, out) != 0      # beyond 2^30 stages: rejected (the launch falls back)


def test_stream_k_plans_are_priced_and_flags_are_not_split_counts(lib):
    """hgemm_mi355x_model_us takes `splits` as the launch does (a row with HGEMM_PLAN_NT_STORE was priced as 131073
    splits); stream-K plans have a finite estimate where the geometry has the kernel."""
    lib.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    q = lib.hgemm_mi355x_config_by_name(b"q256x256_w2x2")
    assert lib.hgemm_mi355x_model_us(q, 1, 4096, 4096, 4096) == lib.hgemm_mi355x_model_us(q, 1 | 0x20000, 4096, 4096, 4096)
    assert lib.hgemm_mi355x_model_us(q, 2 | 0x10000, 4096, 4096, 4096) == lib.hgemm_mi355x_model_us(q, 2, 4096, 4096, 4096)
    assert lib.hgemm_mi355x_config_streamk(q) == 0
    for name in (b"r128x128_k128", b"t128x64_w4x2_m16_s4", b"t128x128_w2x2_m16_s3", b"r64x64_k256"):
        c = lib.hgemm_mi355x_config_by_name(name)
        assert lib.hgemm_mi355x_config_streamk(c) >= 1
        us = lib.hgemm_mi355x_model_us(c, 0x40000, 12288, 128, 8192)
        assert 10.0 < us < 500.0
    assert lib.hgemm_mi355x_config_streamk(lib.hgemm_mi355x_config_by_name(b"t256x256_w2x4_m16_s2")) == 0
    assert lib.hgemm_mi355x_workspace_bytes(512, 512, 0x40000 | 256) >= (256 << 10) + 2 * 256 * 128 * 128 * 4


def test_stream_k_query_says_whether_a_plan_really_runs_and_what_workspace_it_takes(lib):
    """a HGEMM_PLAN_STREAMK plan used to degrade to the plain launch silently (direct K tail, > 65536 tiles) while the
    tuner recorded it as stream-K, and hgemm_mi355x_workspace_bytes asked for 0.5-2 GiB where a few MiB are used.  One
    predicate now answers for the launch, the planner, the tuner and the candidate generators; the config-aware workspace
    query returns exactly what the launch asks for."""
    lib.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    lib.hgemm_mi355x_plan_workspace_bytes.restype = ctypes.c_size_t
    r = lib.hgemm_mi355x_config_by_name(b"r128x128_k128")
    t = lib.hgemm_mi355x_config_by_name(b"t128x128_w2x2_m16_s3")
    q = lib.hgemm_mi355x_config_by_name(b"q256x256_w2x2")
    assert lib.hgemm_mi355x_streamk_runs(r, 12288, 128, 8192) == 1
    assert lib.hgemm_mi355x_streamk_runs(r, 12288, 128, 8192 + 64) == 0      # family r: direct K tail -> plain launch
    assert lib.hgemm_mi355x_streamk_runs(t, 12288, 128, 8192 + 8) == 1       # classic family pads its last step: still stream-K
    assert lib.hgemm_mi355x_streamk_runs(t, 128 * 300, 128 * 300, 256) == 0  # 90000 tiles > the 65536 arrival counters
    assert lib.hgemm_mi355x_streamk_runs(q, 4096, 4096, 4096) == 0           # no stream-K kernel in family q
    assert lib.hgemm_mi355x_streamk_runs(-1, 64, 64, 64) == 0 and lib.hgemm_mi355x_streamk_runs(r, 0, 64, 64) == 0
    # workspace: exact and small for stream-K; the geometry-blind bound is bounded by 256 x 128 tiles now
    ws = lib.hgemm_mi355x_plan_workspace_bytes(r, 0x40000 | 256, 12288, 128, 8192)
    assert ws == (256 << 10) + 2 * 256 * 128 * 128 * 4
    assert lib.hgemm_mi355x_plan_workspace_bytes(r, 0x40000 | 256, 12288, 128, 8192 + 64) == 0     # degraded: needs none
    assert lib.hgemm_mi355x_workspace_bytes(12288, 128, 0x40000 | 256) == (256 << 10) + 2 * 1024 * 256 * 128 * 4   # 256 MiB, was 512
    assert ws <= lib.hgemm_mi355x_workspace_bytes(12288, 128, 0x40000 | 256)
    assert lib.hgemm_mi355x_plan_workspace_bytes(q, 1 | 0x20000, 4096, 4096, 4096) == 0
    assert lib.hgemm_mi355x_plan_workspace_bytes(q, 2, 4096, 4096, 4096) == (256 << 10) + 2 * 4096 * 4096 * 4
    assert lib.hgemm_mi355x_plan_workspace_bytes(q, 2 | 0x10000, 4096, 4096, 4096) == (256 << 10) + 2 * 256 * 256 * 256 * 4
    # the candidate generator asks the same question
    text = (PKG / "tools" / "make_streamk_candidates.py").read_text()
    assert "hgemm_mi355x_streamk_runs" in text


FORMS = ["reference", "ragged", "stream-K", "split-K", "fused", "hybrid", "plain"]
THUNKS = ["entry", "splitk_reduce", "tail_reduce", "ragged", "generic"]
COUNTERS = 256 << 10          # arrival counters in front of the slabs


def _resolve(lib, cfg, splits, m, n, k, lds=None, operands=7, ruled_out=0, group=4):
    """hgemm_mi355x_launch's decision for one call, nothing launched (hgemm_mi355x_selfcheck_launch): operands = b | b_col_major << 1 |
    aligned pointers << 2, ruled_out = 1 << form of the workspace-backed forms that got no workspace.  Returns (status, form, slab
    bytes, counters, [(thunk, grid, epi, splits, k_chunk, items, start, stop)])."""
    if isinstance(cfg, str):
        lib.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
        cfg = lib.hgemm_mi355x_config_by_name(cfg.encode())
        assert cfg >= 0
    lda, ldb, ldc = lds or (k, k, n)
    out = (ctypes.c_longlong * 28)()
    st = lib.hgemm_mi355x_selfcheck_launch(cfg, splits, group, operands, m, n, k, lda, ldb, ldc, ruled_out, out)
    disp = [(THUNKS[out[4 + 8 * i]],) + tuple(out[5 + 8 * i:12 + 8 * i]) for i in range(out[1])]
    return st, FORMS[out[0]], out[2], out[3], disp


def test_workspace_query_is_what_the_launch_asks_for(lib):
    """hgemm_mi355x_plan_workspace_bytes promises exactly the launch's request (counters + slabs, 0 for none) on the operands
    hgemm_mi355x_fp32 / _fp16 pass.  It used to size the plan by a copy of the launch's logic, which missed the hybrid tail's
    slabs (0 reported, up to 64 MiB asked).  Every tuned row, every alternate, the planner's plan of every off-grid shape and
    of a seeded fuzz, and random explicit plans; every form issues 1-3 dispatches, the first carrying the timing start event and
    the last the stop event."""
    import random

    lib.hgemm_mi355x_plan_workspace_bytes.restype = ctypes.c_size_t
    plans = []
    for inc in ("hgemm_tuned_table.inc", "hgemm_tuned_alternates.inc"):
        for ln in (PKG / "csrc" / inc).read_text().splitlines():
            mm = re.match(r'\s*\{(\d+), (\d+), (\d+), "([^"]+)", (\d+), (\d+)\}', ln)
            if mm:
                plans.append((lib.hgemm_mi355x_config_by_name(mm[4].encode()), int(mm[5]), int(mm[1]), int(mm[2]), int(mm[3])))
    assert len(plans) == 1000 + 1791
    shapes = [tuple(map(int, ln.split("_"))) for ln in (PKG / "tools" / "offgrid_shapes.txt").read_text().split()
              if not ln.startswith("#") and "_" in ln]
    assert len(shapes) == 80
    rnd = random.Random(23)
    shapes += [(rnd.randrange(1, 20000), rnd.randrange(1, 5000) * 4, rnd.randrange(1, 2500) * 8) for _ in range(400)]
    c, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for (m, n, k) in shapes:
        assert lib.hgemm_mi355x_plan(m, n, k, ctypes.byref(c), ctypes.byref(s), ctypes.byref(g)) == 0
        if c.value >= 0:
            plans.append((c.value, s.value, m, n, k))
    n_cfg = lib.hgemm_mi355x_num_configs()
    for _ in range(1500):
        sp = rnd.choice([1, 2, 3, 4, 8, 2 | 0x10000, 4 | 0x10000, 0x40000, 0x40000 | 300, 0x40000 | 5000]) | rnd.choice([0, 0x20000, 0x80000])
        plans.append((rnd.randrange(n_cfg), sp, rnd.choice([64, 200, 1000, 4096, 4352, 7168]), rnd.choice([64, 128, 1000, 4096, 4352]),
                      rnd.choice([64, 128, 520, 1024, 4096, 4440, 8192])))
    forms = set()
    for (cfg, sp, m, n, k) in plans:
        st, form, slab, _, disp = _resolve(lib, cfg, sp, m, n, k)
        want = (COUNTERS + slab) if st == 0 and slab else 0
        assert lib.hgemm_mi355x_plan_workspace_bytes(cfg, sp, m, n, k) == want, (cfg, hex(sp), m, n, k, form)
        if st == 0:
            forms.add(form)
            assert 1 <= len(disp) <= 3 and [d[6] for d in disp] == [1] + [0] * (len(disp) - 1), (cfg, sp, m, n, k)
            assert [d[7] for d in disp] == [0] * (len(disp) - 1) + [1], (cfg, sp, m, n, k)
    assert forms >= {"stream-K", "split-K", "fused", "hybrid", "plain", "ragged"}


def test_launch_decisions_of_the_persistent_families_are_pinned(lib):
    """The combined decision of hgemm_mi355x_launch, worked out by hand from its rules: which form a call takes, with which grids,
    splits and K chunks, and what it falls back to without workspace.  A silent change of form would still pass every exactness
    test on the GPU (one launch instead of three shows up as a timing shift only)."""
    lib.hgemm_mi355x_model_us.restype = ctypes.c_double
    # 4352^2 x 4096 (test_hybrid_tail_schedule_is_exact_on_zero_one_inputs), splits = 1: K = 64 stages of 64.  The hybrid tail runs
    # when the tile count is not a multiple of the resident workgroups G, S = min(G // tail, stages // 4) >= 2, and
    # 0.6 tile_us - tile_us / S > 25 (tile_us: the model's time of one tile without the launch)
    m = n = 4352
    k = 4096

    def tile_us(name):
        return lib.hgemm_mi355x_model_us(lib.hgemm_mi355x_config_by_name(name.encode()), 1, *{"s256x256_w2x2": (256, 256),
                                         "q256x256_w2x2": (256, 256), "s128x256_w2x2": (128, 256), "q256x128_w2x2": (256, 128)}[name], k) - 2.0

    for name in ("s256x256_w2x2", "q256x256_w2x2"):
        # 17 x 17 = 289 tiles, G = 256 (one 128 KiB workgroup per CU): 256 full + 33 tail tiles, S = min(256 // 33, 64 // 4) = 7,
        # per slice ceil(64 / 7) = 10 stages (S stays ceil(64 / 10) = 7), 33 x 7 = 231 tail items of one 256 x 256 fp32 slab each
        assert 0.6 * tile_us(name) - tile_us(name) / 7 > 25.0
        assert _resolve(lib, name, 1, m, n, k) == (0, "hybrid", 231 * 256 * 256 * 4, 0, [
            ("entry", 256, 0, 1, k, 256, 1, 0), ("entry", 231, 1, 7, 10 * 64, 231, 0, 0), ("tail_reduce", 0, 1, 7, 10 * 64, 231, 0, 1)])
    for name in ("s128x256_w2x2", "q256x128_w2x2"):
        # 34 x 17 = 578 tiles, G = 256 (96 KiB + 64 B per workgroup: one per CU): 66 tail tiles, S = min(256 // 66, 16) = 3, and a
        # third of a ~44 us tile does not pay for the tail pass
        assert 0.6 * tile_us(name) - tile_us(name) / 3 < 25.0
        assert _resolve(lib, name, 1, m, n, k) == (0, "plain", 0, 0, [("entry", 256, 0, 1, k, 578, 1, 1)])
    # fallbacks: split-K without workspace runs as splits = 1 -- and then takes the hybrid form; a hybrid tail without workspace runs
    # the plain launch (one resident wave walking all 289 tiles)
    q = "q256x256_w2x2"
    hybrid = _resolve(lib, q, 1, m, n, k)
    assert _resolve(lib, q, 2, m, n, k) == (0, "split-K", 2 * m * n * 4, 0, [("entry", 256, 1, 2, 32 * 64, 578, 1, 0),
                                                                            ("splitk_reduce", 0, 1, 2, 32 * 64, 578, 0, 1)])
    assert _resolve(lib, q, 2 | 0x10000, m, n, k) == (0, "fused", 289 * 2 * 256 * 256 * 4, 1, [("entry", 256, 2, 2, 32 * 64, 578, 1, 1)])
    assert _resolve(lib, q, 2, m, n, k, ruled_out=1 << 3) == hybrid
    assert _resolve(lib, q, 2 | 0x10000, m, n, k, ruled_out=1 << 4) == hybrid
    assert _resolve(lib, q, 1, m, n, k, ruled_out=1 << 5) == (0, "plain", 0, 0, [("entry", 256, 0, 1, k, 289, 1, 1)])
    assert _resolve(lib, q, 2, m, n, k, ruled_out=(1 << 3) | (1 << 5)) == (0, "plain", 0, 0, [("entry", 256, 0, 1, k, 289, 1, 1)])
    # stream-K asked of a family without the kernel: splits = 1, which may again be the hybrid form
    assert _resolve(lib, q, 0x40000 | 256, m, n, k) == hybrid

    # fused split-K on the two-resident members: G = 512, but 80 KiB of stages + the 64-byte vote word fit once per CU -> 256
    # workgroups.  4096^3: 22 x 32 = 704 tiles of 192 x 128 (32 x 22 of 128 x 192), two splits of 32 stages.
    for name, tiles in (("q192x128_w2x2", 22 * 32), ("q128x192_w2x2", 32 * 22)):
        assert _resolve(lib, name, 2 | 0x10000, 4096, 4096, 4096) == (0, "fused", tiles * 2 * 192 * 128 * 4, 1, [
            ("entry", 256, 2, 2, 32 * 64, 2 * tiles, 1, 1)])
        assert _resolve(lib, name, 2, 4096, 4096, 4096)[4][0] == ("entry", 512, 1, 2, 32 * 64, 2 * tiles, 1, 0)   # two-pass: 512
    # (64 KiB of stages fit twice even with the vote word: no clamp)
    assert _resolve(lib, "q128x128_w2x2", 2 | 0x10000, 4096, 4096, 4096)[4] == [("entry", 512, 2, 2, 32 * 64, 2 * 32 * 32, 1, 1)]

    # stream-K: G = min(the plan's workgroups (<= 4096; 0 / 1: 256 x workgroups per CU), tiles x stages // min stages per run), with
    # r128x128_k128 (stages of 128, at least 3 per run) on 12288 x 128 x 8192: 96 tiles x 64 stages = 6144 -> at most 2048 runs
    r = "r128x128_k128"
    sk_per_cu = lib.hgemm_mi355x_config_streamk(lib.hgemm_mi355x_config_by_name(r.encode()))
    for g_plan, G in ((256, 256), (5000, 6144 // 3), (0, 256 * sk_per_cu), (3000, 6144 // 3)):
        assert _resolve(lib, r, 0x40000 | g_plan, 12288, 128, 8192) == (0, "stream-K", 2 * G * 128 * 128 * 4, 1, [
            ("entry", G, 3, 1, 8192, 96, 1, 1)]), g_plan
    # 256 x 128 x 512: 2 tiles x 4 stages -> 8 // 3 = 2 workgroups
    assert _resolve(lib, r, 0x40000 | 256, 256, 128, 512)[1:3] == ("stream-K", 2 * 2 * 128 * 128 * 4)
    # no workspace, or a direct K tail (family r has no stream-K kernel with one): the plain launch, one workgroup per tile
    plain = (0, "plain", 0, 0, [("entry", 96, 0, 1, 8192, 96, 1, 1)])
    assert _resolve(lib, r, 0x40000 | 256, 12288, 128, 8192, ruled_out=1 << 2) == plain
    assert _resolve(lib, r, 0x40000 | 256, 12288, 128, 8192 + 64)[1:3] == ("plain", 0)


def test_launch_decisions_off_the_lds_dma_path_are_pinned(lib):
    """Calls the LDS-DMA kernels cannot take: unaligned operands, strides beyond the 32-bit reach, K the geometry does not accept
    -> the ragged kernel (HGEMM_ERR_TOO_LARGE past 2^31 tiles of 64 x 64); HGEMM_CONFIG_GENERIC or no b_col_major -> the
    reference kernel (HGEMM_ERR_BAD_ARG without b); a K that is whole 64-steps but not the geometry's stages -> HGEMM_ERR_BAD_ARG."""
    q = "q256x256_w2x2"
    ragged = (0, "ragged", 0, 0, [("ragged", 0, 0, 1, 4096, 1, 1, 1)])
    reference = (0, "reference", 0, 0, [("generic", 0, 0, 1, 4096, 1, 1, 1)])
    assert _resolve(lib, q, 2, 4096, 4096, 4096, operands=3) == ragged                             # pointers not 16-byte aligned
    assert _resolve(lib, q, 2, 4096, 4096, 4096, lds=(4100, 4096, 4096)) == ragged                # lda % 8 != 0
    assert _resolve(lib, q, 1, 4096, 4096, 4096, lds=(1 << 23, 4096, 4096)) == ragged            # 256 rows x 16 MiB >= 4 GiB
    assert _resolve(lib, "q128x128_w2x2", 1, 4096, 4096, 4096, lds=(1 << 23, 4096, 4096))[1] == "plain"   # 128 rows: < 4 GiB
    assert _resolve(lib, "t128x128_w2x2_m16_s3", 1, 4096, 4096, 4096, lds=(1 << 23, 4096, 4096)) == ragged   # classic: 2 GiB
    assert _resolve(lib, q, 1, 4096, 4096, 100)[1] == "ragged"                                     # K % 8 != 0
    assert _resolve(lib, -2, 1, 4096, 4096, 4096) == ragged
    assert _resolve(lib, -1, 1, 4096, 4096, 4096) == reference
    assert _resolve(lib, q, 1, 4096, 4096, 4096, operands=1 | 4) == reference                     # no b_col_major
    assert _resolve(lib, -1, 1, 4096, 4096, 4096, operands=2 | 4)[0] == -1                        # no b
    assert _resolve(lib, q, 1, 4096, 4096, 4096, operands=4)[0] == -1
    assert _resolve(lib, "q128x128_w2x2_k128", 1, 4096, 4096, 64)[0] == -1                        # 64 < one stage of 128
    big = 1 << 30                                                                                  # 2^24 x 2^24 tiles of 64 x 64
    assert _resolve(lib, -2, 1, big, big, 64, operands=3)[0] == -2
    assert _resolve(lib, q, 1, big, big, 64, operands=3)[0] == -2
    # strides below the row length (overlapping rows; ldc = 0 passes the alignment rule and writes every row over row 0; a negative
    # ldc writes in front of C) -> HGEMM_ERR_BAD_ARG on every path; ldb only where b_col_major is given
    k = n = 4096
    for lds in ((k - 8, k, n), (k, k - 8, n), (k, k, n - 4), (0, k, n), (k, 0, n), (k, k, 0), (-k, k, n), (k, -k, n), (k, k, -n)):
        for cfg, operands in ((q, 7), (q, 3), ("t128x128_w2x2_m16_s3", 7), ("r64x64_k256", 7), (-2, 7), (-1, 7)):
            for splits in (1, 2, 2 | 0x10000, 0x40000 | 64):
                assert _resolve(lib, cfg, splits, 4096, n, k, lds=lds, operands=operands)[0] == -1, (cfg, lds, operands, hex(splits))
    for lds in ((k, k - 8, n), (k, 0, n), (k, -k, n)):                                             # no b_col_major: ldb unused
        assert _resolve(lib, q, 1, 4096, n, k, lds=lds, operands=1 | 4) == reference
        assert _resolve(lib, -1, 1, 4096, n, k, lds=lds, operands=1 | 4) == reference
    # (K, K, N) and wider strides resolve as before
    for cfg, splits in ((q, 1), (q, 2), (q, 2 | 0x10000), ("r128x128_k128", 0x40000 | 256), ("t128x128_w2x2_m16_s3", 3), (-2, 1), (-1, 1)):
        want = _resolve(lib, cfg, splits, 4096, n, k)
        assert want[0] == 0
        for lds in ((k, k, n), (k + 64, k + 64, n + 64), (k + 8, k + 16, n + 4)):
            assert _resolve(lib, cfg, splits, 4096, n, k, lds=lds) == want, (cfg, hex(splits), lds)
        assert _resolve(lib, cfg, splits, 4096, n, k, lds=(k + 4, k, n))[1] == ("reference" if cfg == -1 else "ragged")


def test_plan_flags_of_round_5_are_flags_not_split_counts(lib):
    """HGEMM_PLAN_XCD_STAGGER (family q's kstagger variant), HGEMM_PLAN_PHASE_OFFSET(4), HGEMM_PLAN_WAVE_PRIORITY ride in `splits`
    like the older flags: the model prices the plan, never the flag bits; the two-resident members report two workgroups per
    CU; every annotation tool decodes them."""
    lib.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    q = lib.hgemm_mi355x_config_by_name(b"q256x256_w2x2")
    base = lib.hgemm_mi355x_model_us(q, 1, 8192, 8192, 512)
    for flag in (0x80000, 0x200000, 0x400000, 0x800000, 0x80000 | 0x200000 | 0x20000):
        assert lib.hgemm_mi355x_model_us(q, 1 | flag, 8192, 8192, 512) == base
    info = (ctypes.c_int * 8)()
    for name, lds in ((b"q192x128_w2x2", 80 * 1024), (b"q128x192_w2x2", 80 * 1024), (b"q128x128_w2x2", 64 * 1024)):
        c = lib.hgemm_mi355x_config_by_name(name)
        assert c >= 0, name
        lib.hgemm_mi355x_config_info(c, info)
        assert info[7] == lds and 2 * info[7] <= 160 * 1024          # exactly the two stages: two workgroups per CU
    sys.path.insert(0, str(PKG))
    from tools.update_tuned_table import form_text
    import bench

    assert form_text(1 | 0x20000) == "" and form_text(2 | 0x10000) == " fused split-K"
    assert form_text(1 | 0x80000) == " K stagger per XCD" and form_text(4 | 0x80000 | 0x100000) == " two-pass split-K, K stagger per XCD, NT loads of the streamed operand"
    assert form_text(1 | 0x200000 | 0x20000) == " phase offset"
    d = bench.plan_dict(b"q256x256_w2x2", 2 | 0x10000 | 0x20000 | 0x80000 | 0x200000, 4)
    assert d == {"config": "q256x256_w2x2", "splits": 2, "group_m": 4, "fused_split_k": True, "nt_store": True, "streamk": False,
                 "xcd_stagger": True, "nt_loads": False, "phase_offset": True, "wave_priority": False, "phase_offset4": False}


def test_first_use_selection_is_off_by_default_and_lists_launchable_candidates(lib):
    """VERDICT r4 item 8 (the reference re-tunes in situ, kernels/h100_F32F16F16F32/64_4096_64.cu:623-690): opt-in, so the default
    hot path stays a table probe.  Without a GPU only the candidate list can be checked: the table's plan first, at most three,
    no duplicates, every geometry accepts the K, alternates of grid shapes come from the generated table whose rows name
    existing geometries."""
    lib.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    lib.hgemm_mi355x_set_insitu(0)                      # (whatever HGEMM_MI355X_INSITU says: off, nothing recorded)
    assert lib.hgemm_mi355x_insitu_enabled() == 0 and lib.hgemm_mi355x_set_insitu(0) == 0
    cfg, sp, gm = (ctypes.c_int * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    c0, s0, g0 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for mnk in ((4096, 4096, 4096), (16384, 256, 16384), (8192, 8192, 256), (64, 4096, 64), (1000, 520, 200), (4000, 4000, 4000), (65, 30, 100)):
        n = lib.hgemm_mi355x_insitu_candidates(*mnk, cfg, sp, gm)
        assert 1 <= n <= 3
        lib.hgemm_mi355x_plan(*mnk, ctypes.byref(c0), ctypes.byref(s0), ctypes.byref(g0))
        assert (cfg[0], sp[0], gm[0]) == (c0.value, s0.value, g0.value)
        assert len({(cfg[i], sp[i], gm[i]) for i in range(n)}) == n
        for i in range(n):
            assert cfg[i] < 0 or lib.hgemm_mi355x_config_accepts_k(cfg[i], mnk[2]) == 1
        assert lib.hgemm_mi355x_insitu_choice(*mnk, ctypes.byref(c0), ctypes.byref(s0), ctypes.byref(g0)) == 0   # nothing measured
    rows = re.findall(r'\{(\d+), (\d+), (\d+), "([^"]+)", (\d+), (\d+)\}', (PKG / "csrc" / "hgemm_tuned_alternates.inc").read_text())
    per_shape = {}
    for m, n_, k, name, s, g in rows:
        assert lib.hgemm_mi355x_config_by_name(name.encode()) >= 0, name
        per_shape.setdefault((m, n_, k), []).append((name, s, g))
    assert all(len(v) <= 2 and len(set(v)) == len(v) for v in per_shape.values())


def test_autotune_cache_file_is_read_and_counts_records(lib, tmp_path):
    """Round 6: the on-disk cache of hipBLASLt autotune winners (include/hgemm_mi355x.h: hgemm_hipblaslt_autotune_set_cache).  Without
    a GPU only the file handling can run: comment and malformed lines are skipped, records are counted, an unset / missing file is
    an empty cache, and find_best_* without its init still answers NOT_READY (it never touches the cache then)."""
    f = tmp_path / "cache.txt"
    f.write_text("# header\n"
                 "1 64 4096 64 0 73412 0.004321 37 50 100 1.000 Cijk_Alik_Bljk_HHS_BH_MT32x32x64\n"
                 "0 64 4096 64 0 73999 0.005000 37 50 100 1.000 -\n"
                 "garbage line\n"
                 "1 512 4096 4096 0 12 0.027 100 12 25 1.000\n")          # (no solution name: still a record)
    lib.hgemm_hipblaslt_autotune_set_cache.argtypes = [ctypes.c_char_p]
    h, m = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.hgemm_hipblaslt_autotune_set_cache(str(f).encode()) == 0
    assert lib.hgemm_hipblaslt_autotune_cache_stats(ctypes.byref(h), ctypes.byref(m)) == 3
    assert (h.value, m.value) == (0, 0)
    assert lib.hgemm_hipblaslt_autotune_set_cache(str(tmp_path / "missing.txt").encode()) == 0
    assert lib.hgemm_hipblaslt_autotune_cache_stats(None, None) == 0
    assert lib.hgemm_hipblaslt_autotune_set_cache(None) == 0
    assert lib.hgemm_hipblaslt_autotune_cache_stats(None, None) == 0
    assert lib.hgemm_hipblaslt_autotune_from_cache(1) == 0
    assert lib.hgemm_hipblaslt_autotune_find_best_tn(64, 4096, 64, 0) == -5     # HGEMM_ERR_NOT_READY: no init, no GPU


def test_bench_dump_outputs_writes_the_c_of_each_set_as_float32(tmp_path, monkeypatch):
    """bench.py --dump-outputs: one float32 file per operand set, the whole C while it fits the budget, else the same seeded
    sample of flat indices in every file; --steps / --batch below 1 are refused before anything touches a device."""
    import numpy as np
    import torch

    import bench

    torch.manual_seed(0)
    p = bench.Problem("96_80_64", "fp16", "cpu")
    for a, b, _, c in p.sets:
        c.copy_((a.float() @ b.float()).half())
    info = bench.dump_outputs(p, [0, 2], tmp_path / "whole")
    assert info["files"] == ["c_set0.npy", "c_set2.npy"] and not info["sampled"]
    for s in (0, 2):
        got = np.load(tmp_path / "whole" / f"c_set{s}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, p.sets[s][3].float().numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4 * 1000)
    info = bench.dump_outputs(p, [1, 3], tmp_path / "sample")
    assert info["sampled"] and info["elements_per_file"] == 1000
    idx = np.sort(np.random.default_rng(0).choice(96 * 80, 1000, replace=False))
    for s in (1, 3):
        got = np.load(tmp_path / "sample" / f"c_set{s}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, p.sets[s][3].float().numpy().reshape(-1)[idx])
    for bad in (["--steps", "0"], ["--batch", "0"]):
        with pytest.raises(SystemExit) as e:
            bench.main(bad)
        assert e.value.code == 2
