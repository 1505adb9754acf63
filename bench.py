"""bench.py -- headline benchmark of the MI355X HGEMM hot path (driver contract: one JSON line).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--workload M_N_K[:fp16|fp32]]
                    [--dump-outputs DIR] [--full [--no-shapes] [--no-cpu-baseline]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, runs the W warm-up and K timed steps, writes the outputs if --dump-outputs is given, and prints the
JSON line (headline + `roofline`, whose clock rides on the timed launches themselves).  --full adds everything that takes
runs of its own: `shapes` (hipBLASLt / rocBLAS on BASELINE's shapes, incl. the hipBLASLt autotune) and `cpu_baseline`.

--dump-outputs DIR writes, after the timed steps, the C matrices the last timed step computed: one DIR/c_set<i>.npy (float32)
per rotating operand set written in that step, rank 0's when N > 1 (the operands are seeded, so the same arguments give the
same inputs).  When all of them exceed DUMP_BUDGET_BYTES together, each file holds the same fixed sample of C's elements
instead: flat row-major indices drawn once by numpy.random.default_rng(0) without replacement, sorted, a 1-D array.

Workload (config.workload): BASELINE.json configs[2], the 4096x4096x4096 fp16-accumulate HGEMM -- the single-GPU
configuration whose MFMA utilisation BASELINE.json asks for (configs[1], 64x4096x64, is a 7-microsecond
launch-bound call; it and configs[3] are reported per shape in `shapes`).  A "step" is one pass of the hot path
over one batch of synthetic input: --batch (default 1024) independent GEMM problems of that shape, one C-ABI call
each (hgemm_mi355x_fp16, the entry point behind cuda_l2_mi355x_fp16), fp16 N(0,1) operands already resident in
HBM (rotating buffer sets, so successive calls do not re-hit L2 / MALL).  A step is ~0.1 s, so the default K = 20
timed steps are a >= 2 s steady-state region behind W = 5 warm-up steps (the board's power limiter settles within
the first milliseconds).  K steps are issued back to back between barrier + device sync on both sides;
value = total FLOPs of all ranks / max-over-ranks time, in TFLOP/s.  A single GEMM never spans GPUs, so N > 1 runs
N independent replicas (weak scaling, no collective on the data path).

Extra objects on the JSON line:
  roofline      the workload's kernel (MFMA-bound): 2MNK / launch duration vs the 2.5 PFLOP/s dense fp16 MFMA peak.  `launch_us`
                is ONE clock: the mean of HIP events that ride on the dispatch packets of every 16th launch of the timed region
                (on the launch stream, hipExtLaunchKernel start / stop events).  In a back-to-back stream a dispatch's start
                event fires while its predecessor is still draining, so the mean overstates the kernel by ~1 % and `achieved` /
                `frac` understate it slightly.  `wall_per_call_us` -- the rank's wall clock of the timed region divided by the
                launches in it -- is reported beside it as the stream's THROUGHPUT interval (it contains the ~2 us between
                launches but overlaps a launch's head with its predecessor's drain, so it is not a bound on one kernel's
                duration and is never substituted for the event clock).  The committed rocprofv3 --kernel-trace --stats summary
                of the same command is the independent third clock.
                `traffic` (HBM + Infinity-Cache bytes per launch) is NOT measured in this run: it is read from the
                committed rocprofv3 PMC summary named in `traffic_source` (profiles/), collected as
                MI355X_MICROARCH.md prescribes (separate --pmc passes, FETCH_SIZE doubled on gfx950)
  cpu_baseline  (--full) the reference's CPU oracle expression (fp32 torch.matmul on the host, rounded to fp16) timed on
                rank 0 (any N: after the timed region, while the other ranks wait in the closing barrier) over a bounded
                sample of the same shape
  shapes        (--full) BASELINE.json's three single-GPU shapes: device-timed TFLOP/s of ours, hipBLASLt heuristic AND
                autotune (tn, nn), rocBLAS; the reference-style host wall-clock (sync either side of each call);
                our per-call time inside a 32-launch hipGraph replay; a roofline entry per shape
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent
PKG = REPO / "cuda-l2_amd"
for p in (str(REPO), str(PKG)):
    if p not in sys.path:
        sys.path.insert(0, p)

MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16 MFMA peak, MI355X_MICROARCH.md
HBM_PEAK_TBPS = 8.0            # HBM3E spec, MI355X_MICROARCH.md
BASELINE3 = [("64_4096_64", "fp32"), ("512_4096_4096", "fp32"), ("4096_4096_4096", "fp16")]
WORKLOAD = ("4096_4096_4096", "fp16")
EVENT_STRIDE = 16              # every 16th launch of the timed region carries dispatch-attached timing events
DUMP_BUDGET_BYTES = 32 << 20   # --dump-outputs: float32 bytes written in all


PLAN_FLAGS = (("fused_split_k", 0x10000), ("nt_store", 0x20000), ("streamk", 0x40000), ("xcd_stagger", 0x80000), ("nt_loads", 0x100000),
              ("phase_offset", 0x200000), ("wave_priority", 0x400000), ("phase_offset4", 0x800000))


def plan_dict(name, splits: int, group_m: int) -> dict:
    """A plan as the records show it: geometry, split count (or stream-K workgroups) and every plan flag of include/hgemm_mi355x.h."""
    d = {"config": name.decode() if name else "ragged", "splits": splits & 0xFFFF, "group_m": group_m}
    d.update({k: bool(splits & bit) for k, bit in PLAN_FLAGS})
    return d


def load_library():
    """The product path: libhgemm_mi355x.so through its C ABI.  No fallback of any kind."""
    # (HGEMM_LIB_DIR: an experiment build of the same library, cuda-l2_amd/lib_<suffix>/, for A/B runs of the tools)
    so = Path(os.environ.get("HGEMM_LIB_DIR", PKG / "lib")) / "libhgemm_mi355x.so"
    if not so.exists():
        raise RuntimeError(f"{so} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` first")
    lib = ctypes.CDLL(str(so))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for name in ("hgemm_mi355x_fp32", "hgemm_mi355x_fp16"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, ci, ci, ci, vp]
    for name in ("hgemm_rocblas_nn", "hgemm_rocblas_tn", "hgemm_hipblaslt_heuristic_nn", "hgemm_hipblaslt_heuristic_tn",
                 "hgemm_hipblaslt_autotune_nn", "hgemm_hipblaslt_autotune_tn"):
        getattr(lib, name).argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]
    lib.hgemm_mi355x_config_name.restype = ctypes.c_char_p
    lib.hgemm_mi355x_event_create.restype = vp
    lib.hgemm_mi355x_event_destroy.argtypes = [vp]
    lib.hgemm_mi355x_time_next_launch.argtypes = [vp, vp]
    lib.hgemm_mi355x_event_elapsed_us.argtypes = [vp, vp]
    lib.hgemm_mi355x_event_elapsed_us.restype = ctypes.c_double
    lib.hgemm_mi355x_strerror.restype = ctypes.c_char_p
    return lib


def check(lib, status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"{what} failed: {lib.hgemm_mi355x_strerror(status).decode()} ({status})")


def reduce_over_ranks(elapsed_s: float, flops: float, device) -> tuple[float, float]:
    """(max elapsed over ranks, sum of flops over ranks); identity when not distributed."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return elapsed_s, flops
    t = torch.tensor([elapsed_s], dtype=torch.float64, device=device)
    f = torch.tensor([flops], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(f, op=dist.ReduceOp.SUM)
    return float(t.item()), float(f.item())


class Problem:
    """One (M,N,K): rotating sets of HBM-resident operands so successive launches do not re-hit cache."""

    def __init__(self, mnk: str, acc: str, device, budget_bytes: int = 1 << 30):
        self.mnk, self.acc = mnk, acc
        self.m, self.n, self.k = (int(x) for x in mnk.split("_"))
        self.flops = 2.0 * self.m * self.n * self.k
        self.bytes = 2.0 * (self.m * self.k + self.k * self.n + self.m * self.n)
        set_bytes = 2 * (self.m * self.k + 2 * self.k * self.n + self.m * self.n)
        nsets = max(1, min(4, budget_bytes // set_bytes))
        self.sets = []
        for _ in range(nsets):
            a = torch.randn((self.m, self.k), dtype=torch.half, device=device)
            b = torch.randn((self.k, self.n), dtype=torch.half, device=device)
            bt = b.t().contiguous()  # storage of b_col_major
            c = torch.empty((self.m, self.n), dtype=torch.half, device=device)
            self.sets.append((a, b, bt, c))
        self.i = 0

    def next(self):
        s = self.sets[self.i % len(self.sets)]
        self.i += 1
        return s


def dump_outputs(prob: Problem, last_step_sets: list[int], out_dir: Path) -> dict:
    """Write the C of every operand set the last timed step wrote (each set always gets the same product, so its C is what
    that step's launches on it returned) as float32 .npy files; a fixed seeded element sample when over DUMP_BUDGET_BYTES."""
    import numpy as np

    out_dir.mkdir(parents=True, exist_ok=True)
    numel = prob.m * prob.n
    per_set = min(numel, DUMP_BUDGET_BYTES // 4 // len(last_step_sets))
    idx = None
    if per_set < numel:
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(numel, per_set, replace=False))).to(prob.sets[0][3].device)
    for s in last_step_sets:
        c = prob.sets[s][3]
        out = (c.float() if idx is None else c.reshape(-1)[idx].float()).cpu().numpy()
        np.save(out_dir / f"c_set{s}.npy", out)
    return {"dir": str(out_dir), "files": [f"c_set{s}.npy" for s in last_step_sets], "dtype": "float32",
            "elements_per_file": per_set, "sampled": idx is not None}


def launch_ours(lib, prob: Problem, stream: int):
    a, b, bt, c = prob.next()
    fn = lib.hgemm_mi355x_fp16 if prob.acc == "fp16" else lib.hgemm_mi355x_fp32
    check(lib, fn(a.data_ptr(), b.data_ptr(), bt.data_ptr(), c.data_ptr(), prob.m, prob.n, prob.k, stream), "hgemm_mi355x")
    return c


def settle(fn, seconds: float) -> None:
    """Run fn back to back for `seconds` (clock / power state and caches in steady state before a measurement)."""
    t0 = time.time()
    while time.time() - t0 < seconds:
        for _ in range(8):
            fn()
        torch.cuda.synchronize()


def device_time_us(fn, reps: int) -> float:
    """Median device time of fn() with HIP events on the current stream."""
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs)
    return ts[len(ts) // 2]


def isolated_time_us(fn, reps: int) -> float:
    """Median device time of ONE call with the device idle before and after it (event, call, event, sync): the
    device-side counterpart of the reference's per-call measurement, which syncs either side of every call
    (benchmarking_utils.py:23-31).  device_time_us() above is the back-to-back (stream throughput) figure, where the
    tail of one kernel overlaps the head of the next if both fit on a CU together."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def wall_time_us(fn, reps: int) -> float:
    """Reference-style timing (benchmarking_utils.py:23-31): sync, t0, call, sync, t1; mean."""
    tot = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        tot += time.time() - t0
    return tot / reps * 1e6


GRAPH_LAUNCHES = 32


def graph_time_us(lib, p, reps: int = 7) -> dict:
    """Per-call time of OUR entry point inside a hipGraph of GRAPH_LAUNCHES back-to-back calls (rotating operand
    sets): device time between events around one replay, and the reference-style host wall-clock (sync, t0,
    replay, sync), both divided by the launches in the graph.  What a serving loop that captures its GEMM calls
    pays per call; for the launch-bound 64x4096x64 this is where the ~7 us host launch path goes away."""
    lib.hgemm_mi355x_reserve_workspace.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    s = torch.cuda.Stream()
    check(lib, lib.hgemm_mi355x_reserve_workspace(p.m, p.n, p.k, s.cuda_stream), "reserve_workspace")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for _ in range(GRAPH_LAUNCHES):
            launch_ours(lib, p, torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.time()
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.time() - t0) * 1e6 / GRAPH_LAUNCHES)
        dev.append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
    del graph
    return {"ours_graph_us": sorted(dev)[len(dev) // 2], "ours_graph_wall_us": sorted(wall)[len(wall) // 2],
            "graph_launches": GRAPH_LAUNCHES}


def roofline_entry(p, us: float, traffic=None) -> dict:
    """Which roof bounds the shape (arithmetic intensity vs the ridge 2.5 PF / 8 TB/s = 312 flop/B) and how close
    the measured launch is.  Algorithmic work: 2MNK flop; 2(MK + KN + MN) bytes (A, B read once, C written once)."""
    ai = p.flops / p.bytes
    if ai >= MFMA_F16_PEAK_TFLOPS / HBM_PEAK_TBPS:
        ach = p.flops / us * 1e-6
        return {"bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / MFMA_F16_PEAK_TFLOPS, 4), "traffic": traffic, "arithmetic_intensity": round(ai, 1)}
    ach = p.bytes / us * 1e-6  # TB/s
    return {"bound": "hbm", "achieved": round(ach * 1e3, 2), "peak": HBM_PEAK_TBPS * 1e3, "unit": "GB/s",
            "frac": round(ach / HBM_PEAK_TBPS, 4), "traffic": traffic, "arithmetic_intensity": round(ai, 1)}


def per_shape_report(lib, probs, stream) -> dict:
    acc_id = {"fp32": 0, "fp16": 1}
    out = {}
    lib.hgemm_rocblas_init()
    lib.hgemm_hipblaslt_heuristic_init()
    lib.hgemm_hipblaslt_autotune_init()
    os.environ.setdefault("HGEMM_AUTOTUNE_MAX_SECONDS", "1.0")
    for p in probs:
        reps = 40 if p.flops < 1e11 else 20

        def base(fname, use_bt):
            def run():
                a, b, bt, c = p.next()
                check(lib, getattr(lib, fname)(a.data_ptr(), (bt if use_bt else b).data_ptr(), c.data_ptr(), p.m, p.n, p.k,
                                               acc_id[p.acc], stream), fname)
            return run

        ours = lambda: launch_ours(lib, p, stream)  # noqa: E731
        auto_ok = (lib.hgemm_hipblaslt_autotune_find_best_tn(p.m, p.n, p.k, acc_id[p.acc]) == 0 and
                   lib.hgemm_hipblaslt_autotune_find_best_nn(p.m, p.n, p.k, acc_id[p.acc]) == 0)
        fns = {"ours": ours, "hipblaslt_heur_tn": base("hgemm_hipblaslt_heuristic_tn", True),
               "hipblaslt_heur_nn": base("hgemm_hipblaslt_heuristic_nn", False), "rocblas_tn": base("hgemm_rocblas_tn", True)}
        if auto_ok:
            fns["hipblaslt_auto_tn"] = base("hgemm_hipblaslt_autotune_tn", True)
            fns["hipblaslt_auto_nn"] = base("hgemm_hipblaslt_autotune_nn", False)
        row = {"acc": p.acc}
        # interleaved rounds (all functions share the clock / thermal history), median of the per-round medians
        for f in fns.values():
            settle(f, 0.15)
        rounds = {k: [] for k in fns}
        iso = {k: [] for k in fns}
        for _ in range(3):
            for k, f in fns.items():
                settle(f, 0.05)
                rounds[k].append(device_time_us(f, reps))
                iso[k].append(isolated_time_us(f, reps))
        for k, v in rounds.items():
            row[k + "_us"] = sorted(v)[1]                       # back-to-back launches (stream throughput)
            row[k + "_isolated_us"] = sorted(iso[k])[1]         # one call, device idle either side
        row["ours_wall_us"] = wall_time_us(ours, reps)
        lt = {k: row[k + "_us"] for k in fns if k.startswith("hipblaslt")}
        best_lt = min(lt, key=lt.get)
        row["hipblaslt_best"] = best_lt
        row["hipblaslt_best_wall_us"] = wall_time_us(fns[best_lt], reps)
        row["ours_tflops"] = p.flops / row["ours_us"] * 1e-6
        heur = min(row["hipblaslt_heur_tn_us"], row["hipblaslt_heur_nn_us"])
        row["hipblaslt_heur_max_tflops"] = p.flops / heur * 1e-6
        row["speedup_vs_hipblaslt_heur_max"] = heur / row["ours_us"]
        if auto_ok:
            auto = min(row["hipblaslt_auto_tn_us"], row["hipblaslt_auto_nn_us"])
            row["hipblaslt_auto_max_tflops"] = p.flops / auto * 1e-6
            row["speedup_vs_hipblaslt_auto_max"] = min(auto, heur) / row["ours_us"]   # strongest hipBLASLt variant
        row["speedup_wall_vs_hipblaslt_best"] = row["hipblaslt_best_wall_us"] / row["ours_wall_us"]
        try:
            row.update(graph_time_us(lib, p))
        except RuntimeError as e:   # reported, never fatal: the headline number does not depend on it
            row["ours_graph_error"] = str(e)[:200]
        row["speedup_isolated_vs_hipblaslt_max"] = min(row[k + "_isolated_us"] for k in lt) / row["ours_isolated_us"]
        row["hipblaslt_compute16_fallback"] = bool(lib.hgemm_hipblaslt_compute16_fallback(0, 1) == 1)
        cfg, sp, gm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib.hgemm_mi355x_plan(p.m, p.n, p.k, ctypes.byref(cfg), ctypes.byref(sp), ctypes.byref(gm))
        name = lib.hgemm_mi355x_config_name(cfg.value)
        row["plan"] = plan_dict(name, sp.value, gm.value)
        row["roofline"] = roofline_entry(p, row["ours_us"], measured_traffic_bytes(p.mnk))
        out[p.mnk] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}
    lib.hgemm_hipblaslt_autotune_destroy()
    lib.hgemm_hipblaslt_heuristic_destroy()
    lib.hgemm_rocblas_destroy()
    return out


def cpu_baseline(workload, seconds: float = 12.0) -> dict:
    """The reference's CPU oracle expression, (a.float() @ b.float()).half(), on the host cores."""
    from oracle import hgemm_oracle as oracle  # checker only: timed as the CPU baseline, never shipped

    shapes = [tuple(int(x) for x in mnk.split("_")) for mnk, _ in workload]
    ops = [(torch.randn((m, k)).half(), torch.randn((k, n)).half(), 2.0 * m * n * k) for m, n, k in shapes]
    flops = passes = 0
    t0 = time.time()
    while time.time() - t0 < seconds:
        for a, b, f in ops:
            torch.matmul(a.float(), b.float()).half()
            flops += f
        passes += 1
    dt = time.time() - t0
    # sanity: the C restatement and the torch expression agree on a small 0/1 case (oracle pinned in tests/)
    import numpy as np

    za, zb = oracle.zero_one_inputs(32, 48, 64, np.random.default_rng(0))
    assert oracle.masked_max_diff(oracle.truth_f32acc(za, zb),
                                  torch.matmul(torch.from_numpy(za).float(), torch.from_numpy(zb).float()).half().numpy()) == 0.0
    return {"value": round(flops / dt * 1e-12, 4), "unit": "TFLOP/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{passes} passes of the workload's shapes as (a.float() @ b.float()).half() on the host in {dt:.1f} s"}


def measured_traffic(mnk: str) -> tuple[float | None, str | None]:
    """(HBM bytes per launch, source file) of the shape's kernel from the committed rocprofv3 PMC summaries (profiles/),
    newest round first; (None, None) when no summary covers the shape."""
    for name in (f"r06_pmc_{mnk}.json", f"r05_pmc_{mnk}.json", f"r04_pmc_{mnk}.json", f"r03_pmc_{mnk}.json", "pmc_summary.json", f"r02_pmc_{mnk}.json", f"r01_pmc_{mnk}.json"):
        f = REPO / "profiles" / name
        if f.exists():
            try:
                d = json.loads(f.read_text())["dominant_kernel"]
                if d.get("mnk") == mnk:
                    return float(d["hbm_bytes_per_launch"]), f"profiles/{name}"
            except Exception:
                continue
    return None, None


def measured_traffic_bytes(mnk: str) -> float | None:
    return measured_traffic(mnk)[0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024, help="GEMM problems per step (one C-ABI call each)")
    ap.add_argument("--workload", type=str, default=":".join(WORKLOAD), help="M_N_K[:fp16|fp32] (default: BASELINE.json configs[2])")
    ap.add_argument("--dump-outputs", type=Path, default=None, metavar="DIR",
                    help="after the timed steps, write the last step's outputs as DIR/c_set<i>.npy (float32)")
    ap.add_argument("--full", action="store_true", help="also measure what takes runs of its own: the per-shape report and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-shapes", action="store_true", help="with --full: skip the per-shape report (ours / hipBLASLt / rocBLAS on BASELINE's shapes)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0 or args.batch < 1:
        ap.error("--steps and --batch must be >= 1, --warmup >= 0")

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run (one rank per GPU)")
        args.gpus = world
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    mnk, acc = (args.workload.split(":") + ["fp32"])[:2]
    lib = load_library()
    torch.manual_seed(1234 + rank)
    prob = Problem(mnk, acc, device)
    stream = torch.cuda.current_stream().cuda_stream

    # HIP events for a sample of the timed region's launches.  They ride on the kernel's own dispatch packet
    # (hgemm_mi355x_time_next_launch -> hipExtLaunchKernel on the launch stream), so they measure the kernel
    # exactly as rocprofv3 does and put no marker packets between launches.
    n_ev = max(1, (args.steps * args.batch + EVENT_STRIDE - 1) // EVENT_STRIDE)
    pool = [(lib.hgemm_mi355x_event_create(), lib.hgemm_mi355x_event_create()) for _ in range(n_ev)]
    if any(e0 is None or e1 is None for e0, e1 in pool):
        raise RuntimeError("hipEventCreate failed")

    def step(events=None, first_launch=0):
        for i in range(args.batch):
            if events is not None and (first_launch + i) % EVENT_STRIDE == 0:
                e0, e1 = pool[len(events)]
                check(lib, lib.hgemm_mi355x_time_next_launch(e0, e1), "time_next_launch")
                events.append((e0, e1))
            launch_ours(lib, prob, stream)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    events = []
    t0 = time.perf_counter()
    for s_i in range(args.steps):
        step(events, s_i * args.batch)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    last_step_sets = sorted({(prob.i - 1 - j) % len(prob.sets) for j in range(min(args.batch, len(prob.sets)))})
    dumped = dump_outputs(prob, last_step_sets, args.dump_outputs) if args.dump_outputs is not None and rank == 0 else None

    wall_per_call_us = elapsed / (args.steps * args.batch) * 1e6     # this rank's clock, before the reduction over ranks
    elapsed, total_flops = reduce_over_ranks(elapsed, prob.flops * args.batch * args.steps, device)
    durs = sorted(lib.hgemm_mi355x_event_elapsed_us(e0, e1) for e0, e1 in events)
    event_mean_us = sum(durs) / len(durs)
    # ONE clock for the roofline: the dispatch-attached events (a dispatch's start event fires while its predecessor drains, so the
    # mean overstates the kernel by ~1 % and `achieved` / `frac` understate it).  wall_per_call_us is a THROUGHPUT interval of the
    # back-to-back stream (it contains the gap between launches but overlaps a launch's head with its predecessor's drain), not a
    # bound on one kernel's duration: reported beside it, never substituted.
    dom_us = event_mean_us
    for e0, e1 in pool:
        lib.hgemm_mi355x_event_destroy(e0)
        lib.hgemm_mi355x_event_destroy(e1)
    traffic, traffic_source = measured_traffic(prob.mnk)
    roof = roofline_entry(prob, dom_us, traffic)
    roof.update({"traffic_source": traffic_source, "kernel": prob.mnk, "launch_us": round(dom_us, 2),
                 "clock": "dispatch-attached HIP events on the launch stream (mean of every 16th launch of the timed region)",
                 "avg_launch_us": round(event_mean_us, 2), "median_launch_us": round(durs[len(durs) // 2], 2), "wall_per_call_us": round(wall_per_call_us, 2),
                 "throughput_tflops_wall": round(prob.flops / wall_per_call_us * 1e-6, 2),
                 "bound_kind": "a dispatch's start event fires while its predecessor drains: launch_us overstates the kernel by ~1 %, achieved and frac "
                               "understate it; wall_per_call_us is the stream's throughput interval, reported separately",
                 "launches_timed": len(durs), "algorithmic_flops_per_launch": prob.flops, "algorithmic_bytes_per_launch": prob.bytes})
    cfg, sp, gm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.hgemm_mi355x_plan(prob.m, prob.n, prob.k, ctypes.byref(cfg), ctypes.byref(sp), ctypes.byref(gm))
    cname = lib.hgemm_mi355x_config_name(cfg.value)
    result = {
        "metric": "HGEMM TFLOP/s", "value": round(total_flops / elapsed * 1e-12, 3), "unit": "TFLOP/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 5), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f16", "data": "synthetic",
        "config": {"workload": f"{mnk} {acc}-acc HGEMM (BASELINE.json configs[2]); step = {args.batch} independent GEMM problems, one C-ABI "
                               "call each, fp16 N(0,1) operands resident in HBM; replicas per GPU",
                   "batch": args.batch, "timed_region_s": round(elapsed, 3),
                   "accumulate": "fp32 MFMA (both modes; CDNA4 has no fp16-accumulate MFMA)",
                   "plan": plan_dict(cname, sp.value, gm.value)},
        "roofline": roof,
    }
    if dumped is not None:
        result["outputs"] = dumped
    if rank == 0:
        if args.full and not args.no_shapes:
            others = [Problem(m_, a_, device) for m_, a_ in BASELINE3 if (m_, a_) != (mnk, acc)]
            result["shapes"] = per_shape_report(lib, others + [prob], stream)
            sp_h = [v["speedup_vs_hipblaslt_heur_max"] for v in result["shapes"].values()]
            result["geomean_speedup_vs_hipblaslt_heuristic_max"] = round(math.exp(sum(map(math.log, sp_h)) / len(sp_h)), 4)
            sp_a = [v["speedup_vs_hipblaslt_auto_max"] for v in result["shapes"].values() if "speedup_vs_hipblaslt_auto_max" in v]
            if sp_a:
                result["geomean_speedup_vs_hipblaslt_autotune_max"] = round(math.exp(sum(map(math.log, sp_a)) / len(sp_a)), 4)
            # the headline's own denominator (BASELINE.md holds no published absolute figure, so `vs_baseline` stays null): the
            # strongest hipBLASLt variant (autotune or heuristic, tn or nn) on the workload shape, same run, back-to-back launches
            w = result["shapes"].get(prob.mnk, {})
            if "speedup_vs_hipblaslt_auto_max" in w:
                lt_us = w["ours_us"] * w["speedup_vs_hipblaslt_auto_max"]     # speedup = hipBLASLt time / our time
                result["vs_hipblaslt_autotune_max"] = {"ratio": round(w["speedup_vs_hipblaslt_auto_max"], 4), "ours_tflops": round(w["ours_tflops"], 1),
                                                       "hipblaslt_tflops": round(prob.flops / lt_us * 1e-6, 1), "clock": "HIP events, back-to-back launches, same run"}
        if args.full and not args.no_cpu_baseline:
            # rank 0, any N (north_star: the 2 / 4 / 8-GPU figures stand "next to torch.matmul on the box's host CPU cores ... in
            # the same run").  The other ranks wait in the closing barrier meanwhile: their timed regions are over.
            result["cpu_baseline"] = cpu_baseline([(mnk, acc)], seconds=12.0 if world == 1 else 6.0)
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
