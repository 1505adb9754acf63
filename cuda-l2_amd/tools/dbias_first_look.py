"""First look at the bias gradient's fused call: per shape and activation, interleaved rounds of

  fused        bgemm_mi355x_launch_nn_dact_dbias at the NN plan
  colsum       bgemm_mi355x_launch_nn_dact at the same member and splits, then bgemm_mi355x_colsum_c32 over the dZ just written
  torch_sum    the same dact call, then torch's dZ.sum(0, dtype=torch.float32)
  dact         (context) the dact call alone

One JSON record per (shape, activation); a time is the median over the rounds of the mean of `--reps` back-to-back calls between two
events, and each round starts with another contender.  Recorded, not gated.

    python cuda-l2_amd/tools/dbias_first_look.py > cuda-l2_amd/tuning/dbias_first_look_mi355x.jsonl        (on an MI355X)
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

PKG = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(PKG.parent))
import bench  # noqa: E402  (bench.load_library: the library through its C ABI, HGEMM_LIB_DIR honoured)

SHAPES = [(4096, 4096, 4096), (4096, 16384, 4096), (512, 4096, 4096), (8192, 1024, 4096)]     # section 4.29's four
ACTS = {"relu": 1, "gelu": 2, "gelu_tanh": 3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    L = bench.load_library()
    p, i = ctypes.c_void_p, ctypes.c_int
    L.bgemm_mi355x_launch_nn_dact.argtypes = [i] * 2 + [p] * 4 + [i] * 8 + [p]
    L.bgemm_mi355x_launch_nn_dact_dbias.argtypes = [i] * 2 + [p] * 5 + [i] * 9 + [p]
    L.bgemm_mi355x_colsum_c32.argtypes = [p] * 2 + [i] * 4 + [p]
    L.bgemm_mi355x_nn_dact_dbias_reserve_workspace.argtypes = [i] * 3 + [p]
    L.hgemm_mi355x_nn_config_name.restype = ctypes.c_char_p
    stream = torch.cuda.current_stream().cuda_stream
    for m, n, k in SHAPES:
        cfg, splits = ctypes.c_int(), ctypes.c_int()
        assert L.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)) == 0
        assert L.bgemm_mi355x_nn_dact_dbias_reserve_workspace(m, n, k, stream) == 0
        gen = torch.Generator(device="cuda").manual_seed(m + n + k)
        x = torch.randn((m, k), generator=gen, device="cuda").bfloat16()
        w = torch.randn((k, n), generator=gen, device="cuda").bfloat16()
        z = (torch.randn((m, n), generator=gen, device="cuda") * 2).bfloat16()
        dz = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
        db = torch.empty((n,), dtype=torch.float32, device="cuda")
        ptr = [t.data_ptr() for t in (x, w, z, dz)]
        for name, act in ACTS.items():
            def dact():
                assert L.bgemm_mi355x_launch_nn_dact(cfg.value, splits.value, *ptr, m, n, k, k, n, n, n, act, stream) == 0

            def fused():
                assert L.bgemm_mi355x_launch_nn_dact_dbias(cfg.value, splits.value, *ptr, db.data_ptr(), m, n, k, k, n, n, n, act, 0, stream) == 0

            def colsum():
                dact()
                assert L.bgemm_mi355x_colsum_c32(dz.data_ptr(), db.data_ptr(), m, n, n, 0, stream) == 0

            def torch_sum():
                dact()
                torch.sum(dz, 0, dtype=torch.float32, out=db)

            contenders = [("fused", fused), ("colsum", colsum), ("torch_sum", torch_sum), ("dact", dact)]
            for _, f in contenders:                                  # warm: workspaces, torch's kernel choice
                f()
                f()
            torch.cuda.synchronize()
            times = {key: [] for key, _ in contenders}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for r in range(a.rounds):
                for c in range(len(contenders)):
                    key, f = contenders[(r + c) % len(contenders)]
                    e0.record()
                    for _ in range(a.reps):
                        f()
                    e1.record()
                    e1.synchronize()
                    times[key].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            rec = {"mnk": f"{m}_{n}_{k}", "layout": "nn", "output": "c16_dact_dbias", "act": name, "elem": "bf16",
                   "config": L.hgemm_mi355x_nn_config_name(cfg.value).decode(), "splits": splits.value, "rounds": a.rounds, "reps": a.reps,
                   "protocol": "interleaved"}
            for key, _ in contenders:
                rec[f"{key}_us"] = round(statistics.median(times[key]), 3)
                rec[f"{key}_spread_us"] = round(max(times[key]) - statistics.median(times[key]), 3)
            rec["fused_le_colsum"] = rec["fused_us"] <= rec["colsum_us"]
            rec["fused_le_torch_sum"] = rec["fused_us"] <= rec["torch_sum_us"]
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
