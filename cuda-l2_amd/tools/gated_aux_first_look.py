"""First look at the gated forward's training form (bgemm_mi355x_tn_gated_aux) against the route a training caller has without it.
Recorded, not gated.

    python tools/gated_aux_first_look.py > tuning/gated_aux_first_look_mi355x.jsonl          (an MI355X; about a minute)

Per shape (M, N output, K) and activation, at the member and splits of bgemm_mi355x_tn_plan(M, 2N, K): 15 interleaved rounds of 10 calls
of each column, the median round in microseconds per call.
  fused_aux_us      bgemm_mi355x_launch_tn_gated_aux on the fused [2N][K] weight: H and the fused [M][2N] g|u buffer (u_out = g_out + N)
  stacked_torch_us  bgemm_mi355x_launch_tn_bias at width 2N on the same weight with the stacked bias, which writes g|u, then torch's
                    act(g) * u into H
  gated_us          bgemm_mi355x_launch_tn_gated alone: the difference to fused_aux_us is the price of the two extra stores
One line of JSON per (shape, activation), rows as they fall."""
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402

SHAPES = [(4096, 4096, 4096), (4096, 11008, 4096), (8192, 14336, 4096), (512, 14336, 4096)]
ACTS = {"silu": 4, "gelu": 2}
ROUNDS, CALLS = 15, 10


def main():
    lib = bench.load_library()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_tn_gated_aux.argtypes = [i] * 2 + [p] * 8 + [i] * 8 + [p]
    lib.bgemm_mi355x_launch_tn_gated.argtypes = [i] * 2 + [p] * 6 + [i] * 7 + [p]
    lib.bgemm_mi355x_launch_tn_bias.argtypes = [i] * 2 + [p] * 4 + [i] * 6 + [p]
    lib.bgemm_mi355x_tn_config_name.restype = ctypes.c_char_p
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    for m, n, k in SHAPES:
        x = torch.randn(m, k, generator=gen, device="cuda").to(torch.bfloat16)
        w = (torch.randn(2 * n, k, generator=gen, device="cuda") / k ** 0.5).to(torch.bfloat16)
        bias = torch.randn(2 * n, generator=gen, device="cuda").to(torch.bfloat16)
        h, gu = torch.empty(m, n, dtype=torch.bfloat16, device="cuda"), torch.empty(m, 2 * n, dtype=torch.bfloat16, device="cuda")
        cfg, splits = ctypes.c_int(), ctypes.c_int()
        bench.check(lib, lib.bgemm_mi355x_tn_plan(m, 2 * n, k, ctypes.byref(cfg), ctypes.byref(splits)), "bgemm_mi355x_tn_plan")
        c, s = cfg.value, splits.value
        wu, bu = w.data_ptr() + n * k * 2, bias.data_ptr() + n * 2
        for name, act in ACTS.items():
            tact = F.silu if name == "silu" else F.gelu

            def fused_aux():
                bench.check(lib, lib.bgemm_mi355x_launch_tn_gated_aux(c, s, x.data_ptr(), w.data_ptr(), wu, bias.data_ptr(), bu, h.data_ptr(), gu.data_ptr(),
                                                                      gu.data_ptr() + n * 2, m, n, k, k, k, n, 2 * n, act, stream), "fused aux")

            def stacked():
                bench.check(lib, lib.bgemm_mi355x_launch_tn_bias(c, s, x.data_ptr(), w.data_ptr(), bias.data_ptr(), gu.data_ptr(), m, 2 * n, k, k, k, 2 * n, stream),
                            "stacked")
                torch.mul(tact(gu[:, :n]), gu[:, n:], out=h)

            def gated():
                bench.check(lib, lib.bgemm_mi355x_launch_tn_gated(c, s, x.data_ptr(), w.data_ptr(), wu, bias.data_ptr(), bu, h.data_ptr(), m, n, k, k, k, n, act,
                                                                  stream), "gated")

            cols = {"fused_aux_us": fused_aux, "stacked_torch_us": stacked, "gated_us": gated}
            for fn in cols.values():
                fn()
            torch.cuda.synchronize()
            times = {key: [] for key in cols}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            order = list(cols)
            for r in range(ROUNDS):
                for key in order[r % len(order):] + order[:r % len(order)]:   # interleaved, the first column rotating
                    e0.record()
                    for _ in range(CALLS):
                        cols[key]()
                    e1.record()
                    e1.synchronize()
                    times[key].append(e0.elapsed_time(e1) * 1e3 / CALLS)
            rec = {"mnk": f"{m}_{n}_{k}", "act": name, "config": lib.bgemm_mi355x_tn_config_name(c).decode(), "splits": s, "rounds": ROUNDS, "calls": CALLS}
            rec.update({key: round(statistics.median(v), 3) for key, v in times.items()})
            print(json.dumps(rec), flush=True)
        del x, w, h, gu
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
