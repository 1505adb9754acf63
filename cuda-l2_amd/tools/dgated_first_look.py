"""First look at the gated MLP's input gradient (bgemm_mi355x_nn_dgated) against the route it replaces.  Recorded, not gated.

    python tools/dgated_first_look.py > tuning/dgated_first_look_mi355x.jsonl          (an MI355X; about a minute)

Per shape (M, N inner width, K model width) and activation, at the member and splits of hgemm_mi355x_nn_plan(M, N, K): 15 interleaved
rounds of 10 calls of each column, the median round in microseconds per call.
  fused_us          bgemm_mi355x_launch_nn_dgated on a fused [M][2N] g|u buffer into a fused [M][2N] dg|du buffer
  unfused_torch_us  bgemm_mi355x_launch_nn into a bf16 dH, then torch's element-wise backward: du = act(g) * dH and
                    dg = act_backward(dH * u, g) (aten's silu_backward / gelu_backward), into the same fused buffer
  product_us        the NN product alone, as context
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

SHAPES = [(4096, 11008, 4096), (8192, 14336, 4096), (512, 14336, 4096), (4096, 4096, 4096)]
ACTS = {"silu": 4, "gelu": 2}
ROUNDS, CALLS = 15, 10


def main():
    lib = bench.load_library()
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_nn_dgated.argtypes = [i] * 2 + [p] * 6 + [i] * 8 + [p]
    lib.bgemm_mi355x_launch_nn.argtypes = [i] * 2 + [p] * 3 + [i] * 6 + [p]
    lib.hgemm_mi355x_nn_config_name.restype = ctypes.c_char_p
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    for m, n, k in SHAPES:
        dy = torch.randn(m, k, generator=gen, device="cuda").to(torch.bfloat16)
        wd = (torch.randn(k, n, generator=gen, device="cuda") / k ** 0.5).to(torch.bfloat16)
        gu = torch.randn(m, 2 * n, generator=gen, device="cuda").to(torch.bfloat16)
        dgu, dh = torch.empty(m, 2 * n, dtype=torch.bfloat16, device="cuda"), torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
        cfg, splits = ctypes.c_int(), ctypes.c_int()
        bench.check(lib, lib.hgemm_mi355x_nn_plan(m, n, k, ctypes.byref(cfg), ctypes.byref(splits)), "hgemm_mi355x_nn_plan")
        c, s = cfg.value, splits.value
        g, u = gu[:, :n], gu[:, n:]
        for name, act in ACTS.items():
            tact, tback = (F.silu, torch.ops.aten.silu_backward) if name == "silu" else (F.gelu, torch.ops.aten.gelu_backward)

            def fused():
                bench.check(lib, lib.bgemm_mi355x_launch_nn_dgated(c, s, dy.data_ptr(), wd.data_ptr(), gu.data_ptr(), gu.data_ptr() + n * 2, dgu.data_ptr(),
                                                                   dgu.data_ptr() + n * 2, m, n, k, k, n, 2 * n, 2 * n, act, stream), "fused")

            def product():
                bench.check(lib, lib.bgemm_mi355x_launch_nn(c, s, dy.data_ptr(), wd.data_ptr(), dh.data_ptr(), m, n, k, k, n, n, stream), "product")

            def unfused():
                product()
                torch.mul(tact(g), dh, out=dgu[:, n:])
                dgu[:, :n] = tback(dh * u, g)

            cols = {"fused_us": fused, "unfused_torch_us": unfused, "product_us": product}
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
            rec = {"mnk": f"{m}_{n}_{k}", "act": name, "config": lib.hgemm_mi355x_nn_config_name(c).decode(), "splits": s, "rounds": ROUNDS, "calls": CALLS}
            rec.update({key: round(statistics.median(v), 3) for key, v in times.items()})
            print(json.dumps(rec), flush=True)
        del dy, wd, gu, dgu, dh, g, u
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
