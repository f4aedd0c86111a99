#!/usr/bin/env python3
"""Explicit controller against the implicit path (DESIGN.md "Explicit MPC"): one JSON line per problem with the
points/s of ExplicitController.evaluate_device -- kernel only (event-timed, rocprofv3 for the split) and end to end
with the fallback -- and of qp.solve_device on the same batch, the located fraction, mean rows checked per point and
the tree statistics.  Problems: pendulum_N50 (10^6 perturbed closed-loop points, bench.make_theta) and pendulum on
the example's +-20 range."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import linearmpc_jl_amd as lmpc  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e-3 * e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) / reps


def main():
    N = int(os.environ.get("EXPLICIT_N", 1_000_000))
    for name, hard, ntrain in (("pendulum_N50", False, 1_000_000), ("pendulum", True, 1_000_000)):
        g = bench.make_problem(name)
        qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
        t0 = time.perf_counter()
        ec = lmpc.explicit.ExplicitController.from_sample(qp, bench.make_theta(name, ntrain, 101, hard))
        build_s = time.perf_counter() - t0
        th_np = bench.make_theta(name, N, 102, hard)
        th = torch.from_numpy(th_np).cuda()
        x = torch.empty((N, 1), dtype=torch.float64, device="cuda")
        f = torch.empty(N, dtype=torch.int32, device="cuda")
        r = torch.empty(N, dtype=torch.int32, device="cuda")
        xi = torch.empty_like(x)
        fi = torch.empty_like(f)
        dt_e2e, wall_e2e = timed(lambda: ec.evaluate_device(th, x, f, r), 10)
        dt_imp, _ = timed(lambda: qp.solve_device(th, xi, fi), 10)
        torch.cuda.synchronize()
        reg = r.cpu().numpy()
        _, _, _, rows = ec.locate_host(th_np[:20000])
        line = {"problem": name + ("_pm20" if hard else ""), "N": N, "train": ntrain, "build_s": round(build_s, 2),
                "explicit_e2e_points_per_s": N / dt_e2e, "explicit_e2e_wall_points_per_s": N / wall_e2e,
                "implicit_points_per_s": N / dt_imp, "speedup_e2e": dt_imp / dt_e2e,
                "located_fraction": float(np.mean(reg >= 0)), "mean_rows_checked": float(rows.mean()),
                "flags_equal": bool(torch.equal(f, fi)), "tree": ec.info(),
                "note": "kernel-only time: rocprofv3 --kernel-trace --stats (explicit_eval_kernel)"}
        print(json.dumps(line), flush=True)
        ec.close()
        qp.close()


if __name__ == "__main__":
    main()
