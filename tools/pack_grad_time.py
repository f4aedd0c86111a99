#!/usr/bin/env python3
"""Gradient with respect to the pack against the VJP and the forward solve: one JSON line per problem
with the time per 10^6 points of solve_pack_vjp_device (thbar asked for), solve_vjp_device and solve_device on the same
batch in the same job, the ratio to each, the launch record, and the reduce stage's algorithmic bytes (per point: the
record it reads, 16 x min(m, 64); its mask, status, theta and xbar; per 64 points one partial of G doubles written)
over the call's time.  Every timed call works on the next of SETS copies of the batch, so that the sets together (more
than the 256 MB of last-level cache) keep every call reading from HBM.  Event-timed on the stream.  The share of the
time in stage 1 (pack_grad_lane_kernel, pack_grad_wave_kernel), the reduce kernel and the tree kernel comes from a run of
its own under rocprofv3 --kernel-trace --stats with PACK_GRAD_ONLY=1, which makes the pack-gradient calls alone."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import bench  # noqa: E402
import linearmpc_jl_amd as lmpc  # noqa: E402
from sens_time import CACHE_BYTES, HBM_PEAK, timed  # noqa: E402


def main():
    N = int(os.environ.get("PACK_GRAD_N", 1_000_000))
    reps = int(os.environ.get("PACK_GRAD_REPS", 4000))      # upper limit of the calls in one timed window
    only = bool(int(os.environ.get("PACK_GRAD_ONLY", 0)))   # the pack-gradient calls alone, a few of them (for a kernel trace)
    for label, name, hard in (("pendulum", "pendulum", False), ("pendulum_hard", "pendulum", True),
                              ("mass_spring_3in", "mass_spring_3in", False)):
        g = bench.make_problem(name)
        qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
        nth, nout, words, m, n = qp.nth, qp.nout, qp.words, qp.m, qp.n
        G = m * (n + nth + 2) + nout * (n + nth + 1)
        per_point = 8 * words + 4 + 8 * nout + 8 * nth + 4
        sets = max(2, -(-2 * CACHE_BYTES // (N * per_point)))
        dev = torch.device("cuda", qp.device)
        bufs = []
        for s in range(sets):
            th = torch.from_numpy(bench.make_theta(name, N, 500 + s, hard)).to(dev)
            act = torch.zeros((N, words), dtype=torch.int64, device=dev)
            x, ef = qp.solve_device(th, active=act)
            bufs.append(dict(th=th, act=act, x=x, ef=ef, xbar=torch.randn((N, nout), dtype=torch.float64, device=dev),
                             thbar=torch.empty((N, nth), dtype=torch.float64, device=dev),
                             st=torch.empty(N, dtype=torch.int32, device=dev)))
        outs = {k: torch.empty(s, dtype=torch.float64, device=dev)
                for k, s in (("M", (m, n)), ("du", (m,)), ("dl", (m,)), ("Dth", (m, nth)), ("Rout", (nout, n)), ("x0", (nout,)),
                             ("Xth", (nout, nth)))}
        qp.set_option("sens_reserve", 1)
        qp.set_option("pack_grad_reserve", 1)
        qp.reserve(N)
        torch.cuda.synchronize()
        pg = [lambda b=b: qp.solve_pack_vjp_device(b["th"], b["act"], b["ef"], b["xbar"], status=b["st"], out=outs,
                                                   thbar=b["thbar"]) for b in bufs]
        if only:
            for f in pg:
                f()
            torch.cuda.synchronize()
            qp.check()
            print(json.dumps({"problem": label, "N": N, "calls": len(pg), "record": qp.pack_grad_launch_info()[-1]}), flush=True)
        else:
            t_fwd = timed([lambda b=b: qp.solve_device(b["th"], b["x"], b["ef"], active=b["act"]) for b in bufs], reps)
            t_vjp = timed([lambda b=b: qp.solve_vjp_device(b["act"], b["ef"], b["xbar"], b["thbar"], b["st"]) for b in bufs], reps)
            t_pg = timed(pg, reps)
            qp.check()
            rec = qp.pack_grad_launch_info()[-1]
            status = bufs[0]["st"].cpu().numpy()
            reduce_bytes = N * (16 * min(m, 64) + per_point) + (N // 64) * 8 * G
            line = {"problem": label, "N": N, "sets": sets, "n": n, "m": m, "nth": nth, "nout": nout, "doubles": G,
                    "kernel": qp.kernel_name, "record": rec,
                    "forward_with_masks_ms_per_1e6": 1e3 * t_fwd * 1e6 / N, "vjp_ms_per_1e6": 1e3 * t_vjp * 1e6 / N,
                    "pack_vjp_ms_per_1e6": 1e3 * t_pg * 1e6 / N, "pack_vjp_over_vjp": t_pg / t_vjp, "pack_vjp_over_forward": t_pg / t_fwd,
                    "reduce_bytes": reduce_bytes, "reduce_bytes_over_call_time_fraction_of_hbm_peak": reduce_bytes / t_pg / HBM_PEAK,
                    "status_counts": {int(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
                    "note": "times are whole calls (memsets + kernels of every slab) between stream events"}
            print(json.dumps(line), flush=True)
        del bufs, outs, pg
        qp.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
