#!/usr/bin/env python3
"""Differentiable solve against its forward solve: one JSON line per problem with the time per 10^6
points of solve_vjp_device, solve_jacobian_device and solve_device on the same batch in the same job, the share of
points each derivative kernel finished, and the VJP's algorithmic bytes (8 words + 4 + 8 nout + 8 nth + 4 per point)
over its time as a fraction of the 8 TB/s HBM peak.  Every timed call works on the next of SETS copies of the batch, so
that the sets together (more than the 256 MB of last-level cache) keep every call reading from HBM.  Event-timed on
the stream; kernel-only times: rocprofv3 --kernel-trace --stats in a run of its own (sens_lane_kernel, sens_wave_kernel)."""
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

HBM_PEAK = 8.0e12
CACHE_BYTES = 256 << 20


def timed(fns, reps):
    """Seconds per call of the calls fns[0], fns[1], ... taken in turn (one per set of buffers)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in fns:
        f()
    torch.cuda.synchronize()
    e0.record()
    fns[0]()
    e1.record()
    torch.cuda.synchronize()
    one = 1e-3 * e0.elapsed_time(e1)
    reps = max(2 * len(fns), min(reps, int(0.5 / max(one, 1e-6))))         # a window of about half a second
    e0.record()
    for r in range(reps):
        fns[r % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return 1e-3 * e0.elapsed_time(e1) / reps


def main():
    N = int(os.environ.get("SENS_N", 1_000_000))
    reps = int(os.environ.get("SENS_REPS", 4000))           # upper limit of the calls in one timed window
    for label, name, hard in (("pendulum", "pendulum", False), ("pendulum_hard", "pendulum", True),
                              ("mass_spring_3in", "mass_spring_3in", False)):
        g = bench.make_problem(name)
        qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
        nth, nout, words = qp.nth, qp.nout, qp.words
        vjp_bytes = 8 * words + 4 + 8 * nout + 8 * nth + 4
        jac_bytes = 8 * words + 4 + 8 * nout * nth + 4
        sets = max(2, -(-2 * CACHE_BYTES // (N * max(vjp_bytes, 8 * nth + 8 * nout + 4))))
        dev = torch.device("cuda", qp.device)
        bufs = []
        for s in range(sets):
            th = torch.from_numpy(bench.make_theta(name, N, 500 + s, hard)).to(dev)
            act = torch.zeros((N, words), dtype=torch.int64, device=dev)
            x, ef = qp.solve_device(th, active=act)
            bufs.append(dict(th=th, act=act, x=x, ef=ef, xbar=torch.randn((N, nout), dtype=torch.float64, device=dev),
                             thbar=torch.empty((N, nth), dtype=torch.float64, device=dev),
                             st=torch.empty(N, dtype=torch.int32, device=dev)))
        J = torch.empty((N, nout, nth), dtype=torch.float64, device=dev)
        qp.set_option("sens_reserve", 1)
        qp.reserve(N)
        torch.cuda.synchronize()
        t_fwd = timed([lambda b=b: qp.solve_device(b["th"], b["x"], b["ef"]) for b in bufs], reps)
        t_fwd_act = timed([lambda b=b: qp.solve_device(b["th"], b["x"], b["ef"], active=b["act"]) for b in bufs], reps)
        t_vjp = timed([lambda b=b: qp.solve_vjp_device(b["act"], b["ef"], b["xbar"], b["thbar"], b["st"]) for b in bufs], reps)
        t_jac = timed([lambda b=b: qp.solve_jacobian_device(b["act"], b["ef"], J, b["st"]) for b in bufs], reps)
        qp.check()
        rec = qp.sens_launch_info()[-1]
        import sens_cases as sc
        b0 = bufs[0]
        sizes = sc.set_sizes(b0["act"].cpu().numpy().view(np.uint64), qp.m)
        ef = b0["ef"].cpu().numpy()
        fate = sc.fates(sizes, ef, rec["cap"])
        status = b0["st"].cpu().numpy()
        line = {"problem": label, "N": N, "sets": sets, "reps": reps, "n": qp.n, "m": qp.m, "nth": nth, "nout": nout,
                "kernel": qp.kernel_name, "CAP": rec["CAP"], "staged": rec["staged"], "lds": rec["lds"],
                "list_pass": rec["list_pass"],
                "forward_ms_per_1e6": 1e3 * t_fwd * 1e6 / N, "forward_with_masks_ms_per_1e6": 1e3 * t_fwd_act * 1e6 / N,
                "vjp_ms_per_1e6": 1e3 * t_vjp * 1e6 / N, "jacobian_ms_per_1e6": 1e3 * t_jac * 1e6 / N,
                "vjp_over_forward": t_vjp / t_fwd, "jacobian_over_forward": t_jac / t_fwd,
                "vjp_bytes_per_point": vjp_bytes, "vjp_fraction_of_hbm_peak": vjp_bytes * N / t_vjp / HBM_PEAK,
                "jacobian_bytes_per_point": jac_bytes, "jacobian_fraction_of_hbm_peak": jac_bytes * N / t_jac / HBM_PEAK,
                "share_lane_kernel": float(np.mean(fate == "finished")), "share_wave_kernel": float(np.mean(fate == "queued")),
                "share_failed_points": float(np.mean(ef < 1)), "max_set": int(sizes.max()),
                "status_counts": {int(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
                "note": "times are whole calls (memset + kernels) between stream events; kernel-only: rocprofv3 --kernel-trace --stats"}
        print(json.dumps(line), flush=True)
        del bufs, J
        qp.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
