"""Scenario-steps/s of the uncertain scenario loop (lmpc_simulate_scenario_uncertain_device) with its noise sources
off, drawn uniform, drawn Gaussian and read from a supplied block -- same controller (the pendulum, Np 50, Nc 5, its
own F, G as the plant), same N and T, same initial states, the forms alternating in one process:

    off        every source absent
    uniform    process noise drawn on the device, uniform in a box, one component per state
    gaussian   process noise drawn on the device, Gaussian, one component per state
    block      the SAME Gaussian numbers (lmpc_noise_draw_device's output) read as a per-scenario supplied block; the
               time to make or upload the block is NOT in this figure (`upload` is the host-to-device copy alone)
    draw       lmpc_noise_draw_device alone: N x T x nx Gaussian draws in one kernel, in draws/s

Device events around each run; the median of `--reps` warm runs per form and every run's time (the spread).  One JSON
line.  With a build of the library that lacks the Gaussian draw (LMPC_HIP_LIB=..., for an A/B of "off" and "uniform"
against an older commit) the last three forms are left out.  `--one FORM` runs a single form twice, for a kernel trace.

    python tools/gaussian_time.py [--n 200000] [--steps 100] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

FORMS = ("off", "uniform", "gaussian", "block", "draw")


def main():
    import torch
    import linearmpc_jl_amd as lmpc
    from oracle import mpc2mpqp as omm
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", choices=FORMS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gaussian_time.py needs a GPU: a rate measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    N, T = a.n, a.steps
    p = omm.pendulum(Np=50, Nc=5)
    q = omm.mpc2mpqp(p)
    nx, nr, nd, nup, npp = p.parameter_dims()
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, is_symmetric=q.is_symmetric), nx=nx, nu=p.nu,
                   nr=nr, nd=nd, nuprev=nup, np_=npp, K=p.K, Np=p.Np, reference_preview=p.reference_preview,
                   disturbance_preview=p.disturbance_preview, parameter_preview=p.parameter_preview)
    model = mpc.control_model()
    lin = lmpc.Plant(p.F, p.G, C=p.C)
    has_gauss = hasattr(lmpc.lib(), "lmpc_noise_draw_device")
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    f64 = dict(dtype=torch.float64, device=dev)
    x0 = (torch.rand((N, 4), generator=gen, **f64) - 0.5) * torch.tensor([2.0, 2.0, 1.0, 2.0], **f64)
    std = np.array([0.002, 0.01, 0.001, 0.01])
    box = lmpc.Uniform(-np.sqrt(3.0) * std, np.sqrt(3.0) * std)         # the same variance
    normal = lmpc.Gaussian(np.zeros(4), std)
    kw = dict(ny=2, r_width=2, want=("U",), seed=11)
    state = {}

    def run(**un):
        x = x0.clone()
        return x, model.simulate_scenario_uncertain(x, T, lin.dynamics_rows(), lin.measurement_rows(), **un, **kw)

    def draw():
        return model.noise_draw(normal, N, T, seed=11, stream=0), None

    forms = dict(off=run, uniform=lambda: run(process=box))
    if has_gauss:
        forms.update(gaussian=lambda: run(process=normal), block=lambda: run(process=state["block"]), draw=draw)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        model.check()
        return e0.elapsed_time(e1) * 1e-3, res

    if has_gauss:
        state["block"] = timed(draw)[1][0]
    if a.one:
        timed(forms[a.one])                                         # (a first call, so code loading is in the trace)
        timed(forms[a.one])
        return
    res = {k: timed(fn)[1] for k, fn in forms.items()}              # warm-up of every form; the results that must agree
    rec = dict(problem="pendulum Np50 Nc5", kernel=model.kernel_name, n=N, steps=T, nx=4, gaussian_build=has_gauss,
               smallest_flag={k: int(res[k][1]["flag_min"].min()) for k in forms if k != "draw"})
    if has_gauss:
        rec["block_identical_to_gaussian"] = bool(torch.equal(res["gaussian"][0], res["block"][0])
                                                  and torch.equal(res["gaussian"][1]["U"], res["block"][1]["U"]))
        rec["gaussian_differs_from_off"] = bool(not torch.equal(res["gaussian"][0], res["off"][0]))
        host = torch.empty((N, T, 4), dtype=torch.float64).pin_memory()
        host.copy_(state["block"].transpose(1, 2))
        up = []
        for _ in range(a.reps):
            up.append(timed(lambda: (host.to(dev, non_blocking=True), None))[0])
        rec["upload_pinned_s"], rec["upload_pinned_runs"], rec["block_bytes"] = float(np.median(up)), up, host.numel() * 8
    runs = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            runs[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in runs.items()}
    loops = [k for k in forms if k != "draw"]
    rec.update(uniform_over_off=med["uniform"] / med["off"], **{k + "_s": v for k, v in med.items()},
               **{k + "_steps_per_s": N * T / med[k] for k in loops}, **{k + "_runs": v for k, v in runs.items()})
    if has_gauss:
        rec.update(gaussian_over_uniform=med["gaussian"] / med["uniform"], gaussian_over_block=med["gaussian"] / med["block"],
                   gaussian_over_block_plus_upload=med["gaussian"] / (med["block"] + rec["upload_pinned_s"]),
                   draws_per_s=N * T * 4 / med["draw"])
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
