#!/usr/bin/env python3
"""Scenario loop adjoint against its forward run: one JSON line per problem and batch size with the
time of the plain forward (lmpc_simulate_scenario_device), the taped forward (lmpc_simulate_scenario_taped_device) and
the backward sweep (lmpc_scenario_vjp_device) of the same closed loop in the same job, whole calls between stream
events.  Every timed call works on the next of SETS copies of the inputs (initial states, cotangents, tape), so that no
call finds its data in the 256 MB last-level cache; the outputs of a forward call are allocated by the binding from
torch's cache.  The line also carries the algorithmic bytes of one launch of scenario_adjoint_kernel; its kernel-only
time comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/scenario_adjoint_time.py --one backward --only pendulum --n 1000000

    python tools/scenario_adjoint_time.py [--n 100000 1000000] [--steps 50] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
SETS = 2


def problems():
    """name -> (MPCProblem, x0 range, reference column or None): the pendulum (theta = [x; r; uprev], nth 7, box rows)
    and mass_spring_3in (theta = x, nth 12, 84 rows)."""
    from oracle import mpc2mpqp as omm
    return {"pendulum": (omm.pendulum(), np.array([1.0, 1.0, 0.1, 0.5]), np.array([[0.5], [0.0]])),
            "mass_spring_3in": (omm.mass_spring_3in(), 1.5 * np.ones(12), None)}


def build(lmpc, p):
    from oracle import mpc2mpqp as omm
    q = omm.mpc2mpqp(p)
    nx, nr, nd, nup, npp = p.parameter_dims()
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses), nx=nx, nu=p.nu, nr=nr, nd=nd, nuprev=nup,
                   np_=npp, K=p.K, Np=p.Np)
    return mpc, lmpc.Plant(p.F, p.G, C=p.C)


def glue_bytes(nx, nu, nth, nup, grad_entries):
    """Algorithmic bytes per scenario of a middle launch of scenario_adjoint_kernel without observer: alpha in and out,
    theta-bar, the step's status, the Xbar and Ubar slices, gamma out and back in, ubar out, status_min in and out, and
    a read-modify-write of every gradient entry the step touches."""
    return 2 * 8 * nx + 8 * nth + 4 + 8 * nx + 8 * nu + 2 * 8 * nup + 8 * nu + 8 + 2 * 8 * grad_entries


def main():
    import torch
    import linearmpc_jl_amd as lmpc
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=list(problems()))
    ap.add_argument("--one", choices=["plain", "taped", "backward"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scenario_adjoint_time.py needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    T = a.steps
    f64 = dict(dtype=torch.float64, device=dev)
    lines = []
    for name, (p, xr, rcol) in problems().items():
        if a.only and a.only != name:
            continue
        mpc, plant = build(lmpc, p)
        model = mpc.control_model()
        dyn = plant.dynamics_rows()
        nx, nu, nup = plant.nx, plant.nu, mpc.nuprev
        r = None if rcol is None else torch.from_numpy(rcol).to(dev)
        for N in a.n:
            gen = torch.Generator(device=dev)
            gen.manual_seed(11)
            sets = []
            for s in range(SETS):
                x0 = (2.0 * torch.rand((N, nx), generator=gen, **f64) - 1.0) * torch.from_numpy(xr).to(dev)
                sets.append(dict(x0=x0, Xbar=torch.randn((T + 1, N, nx), generator=gen, **f64),
                                 Ubar=torch.randn((T, N, nu), generator=gen, **f64)))

            def forward(b, tape):
                return model.simulate_scenario(b["x0"].clone(), T, dyn, None, nd=0, ny=0, r=r, r_width=mpc.ny if mpc.nr else 0,
                                               want=("U", "X"), tape=tape)

            def backward(b):
                return model.scenario_vjp(b["tape"], Xbar=b["Xbar"], Ubar=b["Ubar"])

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e-3, res

            same = True
            for b in sets:                                          # warm-up of all three, and the two forwards must agree
                plain, taped = forward(b, False), forward(b, True)
                b["tape"] = taped["tape"]
                g = backward(b)
                torch.cuda.synchronize()
                same = same and bool(torch.equal(plain["U"], taped["U"]) and torch.equal(plain["X"], taped["X"]))
                b["flag_min"], b["status_min"] = int(taped["flag_min"].min()), g["status_min"]
                del plain, taped
            model.check()
            if a.one:
                b = sets[0]
                timed({"plain": lambda: forward(b, False), "taped": lambda: forward(b, True), "backward": lambda: backward(b)}[a.one])
                continue
            tp, tt, tb = [], [], []
            for q in range(a.reps * SETS):
                b = sets[q % SETS]
                tp.append(timed(lambda: forward(b, False))[0])
                tt.append(timed(lambda: forward(b, True))[0])
                tb.append(timed(lambda: backward(b))[0])
            rec = model.scenario_adjoint_launch_info()[-1]
            st = torch.cat([b["status_min"] for b in sets]).cpu().numpy()
            sizes = np.unpackbits(sets[0]["tape"]["active"].cpu().numpy().view(np.uint8), axis=-1).sum(axis=-1)
            entries = (mpc.ny if mpc.nr else 0)
            gb = glue_bytes(nx, nu, model.nth, nup, entries)
            med = lambda v: float(np.median(v))
            line = dict(problem=name, kernel=model.kernel_name, N=N, T=T, nth=model.nth, m=model.m, sets=SETS, reps=a.reps * SETS,
                        identical_forwards=same, plain_s=med(tp), taped_s=med(tt), backward_s=med(tb),
                        taped_over_plain=med(tt) / med(tp), backward_over_taped=med(tb) / med(tt),
                        backward_us_per_scenario_step=1e6 * med(tb) / (N * T), adjoint_NX=rec["NX"], adjoint_grid=rec["grid"],
                        adjoint_lds=rec["lds"], list_pass=rec["list_pass"], glue_bytes_per_scenario_launch=gb,
                        glue_bytes_per_sweep=gb * N * (T + 1), hbm_peak=HBM_PEAK,
                        share_steps_differentiated=float(np.mean(st == 1)), worst_flag=min(b["flag_min"] for b in sets),
                        mean_set=float(sizes.mean()), max_set=int(sizes.max()), plain_runs=tp, taped_runs=tt, backward_runs=tb)
            out = json.dumps(line)
            print(out, flush=True)
            lines.append(out)
            del sets
            torch.cuda.empty_cache()
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
