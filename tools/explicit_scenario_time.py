#!/usr/bin/env python3
"""Scenario-steps/s of the scenario loop with an explicit controller, on the two controllers of
tools/explicit_time.py: `pendulum` trained on the example's +-20 range and `pendulum_N50` trained on perturbed
closed-loop points; x0, r drawn the way the training sample was (another seed), uprev0 = 0, no observer, no noise.

Timed forms, alternating in one process, device events around each run, the median of `--reps` runs:
    composed   the loop stitched together from the entry points that existed before the explicit scenario loop:
               form_parameter_device -> ExplicitController.evaluate_device -> predict_state on a second handle that
               holds the plant's arrays, driven from Python (no observer here, so no correct_state / predict_state on
               the handle itself)
    mode0      lmpc_explicit_simulate_scenario_device, lock-step from the older kernels
    mode1      the same entry point, run-ahead kernel with the fallback in rounds
    implicit   lmpc_simulate_scenario_device on the same handle, cold
Every form's first run is the warm-up (scratch grows, statistics settle) and is reported apart as `first_s`; the
results of the three explicit forms must be identical.  One JSON line per problem with launches (`rounds`), the
fallback share and the bytes of state a located scenario-step has to move; `--one FORM` runs a single form once
after its warm-up (for a kernel trace).

    python tools/explicit_scenario_time.py [--n 200000] [--steps 100] [--reps 5] [--train 1000000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

FORMS = ("composed", "mode0", "mode1", "implicit")
PROBLEMS = ("pendulum_pm20", "pendulum_N50")


def problem(name):
    """(oracle MPCProblem, name of bench.make_theta's sample, its `hard` switch)"""
    from oracle import mpc2mpqp as omm
    if name == "pendulum_pm20":
        return omm.pendulum(), "pendulum", True
    return omm.pendulum_benchmark(50), "pendulum_N50", False


def build(lmpc, p):
    from oracle import mpc2mpqp as omm
    q = omm.mpc2mpqp(p)
    nx, nr, nd, nup, npp = p.parameter_dims()
    mq = lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, is_symmetric=q.is_symmetric)
    mpc = lmpc.MPC(mq, nx=nx, nu=p.nu, nr=nr, nd=nd, nuprev=nup, np_=npp, K=p.K, Np=p.Np,
                   reference_preview=p.reference_preview, disturbance_preview=p.disturbance_preview)
    plant = lmpc.Plant(p.F, p.G, C=p.C)
    twin = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=p.nu)
    twin.set_observer(plant.dynamics_rows(), np.zeros((1, 1 + plant.nx)), np.zeros((1, plant.nx)), plant.nx, plant.nu, 0, 1)
    return mpc, plant, twin


def main():
    import torch
    import bench
    import linearmpc_jl_amd as lmpc
    from linearmpc_jl_amd.explicit import ExplicitController
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train", type=int, default=1000000)
    ap.add_argument("--one", choices=FORMS)
    ap.add_argument("--only", choices=PROBLEMS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explicit_scenario_time.py needs a GPU: a rate measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    N, T = a.n, a.steps
    f64 = dict(dtype=torch.float64, device=dev)
    lines = []
    for name in PROBLEMS:
        if a.only and a.only != name:
            continue
        p, sample, hard = problem(name)
        mpc, plant, twin = build(lmpc, p)
        model = mpc.control_model()
        nx, nu, nr, nup = plant.nx, plant.nu, mpc.nr, mpc.nuprev
        if model.nth != nx + nr + nup or mpc.reference_preview:
            raise SystemExit(f"{name}: theta is not [x; r; uprev]")
        t0 = time.perf_counter()
        ec = ExplicitController.from_sample(model, bench.make_theta(sample, a.train, 101, hard))
        build_s = time.perf_counter() - t0
        th0 = bench.make_theta(sample, N, 103, hard)
        x0 = torch.from_numpy(np.ascontiguousarray(th0[:, :nx])).to(dev)
        r = torch.from_numpy(np.ascontiguousarray(th0[:, nx:nx + nr, None])).to(dev)      # (N, nr, 1): held over the run
        dyn = plant.dynamics_rows()
        U = torch.empty((T, N, nu), **f64)
        theta = torch.empty((N, model.nth), **f64)
        u = torch.empty((N, nu), **f64)
        flag = torch.empty(N, dtype=torch.int32, device=dev)
        reg = torch.empty(N, dtype=torch.int32, device=dev)
        stats = {}

        def composed():
            x, up = x0.clone(), torch.zeros((N, nup), **f64)
            for k in range(T):
                model.form_parameter_device(x, r=r, uprev=up, k0=k, theta=theta)
                ec.evaluate_device(theta, u, flag, reg)
                twin.predict_state(x, u)
                up.copy_(u[:, :nup])
                U[k].copy_(u)
            return x, U

        def explicit(mode):
            def run():
                x, up = x0.clone(), torch.zeros((N, nup), **f64)
                out = ec.simulate_scenario_device(x, T, dyn, None, mode=mode, r=r, r_width=nr, uprev=up, want=("U",))
                stats[mode] = out["stats"]
                return x, out["U"]
            return run

        def implicit():
            x, up = x0.clone(), torch.zeros((N, nup), **f64)
            out = model.simulate_scenario(x, T, dyn, None, r=r, r_width=nr, uprev=up, want=("U",))
            return x, out["U"]

        forms = dict(composed=composed, mode0=explicit(0), mode1=explicit(1), implicit=implicit)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, res

        if a.one:
            timed(forms[a.one])
            timed(forms[a.one])
            continue
        first, res = {}, {}
        for k in FORMS:                                             # warm-up of each form; the results must agree
            first[k], (xk, Uk) = timed(forms[k])
            res[k] = (xk.clone(), Uk.clone())
        same = all(torch.equal(res[k][0], res["mode1"][0]) and torch.equal(res[k][1], res["mode1"][1])
                   for k in ("composed", "mode0"))
        same_implicit = bool(torch.equal(res["implicit"][0], res["mode1"][0]) and torch.equal(res["implicit"][1], res["mode1"][1]))
        finite = bool(torch.isfinite(res["mode1"][0]).all())
        res.clear()
        runs = {k: [] for k in FORMS}
        for _ in range(a.reps):
            for k in FORMS:
                runs[k].append(timed(forms[k])[0])
        med = {k: float(np.median(v)) for k, v in runs.items()}
        s1 = stats[1]
        # what a located scenario-step has to move: x read and written, the r column, uprev read and written, U_traj,
        # the region index (the table's rows come out of the caches and are not counted)
        nbytes = 8 * (2 * nx + nr + 2 * nup + nu) + 4
        rec = dict(problem=name, kernel=model.kernel_name, n=N, steps=T, nth=model.nth, train=a.train,
                   build_s=round(build_s, 2), tree=ec.info(), identical=bool(same), implicit_identical=same_implicit,
                   finite=finite, rounds=s1["rounds"], fallback_share=s1["fallback_steps"] / float(N * T),
                   largest_batch=s1["largest_batch"], mode0_launch_steps=stats[0]["rounds"],
                   bytes_per_located_step=nbytes,
                   mode1_fraction_of_8TBs=nbytes * N * T / med["mode1"] / 8e12,
                   **{k + "_steps_per_s": N * T / med[k] for k in FORMS}, **{k + "_s": med[k] for k in FORMS},
                   first_s=first, runs=runs)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        ec.close()
        twin.close()
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
