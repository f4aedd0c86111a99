"""Scenario-steps/s of the scenario loop (lmpc_simulate_scenario_device) against the same loop composed from the
entry points that existed before it -- form_parameter_device -> solve_device -> predict_state on a second handle
that holds the plant's arrays -- driven from Python in the same process, the two alternating.

Two problems: the disturbance-preview double integrator (small, box-constrained: the glue dominates) and the
soft-row preview problem with a measured disturbance (the solve dominates).  Device events around each run; the
median of `--reps` runs each way.  One JSON line per problem; `--one fused|composed` runs a single variant once
(for a kernel trace).

    python tools/scenario_time.py [--n 200000] [--steps 100] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def problems():
    from oracle import mpc2mpqp as omm
    a = omm.make_mpc([[1, 1], [0, 1]], [[0], [1]], [[1.0, 0.0]], Np=5, Nc=5, Q=[10.0], R=[0.1], umin=[-0.5], umax=[0.5],
                     Gd=[[0], [1]])
    a.disturbance_preview = True
    b = omm.preview_sim_kat(True)
    b.Gd = np.array([[0.0], [1.0]])
    b.Dd = np.zeros((2, 1))
    return {"dist_preview": a, "soft_rows": b}


def build(lmpc, p):
    from oracle import mpc2mpqp as omm
    q = omm.mpc2mpqp(p)
    nx, nr, nd, nup, npp = p.parameter_dims()
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses), nx=nx, nu=p.nu, nr=nr, nd=nd,
                   nuprev=nup, np_=npp, Np=p.Np, reference_preview=p.reference_preview,
                   disturbance_preview=p.disturbance_preview)
    plant = lmpc.Plant(p.F, p.G, Gd=p.Gd, C=p.C, Dd=p.Dd)
    twin = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=p.nu)
    twin.set_observer(plant.dynamics_rows(), np.zeros((1, 1 + plant.nx + plant.nd)), np.zeros((1, plant.nx)),
                      plant.nx, plant.nu, plant.nd, 1)
    return mpc, plant, twin


def main():
    import torch
    import linearmpc_jl_amd as lmpc
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", choices=["fused", "composed"])
    ap.add_argument("--only", choices=["dist_preview", "soft_rows"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scenario_time.py needs a GPU: a rate measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    N, T = a.n, a.steps
    lines = []
    for name, p in problems().items():
        if a.only and a.only != name:
            continue
        mpc, plant, twin = build(lmpc, p)
        model = mpc.control_model()
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        f64 = dict(dtype=torch.float64, device=dev)
        x0 = (torch.rand((N, plant.nx), generator=gen, **f64) - 0.5) * 0.8
        ds = (torch.rand((N, T, plant.nd), generator=gen, **f64) - 0.5) * 0.4
        d = ds.transpose(1, 2)
        dT = ds.permute(1, 0, 2).contiguous()                       # (T, N, nd): d_k without a gather per step
        # trajectories are stored column after column ((N, T, w): the layout the C side reads) and handed over as
        # (N, w, T) views, so that the binding's transpose is a no-op and no run pays for a copy of them
        r = rsh = None
        if mpc.reference_preview:
            rs = torch.zeros((N, T, mpc.ny), **f64)
            rs[:, T // 3:, 0] = 0.5 + torch.rand((N, 1), generator=gen, **f64)
            r = rs.transpose(1, 2)
            rsh = rs[:, torch.clamp(torch.arange(T, device=dev) + 1, max=T - 1)].contiguous().transpose(1, 2)
        H = mpc.Np
        rH, dH = (H if mpc.reference_preview else 0), (H if mpc.disturbance_preview else 0)
        rz = torch.zeros((mpc.ny, 1), **f64) if r is None else None
        U = torch.empty((T, N, plant.nu), **f64)
        theta = torch.empty((N, model.nth), **f64)
        u = torch.empty((N, plant.nu), **f64)
        flag = torch.empty(N, dtype=torch.int32, device=dev)
        dyn, meas = plant.dynamics_rows(), plant.measurement_rows()

        def fused():
            x = x0.clone()
            out = model.simulate_scenario(x, T, dyn, None, nd=plant.nd, ny=0, r=r, d=d, r_preview=rH, d_preview=dH,
                                          r_width=mpc.ny, want=("U",))
            return x, out["U"]

        def composed():
            x = x0.clone()
            for k in range(T):
                model.form_parameter_device(x, r=rsh if r is not None else rz, d=d, r_preview=rH, d_preview=dH, k0=k,
                                            theta=theta)
                model.solve_device(theta, x=u, exitflag=flag)
                twin.predict_state(x, u, dT[k])
                U[k].copy_(u)
            return x, U

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, res

        if a.one:
            timed(fused if a.one == "fused" else composed)
            continue
        _, (xa, Ua) = timed(fused)                                  # warm-up of both, and the results must agree
        _, (xb, Ub) = timed(composed)
        same = bool(torch.equal(xa, xb) and torch.equal(Ua, Ub))
        tf, tc = [], []
        for _ in range(a.reps):
            tf.append(timed(fused)[0])
            tc.append(timed(composed)[0])
        nth = model.nth
        rec = dict(problem=name, kernel=model.kernel_name, n=N, steps=T, nth=nth, identical=same,
                   fused_s=float(np.median(tf)), composed_s=float(np.median(tc)),
                   fused_steps_per_s=N * T / float(np.median(tf)), composed_steps_per_s=N * T / float(np.median(tc)),
                   fused_runs=tf, composed_runs=tc)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        twin.close()
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
