"""Scenario-steps/s of the scenario loop with a nonlinear true plant (lmpc_simulate_scenario_nonlinear_device, the
cart-pole as a traced plant program) against the uncertain loop with the linearised plant
(lmpc_simulate_scenario_uncertain_device) -- same controller (the pendulum, Np 50, Nc 5), same N and T, same initial
states, the forms alternating in one process:

    linear       lmpc_simulate_scenario_uncertain_device, the controller's own F, G as the plant
    nonlinear    lmpc_simulate_scenario_nonlinear_device, the cart-pole program, q shared
    nonlinear_q  the same with q (M, m, l) per scenario
    step         lmpc_plant_program_eval_device alone: one plant step of the N scenarios (the interpreter without the
                 loop's glue), per call

Device events around each run; the median of `--reps` warm runs per form and every run's time (the spread).  One JSON
line; `--one FORM` runs a single form twice, for a kernel trace (per-kernel times of the POST kernels and of the solve
come from `rocprofv3 --kernel-trace --stats -- python tools/nonlinear_time.py --one nonlinear`).

    python tools/nonlinear_time.py [--n 100000] [--steps 100] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

FORMS = ("linear", "nonlinear", "nonlinear_q", "step")


def cartpole(lmpc):
    """the reference's invpend example (src/mpc_examples.jl:113-116): q = (M, m, l), damping 10, Ts 0.01"""
    def f(x, u, d, q):
        M, mp, l = q
        s, c = lmpc.sin(x[2]), lmpc.cos(x[2])
        force = 100.0 * u[0] - 10.0 * x[1] - mp * l * x[3] ** 2 * s
        return [x[1], (force + mp * 9.81 * s * c) / (M + mp * s ** 2), x[3],
                (9.81 * s + force * c / (M + mp)) / (l - mp * l * c ** 2 / (M + mp))]
    return f


def main():
    import torch
    import linearmpc_jl_amd as lmpc
    from oracle import mpc2mpqp as omm
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", choices=FORMS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nonlinear_time.py needs a GPU: a rate measured anywhere else says nothing")
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
    plant = lmpc.NonlinearPlant(cartpole(lmpc), 4, 1, nq=3, Ts=0.01, C=p.C)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    f64 = dict(dtype=torch.float64, device=dev)
    x0 = (torch.rand((N, 4), generator=gen, **f64) - 0.5) * torch.tensor([2.0, 2.0, 1.0, 2.0], **f64)
    u0 = (torch.rand((N, 1), generator=gen, **f64) - 0.5) * 4.0
    q_shared = np.array([1.0, 1.0, 0.5])
    q_each = torch.tensor(q_shared, **f64) * (0.8 + 0.4 * torch.rand((N, 3), generator=gen, **f64))
    kw = dict(ny=2, r_width=2, want=("U",))

    def linear():
        x = x0.clone()
        return x, model.simulate_scenario_uncertain(x, T, lin.dynamics_rows(), lin.measurement_rows(), **kw)

    def nonlinear(params=q_shared):
        x = x0.clone()
        return x, model.simulate_scenario_nonlinear(x, T, plant, params=params, **kw)

    def step():
        return model.plant_program_eval_device(plant, x0, u0, None, params=q_shared), None

    forms = dict(linear=linear, nonlinear=nonlinear, nonlinear_q=lambda: nonlinear(q_each), step=step)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        model.check()
        return e0.elapsed_time(e1) * 1e-3, res

    if a.one:
        timed(forms[a.one])                                         # (a first call, so code loading is in the trace)
        timed(forms[a.one])
        return
    res = {k: timed(fn)[1] for k, fn in forms.items()}              # warm-up of every form
    flags = {k: int(res[k][1]["flag_min"].min()) for k in ("linear", "nonlinear", "nonlinear_q")}
    differ = bool(not torch.equal(res["linear"][0], res["nonlinear"][0]))
    runs = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            runs[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in runs.items()}
    rec = dict(problem="pendulum Np50 Nc5", kernel=model.kernel_name, n=N, steps=T, n_ins=int(plant.ins.shape[0]),
               n_slots=int(plant.n_slots), n_consts=int(plant.consts.size), smallest_flag=flags, nonlinear_differs_from_linear=differ,
               nonlinear_over_linear=med["nonlinear"] / med["linear"], nonlinear_q_over_linear=med["nonlinear_q"] / med["linear"],
               per_step_us={k: 1e6 * med[k] / T for k in ("linear", "nonlinear", "nonlinear_q")}, step_alone_us=1e6 * med["step"],
               **{k + "_s": v for k, v in med.items()},
               **{k + "_steps_per_s": N * T / med[k] for k in ("linear", "nonlinear", "nonlinear_q")},
               **{k + "_runs": v for k, v in runs.items()})
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
