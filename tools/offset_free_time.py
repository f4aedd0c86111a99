"""Scenario-steps/s of the offset-free scenario loop (lmpc_simulate_scenario_offset_free_device) against the same loop
composed from the four entry points that existed before it -- correct_state -> compute_control_observer_device ->
predict_state, and predict_state on a second handle that holds the true plant's arrays, the measurement formed by the
caller (one addmm) -- driven from Python in the same process, the two alternating.  For context the scenario loop
with the plain Kalman observer (lmpc_simulate_scenario_device) on the same plant and the nominal controller.

Two problems: the reference's offset-free test (double integrator, velocity form, na = 3: the glue dominates) and a
member of the tests' family with nx = 6, ny = 3, two measured disturbances (na = 9: the run-time kernels).  Device
events around each run; the median of `--reps` warm runs each way.  One JSON line per problem; `--one
fused|composed|kalman` runs a single variant once (for a kernel trace).

    python tools/offset_free_time.py [--n 200000] [--steps 100] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def problems():
    """name -> (nominal problem, controller problem with Gd = [Gd Bd], Dd = [Dd Cd], true plant, observer, ndm)"""
    import offset_free_reference as ofr
    import scenario_reference as sr
    from oracle import mpc2mpqp as omm
    mk = lambda Gd=None: omm.make_mpc([[1, 0.1], [0, 1]], [[0.005], [0.1]], [[1.0, 0.0]], Np=20, Q=[1.0], R=[0.0], Rr=[0.1],
                                      umin=[-1.0], umax=[1.0], Gd=Gd)
    nominal = mk()
    obs = ofr.build_observer(nominal.F, nominal.G, nominal.C, method="velocity", Q=[1e-3, 1e-3], R=[1e-4])
    tracked = mk(Gd=obs.Bd)
    tracked.Dd = obs.Cd
    true = sr.plant_of(nominal)
    true.f_offset = np.array([0.01, 0.0])
    out = {"double_integrator": SimpleNamespace(nominal=nominal, prob=tracked, plant=true, obs=obs, ndm=0, method="velocity")}
    case = next(c for c in ofr.TABLE if c.name == "t-nx6-vel-gate9")
    data = ofr.case_data(case)
    out["chain_nx6"] = SimpleNamespace(nominal=data.base, prob=data.prob, plant=data.plant, obs=data.obs, ndm=case.ndm,
                                       method=case.method)
    return out


def build(lmpc, p):
    from oracle import mpc2mpqp as omm
    q = omm.mpc2mpqp(p)
    nx, nr, nd, nup, npp = p.parameter_dims()
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses), nx=nx, nu=p.nu, nr=nr, nd=nd,
                   nuprev=nup, np_=npp, Np=p.Np, reference_preview=p.reference_preview,
                   disturbance_preview=p.disturbance_preview)
    return mpc, q


def main():
    import torch
    import linearmpc_jl_amd as lmpc
    from oracle import observer as oobs
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", choices=["fused", "composed", "kalman"])
    ap.add_argument("--only", choices=["double_integrator", "chain_nx6"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("offset_free_time.py needs a GPU: a rate measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    N, T = a.n, a.steps
    lines = []
    for name, P in problems().items():
        if a.only and a.only != name:
            continue
        mpc, q = build(lmpc, P.prob)
        model = mpc.control_model()
        t = P.plant
        plant = lmpc.Plant(t.F, t.G, Gd=t.Gd, f_offset=t.f_offset, C=t.C, Dd=t.Dd, h_offset=t.h_offset)
        nx, nu, ny, ndm, ndo = plant.nx, plant.nu, plant.ny, P.ndm, P.obs.nd_offsetfree
        model.set_observer(*P.obs.codegen_arrays(), nx + ndo, nu, ndm, ny)
        model.set_parameter_layout(nx, nr=ny, nd=ndm + ndo, nuprev=nu)
        twin = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=nu)
        twin.set_observer(plant.dynamics_rows(), np.zeros((1, 1 + nx + ndm)), np.zeros((1, nx)), nx, nu, ndm, 1)
        # the context run: the nominal controller with the plain Kalman filter of the nominal model
        kmpc, _ = build(lmpc, P.nominal)
        kmodel = kmpc.control_model()
        b = P.nominal
        kf = oobs.kalman_filter(b.F, b.G, b.C, Gd=b.Gd, Dd=b.Dd, f_offset=b.f_offset, h_offset=b.h_offset, Q=np.ones(nx),
                                R=1e-2 * np.ones(ny))
        kmodel.set_observer(*kf.codegen_arrays(), nx, nu, ndm, ny)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        f64 = dict(dtype=torch.float64, device=dev)
        x0 = (torch.rand((N, nx), generator=gen, **f64) - 0.5) * 2.0
        rs = (torch.rand((N, 1, ny), generator=gen, **f64) - 0.5).expand(N, T, ny).contiguous()      # constant per scenario
        r = rs.transpose(1, 2)                                       # (N, w, T) views of column-after-column storage
        rk = rs[:, 0].contiguous()
        d = dT = None
        if ndm:
            ds = (torch.rand((N, T, ndm), generator=gen, **f64) - 0.5) * 0.6
            d, dT = ds.transpose(1, 2), ds.permute(1, 0, 2).contiguous()
        dyn, meas = plant.dynamics_rows(), plant.measurement_rows()
        Ct, Ddt, h = (torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in (t.C.T, t.Dd.reshape(ny, ndm).T, t.h_offset))
        U = torch.empty((T, N, nu), **f64)
        flag = torch.empty(N, dtype=torch.int32, device=dev)

        def fused():
            x = x0.clone()
            out = model.simulate_scenario_offset_free(x, T, dyn, meas, ndo, nd=ndm, ny=ny, r=r, d=d, want=("U",))
            return x, out["U"]

        def kalman():
            x = x0.clone()
            out = kmodel.simulate_scenario(x, T, dyn, meas, nd=ndm, ny=ny, r=r, d=d, r_width=ny, use_observer=True, want=("U",))
            return x, out["U"]

        def composed():
            x = x0.clone()
            xaug = torch.cat([x0, torch.zeros((N, ndo), **f64)], dim=1)
            u = torch.zeros((N, nu), **f64)
            for k in range(T):
                dk = dT[k] if ndm else None
                ym = torch.addmm(h, x, Ct)
                if ndm:
                    ym = torch.addmm(ym, dk, Ddt)
                model.correct_state(xaug, ym, dk)
                model.compute_control_observer_device(u, xaug, n_measured=ndm, reference=rk, measured_disturbance=dk,
                                                      exitflag=flag)
                model.predict_state(xaug, u, dk)
                twin.predict_state(x, u, dk)
                U[k].copy_(u)
            return x, U

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, res

        forms = dict(fused=fused, composed=composed, kalman=kalman)
        if a.one:
            timed(forms[a.one])                                      # (a first call, so code loading is in the trace)
            timed(forms[a.one])
            continue
        _, (xa, Ua) = timed(fused)                                   # warm-up of all three
        _, (xb, Ub) = timed(composed)
        timed(kalman)
        # the composed loop forms ym with a matrix product (another summation order): agreement to rounding, not bitwise
        diff = float((Ua - Ub).abs().max())
        runs = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():
                runs[k].append(timed(fn)[0])
        med = {k: float(np.median(v)) for k, v in runs.items()}
        rec = dict(problem=name, kernel=model.kernel_name, n=N, steps=T, nth=model.nth, nx=nx, ndo=ndo, ndm=ndm,
                   max_abs_diff_u_fused_composed=diff, **{k + "_s": v for k, v in med.items()},
                   **{k + "_steps_per_s": N * T / v for k, v in med.items()}, **{k + "_runs": v for k, v in runs.items()})
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        twin.close()
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
