"""Scenario-steps/s of the scenario loop under uncertainty (lmpc_simulate_scenario_uncertain_device) against the plain
scenario loop (lmpc_simulate_scenario_device) on the same handle, the forms alternating in one process:

    plain      lmpc_simulate_scenario_device
    off        the new loop with every source absent and no plant table (the same numbers, bit for bit)
    drawn      process noise drawn on the device, uniform in a box, one component per state
    block      the SAME noise (the W_traj of a drawn run) uploaded as a per-scenario process.src block
    plants1 / plants16 / plantsN    a table of 1, 16 and N perturbed plants, default index

on the two problems of tools/scenario_time.py.  Device events around each run; the median of `--reps` warm runs per
form and every run's time (the spread).  One JSON line per problem; `--one FORM` runs a single form twice (for a kernel
trace).

    python tools/uncertain_time.py [--n 200000] [--steps 100] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FORMS = ("plain", "off", "drawn", "block", "plants1", "plants16", "plantsN")


def main():
    import torch
    import linearmpc_jl_amd as lmpc
    from scenario_time import build, problems
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", choices=FORMS)
    ap.add_argument("--only", choices=["dist_preview", "soft_rows"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uncertain_time.py needs a GPU: a rate measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    N, T = a.n, a.steps
    lines = []
    for name, p in problems().items():
        if a.only and a.only != name:
            continue
        mpc, plant, twin = build(lmpc, p)
        twin.close()
        model = mpc.control_model()
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        f64 = dict(dtype=torch.float64, device=dev)
        nx = plant.nx
        x0 = (torch.rand((N, nx), generator=gen, **f64) - 0.5) * 0.8
        ds = (torch.rand((N, T, plant.nd), generator=gen, **f64) - 0.5) * 0.4
        d = ds.transpose(1, 2)                                      # (N, w, T) views of column-after-column storage
        r = None
        if mpc.reference_preview:
            rs = torch.zeros((N, T, mpc.ny), **f64)
            rs[:, T // 3:, 0] = 0.5 + torch.rand((N, 1), generator=gen, **f64)
            r = rs.transpose(1, 2)
        H = mpc.Np
        rH, dH = (H if mpc.reference_preview else 0), (H if mpc.disturbance_preview else 0)
        dyn = plant.dynamics_rows()
        kw = dict(nd=plant.nd, ny=0, r=r, d=d, r_preview=rH, d_preview=dH, r_width=mpc.ny)
        box = lmpc.Uniform(-0.01 * np.ones(nx), 0.01 * np.ones(nx))
        rng = np.random.default_rng(9)
        table = dyn[None] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (N,) + dyn.shape))
        state = {}

        def plain():
            x = x0.clone()
            return x, model.simulate_scenario(x, T, dyn, None, want=("U",), **kw)

        def run(want=("U",), **un):
            x = x0.clone()
            return x, model.simulate_scenario_uncertain(x, T, dyn, None, want=want, seed=11, **un, **kw)

        forms = dict(plain=plain, off=run, drawn=lambda: run(process=box), block=lambda: run(process=state["block"]),
                     plants1=lambda: run(plants=table[:1]), plants16=lambda: run(plants=table[:16]),
                     plantsN=lambda: run(plants=table))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, res

        # the drawn run's W_traj (T, N, nx) as a block: (N, T, nx) storage handed over as its (N, nx, T) view
        _, (xd, od) = timed(lambda: run(want=("U", "W"), process=box))
        state["block"] = od["W"].permute(1, 0, 2).contiguous().transpose(1, 2)
        if a.one:
            timed(forms[a.one])                                     # (a first call, so code loading is in the trace)
            timed(forms[a.one])
            continue
        res = {k: timed(fn)[1] for k, fn in forms.items()}          # warm-up of every form; the results that must agree
        same_off = bool(torch.equal(res["plain"][0], res["off"][0]) and torch.equal(res["plain"][1]["U"], res["off"][1]["U"]))
        same_block = bool(torch.equal(res["drawn"][0], res["block"][0]) and torch.equal(res["drawn"][1]["U"], res["block"][1]["U"])
                          and torch.equal(xd, res["drawn"][0]))
        runs = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():
                runs[k].append(timed(fn)[0])
        med = {k: float(np.median(v)) for k, v in runs.items()}
        rec = dict(problem=name, kernel=model.kernel_name, n=N, steps=T, nth=model.nth, nx=nx, off_identical_to_plain=same_off,
                   block_identical_to_drawn=same_block, off_over_plain=med["off"] / med["plain"],
                   drawn_over_block=med["drawn"] / med["block"], **{k + "_s": v for k, v in med.items()},
                   **{k + "_steps_per_s": N * T / v for k, v in med.items()}, **{k + "_runs": v for k, v in runs.items()})
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
