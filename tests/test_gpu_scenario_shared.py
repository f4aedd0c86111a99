"""What the scenario loops share on the host -- one step driver and one [observer state | ulast] scratch per handle or
controller -- under a change of loop and of batch size: the loops in turn on ONE handle with N = 300, 65, 300 and T = 3
(the scratch grows, is reused while larger than needed, and N crosses the 256-lane and the 64-lane block edge), every run
bit for bit against the host reference its own suite compares it with."""
import dataclasses

import numpy as np
import pytest

import test_gpu_explicit_scenario as tes
import test_gpu_nonlinear as tnl
import test_gpu_offset_free as tof
import test_gpu_uncertain as tun

pytestmark = pytest.mark.gpu

SIZES = (300, 65, 300)
T = 3


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def test_four_loops_in_turn_on_one_handle(lmpc):
    # plain, uncertain (process noise drawn through a Gw) and nonlinear (a linear program), each with the cost's Rr and
    # the observer but no caller xhat: both scratch halves live; then the plain loop without observer and cost: no scratch
    import torch
    import scenario_reference as sr
    import uncertain_reference as ur
    base = ur.Case("shared", 4, nu=3, ny=2, nd=1, seed=61, T=T, cost=True, x0=0.3, pool=300, nw=2)
    kinds = dict(plain=dict(process=None, meas=None, nw=0, noise=True), uncertain={},
                 bare=dict(process=None, meas=None, nw=0, observer=False, cost=False))
    mpc, refs = None, {}
    for S in SIZES:
        for kind, over in kinds.items():
            case = dataclasses.replace(base, name=f"shared-{kind}-S{S}", S=S, **over)
            data = ur.case_data(case)
            mpc = tun._mpc(lmpc, data.prob) if mpc is None else mpc
            if (kind, S) not in refs:
                refs[kind, S] = tun._reference(mpc, case, data)
            ref = refs[kind, S]
            out = tun._direct(lmpc, mpc, case, data, plain=kind != "uncertain")
            tun._assert_equal(case, out, ref)
            assert (ref.ws is not None) == (kind == "uncertain") and (kind == "bare" or ref.cost.min() > 0)
            if kind != "uncertain":
                continue
            # the nonlinear loop on the plant's own rows as a program: the uncertain run's reference, output for output
            model, nominal = mpc.control_model(), sr.plant_of(data.prob)
            dev = torch.device("cuda", model.device)
            lin = tun._plant(lmpc, nominal)
            prog = lmpc.NonlinearPlant(tnl._linear_program(lmpc, lin.dynamics_rows(), case.nx, case.nu, case.nd), case.nx, case.nu,
                                       case.nd, C=nominal.C, Dd=nominal.Dd, h_offset=nominal.h_offset)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            res = model.simulate_scenario_nonlinear(
                t(data.x0), T, prog, process=tun._source(lmpc, data.process, dev), Gw=data.Gw, seed=case.key,
                measurement_noise=tun._source(lmpc, data.measurement_noise, dev), nd=case.nd, ny=case.ny, r=t(data.r), d=t(data.d),
                use_observer=True, cost=lmpc.BatchedQP.sim_cost(case.nx, case.nu, **data.cost), want_cost=True, want_violation=True,
                want=("U", "X", "Y", "Ym", "Xhat", "D", "W"))
            torch.cuda.synchronize(dev)
            model.check()
            tun._assert_equal(case, {k: v.cpu().numpy() for k, v in res.items() if isinstance(v, torch.Tensor)}, ref)


def test_offset_free_loop_with_and_without_caller_xaug(lmpc):
    # per size the handle's scratch as [xaug | ulast] (Simulation: no caller xaug), then the caller's xaug and ulast alone
    import offset_free_reference as ofr
    mpc = None
    for S in SIZES:
        case = dataclasses.replace(ofr.COST, name=f"shared-S{S}", S=S, T=T, pool=300)
        _, ref, data, mpc = tof._run_and_compare(lmpc, case, mpc, composed=False)
        assert data.cost["Rr"] is not None and ref.cost.min() > 0


def test_explicit_lock_step_then_run_ahead_on_one_controller(lmpc):
    # mode 0 (the shared driver) then mode 1 (the run-ahead kernel) share the controller's [xhat | ulast] scratch
    import explicit_scenario_reference as er
    cost = er.COST[0]
    built = tes._controller(lmpc, cost)
    empc, tab, ldp = built
    for S in SIZES:
        case = dataclasses.replace(cost, base=dataclasses.replace(cost.base, name=f"{cost.base.name}-S{S}", S=S, T=T, pool=300))
        data = er.case_data(case)
        ref = tes._reference(case, empc, tab, ldp, data)
        for mode, what in ((0, "lock-step"), (1, "run-ahead")):
            sim = tes._simulate(lmpc, case, empc, mode, data)
            tes._assert_bitwise(case, sim, ref, f"{what} against the host reference")
        assert data.cost["Rr"] is not None and data.kf is not None and np.abs(ref.cost).min() > 0
