"""The handle owns its memory (csrc/lmpc_buffer.hpp): every buffer grows once, is given back by lmpc_release_scratch
and grows again, and nothing a call computes depends on it.

One handle per path, each from the existing case tables at its smallest shape: the one-launch kernel and the lane
kernel (smallest n), the wavefront kernel and a search (MR = 1), the row kernel, the tiers pass, the variational chain
(n = 2) and an ExplicitMPC.  Per handle: solve 65 points (one wavefront plus a lane), 130, 65 again, then, where the
path has them, the closed loop (T = 3) and lmpc_compute_control; lmpc_release_scratch; the same calls again.  Every
result equals the same call's result before the release and the oracle (plain solves, lmpc_compute_control) or
tests/loop_reference.py (loops), bit for bit, and the launch records' `seq` advance by exactly the launches made.  The
wavefront handle then runs a kept-factor loop, changes "wave_cap" (which drops the kept state) and runs the loop again.

lmpc_compute_control runs with the layout "theta is the state" (set_parameter_layout(nth)), so that a call solves the
batch the plain solves do: warm pairs of lmpc_compute_control_device at 65 and 130 points (the second call of a pair
starts from the sets the first one left in the handle: the oracle warm-started from the cold run's sets), the
host-pointer call at 65 and 130 points (the block in mapped memory) and, on the lane handle, at the condition batch
(device copies of the arrays), and one more warm pair at 65.  That last pair leaves "these sets belong to a batch of
65" in the handle; the first lmpc_compute_control after the release is a warm call at 65 points again, which has to
start cold.  The lane and the wavefront handle also take the host-pointer solve, cold and warm (the staging group).

The second test reads lmpc_debug_live_blocks() around each handle's life: equal before setup and after the free; after
lmpc_release_scratch it is the count straight after setup plus the kept blocks that the sequence's calls create, counted
from the tables of DESIGN.md ("Handle memory"): the rows "first use" whose call the path's sequence makes."""
import os
import re

import numpy as np
import pytest

import avi_cases as ac
import fast_cases as fc
import lane_cases as lc
import loop_reference as lr
import row_cases as rc
import test_gpu_avi as ta
import test_gpu_explicit as te
import test_gpu_fast as tf
import test_gpu_lane as tl
import test_gpu_row as tr
import test_gpu_tiers as tt
import test_gpu_wave as tw
import tiers_cases as tc
import wave_cases as wc

pytestmark = pytest.mark.gpu

SIZES = (65, 130, 65)
T = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the calls of DESIGN.md's table of kept buffers (its third column)
WAVE_LAUNCH, WAVE_STATS, CC_SMALL = "wavefront-path launch", "wavefront-path launch without a search", \
    "lmpc_compute_control, small batch"


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _live(lmpc):
    return int(lmpc.lib().lmpc_debug_live_blocks())


def _last(recs):
    return recs[-1]["seq"] if recs else 0


def _equal(a, b, what):
    a, b = (list(v.values()) if isinstance(v, dict) else list(v) for v in (a, b))
    assert len(a) == len(b) and len(a) > 0, what
    for k, (p, q) in enumerate(zip(a, b)):
        assert isinstance(p, np.ndarray) and isinstance(q, np.ndarray), (what, k, type(p), type(q))
        assert p.shape == q.shape and p.dtype == q.dtype and np.array_equal(p, q), (what, k)


def _control_calls(qp, name, th, ref, refw, big=None):
    """The lmpc_compute_control part of a sequence (module docstring).  th: the case's condition batch; ref, refw: the
    oracle's (x, exitflag, ...) on it, cold and warm-started from the cold run's sets; big: a batch size at which the
    host-pointer call takes device copies of its arrays instead of the mapped block (None: none)."""
    import torch
    qp.set_parameter_layout(qp.nth)

    def device_pair(N):
        th_d = torch.from_numpy(np.ascontiguousarray(th[:N])).cuda()
        out = []
        for k, want in enumerate((ref, refw)):
            u = torch.full((N, qp.nout), float("nan"), dtype=torch.float64, device="cuda:0")
            ef = torch.full((N,), 12345, dtype=torch.int32, device="cuda:0")
            qp.compute_control_device(u, th_d, exitflag=ef, warm=True)
            torch.cuda.synchronize()
            got = (u.cpu().numpy(), ef.cpu().numpy())
            _equal(got, (want[0][:N], want[1][:N]), (name, "compute_control_device", N, "warm" if k else "first"))
            out += got
        return tuple(out), None                             # (launches: the path's own solves count them)

    def host(N):
        assert (N == big) == (N * (qp.nout + qp.nth) * 8 > 64 * 1024), "which of the two host forms a batch takes"
        u = np.zeros((N, qp.nout))
        ef = qp.compute_control(u, th[:N])
        _equal((u, ef), (ref[0][:N], ref[1][:N]), (name, "compute_control", N))
        return (u, ef), None
    pair = lambda N: (f"compute_control_device, warm pair, {N}", (lambda: device_pair(N)))
    return [pair(65), pair(130)] + [(f"compute_control {N}", (lambda N=N: host(N))) for N in (65, 130) + ((big,) if big else ())] + \
        [pair(65)]


def _host_solves(qp, name, th, ref, refw):
    """lmpc_solve_batch on host arrays, cold and warm from the cold run's sets: the staging group and its warm member."""
    def run(N, warm):
        got = qp.solve(th[:N], warm=np.ascontiguousarray(ref[3][:N]) if warm else None)
        _equal(got, tuple(a[:N] for a in (refw if warm else ref)), (name, "host solve", N, warm))
        return got, None
    return [(f"host solve {N}{', warm' if w else ''}", (lambda N=N, w=w: run(N, w))) for N in (65, 130) for w in (False, True)]


class Path:
    """One handle and the calls of its sequence: each entry of `calls` is (name, run) with run() -> (result, launches)
    that asserts the result against its reference itself (launches None: not counted); `seq()` is the last launch
    number of the path's record; `makes`: the calls of DESIGN.md's table that the sequence contains."""
    makes = ()

    def release(self):
        self.qp.release_scratch()

    def close(self):
        self.qp.close()


class Fast(Path):
    makes = (CC_SMALL,)

    def __init__(self, lmpc):
        from oracle import ldp as oldp
        case = self.case = min(fc.CASES, key=lambda c: (c.n, c.nth))
        self.qp = qp = tf._handle(lmpc, case)
        ref = tf._ref(case, qp)
        th = fc.theta(case, fc.N_COND)
        key = (case, "buffers-warm")
        if key not in tf._REF:
            tf._REF[key] = oldp.solve_batch(tf.oracle_ldp_from(qp.ldp()), th, fc.oracle_settings(case), warm=ref[3])
        self.seq = lambda: (qp.fast_launch_info() or {"seq": 0})["seq"]

        def solve(N):
            import torch
            got = tf._solve_guarded(qp, torch.from_numpy(fc.theta(case, N)).cuda())
            tf._same(got, ref, N, (case.name, N))
            return got, 1
        self.calls = [(f"solve {N}", (lambda N=N: solve(N))) for N in SIZES] + _control_calls(qp, case.name, th, ref, tf._REF[key])


class Lane(Path):
    makes = (CC_SMALL,)

    def __init__(self, lmpc):
        case = self.case = min((c for c in lc.CASES if c.screened), key=lambda c: (c.n, c.nth))
        nx, nr, nup, nu = lc.sim_shape(case)
        self.qp = qp = tl._handle(lmpc, case, nu)
        ref, refw = tl._ref(case, qp, nu), tl._ref_warm(case, qp, nu)
        th = lc.theta(case, lc.N_COND)
        F, G, x0, r, up = lc.sim_data(case, 130)
        loop_ref = tl._cached((case, "buffers-loop"), lambda: lr.simulate_reference(
            tl._ldp(qp), x0, T, F, G, r=r, uprev=up, warm=False, settings=lc.oracle_settings(case)))
        self.seq = lambda: _last(qp.front_pass_info())

        def solve(N):
            got = tl._solve(qp, lc.theta(case, N))
            tl._same(got, ref, N, (case.name, N))
            return got, 1

        def loop(lock_step):
            # lock-step: one screening pass per step; the handle's default (scenario-asynchronous rounds on the second
            # work list and the step counters) makes as many launches as the scenarios need
            qp.set_option("sim_async", 0 if lock_step else 1)
            got = qp.simulate(x0, T, F, G, r=r, uprev=up, warm=False)
            out = {k: got[k] for k in ("U", "X", "x", "flag_min") + (("uprev",) if nup else ())}
            _equal(out, {k: loop_ref[k] for k in out}, (case.name, "loop", lock_step))
            return out, T if lock_step else None
        self.calls = [(f"solve {N}", (lambda N=N: solve(N))) for N in SIZES] + \
            [("loop, lock-step", lambda: loop(True)), ("loop, scenario-asynchronous", lambda: loop(False))] + \
            _host_solves(qp, case.name, th, ref, refw) + _control_calls(qp, case.name, th, ref, refw, big=lc.N_COND)


class Wave(Path):
    makes = (WAVE_LAUNCH, WAVE_STATS, CC_SMALL)

    def __init__(self, lmpc):
        case = self.case = next(c for c in wc.SIM_CASES if c.MR == 1)
        self.qp = qp = tw._sim_handle(lmpc, case)
        qp.set_option("sim_async", 0)
        qp.set_option("sim_keep_factor", 0)
        nu = wc.sim_nu(case)
        ref = tw._ref(case, qp, nu)
        th = wc.theta(case)
        refw = tw._cached((case, "buffers-warm"), lambda: tw._oracle(qp, case, th, warm=ref[3]))
        self.F, self.G, self.x0 = F, G, x0 = wc.sim_data(case, 130)
        loop_ref = tw._cached((case, "buffers-loop"), lambda: lr.simulate_reference(tw._ldp(qp), x0, T, F, G, warm=False,
                                                                                   settings=qp._oset))
        self.seq = lambda: tw._seq(qp)

        def solve(N):
            got, recs = tw._solve(qp, case, wc.theta(case, N))
            tw._same(got, ref, N, (case.name, N))
            return got, len(recs)

        def loop():
            got = qp.simulate(x0, T, F, G, warm=False)
            tw._same_loop(got, loop_ref, (case.name, "loop"))
            return {k: got[k] for k in ("U", "X", "x", "flag_min")}, T
        self.calls = [(f"solve {N}", (lambda N=N: solve(N))) for N in SIZES] + [("loop", loop)] + \
            _host_solves(qp, case.name, th, ref, refw) + _control_calls(qp, case.name, th, ref, refw)

    def kept_factor_then_wave_cap(self):
        """Step 7: a loop on the kept factorisation (the oracle's warm == 2), "wave_cap" 8 -- which gives the kept
        state back -- and the loop again: a solve's arithmetic does not depend on the capacity."""
        from oracle import ldp as oldp
        qp, case = self.qp, self.case
        qp.set_option("sim_keep_factor", 1)
        want = oldp.simulate(tw._ldp(qp), self.x0, T, self.F, self.G, settings=qp._oset, warm=2)
        first = qp.simulate(self.x0, T, self.F, self.G, warm=True)
        tw._same_loop(first, want, (case.name, "kept-factor loop"))
        since = tw._seq(qp)
        qp.set_option("wave_cap", 8)
        again = qp.simulate(self.x0, T, self.F, self.G, warm=True)
        assert tw._seq(qp) - since == T
        assert all(r["cap"] == min(8, case.cap) for r in qp.wave_launch_info(since))
        tw._same_loop(again, want, (case.name, "kept-factor loop after wave_cap 8"))
        qp.set_option("wave_cap", 0)
        qp.set_option("sim_keep_factor", 0)


class Search(Path):
    makes = (WAVE_LAUNCH,)

    def __init__(self, lmpc):
        case = self.case = next(c for c in wc.BNB_CASES if c.MR == 1 and not c.f32)
        self.qp, th, ref = tw._search_handle(lmpc, case)
        qp = self.qp
        self.seq = lambda: tw._seq(qp)

        def solve(N):
            got, recs = tw._solve(qp, case, th[:N])
            tw._same(got, ref, N, (case.name, N))
            return got, len(recs)
        self.calls = [(f"solve {N}", (lambda N=N: solve(N))) for N in SIZES]


class Row(Path):
    makes = (WAVE_LAUNCH, WAVE_STATS)

    def __init__(self, lmpc):
        case = self.case = rc.PLAIN[0]
        self.qp = qp = tr._handle(lmpc, case)
        ref = tr._ref(case, qp)
        self.seq = lambda: tr._seqs(qp)[0]

        def solve(N):
            got, rrecs, wrecs = tr._solve(qp, case, rc.theta(case, N))
            assert len(rrecs) == 1, (case.name, N, rrecs, wrecs)
            tw._same(got, ref, N, (case.name, N))
            return got, 1
        self.calls = [(f"solve {N}", (lambda N=N: solve(N))) for N in SIZES]


class Tiers(Path):
    makes = (WAVE_LAUNCH, WAVE_STATS)

    def __init__(self, lmpc):
        case = self.case = tc.HARD[0]
        self.qp = qp = tt._handle(lmpc, case)
        ref = tt._ref(case, qp)
        self.seq = lambda: tt._seqs(qp)[0]

        def solve(N):
            got, front, wrecs, rrecs = tt._solve(qp, tc.theta(case, N))
            assert [f["kind"] for f in front] == [2], (case.name, N, front)
            tt._same(got, ref, N, (case.name, N))
            return got, 1
        self.calls = [(f"solve {N}", (lambda N=N: solve(N))) for N in SIZES]


class Avi(Path):
    def __init__(self, lmpc):
        case = self.case = next(c for c in ac.CASES if c.n == 2)
        self.qp = qp = ta._handle(lmpc, case)
        ref = ta._ref(case, qp)
        self.seq = lambda: ta._seq(qp)

        def solve(N):
            got, recs = ta._solve(qp, ac.theta(case, N))
            assert len(recs) == 3, (case.name, N, recs)
            ta._same(got, ta._sized(ref, N), (case.name, N))
            return got, 3
        self.calls = [(f"solve {N}", (lambda N=N: solve(N))) for N in SIZES]


class Explicit(Path):
    """An explicit controller of the reference's pendulum: the table's evaluation with the handle's implicit solve
    behind it for the points it does not locate, under the parity rules of tests/test_gpu_explicit.py.  The
    controller's own blocks are not the handle's: lmpc_release_scratch leaves them, lmpc_explicit_free frees them."""
    makes = ("lmpc_explicit_eval_device",)

    def __init__(self, lmpc):
        import bench
        self.qp = qp = te._qp(lmpc, "pendulum", 1)
        self.ec = ec = lmpc.explicit.ExplicitController.from_sample(qp, bench.make_theta("pendulum", 20_000, 27))
        qp.release_scratch()                                # (the training solve's scratch is not part of the set-up state)
        th = bench.make_theta("pendulum", 130, 28)
        self.seq = lambda: 0

        def evaluate(N):
            te._parity(lmpc, qp, ec, th[:N])
            return ec.evaluate(th[:N]), 0
        self.calls = [(f"evaluate {N}", (lambda N=N: evaluate(N))) for N in SIZES]

    def close(self):
        self.ec.close()
        self.qp.close()


PATHS = (Fast, Lane, Wave, Search, Row, Tiers, Avi, Explicit)


def _round(p, tag):
    out = []
    for name, run in p.calls:
        since = p.seq()
        got, launches = run()
        assert launches is None or p.seq() - since == launches, (type(p).__name__, tag, name, "launches made", since, p.seq(), launches)
        out.append(got)
    return out


@pytest.mark.parametrize("make", PATHS, ids=lambda c: c.__name__.lower())
def test_results_do_not_depend_on_the_buffers_history(lmpc, make):
    p = make(lmpc)
    first = _round(p, "fresh handle")
    p.release()
    second = _round(p, "after release_scratch")
    for (name, _), a, b in zip(p.calls, first, second):
        _equal(a, b, (make.__name__, name, "before and after release_scratch"))
    if isinstance(p, Wave):
        p.kept_factor_then_wave_cap()
    p.qp.check()
    p.close()


def _kept_after_release(makes):
    """How many blocks DESIGN.md says a sequence with the calls `makes` leaves behind lmpc_release_scratch beyond what
    setup made: the rows of its "Handle memory" tables marked "first use" whose call (third column) is one of them."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## Handle memory"):]
    sec = sec[:sec.index("\n## ", 4)]
    rows = re.findall(r"^\| `(\w+)` \| (setup|first use) \| ([^|]*?) \|", sec, flags=re.M)
    calls = {call for _, when, call in rows if when == "first use"}
    assert rows and all(m in calls for m in makes), (makes, sorted(calls))
    return sum(1 for _, when, call in rows if when == "first use" and call in makes)


@pytest.mark.parametrize("make", PATHS, ids=lambda c: c.__name__.lower())
def test_live_blocks_return_to_where_they_were(lmpc, make):
    kept = _kept_after_release(make.makes)
    import gc
    gc.collect()
    before = _live(lmpc)
    p = make(lmpc)
    after_setup = _live(lmpc)
    assert after_setup > before
    _round(p, "fresh handle")
    assert _live(lmpc) > after_setup, "the sequence allocates"
    p.release()
    assert _live(lmpc) == after_setup + kept, (make.__name__, before, after_setup, kept, _live(lmpc))
    _round(p, "after release_scratch")
    p.close()
    assert _live(lmpc) == before, (make.__name__, before, _live(lmpc))
