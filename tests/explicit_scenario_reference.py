"""TEST INFRASTRUCTURE: the scenario loop with an explicit controller restated on the host.

The controller is read from its serialised table (`ExplicitController.blob()`, layout in the header comment of
linearmpc.jl_amd/csrc/lmpc_explicit_kernel.hpp) and evaluated in numpy, one IEEE-754 operation at a time, every
multiply-add through the exact `fma` of tests/loop_reference.py, vectorised over the points of a step:

    walk       node 0; at an inner node {row, left, right} go right if fma-chain(a_row, theta, 0) > b_row, else left;
    candidates the leaf's regions in order; a point is in the first one none of whose rows it violates (leaving a
               candidate at its first violated row changes no number, so every row is evaluated under a mask);
    soft       s = sum over the region's soft multipliers l = fma-chain(L_i, theta, from l_i) of fma(l * l, rho, s);
               |s - primal_tol| <= band * primal_tol: the point counts as unlocated; else flag 2 if s > primal_tol, 1;
    law        u_k = fma-chain(F_k, theta, from g_k).

`explicit_solver` plugs that into scenario_reference.reference_run(..., solve=): located points take the law and the
flag, region -1 takes oracle.ldp.solve_batch, cold, on the LDP it is given.  The library's evaluation is never called.

Also here, because the CPU and the GPU tests share them: the cases (`ECase`), their training boxes and
`check_explicit_conditions`, which keeps a case from passing emptily.
"""
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

import scenario_reference as sr
from loop_reference import fma
from oracle import ldp as oldp

BAND = 1e-3            # the soft band every test builds its controllers with (soft_band)


class Table:
    """The sections of a serialised controller."""

    def __init__(self, blob):
        blob = np.ascontiguousarray(np.asarray(blob, np.uint8))
        head = blob[:128].view(np.int64)
        self.nth, self.nout, self.nregions, nnodes, nleaf = (int(head[i]) for i in range(5))
        o = {k: int(head[i]) for k, i in (("nodes", 6), ("leafidx", 7), ("regions", 8), ("rows", 9), ("laws", 10),
                                          ("soft", 11), ("end", 12))}
        w = self.nth + 1
        self.nodes = blob[o["nodes"]:o["nodes"] + 16 * nnodes].view(np.int32).reshape(-1, 4)
        self.leafidx = blob[o["leafidx"]:o["leafidx"] + 4 * nleaf].view(np.int32)
        self.regions = blob[o["regions"]:o["regions"] + 32 * self.nregions].view(np.int32).reshape(-1, 8)
        self.rows = blob[o["rows"]:o["laws"]].view(np.float64).reshape(-1, w)
        self.laws = blob[o["laws"]:o["soft"]].view(np.float64).reshape(-1, w)
        self.soft = blob[o["soft"]:o["end"]].view(np.float64).reshape(-1, w)


def _chain(rec, th, start):
    """fma(rec[k], th[k], acc) for k = 0 .. nth-1, from `start`; rec (P, nth + 1), th (P, nth)."""
    acc = np.array(start, float)
    for k in range(th.shape[1]):
        acc = fma(rec[:, k], th[:, k], acc)
    return acc


def locate(tab, theta, primal_tol, rho_soft, band=BAND):
    """-> (x (P, nout), NaN where unlocated; flag (P,) int32, 0 where unlocated; region (P,) int32, -1 unlocated)."""
    th = np.ascontiguousarray(np.asarray(theta, float).reshape(-1, tab.nth))
    P, nth = th.shape
    node = np.zeros(P, np.int64)
    while True:
        inner = np.flatnonzero(tab.nodes[node, 0] >= 0)
        if inner.size == 0:
            break
        row = tab.rows[tab.nodes[node[inner], 0]]
        right = _chain(row, th[inner], np.zeros(inner.size)) > row[:, nth]
        node[inner] = np.where(right, tab.nodes[node[inner], 2], tab.nodes[node[inner], 1])
    first, cnt = tab.nodes[node, 1].astype(np.int64), tab.nodes[node, 2]
    found = np.full(P, -1, np.int64)
    for c in range(int(cnt.max()) if P else 0):
        todo = np.flatnonzero((found < 0) & (c < cnt))
        if todo.size == 0:
            break
        reg = tab.leafidx[first[todo] + c].astype(np.int64)
        row0, nrows = tab.regions[reg, 0].astype(np.int64), tab.regions[reg, 1]
        inside = np.ones(todo.size, bool)
        for i in range(int(nrows.max())):
            live = np.flatnonzero(inside & (i < nrows))
            if live.size == 0:
                break
            row = tab.rows[row0[live] + i]
            inside[live] = ~(_chain(row, th[todo[live]], np.zeros(live.size)) > row[:, nth])
        found[todo[inside]] = reg[inside]
    flag = np.zeros(P, np.int32)
    region = found.copy()
    loc = np.flatnonzero(found >= 0)
    s = np.zeros(loc.size)
    soft0, nsoft = tab.regions[found[loc], 3].astype(np.int64), tab.regions[found[loc], 4]
    for i in range(int(nsoft.max()) if loc.size else 0):
        live = np.flatnonzero(i < nsoft)
        rec = tab.soft[soft0[live] + i]
        l = _chain(rec, th[loc[live]], rec[:, nth])
        s[live] = fma(l * l, rho_soft, s[live])
    banded = (nsoft > 0) & (np.abs(s - primal_tol) <= band * primal_tol)
    region[loc[banded]] = -1
    flag[loc[~banded]] = np.where(s[~banded] > primal_tol, 2, 1)
    x = np.full((P, tab.nout), np.nan)
    ok = np.flatnonzero(region >= 0)
    law0 = tab.regions[region[ok], 2].astype(np.int64)
    for k in range(tab.nout):
        rec = tab.laws[law0 + k]
        x[ok, k] = _chain(rec, th[ok], rec[:, nth])
    return x, flag, region.astype(np.int32)


def explicit_solver(tab, ldp, settings, primal_tol, rho_soft, band=BAND):
    """solve(theta, warm) for reference_run, and the list it appends each step's regions to."""
    regions = []
    words = (2 * ldp.m + 63) // 64

    def solve(theta, warm):
        assert warm is None
        u, flag, region = locate(tab, theta, primal_tol, rho_soft, band)
        act = np.zeros((theta.shape[0], words), np.uint64)
        miss = np.flatnonzero(region < 0)
        if miss.size:
            xm, fm, _, am = oldp.solve_batch(ldp, np.ascontiguousarray(theta[miss]), settings)
            u[miss], flag[miss], act[miss] = xm, fm, am
        regions.append(region)
        return u, flag.astype(np.int32), act

    return solve, regions


def run_explicit_case(case, tab, ldp, data=None, settings=None, primal_tol=1e-6, rho_soft=1e-6):
    """reference_run of a case with the controller `tab`; the result carries regions (T, S)."""
    data = case_data(case) if data is None else data
    dims, previews = sr.dims_of(data.prob)
    obs = None if data.kf is None else data.kf.codegen_arrays()
    solve, regions = explicit_solver(tab, ldp, settings, primal_tol, rho_soft)
    ref = sr.reference_run(ldp, dims, sr.plant_of(data.prob), data.x0, case.base.T, r=data.r, d=data.d, p=data.p,
                           noise=data.noise, observer=obs, previews=previews, uprev0=getattr(data.prob, "uprev0", None),
                           warm=False, cost=data.cost, settings=settings, solve=solve)
    ref.regions = np.array(regions)
    return ref


# ------------------------------------------------------------------ the cases
@dataclass
class ECase:
    """A scenario case (scenario_reference.Case) and how its controller is trained: a uniform sample of `nsamples`
    points of the box `scale` x the ranges the case draws from (x0, r, d, the input bound), the `max_regions` most
    frequent regions kept.  kind: "mixed" (the shares below), "miss" (a box disjoint from all the loop visits: every
    step falls back), "hit" (no step falls back)."""
    base: sr.Case
    max_regions: int = 3
    nsamples: int = 20000
    scale: float = 1.0
    kind: str = "mixed"
    nt: int = 0                         # the theta class the case is meant for: 8, 16, 32
    extra: dict = field(default_factory=dict)

    @property
    def name(self):
        return self.base.name


def problem_key(case):
    b = case.base
    return (b.nx, b.nu, b.ny, b.nd, b.np_, b.Np, b.Nc, b.previews, b.soft, b.seed, case.extra.get("rr", True))


def case_data(case):
    """scenario_reference.case_data with the family's `rr` (Rr = 0: no uprev block in theta) and `ubound` switches."""
    b = case.base
    data = sr.case_data(b)
    if case.extra:
        prob, kf = sr.chain_problem(b.nx, b.nu, b.ny, b.nd, b.np_, b.Np, b.Nc, b.previews, b.soft, b.seed,
                                    rr=case.extra.get("rr", True), ubound=case.extra.get("ubound", 0.3))
        data.prob, data.kf = prob, kf if b.observer else None
    return data


def training_box(case, data):
    """(lb, ub) of theta = [x; r-block; d-block; uprev] for the case's controller."""
    b = case.base
    dims, previews = sr.dims_of(data.prob)
    nx, nu, wr, nd, nup, wp = dims
    rH, dH, _ = previews
    assert wp == 0
    half = np.concatenate([np.full(nx, b.x0), np.full(wr * max(rH, 1), 0.5), np.full(nd * max(dH, 1), 0.3),
                           np.full(nup, case.extra.get("ubound", 0.3))]) * case.scale
    if case.kind == "miss":             # far from everything the loop visits
        return 50.0 + 0.0 * half, 50.0 + half
    return -half, half


def training_sample(case, data):
    lb, ub = training_box(case, data)
    rng = np.random.default_rng(900 + case.base.seed)
    return np.ascontiguousarray(lb + (ub - lb) * rng.random((case.nsamples, lb.size)))


def check_explicit_conditions(case, ref, regions=None, stats=None):
    """From the reference run (and, given them, again from the GPU's regions / stats): every scenario solved; in a mixed
    case of 40 scenario-steps or more, located and fallback steps between 5 % and 95 % each, a miss at step 0, a miss
    at step T - 1, a scenario that misses in two or more steps (three or more rounds; not with T = 1, which has one step),
    a scenario that never misses; the observer and
    the noise acted (scenario_reference.check_conditions' own checks); with the soft row, a located step with flag 2."""
    b = case.base
    T, S = b.T, b.S
    assert ref.flag_min.min() >= 1, (case.name, int(ref.flag_min.min()))
    for reg in [ref.regions] + ([regions] if regions is not None else []):
        miss = reg < 0
        if case.kind == "miss":
            assert miss.all(), case.name
        elif case.kind == "hit":
            assert not miss.any(), case.name
        elif S * T >= 40:
            share = float(miss.mean())
            assert 0.05 <= share <= 0.95, (case.name, "share of fallback scenario-steps", share)
            assert miss[0].any(), (case.name, "no miss at step 0")
            assert miss[T - 1].any(), (case.name, "no miss at the last step")
            per = miss.sum(axis=0)
            assert T == 1 or (per >= 2).any(), (case.name, "no scenario misses twice")   # (T = 1 has one step to miss in)
            assert (per == 0).any(), (case.name, "every scenario misses")
        else:
            assert b.pool * T >= 40, case.name
    if stats is not None:
        assert stats["fallback_steps"] == int((regions < 0).sum()) and stats["located_steps"] == int((regions >= 0).sum())
    if b.observer:
        assert np.abs(ref.xhats - ref.xs[:-1]).max() > 0
    if b.noise:
        assert ref.noise_acted
        if b.observer:
            assert not np.array_equal(ref.yms, ref.ys)
    if b.soft and case.kind == "mixed":
        assert ((ref.flags == 2) & (ref.regions >= 0)).any(), (case.name, "no located step carries flag 2")
    if b.cost:
        assert ref.violation.max() > 0


# per case: regions kept, and the input bound where 0.3 leaves the rows active too seldom or too often for the shares
KNOBS = {"e-nx1-nt8": (2, 0.15), "e-nx1-nt16": (2, 0.15), "e-nx1-nt32": (5, 0.1), "e-nx2-nt8": (8, 0.3), "e-nx2-nt16": (14, 0.3),
         "e-nx2-nt32": (8, 0.3), "e-nx5-nt8": (14, 0.3), "e-nx6-nt8": (3, 0.12), "e-nx7-nt8": (8, 1.0), "e-nx7-nt16": (30, 0.3),
         "e-nx7-nt32": (30, 0.3), "e-nx8-nt16": (1, 0.2), "e-nx8-nt32": (1, 0.25), "e-cost-obs": (30, 0.3),
         "e-cost-noobs": (14, 0.3), "e-nx5-nt16": (8, 0.3), "e-nx4-nt8": (3, 0.2), "e-nx3-nt32": (14, 0.3),
         "e-rerun": (1, 0.2)}


def _c(name, nx, nt, observer, rr=True, **kw):
    mr, ub = KNOBS.get(name, KNOBS.get(name.rsplit("-S", 1)[0], (3, 0.3)))
    return ECase(sr.Case(name, nx, seed=kw.pop("seed", 100 + nx), observer=observer, **kw), max_regions=mr, nt=nt,
                 extra={"rr": rr, "ubound": ub})


# one case per instantiation explicit_run_kernel<NXT, NT> that the library dispatches: NXT = nx for nx <= 8, else 0;
# NT = 8 (nth <= 8 and nx < 8), 16 (nth <= 16), 32.  nu = 2; ny, nd as the class allows; S = 300, T = 12
NT8 = [_c(f"e-nx{nx}-nt8", nx, 8, nx % 2 == 1, rr=False, ny=ny, nd=nd)
       for nx, ny, nd in ((1, 3, 2), (2, 3, 2), (3, 3, 2), (4, 2, 2), (5, 1, 2), (6, 1, 1), (7, 1, 0))]
NT16 = [_c("e-nx1-nt16", 1, 16, False, previews=(False, True, False))] + \
       [_c(f"e-nx{nx}-nt16", nx, 16, nx % 2 == 0) for nx in range(2, 10)]
NT32 = [_c(f"e-nx{nx}-nt32", nx, 32, nx % 2 == 1, previews=(True, True, False)) for nx in (1, 2, 4, 5)] + \
       [_c(f"e-nx{nx}-nt32", nx, 32, nx % 2 == 1, previews=(True, False, False)) for nx in (3, 6, 7, 8, 9)]
INSTANCES = NT8 + NT16 + NT32

# S = 1, 63, 64, 65, 255, 256, 257 with T = 1, 2: cuts of one pool
SIZES = [_c(f"e-size-S{S}-T{T}", 5, 16, True, seed=150, S=S, T=T, pool=300) for T in (1, 2) for S in (1, 63, 64, 65, 255, 256, 257)]
# cost with Rr (ulast is live across a fallback round), with and without the observer; the soft row
COST = [_c("e-cost-obs", 4, 16, True, seed=161, cost=True, soft=True, T=8), _c("e-cost-noobs", 3, 16, False, seed=162, cost=True, T=8)]
ALL_MISS = ECase(sr.Case("e-all-miss", 4, seed=171, S=257, T=6), kind="miss", nt=16)
ALL_HIT = ECase(sr.Case("e-all-hit", 4, seed=171, S=257, T=6, x0=0.05), kind="hit", nt=16, max_regions=4096,
                extra={"ubound": 5.0})
RERUN = [_c(f"e-rerun-S{S}", 4, 16, True, seed=181, S=S, T=6, pool=700) for S in (200, 700, 50)]
TWIN = _c("e-twin", 6, 16, True, seed=191, S=70, T=7)

ECASES = INSTANCES + SIZES + COST + [ALL_MISS, ALL_HIT] + RERUN + [TWIN]


def expected_class(case, nth):
    """(NXT, NT) the library dispatches for the case"""
    nx = case.base.nx
    return (nx if nx <= 8 else 0), (8 if (nth <= 8 and nx < 8) else 16 if nth <= 16 else 32)
