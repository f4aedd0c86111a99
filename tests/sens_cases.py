"""TEST INFRASTRUCTURE: the case table of the differentiable solve (lmpc_solve_vjp* / lmpc_solve_jacobian*), numpy and
the oracle only.  Shared by tests/test_sens_host.py (CPU) and tests/test_gpu_sens.py.

The result of a derivative call depends on the active-set masks, the exit flags and the pack -- not on theta -- so a
batch holds both kinds of mask:

  synthetic   masks of exact sizes |A| = 0, 1, CAP - 1, CAP, CAP + 1 for every CAP built (5 and 8), 16, 17, 32, 33, 63,
              64, 65, with upper-only, lower-only and mixed side bits, one with both bits of a row, one with an active
              IMMUTABLE row, sets of SOFT rows (more of them than variables), a dependent pair of rows (status -1),
              failed points (status 0).  A set's hard rows are at most n and checked independent with numpy
              (`independent`), so that K_A is positive definite and the expected status is 1.
  solver-made the oracle's masks and exit flags on the case's own theta batch.

Batch layout (N_COND points): wavefront 0 (points 0 .. 63) holds only points the lane kernel finishes under every
capacity (|A| <= 4 or failed), wavefront 1 only points it queues under capacity 5 and 8 (9 <= |A| <= 64), wavefront 2
onwards cycles through every synthetic size and special, and the tail is solver-made.  A prefix of 64 points therefore
leaves the work list empty, a prefix of 65 fills it.
"""
from dataclasses import dataclass

import numpy as np

import fast_cases as fc
import lane_cases as lc
import wave_cases as wc
from oracle import ldp as oldp

CAPS = (5, 8)                   # kSensCaps of lmpc_sens_kernel.hpp
MAX_SET = 64                    # kSensMaxSet
BLOCK = 256                     # kSensBlock
STAGE_MAX = 48 * 1024           # kSensStageMax
STAGE_OUT_MAX = 16              # kSensStageOutMax
LDS_MAX = 64 * 1024             # kSensLdsMax
WAVE_LDS = 8 * (64 * 65 + 2 * 64) + 4 * 64
GUARD = 8                       # sentinel rows before and behind every output
SENT = -7.0e300
SENT_I = -123456789
N_COND = 2309
SIZES = (1, 63, 64, 65, 257, N_COND)
SYNTH_SIZES = (0, 1, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65)
N_SOLVER = 400
SENSE_IMMUTABLE, SENSE_SOFT = 4, 8


@dataclass(frozen=True)
class SensCase:
    name: str
    family: str                 # "own", or the module of an existing family: "fast", "lane", "wave", "slow"
    n: int = 0
    mg: int = 0
    nth: int = 0
    nout: int = 1
    nsoft: int = 0
    key: object = None          # the existing family's case
    seed: int = 0

    @property
    def m(self):
        return self.n + self.mg

    @property
    def words(self):
        return (2 * self.m + 63) // 64


def _own(name, n, mg, nth, nout, nsoft, seed=0):
    assert mg - nsoft >= 3 and n + mg >= 9
    return SensCase(name, "own", n, mg, nth, nout, nsoft, seed=seed)


def _ext(family, key, nout):
    return SensCase(f"{family}-{key.name if hasattr(key, 'name') else f'n{key.n}-nth{key.nth}'}", family, key.n,
                    getattr(key, "mg", 0), key.nth, nout, getattr(key, "nsoft", 0), key)


CASES = (
    # n = 1, 2, 5, 12, 63, 64, 65, 127; one mask word (2m <= 64) and several; nth = 1 and 17; nout = 1 and n
    _own("own-n1-m15-nth1", 1, 14, 1, 1, 11),
    _own("own-n2-m76-nth17", 2, 74, 17, 2, 70),
    _own("own-n5-m25-nth1", 5, 20, 1, 5, 16),
    _own("own-n5-m80-nth17", 5, 75, 17, 1, 66),
    _own("own-n12-m76-nth17", 12, 64, 17, 12, 55),
    _own("own-n63-m80-nth1", 63, 17, 1, 63, 6),
    _own("own-n64-m100-nth17", 64, 36, 17, 1, 10),
    _own("own-n65-m130-nth1", 65, 65, 1, 65, 20),
    _own("own-n127-m140-nth17", 127, 13, 17, 1, 4),
    # the existing families, solver-made masks first of all
    _ext("fast", fc.BY_PAIR[(5, 7)], 5),
    _ext("lane", lc.CASES[0], 1),
    _ext("wave", wc.BY_NAME["mr1-n4-m40-nth7"], 1),
    _ext("wave", wc.BY_NAME["mr2-n3-m65-nth2"], 3),
    _ext("wave", wc.BY_NAME["mr1-n12-m64-nth8"], 1),
    _ext("wave", wc.BY_NAME["deep-n40-m90-nth6"], 1),
    _ext("slow", wc.SLOW, 1),
)
BY_NAME = {c.name: c for c in CASES}


def problem(case):
    """(H, f, f_theta, A, bu, bl, W, sense) of a case."""
    if case.family == "fast":
        H, f, f_theta, bu, bl, W = fc.problem(case.key)
        return H, f, f_theta, np.zeros((0, case.n)), bu, bl, W, np.zeros(case.n, np.int32)
    if case.family == "lane":
        return lc.problem(case.key)
    if case.family == "wave":
        return wc.problem(case.key)
    if case.family == "slow":
        return wc.slow_problem(case.key)
    n, mg, nth, m = case.n, case.mg, case.nth, case.m
    rng = np.random.default_rng(53_000 + 1000 * n + 7 * mg + nth + 100_000 * case.seed)
    Rm = rng.standard_normal((n, n))
    H = Rm @ Rm.T + n * np.eye(n)
    A = rng.standard_normal((mg, n))
    A[2] = A[0]                                            # general rows 0 and 2: the dependent pair (both hard)
    bu, bl = rng.uniform(0.5, 2.0, m), -rng.uniform(0.5, 2.0, m)
    W = 0.3 * rng.standard_normal((m, nth))
    W[:n] = 0.0
    f_theta = rng.standard_normal((n, nth))
    f = H @ rng.uniform(-0.004, 0.004, n)
    sense = np.zeros(m, np.int32)
    sense[n + 1] = SENSE_IMMUTABLE                         # general row 1
    sense[m - case.nsoft:] = SENSE_SOFT
    bu[m - case.nsoft:] *= 0.4
    bl[m - case.nsoft:] *= 0.4
    return H, f, f_theta, A, bu, bl, W, sense


def theta(case, N):
    if case.family == "fast":
        return fc.theta(case.key, N)
    if case.family == "lane":
        return lc.theta(case.key, N)
    if case.family == "wave":
        return wc.theta(case.key, N)
    if case.family == "slow":
        return wc.slow_theta(case.key, N)
    rng = np.random.default_rng(29 + 1000 * case.n + 10 * case.nth + 7919 * case.mg + 100_000 * case.seed)
    sc = np.asarray((0.02, 0.3, 1.0, 3.0, 10.0))[np.arange(N) % 5]
    return np.ascontiguousarray(rng.standard_normal((N, case.nth)) * sc[:, None])


def pack_of(L):
    """The dict form of an oracle LDP (what `BatchedQP.ldp()` returns for a handle)."""
    return dict(n=L.n, m=L.m, ms=L.ms, nth=L.nth, nout=L.nout, M=L.M, du=L.du0, dl=L.dl0, Dth=L.Dth, Rout=L.Rout, x0=L.x0,
                Xth=L.Xth, sense=L.sense)


def ldp_of(pack):
    return oldp.LDP(pack["n"], pack["m"], pack["ms"], pack["nth"], pack["nout"], pack["M"], pack["du"], pack["dl"], pack["Dth"],
                    pack["Rout"], pack["x0"], pack["Xth"], pack["sense"], np.ones(pack["m"])).contiguous()


def host_pack(case):
    """The pack oracle.ldp.qp2ldp makes of the case (numpy alone; the host twins take any raw pack)."""
    return pack_of(oldp.qp2ldp(*problem(case), case.nout))


def dependent_pair(case):
    return (case.n, case.n + 2) if case.family == "own" else None


def immutable_row(pack):
    r = np.nonzero(np.asarray(pack["sense"]) & SENSE_IMMUTABLE)[0]
    return int(r[0]) if len(r) else None


def independent(pack, rows):
    """The hard rows among `rows` are linearly independent (numpy; singular values against the largest)."""
    rows = np.asarray(rows, int)
    hard = rows[(np.asarray(pack["sense"])[rows] & SENSE_SOFT) == 0]
    if len(hard) == 0:
        return True
    if len(hard) > pack["n"]:
        return False
    s = np.linalg.svd(np.asarray(pack["M"])[hard], compute_uv=False)
    return bool(s[-1] > 1e-6 * s[0])


def mask_of(rows, sides, m):
    """Mask words of a set: sides[i] = 1 upper (bit j), 2 lower (bit m + j), 3 both."""
    w = np.zeros((2 * m + 63) // 64, np.uint64)
    for j, s in zip(rows, sides):
        for b in ([j] if s & 1 else []) + ([m + j] if s & 2 else []):
            w[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return w


def synth_rows(case, pack, k, style, rng):
    """k rows for a synthetic set, hard rows first in the draw: style "hard" takes as many hard rows as fit (at most n),
    "soft" half of that -- or None if the problem has no such set."""
    n, m = pack["n"], pack["m"]
    sense = np.asarray(pack["sense"])
    dep = dependent_pair(case)
    hardpool = [j for j in range(m) if not sense[j] & SENSE_SOFT and not (dep and j == dep[1])]
    softpool = [j for j in range(m) if sense[j] & SENSE_SOFT]
    hmax = min(n, len(hardpool))
    h = min(k, hmax) if style == "hard" else min(k, hmax) // 2
    if k - h > len(softpool):
        h = k - len(softpool)
    if h > hmax:
        return None
    for _ in range(20):
        rows = sorted(list(rng.choice(hardpool, h, replace=False)) + list(rng.choice(softpool, k - h, replace=False)))
        if independent(pack, rows):
            return rows
    return None


def build(case, pack=None):
    """The case's batch of N_COND points on `pack` (default: host_pack): dict with active (N, words) uint64, exitflag
    (N,) int32, xbar (N, nout), kind (N,) strings, synthetic (N,) bool, expect_done (N,) bool (synthetic points whose
    status must be 1 by construction).  A smaller batch is a prefix."""
    pack = host_pack(case) if pack is None else pack
    m, nout = pack["m"], pack["nout"]
    rng = np.random.default_rng(4242 + 17 * len(case.name) + case.n + 1000 * case.m)
    sizes = {}
    for k in SYNTH_SIZES:
        if k == 65:
            continue
        for style in ("hard", "soft"):
            r = synth_rows(case, pack, k, style, rng)
            if r is not None:
                sizes.setdefault(k, []).append(r)
    masks, flags, kinds, done = [], [], [], []

    def add(rows, sides, flag, kind, expect):
        masks.append(mask_of(rows, sides, m))
        flags.append(flag)
        kinds.append(kind)
        done.append(expect)

    def sides_for(i, k):
        s = i % 3
        return [1] * k if s == 0 else [2] * k if s == 1 else list(rng.integers(1, 3, k))

    def add_size(i, k, flag=None):
        opts = sizes[k]
        rows = opts[i % len(opts)]
        fl = (1, 2, 1)[i % 3] if flag is None else flag
        add(rows, sides_for(i, k), fl, f"synth{k}", fl >= 1)

    small = [k for k in (0, 1, 4) if k in sizes]
    queued = [k for k in (9, 16, 17, 32, 33, 63, 64) if k in sizes]
    for i in range(64):                                    # wavefront 0: finished under every capacity
        if i % 8 == 7:
            add_size(i, queued[i % len(queued)] if queued else small[-1], flag=(-1, -2, 0)[i % 3])     # failed points
        else:
            add_size(i, small[i % len(small)])
    for i in range(64):                                    # wavefront 1: queued under capacity 5 and 8 (where the problem has such sets)
        add_size(i, queued[i % len(queued)] if queued else small[i % len(small)])
    specials = []
    k0 = max(k for k in sizes if k <= 8)
    rows = sizes[k0][0]
    specials.append((rows, [3] + [1] * (k0 - 1) if k0 else [], 1, "both-bits", True))
    imm = immutable_row(pack)
    if imm is not None:
        for base in (sizes.get(4, [[]])[0], queued and sizes[queued[0]][0] or []):
            rows = sorted(set(list(base)[:-1] + [imm])) if len(base) else [imm]
            if independent(pack, rows) and len(rows) <= pack["n"] + sum(1 for j in rows if pack["sense"][j] & SENSE_SOFT):
                specials.append((rows, [1] * len(rows), 1, "immutable", True))
    dep = dependent_pair(case)
    if dep is not None:
        specials.append((list(dep), [1, 2], 1, "dependent", False))
        if queued:
            extra = [j for j in sizes[queued[0]][-1] if j not in dep][:queued[0] - 2]
            specials.append((sorted(list(dep) + extra), [1] * (len(extra) + 2), 1, "dependent-wave", False))
    if m >= 65:
        specials.append((list(range(65)), [1] * 65, 1, "too-many", False))
        specials.append((list(range(m)), [2] * m, 2, "too-many", False))
        specials.append((list(range(m - 65, m)), [3] * 65, -1, "too-many-failed", False))
    n_synth = N_COND - N_SOLVER
    order = sorted(sizes)
    i = 0
    while len(masks) < n_synth:
        if i % 5 == 4:
            add(*specials[(i // 5) % len(specials)])
        else:
            add_size(i, order[(i - i // 5) % len(order)], flag=-1 if i % 23 == 11 else None)
        i += 1
    th = theta(case, N_SOLVER)
    _, ef, _, act = oldp.solve_batch(ldp_of(pack), th)
    active = np.vstack([np.array(masks, np.uint64).reshape(len(masks), -1), act.view(np.uint64).reshape(N_SOLVER, -1)])
    exitflag = np.concatenate([np.array(flags, np.int32), ef.astype(np.int32)])
    kind = np.array(kinds + ["solver"] * N_SOLVER)
    xbar = np.random.default_rng(99 + case.n).standard_normal((N_COND, nout))
    xbar[::7] = 0.0
    xbar[3::11, 0] = 1.0
    return dict(active=np.ascontiguousarray(active), exitflag=np.ascontiguousarray(exitflag), xbar=np.ascontiguousarray(xbar),
                kind=kind, synthetic=kind != "solver", expect_done=np.array(done + [False] * N_SOLVER), theta=th)


def set_sizes(active, m):
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    bits = np.unpackbits(a.view(np.uint8), axis=1, bitorder="little")[:, :2 * m].astype(bool)
    return (bits[:, :m] | bits[:, m:2 * m]).sum(axis=1)


def lane_cap(pack, option=0):
    """CAP of the sens_lane_kernel instantiation the dispatch picks (sens_cap_of): "sens_cap" 5 / 8, or 0 = by the rows
    a set of the problem reaches."""
    if option in CAPS:
        return option
    nsoft = int(((np.asarray(pack["sense"]) & SENSE_SOFT) != 0).sum())
    return 5 if min(pack["n"] + nsoft, pack["m"]) <= 5 else 8


def pack_bytes(pack):
    m, nth, nout = pack["m"], pack["nth"], pack["nout"]
    return 8 * (m * (m + 1) // 2 + m * nout + m * nth + nout * nth + m)


def expected_record(pack, N, jac, option=0, force=False):
    """What lmpc_sens_launch_info must report for a call (without "seq")."""
    CAP = lane_cap(pack, option)
    cap = 0 if force else CAP
    staged = pack_bytes(pack) <= STAGE_MAX
    lds = pack_bytes(pack) if staged else 0
    per = pack["nout"] * pack["nth"] if jac else pack["nth"]
    tile = BLOCK * (8 * per + 4)
    out = per <= STAGE_OUT_MAX and lds + tile <= LDS_MAX
    lp = pack["m"] > cap
    return dict(jac=int(jac), CAP=CAP, cap=cap, grid=(N + BLOCK - 1) // BLOCK, block=BLOCK, lds=lds + (tile if out else 0),
                staged=int(staged) + 2 * int(out), list_pass=int(lp), wave_lds=WAVE_LDS if lp else 0, nprob=N)


def fates(sizes, exitflag, cap):
    """Per point: "finished" (by the lane kernel: small set, failed point, or beyond the 64 rows) or "queued"."""
    q = (np.asarray(exitflag) >= 1) & (sizes > cap) & (sizes <= MAX_SET)
    return np.where(q, "queued", "finished")


def wavefront_kinds(sizes, exitflag, cap):
    """The kinds of wavefront of the lane kernel in a batch: {"finished", "queued", "mixed"}."""
    f = fates(sizes, exitflag, cap) == "queued"
    out = set()
    for s in range(0, len(f), 64):
        w = f[s:s + 64]
        out.add("queued" if w.all() else "finished" if not w.any() else "mixed")
    return out


def check_conditions(case, pack, batch, status):
    """What keeps a case's batch from passing emptily, on the oracle's and numpy's data alone (`status` = the reference's).
    Raises AssertionError naming the condition."""
    sz = set_sizes(batch["active"], pack["m"])
    ef = batch["exitflag"]
    if case.family != "own":                               # (an existing family: its solver-made masks are the point)
        assert (status[batch["expect_done"]] == 1).all(), f"{case.name}: a synthetic independent set is not status 1"
        assert (~batch["synthetic"]).sum() == N_SOLVER and (ef[~batch["synthetic"]] >= 1).any()
        return
    for cap in CAPS:
        kinds = wavefront_kinds(sz, ef, cap)
        assert kinds == {"finished", "queued", "mixed"}, f"{case.name}: wavefront kinds at capacity {cap}: {sorted(kinds)}"
    assert {"queued", "mixed"} <= wavefront_kinds(sz, ef, 0), f"{case.name}: wavefront kinds of a forced list pass"
    assert not (fates(sz[:64], ef[:64], min(CAPS)) == "queued").any(), f"{case.name}: no batch with an empty work list"
    assert (fates(sz[:65], ef[:65], max(CAPS)) == "queued").any(), f"{case.name}: no small batch with a filled work list"
    assert (status[batch["expect_done"]] == 1).all(), f"{case.name}: a synthetic independent set is not status 1"
    want = {1, 0} | ({-1} if dependent_pair(case) else set()) | ({-7} if pack["m"] >= 65 else set())
    assert want <= set(status.tolist()), f"{case.name}: statuses {sorted(set(status.tolist()))}, wanted {sorted(want)}"
    have = set(sz[batch["synthetic"] & (ef >= 1)].tolist())
    reach = {k for k in SYNTH_SIZES if k <= pack["m"] and (k == 65 or k <= pack["n"] + (np.asarray(pack["sense"]) & SENSE_SOFT != 0).sum())}
    assert reach <= have, f"{case.name}: synthetic sizes missing: {sorted(reach - have)}"
    assert batch["synthetic"].sum() >= 1000 and (~batch["synthetic"]).sum() == N_SOLVER


def check_table(cases, statuses):
    """Conditions on the table as a whole: every status value, the dimensions the issue lists."""
    allst = set()
    for s in statuses.values():
        allst |= set(s.tolist())
    assert allst == {1, 0, -1, -7}, f"statuses over the table: {sorted(allst)}"
    own = [c for c in cases if c.family == "own"]
    assert {c.n for c in own} >= {1, 2, 5, 12, 63, 64, 65, 127}
    assert {c.nth for c in own} >= {1, 17}
    assert any(c.words == 1 for c in own) and any(c.words > 1 for c in own)
    assert any(c.nout == 1 for c in own) and any(c.nout == c.n and c.n > 1 for c in own)
    assert any(c.nsoft > c.n for c in own)
