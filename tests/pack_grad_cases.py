"""TEST INFRASTRUCTURE: the case table of the gradient with respect to the pack (lmpc_solve_pack_vjp*), numpy and the
oracle only.  Shared by tests/test_pack_grad_host.py (CPU) and tests/test_gpu_pack_grad.py.

The 16 cases of sens_cases with their batches (synthetic masks of every size with upper, lower and mixed side bits, the
SOFT / IMMUTABLE / dependent / failed specials, the solver-made tail).  To these a batch adds theta for every point, and
two 64-point blocks made for the reduction: block 5 holds points without any active row (the reduce kernel skips every
row of it), block 6 failed points only (every leaf of it is +0.0).  Both lie behind point 257, so the prefixes of
sens_cases.SIZES keep their work-list properties.
"""
import numpy as np

import sens_cases as sc

CASES = sc.CASES
BY_NAME = sc.BY_NAME
SIZES = sc.SIZES
N_COND = sc.N_COND
SLAB_MIN = 8                    # kPackGradSlabMin: log2 of the smallest slab "pack_grad_slab" takes
STAGE_MAX = 48 * 1024           # kPackGradStageMax
EMPTY_BLOCK, FAILED_BLOCK = 5, 6
NAMES = ("M", "du", "dl", "Dth", "Rout", "x0", "Xth")


def build(case, pack=None):
    """sens_cases.build plus theta (N_COND, nth) for every point and the two special blocks."""
    pack = sc.host_pack(case) if pack is None else pack
    b = dict(sc.build(case, pack))
    th = sc.theta(case, N_COND).copy()
    th[N_COND - sc.N_SOLVER:] = b["theta"]              # the solver-made tail keeps the theta its masks were solved at
    b["theta"] = np.ascontiguousarray(th)
    b["active"] = b["active"].copy()
    b["exitflag"] = b["exitflag"].copy()
    e = slice(64 * EMPTY_BLOCK, 64 * EMPTY_BLOCK + 64)
    b["active"][e] = 0
    b["exitflag"][e] = 1
    b["exitflag"][64 * FAILED_BLOCK:64 * FAILED_BLOCK + 64] = -1
    xb = b["xbar"].copy()
    xb[e] = np.random.default_rng(7 + case.n).standard_normal(xb[e].shape)
    b["xbar"] = np.ascontiguousarray(xb)
    return b


def shapes(pack):
    n, m, nth, nout = (int(pack[k]) for k in ("n", "m", "nth", "nout"))
    return dict(M=(m, n), du=(m,), dl=(m,), Dth=(m, nth), Rout=(nout, n), x0=(nout,), Xth=(nout, nth))


def doubles(pack):
    """Values of one partial (pack_grad_doubles)."""
    return int(sum(int(np.prod(s)) for s in shapes(pack).values()))


def stages_m(pack):
    return 8 * (pack["m"] + pack["nout"]) * pack["n"] <= STAGE_MAX


def default_slab(pack):
    """log2 of the slab that "pack_grad_slab" 0 picks (pg_slab_log): the largest within the 64 MiB budget, 8 .. 20."""
    per = 16 * max(1, min(pack["m"], 64)) + 4 + 8 * doubles(pack) // 64 + 1
    s = SLAB_MIN
    while s < 20 and (per << (s + 1)) <= (64 << 20):
        s += 1
    return s


def expected_record(pack, N, option=0, force=False, slab=0, cus=256, sums=True):
    """What lmpc_pack_grad_launch_info must report for a call on a device of `cus` compute units (without "seq" and
    "scratch_kib"); sums False: no output array was asked for, the reduce and tree fields are 0."""
    CAP = sc.lane_cap(pack, option)
    cap = 0 if force else CAP
    staged = sc.pack_bytes(pack) <= sc.STAGE_MAX
    sm = stages_m(pack)
    slog = slab if slab else default_slab(pack)
    S = 1 << slog
    nslab = (N + S - 1) // S
    lp = pack["m"] > cap
    first = min(N, S)
    trees = 0
    for s in range(nslab):
        cnt = (min(S, N - s * S) + 63) // 64
        while True:
            trees += 1
            if cnt <= 32:
                break
            cnt = (cnt + 31) // 32
    cnt = nslab
    while True:
        trees += 1
        if cnt <= 32:
            break
        cnt = (cnt + 31) // 32
    grid = (first + 255) // 256
    ny = max(1, min(pack["n"], (2 * cus + grid - 1) // grid))
    chunk = (pack["n"] + ny - 1) // ny
    if not sums:
        trees = grid_r = chunks = lds_r = 0
    else:
        grid_r, chunks, lds_r = grid, (pack["n"] + chunk - 1) // chunk, 8 * (pack["m"] + pack["nout"]) * chunk if sm else 0
    return dict(CAP=CAP, cap=cap, grid=grid, lds=sc.pack_bytes(pack) if staged else 0, staged=int(staged) + 2 * int(sm),
                list_pass=int(lp), wave_grid=min(first, 4 * cus) if lp else 0, reduce_grid=grid_r,
                reduce_chunks=chunks, reduce_lds=lds_r, slab=slog, slabs=nslab, tree_launches=trees,
                doubles=doubles(pack), nprob=N)


def check_conditions(case, pack, batch, ref, slab=SLAB_MIN):
    """What keeps a case's batch from passing emptily, on the reference's results alone (`ref` = pack_grad_reference.
    pack_vjp of the batch).  Raises AssertionError naming the condition."""
    import sens_reference as sr
    m = pack["m"]
    N = len(batch["exitflag"])
    for k in NAMES:
        assert np.any(ref[k] != 0.0), f"{case.name}: {k}-bar is all zero"
    assert np.any(ref["du"] != 0.0) and np.any(ref["dl"] != 0.0), f"{case.name}: du-bar or dl-bar is zero"
    done = ref["status"] == 1
    a = np.ascontiguousarray(batch["active"]).view(np.uint64).reshape(N, -1)
    bits = np.unpackbits(a.view(np.uint8), axis=1, bitorder="little")[:, :2 * m].astype(bool)
    up, lo = bits[done, :m], bits[done, m:2 * m] & ~bits[done, :m]
    assert np.any(up.any(axis=0) & lo.any(axis=0)), f"{case.name}: no row active at its upper side in one point and its lower in another"
    rows = sr.rows_of(batch["active"], m) & done[:, None]
    nb = N // 64
    blk_rows = rows[:nb * 64].reshape(nb, 64, m).any(axis=(1, 2))
    blk_done = done[:nb * 64].reshape(nb, 64)
    assert np.any(~blk_rows & blk_done.all(axis=1)), f"{case.name}: no 64-point block of solved points without an active row"
    assert np.any(~blk_done.any(axis=1)), f"{case.name}: no 64-point block of status != 1 only"
    assert N & (N - 1), f"{case.name}: N is a power of two"
    S = 1 << slab
    assert (N + S - 1) // S >= 3 and N % S, f"{case.name}: the batch does not span 3 slabs with a partial last one"
