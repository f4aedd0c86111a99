"""TEST INFRASTRUCTURE: the Gaussian draw of include/lmpc_hip.h restated on the host.

    log_               the header's logarithm on [2^-53, 1]: the exponent / mantissa split on the bits, one division, the
                       polynomial by Horner with glibc's fma, the k * ln2 recombination -- every line one numpy operation
    normals            Box-Muller on the Philox restatement of tests/uncertain_reference.py (`philox4x32_10`, `unit`) and
                       the sine and cosine of tests/nonlinear_reference.py (`sin_cos_`), numpy's correctly rounded sqrt
    draw               e = mean + std * z, a separate multiply and add
    blocks             the draws of a source (a `Normal` or uncertain_reference's `Box`) for S scenarios and T steps as a
                       supplied block (S, w, T)
    gaussian_run / nonlinear_gaussian_run
                       the closed-loop reference: the EXISTING reference loops (uncertain_reference.uncertain_run,
                       nonlinear_reference.nonlinear_run) fed the restated draws as supplied blocks -- a draw depends on
                       nothing of the launch, and the arithmetic after the draw is the supplied path's

numpy and glibc's fma (through loop_reference.fma) only: nothing here imports the library or opens a device.  Also here,
shared by the CPU and the GPU tests: the cases and `check_conditions`.
"""
from dataclasses import dataclass, replace

import numpy as np

import nonlinear_reference as nr
import uncertain_reference as ur
from loop_reference import fma
from nonlinear_reference import _b, sin_cos_
from uncertain_reference import Box, philox4x32_10, unit

TWO_PI = _b(0x401921FB54442D18)
LN2_HI, LN2_LO = _b(0x3FE62E42FEE00000), _b(0x3DEA39EF35793C76)
L1, L2, L3, L4, L5, L6, L7 = (_b(h) for h in (0x3FE5555555555593, 0x3FD999999997FA04, 0x3FD2492494229359, 0x3FCC71C51D8E78AF,
                                              0x3FC7466496CB03DE, 0x3FC39A09D078C69F, 0x3FC2F112DF3E5244))
Z_MAX = 8.572                                   # sqrt(106 ln 2) = 8.5717..., rounded up


# ------------------------------------------------------------------ the logarithm
def log_(t):
    """the header's log_ for t in [2^-53, 1], elementwise"""
    t = np.ascontiguousarray(np.asarray(t, np.float64))
    b = t.view(np.uint64)
    hx = (b >> np.uint64(32)) + np.uint64(0x00095F62)
    k = (hx >> np.uint64(20)).astype(np.int64) - 0x3FF
    hx = (hx & np.uint64(0x000FFFFF)) + np.uint64(0x3FE6A09E)
    m = ((hx << np.uint64(32)) | (b & np.uint64(0xFFFFFFFF))).view(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = np.full(t.shape, L7)
    for c in (L6, L5, L4, L3, L2, L1):
        p = fma(p, z, c)
    R = p * z
    hf = (0.5 * f) * f
    dk = k.astype(np.float64)
    lo = s * (hf + R) + dk * LN2_LO
    return dk * LN2_HI - ((hf - lo) - f)


# ------------------------------------------------------------------ the draw
def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)


def pair(r):
    """the standard normal pair of a Philox block's four words"""
    u1 = 1.0 - unit(r[0], r[1])
    t = TWO_PI * unit(r[2], r[3])
    rho = np.sqrt(-2.0 * log_(u1))
    sn, cs = sin_cos_(t)
    return rho * cs, rho * sn


def normals(seed, g, kglobal, stream, w):
    """z of components 0 .. w-1 for the global scenarios g (uint64 array) at global step kglobal: (len(g), w)"""
    g = np.asarray(g, np.uint64)
    out = np.empty((g.size, w))
    for j in range((w + 1) // 2):
        r = philox4x32_10((g & ur.MASK, g >> ur.SH32, np.full(g.size, kglobal, np.uint64),
                           np.full(g.size, (stream << 16) | j, np.uint64)), _key(seed))
        z0, z1 = pair(r)
        out[:, 2 * j] = z0
        if 2 * j + 1 < w:
            out[:, 2 * j + 1] = z1
    return out


@dataclass
class Normal:
    """a source drawn with means `mean` and standard deviations `std`"""
    mean: np.ndarray
    std: np.ndarray


def draw(seed, g, kglobal, stream, mean, std):
    mean, std = np.asarray(mean, float).reshape(-1), np.asarray(std, float).reshape(-1)
    return mean[None, :] + std[None, :] * normals(seed, g, kglobal, stream, mean.size)


def blocks(source, seed, stream, scenario_offset, S, step_offset, T):
    """the draws of a Normal or a Box as a supplied block (S, w, T): column k is the draw of global step step_offset + k"""
    g = np.arange(S, dtype=np.uint64) + np.uint64(scenario_offset)
    if isinstance(source, Normal):
        cols = [draw(seed, g, step_offset + k, stream, source.mean, source.std) for k in range(T)]
    else:
        cols = [ur.draw(seed, g, step_offset + k, stream, source.lo, source.hi) for k in range(T)]
    return np.ascontiguousarray(np.stack(cols, axis=-1))


# ------------------------------------------------------------------ the closed loop
def _supplied(kw, S, T):
    """run arguments with every Normal source replaced by the block of its restated draws"""
    kw = dict(kw)
    for name, stream in (("process", 0), ("measurement_noise", 1)):
        if isinstance(kw[name], Normal):
            kw[name] = blocks(kw[name], kw["seed"], stream, kw["scenario_offset"], S, kw["step_offset"], T)
    return kw


@dataclass
class Case:
    """an uncertain_reference.Case (problem family, observer, cost, Gw, offsets) and what each slot draws"""
    base: ur.Case
    process: str = "gauss"             # "gauss", "uniform", "block", None
    meas: str = "gauss"                # likewise
    pstd: float = 0.1                  # scale of the process standard deviations
    mstd: float = 0.02

    @property
    def name(self):
        return self.base.name


def _base(name, nx, process="gauss", meas="gauss", **kw):
    kind = {"gauss": "draw", "uniform": "draw", "block": "block", None: None}
    return ur.Case(name, nx, S=65, T=3, process=kind[process], meas=kind[meas], **kw)


def case_data(case):
    """uncertain_reference.case_data of the base case with the Gaussian sources put in: means of a tenth of the standard
    deviations, so that neither is zero"""
    data = ur.case_data(case.base)
    rng = np.random.default_rng(5000 + case.base.seed)
    nw, ny = case.base.nw or case.base.nx, case.base.ny
    ps, ms = case.pstd * rng.uniform(0.5, 1.0, nw), case.mstd * rng.uniform(0.5, 1.0, ny)
    if case.process == "gauss":
        data.process = Normal(0.1 * ps * rng.uniform(-1.0, 1.0, nw), ps)
    if case.meas == "gauss":
        data.measurement_noise = Normal(0.1 * ms * rng.uniform(-1.0, 1.0, ny), ms)
    return data


def gaussian_run(case, ldp, data=None, settings=None, **override):
    data = case_data(case) if data is None else data
    kw = ur.run_kwargs(case.base, data)
    kw.update(override)
    S = np.asarray(kw["x0"]).reshape(-1, case.base.nx).shape[0]
    return ur.uncertain_run(ldp, settings=settings, **_supplied(kw, S, kw["T"]))


def check_conditions(case, ref, ldp, data, settings=None):
    """What keeps a closed-loop case from passing emptily, on the reference alone: every flag >= 1; settled steps (empty
    final working set) and constrained ones; every Gaussian source moved what it acts on; and the Gaussian noise changed
    at least one exit flag or active bound against the same run with the Gaussian sources off."""
    assert ref.flags.min() >= 1, (case.name, int(ref.flags.min()))
    assert (ref.active_sizes == 0).any() and (ref.active_sizes > 0).any(), (case.name, "settled and constrained steps")
    off = {}
    if case.process == "gauss":
        assert ref.ws is not None and (ref.ws != 0).all(axis=(0, 1)).any(), case.name
        off.update(process=None, Gw=None)
    if case.meas == "gauss":
        off.update(measurement_noise=None)
    quiet = gaussian_run(case, ldp, data, settings, **off)
    if case.meas == "gauss":
        assert (ref.yms[0] != quiet.yms[0]).all(), (case.name, "the measurement noise never acted")
    assert not (np.array_equal(ref.active, quiet.active) and np.array_equal(ref.flags, quiet.flags)), \
        (case.name, "the Gaussian noise changed no exit flag and no active bound")


X0 = {1: 1.5}
# nx = 1 .. 8 and 9 (every compile-time instantiation and the run-time one), each also with the cost rows; the observer on
# for odd nx; both sources Gaussian
STATES = [Case(_base(f"nx{nx}{'-cost' if cost else ''}", nx, seed=nx, observer=nx % 2 == 1, cost=cost, x0=X0.get(nx, 1.0)))
          for nx in range(1, 10) for cost in (False, True)]
SHAPES = [
    Case(_base("gw-nw1", 4, seed=11, nw=1)),
    Case(_base("gw-nw3", 5, seed=13, nw=3)),
    Case(_base("ny1", 3, seed=16, ny=1)),
    Case(_base("gauss-process-uniform-measurement", 5, meas="uniform", seed=19), meas="uniform"),
    Case(_base("uniform-process-gauss-measurement", 5, process="uniform", seed=20), process="uniform"),
    Case(_base("gauss-process-supplied-measurement", 4, meas="block", seed=21), meas="block"),
    Case(_base("supplied-process-gauss-measurement", 4, process="block", seed=22), process="block"),
    Case(_base("gauss-process-only", 3, meas=None, seed=23, observer=False), meas=None),
    Case(_base("offsets", 4, seed=24, scenario_offset=2 ** 32 + 1000001, step_offset=11)),
]
SPLIT = Case(replace(_base("split", 5, seed=25, nw=3, scenario_offset=7, step_offset=2), S=130, T=6))
SIMULATION = Case(_base("simulation", 4, seed=26, nw=2))
CASES = STATES + SHAPES + [SPLIT, SIMULATION]


# ------------------------------------------------------------------ the nonlinear loop (the cart-pole)
NONLINEAR = nr.Case("cartpole-gaussian", S=65, T=20, q="scenario", process=True, meas=True, scenario_offset=5, step_offset=3)


def nonlinear_data(case=NONLINEAR):
    """nonlinear_reference.case_data with both boxes replaced by Gaussian sources of comparable size"""
    data = nr.case_data(case)
    data.process = Normal(np.array([0.005, 0.0]), np.array([0.02, 0.05]))
    data.measurement_noise = Normal(np.array([0.0, 0.0005]), np.array([0.01, 0.002]))
    return data


def nonlinear_gaussian_run(case, ldp, prog, data, settings=None, **override):
    kw = nr.run_kwargs(case, data)
    kw.update(override)
    return nr.nonlinear_run(ldp, prog=prog, settings=settings, **_supplied(kw, case.S, kw["T"]))


# ------------------------------------------------------------------ the cases of the draw alone
DRAW_W = (1, 2, 3, 5)
DRAW_N = (1, 63, 64, 65, 257)
DRAW_T = 3
DRAW_OFFSETS = ((0, 0), (2 ** 32 + 12345, 7))          # (scenario_offset, step_offset)
DRAW_SEED = 0x9E3779B97F4A7C15


def draw_source(w, dist):
    """the source of a draw case: std == 0 in the last component of the wider ones"""
    rng = np.random.default_rng(600 + w)
    if dist == "gauss":
        std = rng.uniform(0.1, 2.0, w)
        if w >= 3:
            std[-1] = 0.0
        return Normal(rng.uniform(-1.0, 1.0, w), std)
    lo = rng.uniform(-1.0, 0.0, w)
    return Box(lo, lo + rng.uniform(0.0, 2.0, w))
