// Glue kernels of the scenario loop (lmpc_simulate_scenario_device): one pass of the reference's Simulation
// (reference src/simulation.jl:93-113) around the batched solve, WITH disturbance, affine parameters, plant and
// measurement offsets and the generated state observer -- a PRE kernel (measure, correct, form theta) and a POST
// kernel (predict, true plant step, bookkeeping, running cost and constraint violation) per time step, and the
// stand-alone scoring kernels over stored trajectories (reference src/utils.jl:397-425).
//
// Arithmetic: every sum is written with separate multiply and add (__dmul_rn / __dadd_rn: nothing fuses), in the
// order the public header states.  The observer steps and the plant step are lmpc_sim_kernels.hpp's dynamics_rows /
// correct_row, the functions predict_state_kernel / correct_state_kernel are made of; theta's blocks are its
// ThetaBlock / block_at / block_entry (form_parameter_kernel's); the in-loop cost / violation are the step functions
// below, which the stand-alone scoring kernels call in the same order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_sim_kernels.hpp"

namespace lmpc {

// device-side constants of one scenario run, all in one buffer (`c`), offsets in doubles (-1 = absent)
struct ScnConst {
    const double *c;
    int plant, meas;                 // [f_offset, F, G, Gd] rows / [h_offset, C, Dd] rows of the TRUE plant
    int cC, cQ, cR, cRr, cS;         // cost weights (row-major): C ny_c x nx, Q ny_c x ny_c, R, Rr nu x nu, S nx x nu
    int cAx, cAu, clb, cub;          // constraint rows: Ax nc x nx, Au nc x nu, lb, ub
    int nyc, nc;
};

// sum_j a_j * (sum_l M[j, l] b_l): inner sums from 0 in index order, then the outer one likewise
__device__ __forceinline__ double scn_quad(const double *__restrict__ M, const double *a, int na, const double *b, int nb) {
    double s = 0.0;
    for (int j = 0; j < na; j++) {
        double t = 0.0;
        for (int l = 0; l < nb; l++) t = __dadd_rn(t, __dmul_rn(M[j * nb + l], b[l]));
        s = __dadd_rn(s, __dmul_rn(a[j], t));
    }
    return s;
}

// one step's cost term (NOT halved) of evaluate_cost (utils.jl:403-409):  e'Qe + u'Ru + du'Rr du + x'Su with
// e = C x - r, added in that order starting from 0; absent weights add nothing.  r == nullptr: zeros.
__device__ __forceinline__ double scn_step_cost(const ScnConst &K, const double *x, int nx, const double *u, const double *ulast,
                                                int nu, const ThetaBlock &r, long long i, int k) {
    double c = 0.0;
    if (K.cC >= 0 && K.cQ >= 0) {
        double e[32];
        for (int j = 0; j < K.nyc; j++) {
            double t = 0.0;
            for (int a = 0; a < nx; a++) t = __dadd_rn(t, __dmul_rn(K.c[K.cC + j * nx + a], x[a]));
            e[j] = __dsub_rn(t, r.w > 0 ? block_at(r, i, k, j) : 0.0);
        }
        c = __dadd_rn(c, scn_quad(K.c + K.cQ, e, K.nyc, e, K.nyc));
    }
    if (K.cR >= 0) c = __dadd_rn(c, scn_quad(K.c + K.cR, u, nu, u, nu));
    if (K.cRr >= 0) {
        double du[64];
        for (int l = 0; l < nu; l++) du[l] = __dsub_rn(u[l], ulast[l]);
        c = __dadd_rn(c, scn_quad(K.c + K.cRr, du, nu, du, nu));
    }
    if (K.cS >= 0) c = __dadd_rn(c, scn_quad(K.c + K.cS, x, nx, u, nu));
    return c;
}

// one step's constraint_violation (utils.jl:417-420): max over rows of max(lb - v, v - ub, 0), v = Ax x + Au u
// (Ax terms first, from 0, index order)
__device__ __forceinline__ double scn_step_violation(const ScnConst &K, const double *x, int nx, const double *u, int nu) {
    double worst = 0.0;
    for (int j = 0; j < K.nc; j++) {
        double v = 0.0;
        if (K.cAx >= 0) for (int a = 0; a < nx; a++) v = __dadd_rn(v, __dmul_rn(K.c[K.cAx + j * nx + a], x[a]));
        if (K.cAu >= 0) for (int l = 0; l < nu; l++) v = __dadd_rn(v, __dmul_rn(K.c[K.cAu + j * nu + l], u[l]));
        const double lo = __dsub_rn(K.c[K.clb + j], v), hi = __dsub_rn(v, K.c[K.cub + j]);
        worst = lo > worst ? lo : worst;
        worst = hi > worst ? hi : worst;
    }
    return worst;
}

struct ScnPre {
    const double *x;                  // N x nx true states
    double *xhat;                     // N x nx observer states (in/out) or nullptr = no observer
    const double *uprev;              // N x nup
    double *theta;                    // N x nth (out)
    const double *obs_meas, *obs_kt;  // the handle's MPC_MEASUREMENT_FUNCTION / K_TRANSPOSE_OBSERVER
    ThetaBlock r, d, p, noise;        // r.k0 / d.k0 / p.k0: first column of this step's theta block
    double *ym_out, *y_out, *xhat_out, *d_out;   // this step's slices of the optional trajectories
    int nx, ny, nd, nup, k;
    long long n;
};

// One measurement row of the TRUE plant: ym = h_j + sum_c C_jc x_c + sum_q Dd_jq d_q (what a sensor reads, before any
// noise) and y = the same sum without the offset; `mr` = K.c + K.meas + j * (1 + nx + nd).  The callers add the noise
// terms onto ym: the descriptor's noise block first, then the uncertainty's measurement source.
struct ScnMeas { double ym, y; };
template <int NXT, class D>
__device__ __forceinline__ ScnMeas scn_measure_row(const double *mr, const double *xo, int nx, int nd, D &&dk) {
    double ym = mr[0], y = 0.0;
    for_nx<NXT>(nx, [&](int c) {
        const double t = __dmul_rn(mr[1 + c], xo[c]);
        ym = __dadd_rn(ym, t); y = __dadd_rn(y, t);
    });
    for (int q = 0; q < nd; q++) {
        const double t = __dmul_rn(mr[1 + nx + q], dk(q));
        ym = __dadd_rn(ym, t); y = __dadd_rn(y, t);
    }
    return {ym, y};
}

// Phase 2 of a PRE kernel, the workgroup together: its 256 records theta = [xhat; r-block; d-block; uprev; p-block]
// entry by entry, consecutive lanes on consecutive addresses (form_parameter_kernel's property; a record can be 60+
// doubles wide).  xhat: the first nx entries of the lane's row (ldw doubles) in LDS; dblock(s, sl, e): entry e of the
// d block, ndw wide, for scenario s = lane sl.
template <class DB>
__device__ __forceinline__ void scn_form_theta(double *theta, const double *lds, int ldw, int nx, const ThetaBlock &r, int ndw,
                                               DB &&dblock, const double *uprev, int nup, const ThetaBlock &p, long long base,
                                               long long n) {
    const int nr = r.width(), npw = p.width();
    const int nth = nx + nr + ndw + nup + npw;
    const long long left = n - base;
    const int rows = left < 256 ? (int)left : 256;
    for (int idx = threadIdx.x; idx < rows * nth; idx += 256) {
        const int sl = idx / nth;
        int e = idx - sl * nth;
        const long long s = base + sl;
        double v;
        if (e < nx) v = lds[sl * ldw + e];
        else if ((e -= nx) < nr) v = block_entry(r, s, e);
        else if ((e -= nr) < ndw) v = dblock(s, sl, e);
        else if ((e -= ndw) < nup) v = uprev[s * nup + e];
        else v = block_entry(p, s, e - nup);
        theta[base * nth + idx] = v;
    }
}

// Both phases of the PRE kernel of step k.  Phase 1, one lane per scenario: ym_j / y_j by scn_measure_row (+ v_j from the
// descriptor's noise block, then ym_j = noise(j, ym_j): what the uncertain loop adds, nothing in the plain one), y = ym
// without an observer, xhat <- correct(xhat, ym, d_k) by correct_row, measurement by measurement (else xhat = x), the
// estimate into LDS.  Phase 2: scn_form_theta.  lds: 256 * nx doubles.
template <int NXT, class V>
__device__ __forceinline__ void scn_pre_step(const ScnPre &A, const ScnConst &K, double *lds, V &&noise) {
    constexpr int NXA = NXT > 0 ? NXT : 32;
    const int nx = NXT > 0 ? NXT : A.nx;
    const long long base = (long long)blockIdx.x * 256;
    const long long i = base + threadIdx.x;
    if (i < A.n) {
        double xo[NXA], xh[NXA], xn[NXA];
        auto dk = [&](int q) { return block_at(A.d, i, A.k, q); };
        for_nx<NXT>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
        const bool obs = A.xhat != nullptr;
        if (obs) for_nx<NXT>(nx, [&](int c) { xh[c] = A.xhat[i * nx + c]; xn[c] = xh[c]; });
        else for_nx<NXT>(nx, [&](int c) { xn[c] = xo[c]; });
        const int ms = 1 + nx + A.nd;
        for (int j = 0; j < A.ny; j++) {
            const ScnMeas m = scn_measure_row<NXT>(K.c + K.meas + j * ms, xo, nx, A.nd, dk);
            double ym = m.ym;
            if (A.noise.w > 0) ym = __dadd_rn(ym, block_at(A.noise, i, A.k, j));
            ym = noise(j, ym);
            if (A.ym_out) A.ym_out[i * A.ny + j] = ym;
            if (A.y_out) A.y_out[i * A.ny + j] = obs ? m.y : ym;
            // the innovation against the OBSERVER's model, then the gain
            if (obs) correct_row<NXT>(A.obs_meas + j * ms, A.obs_kt + j * nx, ym, xh, xn, nx, A.nd, dk);
        }
        for_nx<NXT>(nx, [&](int c) {
            if (obs) A.xhat[i * nx + c] = xn[c];
            if (A.xhat_out) A.xhat_out[i * nx + c] = xn[c];
        });
        for_nx<NXT>(nx, [&](int c) { lds[threadIdx.x * nx + c] = xn[c]; });
        if (A.d_out) for (int q = 0; q < A.nd; q++) A.d_out[i * A.nd + q] = dk(q);
    }
    __syncthreads();
    scn_form_theta(A.theta, lds, nx, nx, A.r, A.d.width(), [&](long long s, int, int e) { return block_entry(A.d, s, e); },
                   A.uprev, A.nup, A.p, base, A.n);
}

// PRE kernel of step k (scn_pre_step without further noise).  Dynamic LDS: 256 * nx doubles.
template <int NXT>
__global__ __launch_bounds__(256) void scenario_pre_kernel(ScnPre A, ScnConst K) {
    extern __shared__ double scn_lds[];
    scn_pre_step<NXT>(A, K, scn_lds, [](int, double ym) { return ym; });
}

struct ScnPost {
    double *x;                        // N x nx true states (in/out)
    double *xhat;                     // N x nx observer states (in/out) or nullptr
    double *uprev;                    // N x nup (out)
    const double *u;                  // N x nu: this step's controls
    const int32_t *flag;              // N: this step's exit flags
    const double *obs_dyn;            // the handle's MPC_PLANT_DYNAMICS (observer model)
    ThetaBlock d, r;                  // d: column k acts on the plant; r: column k enters the cost
    double *xtraj_next, *utraj;       // this step's slices or nullptr
    int32_t *flag_min;
    double *cost, *viol, *ulast;      // running sums (cost NOT halved until the last step) / previous control for du
    int nx, nu, nd, nup, k, first, last;
    long long n;
};

// The score of step k for scenario i, on (x_k, u_k) BEFORE the move: the running cost (scn_step_cost added to cost[i],
// halved with the last step; ulast: the scenario's previous control for the du term, kept here) and the running worst
// constraint violation.  u: the scenario's nu controls.  COPYU: the POST kernels read u from global memory and score a
// private copy; explicit_run_kernel's u is private already.
template <bool COPYU>
__device__ __forceinline__ void scn_score_step(const ScnConst &K, const double *xo, int nx, const double *u, int nu, double *cost,
                                               double *viol, double *ulast, const ThetaBlock &r, long long i, int k, int first,
                                               int last) {
    if (cost) {
        double ul[64];
        if (K.cRr >= 0) for (int l = 0; l < nu; l++) ul[l] = first ? 0.0 : ulast[i * nu + l];
        double us[COPYU ? 64 : 1];
        const double *uu = u;
        if constexpr (COPYU) { for (int l = 0; l < nu; l++) us[l] = u[l]; uu = us; }
        const double c = scn_step_cost(K, xo, nx, uu, ul, nu, r, i, k);
        const double run = __dadd_rn(first ? 0.0 : cost[i], c);
        cost[i] = last ? __dmul_rn(0.5, run) : run;
        if (K.cRr >= 0 && !last) for (int l = 0; l < nu; l++) ulast[i * nu + l] = uu[l];
    }
    if (viol) {
        double us[COPYU ? 64 : 1];
        const double *uu = u;
        if constexpr (COPYU) { for (int l = 0; l < nu; l++) us[l] = u[l]; uu = us; }
        const double w = scn_step_violation(K, xo, nx, uu, nu);
        const double old = first ? 0.0 : viol[i];
        viol[i] = w > old ? w : old;
    }
}

// xh <- predict(xh, u, d_k) by dynamics_rows on the observer's model; xh: the scenario's record, NW / nw wide
template <int NW, class D>
__device__ __forceinline__ void scn_observer_predict(const double *obs_dyn, double *xh, int nw, int nu, int nd, const double *u, D &&dk) {
    constexpr int NWA = NW > 0 ? NW : 32;
    double ho[NWA], hn[NWA];
    for_nx<NW>(nw, [&](int c) { ho[c] = xh[c]; });
    dynamics_rows<NW>(obs_dyn, ho, hn, nw, nu, nd, u, dk);
    for_nx<NW>(nw, [&](int c) { xh[c] = hn[c]; });
}

// POST kernel of step k, one lane per scenario: scn_score_step, xhat <- predict(xhat, u, d_k) by scn_observer_predict,
// x <- f_offset + F x + G u + Gd d_k by dynamics_rows on the true plant's array, then step_tail: uprev <- u,
// trajectories, smallest exit flag.
template <int NXT, bool COST>
__global__ __launch_bounds__(256) void scenario_post_kernel(ScnPost A, ScnConst K) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    constexpr int NXA = NXT > 0 ? NXT : 32;
    const int nx = NXT > 0 ? NXT : A.nx;
    const int nu = A.nu;
    const double *u = A.u + i * nu;
    auto dk = [&](int q) { return block_at(A.d, i, A.k, q); };
    double xo[NXA], xn[NXA];
    for_nx<NXT>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
    if constexpr (COST) scn_score_step<true>(K, xo, nx, u, nu, A.cost, A.viol, A.ulast, A.r, i, A.k, A.first, A.last);
    if (A.xhat) scn_observer_predict<NXT>(A.obs_dyn, A.xhat + i * nx, nx, nu, A.nd, u, dk);
    dynamics_rows<NXT>(K.c + K.plant, xo, xn, nx, nu, A.nd, u, dk);
    for_nx<NXT>(nx, [&](int a) { A.x[i * nx + a] = xn[a]; });
    if (A.xtraj_next) for_nx<NXT>(nx, [&](int a) { A.xtraj_next[i * nx + a] = xn[a]; });
    step_tail(i, u, nu, A.uprev + i * A.nup, (double *)nullptr, A.nup, A.utraj, A.flag, A.flag_min, A.first);
}

// Stand-alone scoring of stored trajectories, one thread per scenario: X step-major (step k's states at
// X + k * n * nx, i.e. the first T slices of an X_traj), U step-major (T x n x nu).  The same step functions in the
// same order over k as the loop's POST kernel.  cost / viol: n doubles; viol_steps: T x n or nullptr.
// (`inline`: this header is part of two translation units, as lmpc_sim_kernels.hpp is.)
inline __global__ __launch_bounds__(256) void scenario_cost_kernel(ScnConst K, const double *__restrict__ X, const double *__restrict__ U,
                                                            ThetaBlock r, int nx, int nu, int T, double *__restrict__ cost, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x[32], u[64], ul[64];
    for (int l = 0; l < nu; l++) ul[l] = 0.0;
    double run = 0.0;
    for (int k = 0; k < T; k++) {
        for (int a = 0; a < nx; a++) x[a] = X[((long long)k * n + i) * nx + a];
        for (int l = 0; l < nu; l++) u[l] = U[((long long)k * n + i) * nu + l];
        run = __dadd_rn(run, scn_step_cost(K, x, nx, u, ul, nu, r, i, k));
        for (int l = 0; l < nu; l++) ul[l] = u[l];
    }
    cost[i] = __dmul_rn(0.5, run);
}

inline __global__ __launch_bounds__(256) void scenario_violation_kernel(ScnConst K, const double *__restrict__ X, const double *__restrict__ U,
                                                                 int nx, int nu, int T, double *__restrict__ viol,
                                                                 double *__restrict__ viol_steps, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x[32], u[64];
    double worst = 0.0;
    for (int k = 0; k < T; k++) {
        for (int a = 0; a < nx; a++) x[a] = X[((long long)k * n + i) * nx + a];
        for (int l = 0; l < nu; l++) u[l] = U[((long long)k * n + i) * nu + l];
        const double w = scn_step_violation(K, x, nx, u, nu);
        if (viol_steps) viol_steps[(long long)k * n + i] = w;
        worst = w > worst ? w : worst;
    }
    if (viol) viol[i] = worst;
}

}  // namespace lmpc
