// Glue kernels of the offset-free scenario loop (lmpc_simulate_scenario_offset_free_device): the scenario loop of
// lmpc_scenario_kernels.hpp with the reference's offset-free observer in it (reference src/observer.jl:13-122, 203-225,
// src/setup.jl:392-448) -- a Kalman filter on the state augmented with ndo constant disturbance channels, whose estimate
// dhat enters the controller's d block behind the measured rows, in every preview column.
//
// Two widths live side by side: the TRUE plant and the measurement act on nx states, the observer on na = nx + ndo.
// Template arguments (NX, NDO): both counts at compile time when nx + ndo <= 8 (every index into a scenario's record is
// static, for_nx's property), (0, 0) = run-time counts, na <= 32.  The sums are the ones of the scenario loop:
// scn_measure_row on the true state, correct_row and scn_observer_predict at width na on the observer's arrays,
// dynamics_rows at width nx on the plant's, scn_score_step on the true (x, u), scn_form_theta with the estimate in the
// d block, step_tail last -- called, not restated, so that the loop equals
// lmpc_correct_state_device / lmpc_predict_state_device on the same handle bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_scenario_kernels.hpp"

namespace lmpc {

// xaug_i = [x_i; 0]: set_state!(observer, x0) with no d0 (observer.jl:74-90)
inline __global__ __launch_bounds__(256) void offset_free_init_kernel(double *__restrict__ xaug, const double *__restrict__ x, int nx,
                                                                      int na, long long n) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * na) return;
    const long long i = idx / na;
    const int e = (int)(idx - i * na);
    xaug[idx] = e < nx ? x[i * nx + e] : 0.0;
}

struct OfPre {
    const double *x;                  // N x nx true states
    double *xaug;                     // N x na observer states (in/out)
    const double *uprev;              // N x nup
    double *theta;                    // N x nth (out)
    const double *obs_meas, *obs_kt;  // the handle's MPC_MEASUREMENT_FUNCTION / K_TRANSPOSE_OBSERVER (width na)
    ThetaBlock r, d, p, noise;        // d.w == 0: no measured trajectory (src is nullptr then); d.H still counts
    double *ym_out, *y_out, *xhat_out, *d_out, *dhat_out;   // this step's slices of the optional trajectories
    int nx, ndo, ny, nd, nup, k;      // nd: MEASURED disturbances
    long long n;
};

// PRE kernel of step k.  Phase 1, one lane per scenario: ym / y from the true state as in scenario_pre_kernel,
// xaug <- correct(xaug, ym, d_k) by correct_row at width na, measurement by measurement; xhat = xaug[0:nx] and
// dhat = xaug[nx:na] AFTER the correction; the whole corrected xaug into LDS.  Phase 2, the workgroup together: its
// 256 records theta = [xhat; r-block; d-block; uprev; p-block] entry by entry, consecutive lanes on consecutive
// addresses; the d-block is max(d.H, 1) columns [d column k + c (held at the last); dhat].  Dynamic LDS: 256 * na doubles.
template <int NX, int NDO>
__global__ __launch_bounds__(256) void offset_free_pre_kernel(OfPre A, ScnConst K) {
    extern __shared__ double of_lds[];
    constexpr int NA = NX > 0 ? NX + NDO : 0;
    constexpr int NXA = NX > 0 ? NX : 32, NAA = NA > 0 ? NA : 32, NDT = NX > 0 ? NDO : 0;
    const int nx = NX > 0 ? NX : A.nx;
    const int ndo = NX > 0 ? NDO : A.ndo;
    const int na = nx + ndo;
    const long long base = (long long)blockIdx.x * 256;
    const long long i = base + threadIdx.x;
    if (i < A.n) {
        double xo[NXA], xh[NAA], xn[NAA];
        auto dk = [&](int q) { return block_at(A.d, i, A.k, q); };
        for_nx<NX>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
        for_nx<NA>(na, [&](int c) { xh[c] = A.xaug[i * na + c]; xn[c] = xh[c]; });
        const int ms = 1 + nx + A.nd, os = 1 + na + A.nd;
        for (int j = 0; j < A.ny; j++) {
            const ScnMeas m = scn_measure_row<NX>(K.c + K.meas + j * ms, xo, nx, A.nd, dk);
            double ym = m.ym;
            if (A.noise.w > 0) ym = __dadd_rn(ym, block_at(A.noise, i, A.k, j));
            if (A.ym_out) A.ym_out[i * A.ny + j] = ym;
            if (A.y_out) A.y_out[i * A.ny + j] = m.y;
            correct_row<NA>(A.obs_meas + j * os, A.obs_kt + j * na, ym, xh, xn, na, A.nd, dk);
        }
        for_nx<NA>(na, [&](int c) {
            A.xaug[i * na + c] = xn[c];
            of_lds[threadIdx.x * na + c] = xn[c];
        });
        if (A.xhat_out) for_nx<NX>(nx, [&](int c) { A.xhat_out[i * nx + c] = xn[c]; });
        if (A.dhat_out) for_nx<NDT>(ndo, [&](int q) { A.dhat_out[i * ndo + q] = xn[nx + q]; });
        if (A.d_out) for (int q = 0; q < A.nd; q++) A.d_out[i * A.nd + q] = dk(q);
    }
    __syncthreads();
    // the d block: max(d.H, 1) columns [d column k + c (held at the last); dhat]
    const int dcol = A.nd + ndo;
    scn_form_theta(A.theta, of_lds, na, nx, A.r, dcol * (A.d.H > 0 ? A.d.H : 1), [&](long long s, int sl, int e) {
        const int col = e / dcol, q = e - col * dcol;
        return q < A.nd ? block_at(A.d, s, A.d.k0 + col, q) : of_lds[sl * na + nx + (q - A.nd)];
    }, A.uprev, A.nup, A.p, base, A.n);
}

struct OfPost {
    double *x;                        // N x nx true states (in/out)
    double *xaug;                     // N x na observer states (in/out)
    double *uprev;                    // N x nup (out)
    const double *u;                  // N x nu: this step's controls
    const int32_t *flag;              // N: this step's exit flags
    const double *obs_dyn;            // the handle's MPC_PLANT_DYNAMICS (the augmented model, width na)
    ThetaBlock d, r;                  // d: column k acts on the plant and the observer; r: column k enters the cost
    double *xtraj_next, *utraj;       // this step's slices or nullptr
    int32_t *flag_min;
    double *cost, *viol, *ulast;      // as ScnPost
    int nx, ndo, nu, nd, nup, k, first, last;
    long long n;
};

// POST kernel of step k, one lane per scenario: running cost / violation on the TRUE (x_k, u_k) before the move,
// xaug <- predict(xaug, u, d_k) by dynamics_rows at width na on the observer's model, x <- f_offset + F x + G u + Gd d_k
// by dynamics_rows at width nx on the true plant's array, then step_tail.
template <int NX, int NDO, bool COST>
__global__ __launch_bounds__(256) void offset_free_post_kernel(OfPost A, ScnConst K) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    constexpr int NA = NX > 0 ? NX + NDO : 0;
    constexpr int NXA = NX > 0 ? NX : 32;
    const int nx = NX > 0 ? NX : A.nx;
    const int na = nx + (NX > 0 ? NDO : A.ndo);
    const int nu = A.nu;
    const double *u = A.u + i * nu;
    auto dk = [&](int q) { return block_at(A.d, i, A.k, q); };
    double xo[NXA], xn[NXA];
    for_nx<NX>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
    if constexpr (COST) scn_score_step<true>(K, xo, nx, u, nu, A.cost, A.viol, A.ulast, A.r, i, A.k, A.first, A.last);
    scn_observer_predict<NA>(A.obs_dyn, A.xaug + i * na, na, nu, A.nd, u, dk);
    dynamics_rows<NX>(K.c + K.plant, xo, xn, nx, nu, A.nd, u, dk);
    for_nx<NX>(nx, [&](int a) { A.x[i * nx + a] = xn[a]; });
    if (A.xtraj_next) for_nx<NX>(nx, [&](int a) { A.xtraj_next[i * nx + a] = xn[a]; });
    step_tail(i, u, nu, A.uprev + i * A.nup, (double *)nullptr, A.nup, A.utraj, A.flag, A.flag_min, A.first);
}

}  // namespace lmpc
