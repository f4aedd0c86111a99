// Run-ahead kernel of the scenario loop with an explicit controller (lmpc_explicit_simulate_scenario_device, mode 1):
// one scenario per lane, and the lane runs its scenario forward for as many steps as the table locates -- the PRE part
// of scenario_pre_kernel (measure, correct, form theta), the point location and the law of explicit_eval_kernel, the
// POST part of scenario_post_kernel (cost, violation, predict, plant step, bookkeeping) -- with no launch and no theta
// record in memory in between.  At a point the table does not hold (region -1) the lane writes theta into a dense
// batch for the handle's implicit solve, puts itself on a list and leaves; the same kernel, entered through that list
// with the batch's answers, resumes each listed scenario at the POST part of the step it stopped in.
//
// Arithmetic: the correction, dynamics, cost and violation are the device functions of lmpc_sim_kernels.hpp /
// lmpc_scenario_kernels.hpp (separate multiply and add), the controller is explicit_locate / explicit_affine of
// lmpc_explicit_kernel.hpp (explicit fmas).  The measurement sum, the score of a step and the observer's predict are the
// device functions the PRE / POST kernels are made of (scn_measure_row, scn_score_step, scn_observer_predict); theta is
// formed entry by entry into registers, in scn_form_theta's order.
//
// State: x, xhat and uprev stay in the caller's arrays between two steps (the same lane reads back what it wrote; the
// lines are its own), as the PRE / POST kernels keep them; theta lives in registers (double th[NT], static indices).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_explicit_kernel.hpp"
#include "lmpc_scenario_kernels.hpp"

namespace lmpc {

struct ExpRun {
    double *x, *xhat, *uprev;         // N x nx true states, N x nx observer states or nullptr, N x nup (all in/out)
    const double *obs_dyn, *obs_meas, *obs_kt;   // the handle's observer arrays (with xhat)
    ThetaBlock r, d, p, noise;        // k0 is set per step inside the kernel
    double *ym_traj, *y_traj, *xhat_traj, *d_traj;   // T x N x . or nullptr
    double *u_traj, *x_traj;          // T x N x nu, (T + 1) x N x nx, or nullptr
    int32_t *flag_min, *region_traj;  // N / T x N or nullptr
    double *cost, *viol, *ulast;      // running sums / previous control of the du term, or nullptr
    int32_t *step;                    // N: the step a listed scenario stopped in
    double *fb_theta;                 // dense fallback batch, theta records (out)
    int32_t *list_out, *count;        // this launch's misses: scenario indices, and how many
    const int32_t *list_in;           // resume: lane j takes scenario list_in[j]; nullptr = lane j takes scenario j from step 0
    const double *fb_u;               // resume: record j = the control of step step[i] ...
    const int32_t *fb_flag;           // ... and its exit flag
    int nx, ny, nd, nu, nup, T;
    long long lanes, N;               // lanes of this launch; scenarios of the run (a trajectory slice is N records)
};

template <int NXT, int NT>
__global__ __launch_bounds__(256) void explicit_run_kernel(ExpRun A, ScnConst K, ExplicitView v) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.lanes) return;
    constexpr int NXA = NXT > 0 ? NXT : 32;
    const int nx = NXT > 0 ? NXT : A.nx;
    const int nu = A.nu, nth = v.nth;
    const long long i = A.list_in ? A.list_in[j] : j;
    const bool obs = A.xhat != nullptr;
    double u[64];
    int flag = 0, region = -1;
    int k = 0;
    bool resumed = false;
    if (A.list_in) {
        k = A.step[i];
        for (int l = 0; l < nu; l++) u[l] = A.fb_u[j * nu + l];
        flag = A.fb_flag[j];
        resumed = true;
    }
    for (; k < A.T; k++) {
        auto dk = [&](int q) { return block_at(A.d, i, k, q); };
        if (!resumed) {
            // ---- PRE (scenario_pre_kernel, phase 1)
            double xo[NXA], xh[NXA], xn[NXA];
            for_nx<NXT>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
            if (obs) for_nx<NXT>(nx, [&](int c) { xh[c] = A.xhat[i * nx + c]; xn[c] = xh[c]; });
            else for_nx<NXT>(nx, [&](int c) { xn[c] = xo[c]; });
            const long long row = (long long)k * A.N + i;
            const int ms = 1 + nx + A.nd;
            for (int jm = 0; jm < A.ny; jm++) {
                const ScnMeas m = scn_measure_row<NXT>(K.c + K.meas + jm * ms, xo, nx, A.nd, dk);
                double ym = m.ym;
                if (A.noise.w > 0) ym = __dadd_rn(ym, block_at(A.noise, i, k, jm));
                if (A.ym_traj) A.ym_traj[row * A.ny + jm] = ym;
                if (A.y_traj) A.y_traj[row * A.ny + jm] = obs ? m.y : ym;
                if (obs) correct_row<NXT>(A.obs_meas + jm * ms, A.obs_kt + jm * nx, ym, xh, xn, nx, A.nd, dk);
            }
            for_nx<NXT>(nx, [&](int c) {
                if (obs) A.xhat[i * nx + c] = xn[c];
                if (A.xhat_traj) A.xhat_traj[row * nx + c] = xn[c];
            });
            if (A.d_traj) for (int q = 0; q < A.nd; q++) A.d_traj[row * A.nd + q] = dk(q);
            // theta = [xhat; r-block; d-block; uprev; p-block], entry by entry as phase 2 forms it
            ThetaBlock br = A.r, bd = A.d, bp = A.p;
            br.k0 = br.H > 0 ? k + 1 : k;
            bd.k0 = k; bp.k0 = k;
            const int nr = br.width(), ndw = bd.width();
            double th[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                int e = t;
                double val = 0.0;
                if (t < nth) {
                    if (e < nx) val = xn[t < NXA ? t : 0];
                    else if ((e -= nx) < nr) val = block_entry(br, i, e);
                    else if ((e -= nr) < ndw) val = block_entry(bd, i, e);
                    else if ((e -= ndw) < A.nup) val = A.uprev[i * A.nup + e];
                    else val = block_entry(bp, i, e - A.nup);
                }
                th[t] = val;
            }
            // ---- controller (explicit_eval_kernel's two calls)
            region = explicit_locate<NT>(v, th, &flag, nullptr);
            if (region < 0) {
                // not in the table: theta into the dense batch, the scenario onto the list, and out
                const int slot = atomicAdd(A.count, 1);
#pragma unroll
                for (int t = 0; t < NT; t++)
                    if (t < nth) A.fb_theta[(long long)slot * nth + t] = th[t];
                A.list_out[slot] = (int32_t)i;
                A.step[i] = k;
                return;
            }
            const double *law = v.laws + (int64_t)v.regions[8 * region + 2] * (nth + 1);
            for (int l = 0; l < nu; l++) u[l] = explicit_affine<NT>(law + (int64_t)l * (nth + 1), th, nth);
        }
        resumed = false;
        // ---- POST (scenario_post_kernel)
        const int first = k == 0, last = k == A.T - 1;
        double xo[NXA], xn[NXA];
        for_nx<NXT>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
        scn_score_step<false>(K, xo, nx, u, nu, A.cost, A.viol, A.ulast, A.r, i, k, first, last);
        if (obs) scn_observer_predict<NXT>(A.obs_dyn, A.xhat + i * nx, nx, nu, A.nd, u, dk);
        dynamics_rows<NXT>(K.c + K.plant, xo, xn, nx, nu, A.nd, u, dk);
        for_nx<NXT>(nx, [&](int a) { A.x[i * nx + a] = xn[a]; });
        if (A.x_traj) for_nx<NXT>(nx, [&](int a) { A.x_traj[((long long)(k + 1) * A.N + i) * nx + a] = xn[a]; });
        // (step_tail indexes whole arrays by the scenario: handed the scenario's own records, it is asked for record 0)
        step_tail(0LL, u, nu, A.uprev + i * A.nup, (double *)nullptr, A.nup,
                  A.u_traj ? A.u_traj + ((long long)k * A.N + i) * nu : (double *)nullptr, &flag,
                  A.flag_min ? A.flag_min + i : (int32_t *)nullptr, first);
        if (A.region_traj) A.region_traj[(long long)k * A.N + i] = region;
    }
}

}  // namespace lmpc
