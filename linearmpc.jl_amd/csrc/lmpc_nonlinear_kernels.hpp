// Kernels of the nonlinear true plant (lmpc_plant_program_eval_device, lmpc_simulate_scenario_nonlinear_device): the
// plant-program interpreter of lmpc_plant_program.hpp, one scenario per lane in 64-thread workgroups.
//
// The slot file lives in dynamic LDS laid out [slot][lane]: lane l's slot s is word s * 64 + l, so the 64 lanes of an
// access sit on 64 consecutive doubles (conflict-free) and no lane ever touches another lane's column -- the kernels
// need no barrier.  Its size is the PROGRAM's slot count (n_slots * 64 * 8 bytes), which is what sets residency, not
// the cap.  Instructions, constants and out_slot are read at lane-independent addresses.  The inputs are read from
// global memory where the program asks for them (an index into a private copy would be a runtime index: scratch).
//
// nonlinear_post_kernel is uncertain_post_kernel with dynamics_rows on the plant's rows replaced by the program: cost,
// violation, the observer's predict, the draws and step_tail are the same device functions (scn_step_cost,
// scn_step_violation, dynamics_rows on the OBSERVER's model, unc_value, step_tail), called in the same order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_plant_program.hpp"
#include "lmpc_uncertain_kernels.hpp"

namespace lmpc {

constexpr int NL_LANES = 64;

// where the kernels find the rest of the program and the plant parameters
struct NlPlant {
    const int32_t *out_slot;          // nx (device)
    const double *q;                  // N x nq (qstride = nq) or nq shared (qstride = 0); nullptr with nq == 0
    long long qstride;
};

// the device environment of one lane; D: the disturbance entry a of this scenario and step
template <class D>
struct NlEnv {
    double *col;                      // this lane's column of the slot file: slot s at col[s * NL_LANES]
    const double *xr, *ur, *qr;
    D dist;
    __device__ __forceinline__ double slot(int s) const { return col[s * NL_LANES]; }
    __device__ __forceinline__ void set(int s, double v) { col[s * NL_LANES] = v; }
    __device__ __forceinline__ double x(int a) const { return xr[a]; }
    __device__ __forceinline__ double u(int a) const { return ur[a]; }
    __device__ __forceinline__ double d(int a) const { return dist(a); }
    __device__ __forceinline__ double q(int a) const { return qr[a]; }
};

// one plant step outside any loop: xnext_i = program(x_i, u_i, d_i, q_i)
inline __global__ __launch_bounds__(NL_LANES) void plant_program_eval_kernel(PlantProg P, NlPlant Q, const double *__restrict__ x,
                                                                            const double *__restrict__ u, const double *__restrict__ d,
                                                                            double *__restrict__ xnext, long long n) {
    extern __shared__ double nl_eval_lds[];
    const long long i = (long long)blockIdx.x * NL_LANES + threadIdx.x;
    if (i >= n) return;
    const double *dr = d + i * P.nd;
    auto dist = [&](int a) { return dr[a]; };
    NlEnv<decltype(dist)> E{nl_eval_lds + threadIdx.x, x + i * P.nx, u + i * P.nu, Q.q + i * Q.qstride, dist};
    plant_program_run(P, E);
    for (int a = 0; a < P.nx; a++) xnext[i * P.nx + a] = E.slot(Q.out_slot[a]);
}

// POST kernel of step k of the nonlinear loop
template <int NXT, bool COST, bool GAUSS = false>
__global__ __launch_bounds__(NL_LANES) void nonlinear_post_kernel(ScnPost A, ScnConst K, UncStep U, PlantProg P, NlPlant Q) {
    extern __shared__ double nl_lds[];
    const long long i = (long long)blockIdx.x * NL_LANES + threadIdx.x;
    if (i >= A.n) return;
    constexpr int NXA = NXT > 0 ? NXT : 32;
    const int nx = NXT > 0 ? NXT : A.nx;
    const int nu = A.nu;
    const double *u = A.u + i * nu;
    auto dk = [&](int q) { return block_at(A.d, i, A.k, q); };
    if constexpr (COST) {
        double xo[NXA];
        for_nx<NXT>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
        if (A.cost) {
            double ul[64];
            if (K.cRr >= 0) for (int l = 0; l < nu; l++) ul[l] = A.first ? 0.0 : A.ulast[i * nu + l];
            double us[64];
            for (int l = 0; l < nu; l++) us[l] = u[l];
            const double c = scn_step_cost(K, xo, nx, us, ul, nu, A.r, i, A.k);
            const double run = __dadd_rn(A.first ? 0.0 : A.cost[i], c);
            A.cost[i] = A.last ? __dmul_rn(0.5, run) : run;
            if (K.cRr >= 0 && !A.last) for (int l = 0; l < nu; l++) A.ulast[i * nu + l] = us[l];
        }
        if (A.viol) {
            double us[64];
            for (int l = 0; l < nu; l++) us[l] = u[l];
            const double w = scn_step_violation(K, xo, nx, us, nu);
            const double old = A.first ? 0.0 : A.viol[i];
            A.viol[i] = w > old ? w : old;
        }
    }
    if (A.xhat) {                                      // the observer predicts with the handle's LINEAR model
        double ho[NXA], hn[NXA];
        for_nx<NXT>(nx, [&](int c) { ho[c] = A.xhat[i * nx + c]; });
        dynamics_rows<NXT>(A.obs_dyn, ho, hn, nx, nu, A.nd, u, dk);
        for_nx<NXT>(nx, [&](int c) { A.xhat[i * nx + c] = hn[c]; });
    }
    NlEnv<decltype(dk)> E{nl_lds + threadIdx.x, A.x + i * nx, u, Q.q + i * Q.qstride, dk};
    plant_program_run(P, E);
    double xn[NXA];
    for_nx<NXT>(nx, [&](int a) { xn[a] = E.slot(Q.out_slot[a]); });
    const int nw = U.process.w;
    if (nw > 0) {
        typename std::conditional<GAUSS, UncDrawsGauss, UncDraws>::type de(U, i, 0u);
        if (U.gw < 0) {
            for_nx<NXT>(nx, [&](int a) {
                const double e = unc_value(U.process, K.c, de, i, A.k, a);
                xn[a] = __dadd_rn(xn[a], e);
                if (U.w_out) U.w_out[i * nx + a] = e;
            });
        } else {
            const double *gw = K.c + U.gw;
            double wv[NXA];
            for_nx<NXT>(nx, [&](int a) { wv[a] = 0.0; });
            for (int q = 0; q < nw; q++) {
                const double e = unc_value(U.process, K.c, de, i, A.k, q);
                for_nx<NXT>(nx, [&](int a) {
                    const double t = __dmul_rn(gw[a * nw + q], e);
                    xn[a] = __dadd_rn(xn[a], t);
                    wv[a] = __dadd_rn(wv[a], t);
                });
            }
            if (U.w_out) for_nx<NXT>(nx, [&](int a) { U.w_out[i * nx + a] = wv[a]; });
        }
    }
    for_nx<NXT>(nx, [&](int a) { A.x[i * nx + a] = xn[a]; });
    if (A.xtraj_next) for_nx<NXT>(nx, [&](int a) { A.xtraj_next[i * nx + a] = xn[a]; });
    step_tail(i, u, nu, A.uprev + i * A.nup, (double *)nullptr, A.nup, A.utraj, A.flag, A.flag_min, A.first);
}

}  // namespace lmpc
