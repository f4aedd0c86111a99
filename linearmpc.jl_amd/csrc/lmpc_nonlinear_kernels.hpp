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
// violation, the observer's predict, the process noise and step_tail are the same device functions (scn_score_step,
// scn_observer_predict on the OBSERVER's model, unc_process_noise, step_tail), called in the same order.
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
        scn_score_step<true>(K, xo, nx, u, nu, A.cost, A.viol, A.ulast, A.r, i, A.k, A.first, A.last);
    }
    // the observer predicts with the handle's LINEAR model
    if (A.xhat) scn_observer_predict<NXT>(A.obs_dyn, A.xhat + i * nx, nx, nu, A.nd, u, dk);
    NlEnv<decltype(dk)> E{nl_lds + threadIdx.x, A.x + i * nx, u, Q.q + i * Q.qstride, dk};
    plant_program_run(P, E);
    double xn[NXA];
    for_nx<NXT>(nx, [&](int a) { xn[a] = E.slot(Q.out_slot[a]); });
    unc_process_noise<NXT, typename std::conditional<GAUSS, UncDrawsGauss, UncDraws>::type>(U, K.c, i, A.k, nx, xn);
    for_nx<NXT>(nx, [&](int a) { A.x[i * nx + a] = xn[a]; });
    if (A.xtraj_next) for_nx<NXT>(nx, [&](int a) { A.xtraj_next[i * nx + a] = xn[a]; });
    step_tail(i, u, nu, A.uprev + i * A.nup, (double *)nullptr, A.nup, A.utraj, A.flag, A.flag_min, A.first);
}

}  // namespace lmpc
