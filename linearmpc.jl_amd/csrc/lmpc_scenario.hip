// C ABI of liblmpc_hip.so, the scenario loop: closed-loop simulation of N scenarios with disturbance, affine
// parameters, plant / measurement offsets and the generated state observer (lmpc_simulate_scenario*), and the
// scoring of a run (lmpc_evaluate_cost_device, lmpc_constraint_violation_device).  Lock-step like
// lmpc_simulate_ref_device: per step a PRE kernel, the handle's solve (api_launch), a POST kernel
// (lmpc_scenario_kernels.hpp); nothing but enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_scenario_host.hpp"
#include "lmpc_scenario_kernels.hpp"

using namespace lmpc;

namespace lmpc {
void scenario_preload() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, (const void *)scenario_pre_kernel<0>);
    (void)hipGetLastError();
    offset_free_preload();                             // ... and the offset-free loop's unit
}
}  // namespace lmpc

extern "C" {

int lmpc_scenario_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s) {
    const std::string msg = scenario_problem(nth, nout, observer, s);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_scenario_check: " + msg);
    return LMPC_OK;
}

int lmpc_simulate_scenario_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                  double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    lmpc_observer od{h->obsNx, h->obsNu, h->obsNd, h->obsNy, nullptr, nullptr, nullptr};
    std::string msg = scenario_problem(h->P.nth, h->P.nout, h->obsC ? &od : nullptr, s);
    if (msg.empty()) {
        if (N < 0) msg = "N: negative";
        else if (T < 0) msg = "T: negative";
        else if (N > 0 && !x) msg = "x: NULL";
        else if (N > 0 && s->nuprev > 0 && !uprev) msg = "uprev: NULL with nuprev > 0";
        else if (xhat && !s->use_observer) msg = "xhat: given without use_observer";
    }
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_device: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    const int nx = s->nx, nu = s->nu, nd = s->nd, ny = s->ny, nup = s->nuprev;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, nd, ny, s->plant, s->measurement, s->cost);
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    const bool obs = s->use_observer != 0;
    const bool wantCost = s->cost && (s->cost_out || s->violation_out);
    const bool needUlast = wantCost && s->cost_out && s->cost->Rr;
    // per-run scratch: the observer state when the caller keeps none, the previous control of the cost's du term
    const size_t needScr = (size_t)N * ((obs && !xhat ? (size_t)nx : 0) + (needUlast ? (size_t)nu : 0));
    if (needScr > h->scnScrCap) {
        hipFree(h->scnScr); h->scnScr = nullptr; h->scnScrCap = 0;
        HIP_TRY(h, hipMalloc(&h->scnScr, sizeof(double) * needScr));
        h->scnScrCap = needScr;
    }
    double *scr = h->scnScr;
    if (obs && !xhat) {                                // set_state!(mpc, x0), simulation.jl:92
        xhat = scr; scr += (size_t)N * nx;
        HIP_TRY(h, hipMemcpyAsync(xhat, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    }
    double *ulast = needUlast ? scr : nullptr;
    if (X_traj) HIP_TRY(h, hipMemcpyAsync(X_traj, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    const size_t obs_nd = (size_t)h->obsNx * (1 + h->obsNx + h->obsNu + h->obsNd);
    const size_t obs_nm = (size_t)h->obsNy * (1 + h->obsNx + h->obsNd);
    ScnPre A{};
    A.x = x; A.xhat = obs ? xhat : nullptr; A.uprev = uprev; A.theta = h->simTheta;
    A.obs_meas = obs ? h->obsC + obs_nd : nullptr; A.obs_kt = obs ? h->obsC + obs_nd + obs_nm : nullptr;
    A.r = to_block(&s->r); A.d = to_block(&s->d); A.p = to_block(&s->p); A.noise = to_block(&s->noise);
    A.nx = nx; A.ny = ny; A.nd = nd; A.nup = nup; A.n = (long long)N;
    ScnPost B{};
    B.x = x; B.xhat = obs ? xhat : nullptr; B.uprev = uprev; B.u = h->simU; B.flag = h->simFlag;
    B.obs_dyn = obs ? h->obsC : nullptr; B.d = A.d; B.r = A.r;
    B.flag_min = flag_min; B.cost = wantCost ? s->cost_out : nullptr; B.viol = wantCost ? s->violation_out : nullptr;
    B.ulast = ulast; B.nx = nx; B.nu = nu; B.nd = nd; B.nup = nup; B.n = (long long)N;
    const unsigned grid = (unsigned)((N + 255) / 256);
    for (int k = 0; k < T; k++) {
        A.k = k;
        A.r.k0 = A.r.H > 0 ? k + 1 : k;               // simulation.jl:102 get_preview(rs, k, Np) / rs[:, k]
        A.d.k0 = k; A.p.k0 = k;                       // :103-104 get_preview(ds, k - 1, Np) / ds[:, k]
        A.ym_out = s->Ym_traj ? s->Ym_traj + (size_t)k * N * ny : nullptr;
        A.y_out = s->Y_traj ? s->Y_traj + (size_t)k * N * ny : nullptr;
        A.xhat_out = s->Xhat_traj ? s->Xhat_traj + (size_t)k * N * nx : nullptr;
        A.d_out = s->D_traj ? s->D_traj + (size_t)k * N * nd : nullptr;
        dispatch_nx(nx, [&](auto NX) {
            hipLaunchKernelGGL(scenario_pre_kernel<decltype(NX)::value>, dim3(grid), dim3(256), sizeof(double) * 256 * (size_t)nx, st, A, K);
        });
        HIP_TRY(h, hipGetLastError());
        // warm start = the previous step's final working set, the first step cold (as lmpc_simulate_ref_device)
        const uint64_t *wm = (s->warm && k > 0) ? h->simAct : nullptr;
        const int rc = api_launch(h, N, h->simTheta, h->simU, h->simFlag, nullptr, s->warm ? h->simAct : nullptr, wm, st);
        if (rc != LMPC_OK) return rc;
        B.k = k; B.first = k == 0; B.last = k == T - 1;
        B.xtraj_next = X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr;
        B.utraj = U_traj ? U_traj + (size_t)k * N * nu : nullptr;
        dispatch_nx(nx, [&](auto NX) {
            if (wantCost) hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, true>), dim3(grid), dim3(256), 0, st, B, K);
            else hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, false>), dim3(grid), dim3(256), 0, st, B, K);
        });
        HIP_TRY(h, hipGetLastError());
    }
    return LMPC_OK;
}

int lmpc_simulate_scenario(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                           double *uprev, double *U_traj, double *X_traj, int32_t *flag_min) {
    if (!h) return LMPC_ERR_BADARG;
    {   // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
        lmpc_observer od{h->obsNx, h->obsNu, h->obsNd, h->obsNy, nullptr, nullptr, nullptr};
        std::string msg = scenario_problem(h->P.nth, h->P.nout, h->obsC ? &od : nullptr, s);
        if (msg.empty()) {
            if (N < 0) msg = "N: negative";
            else if (T < 0) msg = "T: negative";
            else if (N > 0 && !x) msg = "x: NULL";
            else if (xhat && !s->use_observer) msg = "xhat: given without use_observer";
        }
        if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario: " + msg);
    }
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = lmpc_simulate_scenario_device(h, N, T, &g.d, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

int lmpc_evaluate_cost_device(lmpc_handle *h, int64_t N, int T, int nx, int nu, const lmpc_sim_cost *cost, const double *X,
                              const double *U, const lmpc_block *r, double *cost_out, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    std::string msg;
    if (N < 0) msg = "N: negative";
    else if (T < 0) msg = "T: negative";
    else if (nx < 1 || nx > 32) msg = "nx: 1 <= nx <= 32";
    else if (nu < 0 || nu > 64) msg = "nu: 0 <= nu <= 64";
    else if (!cost) msg = "cost: NULL";
    else if (cost->ny < 0 || cost->ny > 32) msg = "cost.ny: 0 <= ny <= 32";
    else if (cost->Q && (!cost->C || cost->ny == 0)) msg = "cost.C: Q given without C (ny rows)";
    else if (r && r->src && cost->C && r->w != cost->ny) msg = "r.w: must equal cost.ny";
    else if (r && r->src && (r->T < 1 || r->stride < 0)) msg = "r.T: no columns, or negative stride";
    else if (N > 0 && T > 0 && (!X || !U || !cost_out)) msg = "X / U / cost_out: NULL";
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_evaluate_cost_device: " + msg);
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> hostC;
    lmpc_sim_cost c = *cost;
    c.nc = 0; c.Ax = c.Au = c.lb = c.ub = nullptr;
    ScnConst K = pack_constants(hostC, nx, nu, 0, 0, nullptr, nullptr, &c);
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    const ThetaBlock br = to_block(r && r->src && cost->C ? r : nullptr);
    hipLaunchKernelGGL(scenario_cost_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, K, X, U, br, nx, nu, T,
                       cost_out, (long long)N);
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}

int lmpc_constraint_violation_device(lmpc_handle *h, int64_t N, int T, int nx, int nu, const lmpc_sim_cost *rows, const double *X,
                                     const double *U, double *violation_out, double *violation_steps, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    std::string msg;
    if (N < 0) msg = "N: negative";
    else if (T < 0) msg = "T: negative";
    else if (nx < 1 || nx > 32) msg = "nx: 1 <= nx <= 32";
    else if (nu < 0 || nu > 64) msg = "nu: 0 <= nu <= 64";
    else if (!rows) msg = "rows: NULL";
    else if (rows->nc < 0) msg = "rows.nc: negative row count";
    else if (rows->nc > 0 && (!rows->lb || !rows->ub)) msg = "rows.lb: lb and ub are required with nc > 0";
    else if (N > 0 && T > 0 && (!X || !U || (!violation_out && !violation_steps))) msg = "X / U / violation_out: NULL";
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_constraint_violation_device: " + msg);
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> hostC;
    lmpc_sim_cost c = *rows;
    c.C = c.Q = c.R = c.Rr = c.S = nullptr;
    ScnConst K = pack_constants(hostC, nx, nu, 0, 0, nullptr, nullptr, &c);
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    hipLaunchKernelGGL(scenario_violation_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, K, X, U, nx, nu, T,
                       violation_out, violation_steps, (long long)N);
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}

}  // extern "C"
