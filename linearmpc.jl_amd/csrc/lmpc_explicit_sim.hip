// C ABI of liblmpc_hip.so, the scenario loop with an explicit controller (include/lmpc_hip.h, "Scenario loop with an
// explicit controller"): the refusals, the run-ahead form (mode 1: explicit_run_kernel over all scenarios, then rounds
// of the handle's implicit solve on the unlocated points and the same kernel resumed through the list) and the
// lock-step form (mode 0: scenario_pre_kernel, lmpc_explicit_eval_device, scenario_post_kernel per step).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "lmpc_explicit.hpp"
#include "lmpc_explicit_sim_kernel.hpp"
#include "lmpc_internal.hpp"
#include "lmpc_scenario_host.hpp"

using namespace lmpc;

namespace {

constexpr int kBlock = 256;

// everything lmpc_scenario_check refuses, and what an explicit controller adds
std::string explicit_scenario_problem(int nth, int nout, const lmpc_observer *obs, const lmpc_scenario_sim *s, int mode) {
    std::string msg = scenario_problem(nth, nout, obs, s);
    if (!msg.empty()) return msg;
    if (s->warm != 0) return "warm: an explicit law has no warm start (the fallback solves are cold)";
    if (nth > LMPC_EXPLICIT_MAX_NTH)
        return "nth: at most " + std::to_string(LMPC_EXPLICIT_MAX_NTH) + " with an explicit controller, got " + std::to_string(nth);
    if (mode != 0 && mode != 1) return "mode: 0 (lock-step) or 1 (run-ahead), got " + std::to_string(mode);
    return "";
}

std::string call_problem(lmpc_explicit *e, int64_t N, int T, const lmpc_scenario_sim *s, const double *x, const double *xhat,
                         const double *uprev, int mode, bool device) {
    if (!e->h || !e->dBlob) return "e: built without a handle (lmpc_explicit_build_ldp)";
    lmpc_handle *h = e->h;
    lmpc_observer od{h->obsNx, h->obsNu, h->obsNd, h->obsNy, nullptr, nullptr, nullptr};
    std::string msg = explicit_scenario_problem(h->P.nth, h->P.nout, h->obsC ? &od : nullptr, s, mode);
    if (!msg.empty()) return msg;
    if (N < 0 || N > 0x7fffffffLL) return "N: outside [0, 2^31 - 1]";
    if (T < 0) return "T: negative";
    if (N > 0 && !x) return "x: NULL";
    if (device && N > 0 && s->nuprev > 0 && !uprev) return "uprev: NULL with nuprev > 0";
    if (xhat && !s->use_observer) return "xhat: given without use_observer";
    return "";
}

template <class T>
int grow(lmpc_explicit *e, T **p, size_t count) {
    (void)hipFree(*p); *p = nullptr;
    EXP_TRY(e, hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * (count ? count : 1)));
    return LMPC_OK;
}

// NT = 8 serves nth <= 8 with fewer than 8 states (a record of 8 states and nothing else takes NT = 16: the same
// numbers, as the entries past nth are never read), so every instantiation that is built can be reached
template <int NXT>
void launch_run_nt(int nth, const ExpRun &A, const ScnConst &K, const ExplicitView &v, hipStream_t st) {
    const unsigned grid = (unsigned)((A.lanes + kBlock - 1) / kBlock);
    if constexpr (NXT >= 1 && NXT <= 7) {
        if (nth <= 8) {
            hipLaunchKernelGGL((explicit_run_kernel<NXT, 8>), dim3(grid), dim3(kBlock), 0, st, A, K, v);
            return;
        }
    }
    if (nth <= 16) hipLaunchKernelGGL((explicit_run_kernel<NXT, 16>), dim3(grid), dim3(kBlock), 0, st, A, K, v);
    else hipLaunchKernelGGL((explicit_run_kernel<NXT, 32>), dim3(grid), dim3(kBlock), 0, st, A, K, v);
}

void launch_run(const ExpRun &A, const ScnConst &K, const ExplicitView &v, hipStream_t st) {
    dispatch_nx(A.nx, [&](auto NX) { launch_run_nt<decltype(NX)::value>(v.nth, A, K, v, st); });
}

}  // namespace

extern "C" {

int lmpc_explicit_scenario_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s, int mode) {
    const std::string msg = explicit_scenario_problem(nth, nout, observer, s, mode);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_explicit_scenario_check: " + msg);
    return LMPC_OK;
}

int lmpc_explicit_simulate_scenario_device(lmpc_explicit *e, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                           double *uprev, double *U_traj, double *X_traj, int32_t *flag_min,
                                           int32_t *region_traj, int mode, int64_t *stats, void *stream) {
    if (!e) return LMPC_ERR_BADARG;
    {
        const std::string msg = call_problem(e, N, T, s, x, xhat, uprev, mode, true);
        if (!msg.empty()) return efail(e, LMPC_ERR_BADARG, "lmpc_explicit_simulate_scenario_device: " + msg);
    }
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (N == 0 || T == 0) return LMPC_OK;
    lmpc_handle *h = e->h;
    { const int rcd = need_device(h); if (rcd != LMPC_OK) return efail(e, rcd, lmpc_last_error(h)); }
    DeviceScope scope;
    EXP_TRY(e, scope.enter(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nx = s->nx, nu = s->nu, nd = s->nd, ny = s->ny, nup = s->nuprev, nth = e->nth;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, nd, ny, s->plant, s->measurement, s->cost);
    if (upload_constants(h, hostC, K, st) != LMPC_OK) return efail(e, LMPC_ERR_HIP, lmpc_last_error(h));
    const bool obs = s->use_observer != 0;
    const bool wantCost = s->cost && (s->cost_out || s->violation_out);
    const bool needUlast = wantCost && s->cost_out && s->cost->Rr;
    // scratch of the run: the dense fallback batch, the first list and the count word (shared with
    // lmpc_explicit_eval_device, which mode 1 never calls), the step counters and the second list, [xhat | ulast] when the caller keeps none
    { const int rc = explicit_reserve(e, N); if (rc != LMPC_OK) return rc; }
    if (N > e->simCap) {
        e->simCap = 0;
        int rc = grow(e, &e->simStep, (size_t)N);
        if (rc == LMPC_OK) rc = grow(e, &e->simList2, (size_t)N);
        if (rc != LMPC_OK) return rc;
        e->simCap = N;
    }
    if (mode == 0 && N > e->simLockCap) {
        e->simLockCap = 0;
        int rc = grow(e, &e->simTheta, (size_t)N * nth);
        if (rc == LMPC_OK) rc = grow(e, &e->simU, (size_t)N * nu);
        if (rc == LMPC_OK) rc = grow(e, &e->simFlag, (size_t)N);
        if (rc != LMPC_OK) return rc;
        e->simLockCap = N;
    }
    const size_t needScr = (size_t)N * ((obs && !xhat ? (size_t)nx : 0) + (needUlast ? (size_t)nu : 0));
    if (needScr > e->simScrCap) {
        e->simScrCap = 0;
        const int rc = grow(e, &e->simScr, needScr);
        if (rc != LMPC_OK) return rc;
        e->simScrCap = needScr;
    }
    double *scr = e->simScr;
    if (obs && !xhat) {                                // set_state!(mpc, x0), simulation.jl:92
        xhat = scr; scr += (size_t)N * nx;
        EXP_TRY(e, hipMemcpyAsync(xhat, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    }
    double *ulast = needUlast ? scr : nullptr;
    if (X_traj) EXP_TRY(e, hipMemcpyAsync(X_traj, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    const size_t obs_nd = (size_t)h->obsNx * (1 + h->obsNx + h->obsNu + h->obsNd);
    const size_t obs_nm = (size_t)h->obsNy * (1 + h->obsNx + h->obsNd);
    const int64_t *head = reinterpret_cast<const int64_t *>(e->blob.data());
    const ExplicitView v = explicit_view(e->dBlob, head, e->primal_tol, e->band, e->rho_soft);
    int64_t rounds = 0, fb_steps = 0, largest = 0;

    if (mode == 1) {
        ExpRun A{};
        A.x = x; A.xhat = obs ? xhat : nullptr; A.uprev = uprev;
        A.obs_dyn = obs ? h->obsC : nullptr;
        A.obs_meas = obs ? h->obsC + obs_nd : nullptr; A.obs_kt = obs ? h->obsC + obs_nd + obs_nm : nullptr;
        A.r = to_block(&s->r); A.d = to_block(&s->d); A.p = to_block(&s->p); A.noise = to_block(&s->noise);
        A.ym_traj = s->Ym_traj; A.y_traj = s->Y_traj; A.xhat_traj = s->Xhat_traj; A.d_traj = s->D_traj;
        A.u_traj = U_traj; A.x_traj = X_traj; A.flag_min = flag_min; A.region_traj = region_traj;
        A.cost = wantCost ? s->cost_out : nullptr; A.viol = wantCost ? s->violation_out : nullptr; A.ulast = ulast;
        A.step = e->simStep; A.fb_theta = e->dTheta; A.count = e->dCount;
        A.fb_u = e->dX; A.fb_flag = e->dFlag;
        A.nx = nx; A.ny = ny; A.nd = nd; A.nu = nu; A.nup = nup; A.T = T; A.N = (long long)N;
        int32_t *lists[2] = {e->dList, e->simList2};
        A.list_in = nullptr; A.list_out = lists[0]; A.lanes = (long long)N;
        int64_t lanes = N;
        for (;;) {
            // a listed scenario advances at least one step per round: T + 1 launches at the most
            if (rounds > T) return efail(e, LMPC_ERR_HIP, "lmpc_explicit_simulate_scenario_device: more rounds than steps");
            EXP_TRY(e, hipMemsetAsync(e->dCount, 0, sizeof(int32_t), st));
            launch_run(A, K, v, st);
            EXP_TRY(e, hipGetLastError());
            rounds++;
            // the round's one synchronisation: how many scenarios wait for the implicit solve
            EXP_TRY(e, hipMemcpyAsync(e->hCount, e->dCount, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            EXP_TRY(e, hipStreamSynchronize(st));
            const int64_t cnt = *e->hCount;
            if (cnt < 0 || cnt > lanes)
                return efail(e, LMPC_ERR_HIP, "lmpc_explicit_simulate_scenario_device: unlocated count out of range");
            if (cnt == 0) break;
            fb_steps += cnt;
            largest = std::max(largest, cnt);
            const int rc = lmpc_solve_batch_device(h, cnt, e->dTheta, e->dX, e->dFlag, nullptr, nullptr, nullptr, stream);
            if (rc != LMPC_OK)
                return efail(e, rc, std::string("lmpc_explicit_simulate_scenario_device: implicit solve: ") + lmpc_last_error(h));
            A.list_in = A.list_out;
            A.list_out = A.list_in == lists[0] ? lists[1] : lists[0];
            A.lanes = lanes = cnt;
        }
    } else {
        ScnPre P{};
        P.x = x; P.xhat = obs ? xhat : nullptr; P.uprev = uprev; P.theta = e->simTheta;
        P.obs_meas = obs ? h->obsC + obs_nd : nullptr; P.obs_kt = obs ? h->obsC + obs_nd + obs_nm : nullptr;
        P.r = to_block(&s->r); P.d = to_block(&s->d); P.p = to_block(&s->p); P.noise = to_block(&s->noise);
        P.nx = nx; P.ny = ny; P.nd = nd; P.nup = nup; P.n = (long long)N;
        ScnPost B{};
        B.x = x; B.xhat = obs ? xhat : nullptr; B.uprev = uprev; B.u = e->simU; B.flag = e->simFlag;
        B.obs_dyn = obs ? h->obsC : nullptr; B.d = P.d; B.r = P.r;
        B.flag_min = flag_min; B.cost = wantCost ? s->cost_out : nullptr; B.viol = wantCost ? s->violation_out : nullptr;
        B.ulast = ulast; B.nx = nx; B.nu = nu; B.nd = nd; B.nup = nup; B.n = (long long)N;
        const unsigned grid = (unsigned)((N + kBlock - 1) / kBlock);
        for (int k = 0; k < T; k++) {
            P.k = k;
            P.r.k0 = P.r.H > 0 ? k + 1 : k;
            P.d.k0 = k; P.p.k0 = k;
            P.ym_out = s->Ym_traj ? s->Ym_traj + (size_t)k * N * ny : nullptr;
            P.y_out = s->Y_traj ? s->Y_traj + (size_t)k * N * ny : nullptr;
            P.xhat_out = s->Xhat_traj ? s->Xhat_traj + (size_t)k * N * nx : nullptr;
            P.d_out = s->D_traj ? s->D_traj + (size_t)k * N * nd : nullptr;
            dispatch_nx(nx, [&](auto NX) {
                hipLaunchKernelGGL(scenario_pre_kernel<decltype(NX)::value>, dim3(grid), dim3(kBlock),
                                   sizeof(double) * kBlock * (size_t)nx, st, P, K);
            });
            EXP_TRY(e, hipGetLastError());
            const int rc = lmpc_explicit_eval_device(e, N, e->simTheta, e->simU, e->simFlag,
                                                     region_traj ? region_traj + (size_t)k * N : nullptr, stream);
            if (rc != LMPC_OK) return rc;
            const int64_t cnt = *e->hCount;            // what that call's synchronisation read
            fb_steps += cnt;
            largest = std::max(largest, cnt);
            rounds++;
            B.k = k; B.first = k == 0; B.last = k == T - 1;
            B.xtraj_next = X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr;
            B.utraj = U_traj ? U_traj + (size_t)k * N * nu : nullptr;
            dispatch_nx(nx, [&](auto NX) {
                if (wantCost) hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, true>), dim3(grid), dim3(kBlock), 0, st, B, K);
                else hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, false>), dim3(grid), dim3(kBlock), 0, st, B, K);
            });
            EXP_TRY(e, hipGetLastError());
        }
    }
    if (stats) {
        stats[0] = rounds; stats[1] = fb_steps; stats[2] = N * (int64_t)T - fb_steps; stats[3] = largest;
    }
    return LMPC_OK;
}

int lmpc_explicit_simulate_scenario(lmpc_explicit *e, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                    double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, int32_t *region_traj,
                                    int mode, int64_t *stats) {
    if (!e) return LMPC_ERR_BADARG;
    {   // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
        const std::string msg = call_problem(e, N, T, s, x, xhat, uprev, mode, false);
        if (!msg.empty()) return efail(e, LMPC_ERR_BADARG, "lmpc_explicit_simulate_scenario: " + msg);
    }
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (N == 0 || T == 0) return LMPC_OK;
    lmpc_handle *h = e->h;
    { const int rcd = need_device(h); if (rcd != LMPC_OK) return efail(e, rcd, lmpc_last_error(h)); }
    DeviceScope scope;
    EXP_TRY(e, scope.enter(e->device));
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    int32_t *dreg = (int32_t *)sg.out(region_traj, sizeof(int32_t) * (size_t)T * (size_t)N);
    if (sg.err != hipSuccess) { (void)sg.fail(h); return efail(e, LMPC_ERR_HIP, lmpc_last_error(h)); }
    const int rc = lmpc_explicit_simulate_scenario_device(e, N, T, &g.d, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, dreg, mode, stats,
                                                          nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) {
        (void)sg.fail(h);
        return efail(e, LMPC_ERR_HIP, lmpc_last_error(h));
    }
    if (rc == LMPC_OK && lmpc_check(h) != LMPC_OK)
        return efail(e, LMPC_ERR_HIP, std::string("lmpc_explicit_simulate_scenario: ") + lmpc_last_error(h));
    return rc;
}

}  // extern "C"
