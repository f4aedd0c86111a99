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
    const HandleObserver ob(h);
    std::string msg = explicit_scenario_problem(h->P.nth, h->P.nout, ob.ptr, s, mode);
    if (!msg.empty()) return msg;
    if (N < 0 || N > 0x7fffffffLL) return "N: outside [0, 2^31 - 1]";
    msg = call_size_problem(N, T, x);
    if (msg.empty()) msg = call_array_problem(N, s, xhat, uprev, device);
    return msg;
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

// the run itself, on device arrays, once the call has passed its refusals and the handle's device is current
int run(lmpc_explicit *e, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat, double *uprev, double *U_traj,
        double *X_traj, int32_t *flag_min, int32_t *region_traj, int mode, int64_t *stats, void *stream) {
    lmpc_handle *h = e->h;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nx = s->nx, nu = s->nu, nth = e->nth;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, s->nd, s->ny, s->plant, s->measurement, s->cost);
    if (upload_constants(h, hostC, K, st) != LMPC_OK) return efail(e, LMPC_ERR_HIP, lmpc_last_error(h));
    // scratch of the run: the dense fallback batch, the first list and the count word (shared with
    // lmpc_explicit_eval_device, which mode 1 never calls), the step counters and the second list, [xhat | ulast] when the caller keeps none
    { const int rc = explicit_reserve(e, N); if (rc != LMPC_OK) return rc; }
    const auto atLeast1 = [](size_t count) { return count ? count : (size_t)1; };
    EXP_TRY(e, reserve_group(e->simCap, N, sized(e->simStep, atLeast1((size_t)N)), sized(e->simList2, atLeast1((size_t)N))));
    if (mode == 0)
        EXP_TRY(e, reserve_group(e->simLockCap, N, sized(e->simTheta, atLeast1((size_t)N * nth)),
                                 sized(e->simU, atLeast1((size_t)N * nu)), sized(e->simFlag, atLeast1((size_t)N))));
    ScnPre P; ScnPost B;
    { const int rc = scn_begin(h, e->simScr, N, s, x, xhat, uprev, X_traj, flag_min, e->simTheta, e->simU, e->simFlag, st, P, B);
      if (rc != LMPC_OK) return efail(e, rc, lmpc_last_error(h)); }
    const bool wantCost = scn_want_cost(s);
    const int64_t *head = reinterpret_cast<const int64_t *>(e->blob.data());
    const ExplicitView v = explicit_view(e->dBlob, head, e->primal_tol, e->band, e->rho_soft);
    int64_t rounds = 0, fb_steps = 0, largest = 0;

    if (mode == 1) {
        ExpRun A{};                                    // the PRE and POST records' fields in one
        A.x = x; A.xhat = P.xhat; A.uprev = uprev;
        A.obs_dyn = B.obs_dyn; A.obs_meas = P.obs_meas; A.obs_kt = P.obs_kt;
        A.r = P.r; A.d = P.d; A.p = P.p; A.noise = P.noise;
        A.ym_traj = s->Ym_traj; A.y_traj = s->Y_traj; A.xhat_traj = s->Xhat_traj; A.d_traj = s->D_traj;
        A.u_traj = U_traj; A.x_traj = X_traj; A.flag_min = flag_min; A.region_traj = region_traj;
        A.cost = B.cost; A.viol = B.viol; A.ulast = B.ulast;
        A.step = e->simStep; A.fb_theta = e->dTheta; A.count = e->dCount;
        A.fb_u = e->dX; A.fb_flag = e->dFlag;
        A.nx = nx; A.ny = s->ny; A.nd = s->nd; A.nu = nu; A.nup = s->nuprev; A.T = T; A.N = (long long)N;
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
        const unsigned grid = (unsigned)((N + kBlock - 1) / kBlock);
        bool evalFailed = false;                       // lmpc_explicit_eval_device has put its own text into e
        const int rc = scn_loop(h, s, N, T, U_traj, X_traj, P, B,
            [&](int) {
                dispatch_nx(nx, [&](auto NX) {
                    hipLaunchKernelGGL(scenario_pre_kernel<decltype(NX)::value>, dim3(grid), dim3(kBlock),
                                       sizeof(double) * kBlock * (size_t)nx, st, P, K);
                });
            },
            [&](int k) {
                const int rce = lmpc_explicit_eval_device(e, N, e->simTheta, e->simU, e->simFlag,
                                                          region_traj ? region_traj + (size_t)k * N : nullptr, stream);
                evalFailed = rce != LMPC_OK;
                const int64_t cnt = *e->hCount;        // what that call's synchronisation read
                fb_steps += cnt;
                largest = std::max(largest, cnt);
                rounds++;
                return rce;
            },
            [&](int) {
                dispatch_nx(nx, [&](auto NX) {
                    if (wantCost) hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, true>), dim3(grid), dim3(kBlock), 0, st, B, K);
                    else hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, false>), dim3(grid), dim3(kBlock), 0, st, B, K);
                });
            });
        if (rc != LMPC_OK) return evalFailed ? rc : efail(e, rc, lmpc_last_error(h));
    }
    if (stats) {
        stats[0] = rounds; stats[1] = fb_steps; stats[2] = N * (int64_t)T - fb_steps; stats[3] = largest;
    }
    return LMPC_OK;
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
    const std::string msg = call_problem(e, N, T, s, x, xhat, uprev, mode, true);
    if (!msg.empty()) return efail(e, LMPC_ERR_BADARG, "lmpc_explicit_simulate_scenario_device: " + msg);
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (N == 0 || T == 0) return LMPC_OK;
    lmpc_handle *h = e->h;
    { const int rcd = need_device(h); if (rcd != LMPC_OK) return efail(e, rcd, lmpc_last_error(h)); }
    DeviceScope scope;
    EXP_TRY(e, scope.enter(e->device));
    return run(e, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min, region_traj, mode, stats, stream);
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
    const int rc = run(e, N, T, &g.d, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, dreg, mode, stats, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) {
        (void)sg.fail(h);
        return efail(e, LMPC_ERR_HIP, lmpc_last_error(h));
    }
    if (rc == LMPC_OK && lmpc_check(h) != LMPC_OK)
        return efail(e, LMPC_ERR_HIP, std::string("lmpc_explicit_simulate_scenario: ") + lmpc_last_error(h));
    return rc;
}

}  // extern "C"
