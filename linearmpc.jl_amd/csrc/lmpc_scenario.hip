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

namespace {

std::string call_problem(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const double *x, const double *xhat,
                         const double *uprev, bool device) {
    const HandleObserver ob(h);
    std::string msg = scenario_problem(h->P.nth, h->P.nout, ob.ptr, s);
    if (msg.empty()) msg = call_size_problem(N, T, x);
    if (msg.empty()) msg = call_array_problem(N, s, xhat, uprev, device);
    return msg;
}

// the run itself, on device arrays, once the call has passed its refusals
// tape != nullptr: step k's solve writes its final working set and exit flags into slice k of the tape, a warm step
// reads slice k - 1, and the POST kernel takes the step's flags from the tape
int run(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat, double *uprev, double *U_traj,
        double *X_traj, int32_t *flag_min, const lmpc_scenario_tape *tape, hipStream_t st) {
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    const int nx = s->nx;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, s->nu, s->nd, s->ny, s->plant, s->measurement, s->cost);
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    ScnPre A; ScnPost B;
    { const int rcb = scn_begin(h, h->scnScr, N, s, x, xhat, uprev, X_traj, flag_min, h->simTheta, h->simU, h->simFlag, st, A, B);
      if (rcb != LMPC_OK) return rcb; }
    const bool wantCost = scn_want_cost(s);
    const unsigned grid = (unsigned)((N + 255) / 256);
    const size_t slice = (size_t)N * (size_t)h->P.words();
    return scn_loop(h, s, N, T, U_traj, X_traj, A, B,
        [&](int k) {
            if (tape) B.flag = tape->flag + (size_t)k * N;
            dispatch_nx(nx, [&](auto NX) {
                hipLaunchKernelGGL(scenario_pre_kernel<decltype(NX)::value>, dim3(grid), dim3(256), sizeof(double) * 256 * (size_t)nx, st, A, K);
            });
        },
        [&](int k) {
            if (!tape) return scn_solve(h, s, N, k, st);
            uint64_t *act = tape->active + (size_t)k * slice;
            return api_launch(h, LoopMode{}, N, h->simTheta, h->simU, tape->flag + (size_t)k * N, nullptr, act,
                              (s->warm && k > 0) ? act - slice : nullptr, st);
        },
        [&](int) {
            dispatch_nx(nx, [&](auto NX) {
                if (wantCost) hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, true>), dim3(grid), dim3(256), 0, st, B, K);
                else hipLaunchKernelGGL((scenario_post_kernel<decltype(NX)::value, false>), dim3(grid), dim3(256), 0, st, B, K);
            });
        });
}

}  // namespace

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
    const std::string msg = call_problem(h, N, T, s, x, xhat, uprev, true);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_device: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    return run(h, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min, nullptr, (hipStream_t)stream);
}

int lmpc_simulate_scenario(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                           double *uprev, double *U_traj, double *X_traj, int32_t *flag_min) {
    if (!h) return LMPC_ERR_BADARG;
    // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
    const std::string msg = call_problem(h, N, T, s, x, xhat, uprev, false);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = run(h, N, T, &g.d, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, nullptr, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

int lmpc_simulate_scenario_taped_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                        double *uprev, double *U_traj, double *X_traj, int32_t *flag_min,
                                        const lmpc_scenario_tape *tape, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    std::string msg = call_problem(h, N, T, s, x, xhat, uprev, true);
    if (msg.empty() && N > 0 && T > 0 && (!tape || !tape->active || !tape->flag)) msg = "tape: NULL";
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_taped_device: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    return run(h, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min, tape, (hipStream_t)stream);
}

int lmpc_simulate_scenario_taped(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                 double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, const lmpc_scenario_tape *tape) {
    if (!h) return LMPC_ERR_BADARG;
    std::string msg = call_problem(h, N, T, s, x, xhat, uprev, false);
    if (msg.empty() && N > 0 && T > 0 && (!tape || !tape->active || !tape->flag)) msg = "tape: NULL";
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_taped: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    lmpc_scenario_tape dt;
    dt.active = (uint64_t *)sg.out(tape->active, sizeof(uint64_t) * (size_t)T * (size_t)N * (size_t)h->P.words());
    dt.flag = (int32_t *)sg.out(tape->flag, sizeof(int32_t) * (size_t)T * (size_t)N);
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = run(h, N, T, &g.d, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, &dt, nullptr);
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
