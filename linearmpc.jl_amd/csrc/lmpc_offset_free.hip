// C ABI of liblmpc_hip.so, the scenario loop with the offset-free observer (lmpc_simulate_scenario_offset_free*):
// lmpc_scenario.hip's loop with the observer na = nx + n_offset_free wide and its disturbance estimate in theta's d
// block.  Per step a PRE kernel, the handle's solve (api_launch), a POST kernel (lmpc_offset_free_kernels.hpp); nothing
// but enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_offset_free_kernels.hpp"
#include "lmpc_scenario_host.hpp"

using namespace lmpc;

namespace {

// f(NX, NDO) with both counts as compile-time constants when nx + ndo <= 8, f(0, 0) (run-time counts) otherwise
template <class F>
void dispatch_pair(int nx, int ndo, F &&f) {
    if (nx + ndo > 8) { f(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}); return; }
    dispatch_nx(nx, [&](auto NX) {
        dispatch_nx(ndo, [&](auto ND) {
            constexpr int a = decltype(NX)::value, b = decltype(ND)::value;
            if constexpr (a > 0 && b > 0 && a + b <= 8) f(NX, ND);
        });
    });
}

std::string offset_free_problem(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_offset_free *of,
                                const double *x, const double *xaug, const double *uprev, bool device) {
    if (xaug && !h->obsC) return "xaug: given without an observer (lmpc_set_observer has not been called on this handle)";
    const HandleObserver ob(h);
    std::string msg = scenario_problem(h->P.nth, h->P.nout, ob.ptr, s, of, true);
    if (msg.empty()) msg = call_size_problem(N, T, x);
    if (msg.empty()) msg = call_array_problem(N, s, nullptr, uprev, device);
    return msg;
}

// the run itself, on device arrays, once the call has passed its refusals
int run(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_offset_free *of, double *x, double *xaug,
        double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, hipStream_t st) {
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    const int nx = s->nx, nu = s->nu, nd = s->nd, ny = s->ny, nup = s->nuprev, ndo = of->n_offset_free, na = nx + ndo;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, nd, ny, s->plant, s->measurement, s->cost);
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    const bool wantCost = scn_want_cost(s);
    ScnScratch scr;
    { const int rcs = scn_scratch(h, h->scnScr, N, s, xaug ? 0 : (size_t)na, scr); if (rcs != LMPC_OK) return rcs; }
    if (!xaug) {                                       // set_state!(observer, x0): [x0; 0], observer.jl:74-90
        xaug = scr.state;
        hipLaunchKernelGGL(offset_free_init_kernel, dim3((unsigned)(((size_t)N * na + 255) / 256)), dim3(256), 0, st, xaug, x, nx,
                           na, (long long)N);
        HIP_TRY(h, hipGetLastError());
    }
    if (X_traj) HIP_TRY(h, hipMemcpyAsync(X_traj, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    // the offset-free records: the observer's arrays are na wide, the d block carries the estimate
    const size_t obs_nd = (size_t)na * (1 + na + nu + nd);
    const size_t obs_nm = (size_t)ny * (1 + na + nd);
    OfPre A{};
    A.x = x; A.xaug = xaug; A.uprev = uprev; A.theta = h->simTheta;
    A.obs_meas = h->obsC + obs_nd; A.obs_kt = h->obsC + obs_nd + obs_nm;
    A.r = to_block(&s->r); A.d = to_block(&s->d); A.p = to_block(&s->p); A.noise = to_block(&s->noise);
    if (s->d.w == 0) A.d.src = nullptr;               // no measured trajectory: d_k = 0 (d.H still sets the columns)
    A.nx = nx; A.ndo = ndo; A.ny = ny; A.nd = nd; A.nup = nup; A.n = (long long)N;
    OfPost B{};
    B.x = x; B.xaug = xaug; B.uprev = uprev; B.u = h->simU; B.flag = h->simFlag;
    B.obs_dyn = h->obsC; B.d = A.d; B.r = A.r;
    B.flag_min = flag_min; B.cost = wantCost ? s->cost_out : nullptr; B.viol = wantCost ? s->violation_out : nullptr;
    B.ulast = scr.ulast; B.nx = nx; B.ndo = ndo; B.nu = nu; B.nd = nd; B.nup = nup; B.n = (long long)N;
    const unsigned grid = (unsigned)((N + 255) / 256);
    return scn_loop(h, s, N, T, U_traj, X_traj, A, B,
        [&](int k) {
            A.dhat_out = of->Dhat_traj ? of->Dhat_traj + (size_t)k * N * ndo : nullptr;
            dispatch_pair(nx, ndo, [&](auto NX, auto ND) {
                hipLaunchKernelGGL((offset_free_pre_kernel<decltype(NX)::value, decltype(ND)::value>), dim3(grid), dim3(256),
                                   sizeof(double) * 256 * (size_t)na, st, A, K);
            });
        },
        [&](int k) { return scn_solve(h, s, N, k, st); },
        [&](int) {
            dispatch_pair(nx, ndo, [&](auto NX, auto ND) {
                constexpr int a = decltype(NX)::value, b = decltype(ND)::value;
                if (wantCost) hipLaunchKernelGGL((offset_free_post_kernel<a, b, true>), dim3(grid), dim3(256), 0, st, B, K);
                else hipLaunchKernelGGL((offset_free_post_kernel<a, b, false>), dim3(grid), dim3(256), 0, st, B, K);
            });
        });
}

}  // namespace

namespace lmpc {
void offset_free_preload() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, (const void *)offset_free_pre_kernel<0, 0>);
    (void)hipGetLastError();
}
}  // namespace lmpc

extern "C" {

int lmpc_scenario_offset_free_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s,
                                    const lmpc_offset_free *of) {
    const std::string msg = scenario_problem(nth, nout, observer, s, of, true);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_scenario_offset_free_check: " + msg);
    return LMPC_OK;
}

int lmpc_simulate_scenario_offset_free_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                              const lmpc_offset_free *of, double *x, double *xaug, double *uprev,
                                              double *U_traj, double *X_traj, int32_t *flag_min, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const std::string msg = offset_free_problem(h, N, T, s, of, x, xaug, uprev, true);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_offset_free_device: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    return run(h, N, T, s, of, x, xaug, uprev, U_traj, X_traj, flag_min, (hipStream_t)stream);
}

int lmpc_simulate_scenario_offset_free(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                       const lmpc_offset_free *of, double *x, double *xaug, double *uprev, double *U_traj,
                                       double *X_traj, int32_t *flag_min) {
    if (!h) return LMPC_ERR_BADARG;
    // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
    const std::string msg = offset_free_problem(h, N, T, s, of, x, xaug, uprev, false);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_offset_free: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, nullptr, uprev, U_traj, X_traj, flag_min);
    const size_t n = (size_t)N, ndo = (size_t)of->n_offset_free;
    double *dxaug = (double *)sg.out(xaug, sizeof(double) * n * ((size_t)s->nx + ndo), true);
    lmpc_offset_free dof{of->n_offset_free, (double *)sg.out(of->Dhat_traj, sizeof(double) * T * n * ndo)};
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = run(h, N, T, &g.d, &dof, g.x, dxaug, g.uprev, g.U, g.X, g.flag_min, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

}  // extern "C"
