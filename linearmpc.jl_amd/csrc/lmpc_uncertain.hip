// C ABI of liblmpc_hip.so, the scenario loop under uncertainty (lmpc_simulate_scenario_uncertain*): lmpc_scenario.hip's
// loop with additive process noise on the state, additive measurement noise -- both supplied or drawn on the device --
// and a table of plant variants.  Per step a PRE kernel, the handle's solve (api_launch), a POST kernel
// (lmpc_uncertain_kernels.hpp); nothing but enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_scenario_host.hpp"
#include "lmpc_uncertain_kernels.hpp"

using namespace lmpc;

namespace {

std::string noise_problem(const char *name, const lmpc_noise &n) {
    auto bad = [&](const char *f, const std::string &why) { return std::string(name) + "." + f + ": " + why; };
    if (n.w < 0) return bad("w", "negative count");
    if (n.lo && !n.hi) return bad("hi", "NULL with lo given (both or none)");
    if (n.hi && !n.lo) return bad("lo", "NULL with hi given (both or none)");
    if (n.lo) {
        for (int q = 0; q < n.w; q++) {
            if (!std::isfinite(n.lo[q])) return bad("lo", "non-finite bound at component " + std::to_string(q));
            if (!std::isfinite(n.hi[q])) return bad("hi", "non-finite bound at component " + std::to_string(q));
            if (n.lo[q] > n.hi[q]) return bad("lo", "lo > hi at component " + std::to_string(q));
            if (!std::isfinite(n.hi[q] - n.lo[q])) return bad("hi", "hi - lo overflows at component " + std::to_string(q));
        }
    }
    if (n.src.H != 0) return bad("src.H", "a noise block has no preview");
    if (n.src.w < 0) return bad("src.w", "negative width");
    if (n.src.stride < 0) return bad("src.stride", "negative stride");
    if (!n.lo && n.src.src && n.w > 0) {
        if (n.src.w != n.w) return bad("src.w", "must equal w = " + std::to_string(n.w) + ", got " + std::to_string(n.src.w));
        if (n.src.T < 1) return bad("src.T", "no columns");
    }
    return "";
}

// every check of the uncertainty that needs no device; "" = fine, otherwise the text, the field's name first
std::string uncertain_problem(int nth, int nout, const lmpc_observer *obs, const lmpc_scenario_sim *s, const lmpc_uncertainty *un) {
    std::string msg = scenario_problem(nth, nout, obs, s);
    if (!msg.empty()) return msg;
    if (!un) return "un: NULL descriptor";
    msg = noise_problem("process", un->process);
    if (!msg.empty()) return msg;
    msg = noise_problem("measurement", un->measurement);
    if (!msg.empty()) return msg;
    if (!un->Gw && un->process.w != 0 && un->process.w != s->nx)
        return "process.w: must be nx = " + std::to_string(s->nx) + " (or 0: none) without Gw, got " + std::to_string(un->process.w);
    if (un->measurement.w != 0 && un->measurement.w != s->ny)
        return "measurement.w: must be ny = " + std::to_string(s->ny) + " (or 0: none), got " + std::to_string(un->measurement.w);
    if (un->measurement.w > 0 && s->noise.w > 0) return "measurement.w: given together with the descriptor's noise block";
    if (un->n_plants < 0) return "n_plants: negative";
    if (un->n_plants > 0 && !un->plants) return "plants: NULL with n_plants > 0";
    if (un->plant_index && un->n_plants == 0) return "plant_index: given with n_plants == 0";
    if (un->W_traj && un->process.w == 0) return "W_traj: asked for with process.w == 0";
    if (un->step_offset < 0) return "step_offset: negative";
    return "";
}

std::string call_problem(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un, const double *x,
                         const double *xhat, const double *uprev, bool device) {
    lmpc_observer od{h->obsNx, h->obsNu, h->obsNd, h->obsNy, nullptr, nullptr, nullptr};
    std::string msg = uncertain_problem(h->P.nth, h->P.nout, h->obsC ? &od : nullptr, s, un);
    if (!msg.empty()) return msg;
    if (N < 0) return "N: negative";
    if (T < 0) return "T: negative";
    if ((int64_t)un->step_offset + T > 2147483647LL) return "step_offset: step_offset + T exceeds 2^31 - 1";
    if (N > 0 && !x) return "x: NULL";
    if (device && N > 0 && s->nuprev > 0 && !uprev) return "uprev: NULL with nuprev > 0";
    if (xhat && !s->use_observer) return "xhat: given without use_observer";
    return "";
}

// a source as the kernels take it; the box goes behind the run's constants
UncSource pack_source(std::vector<double> &v, const lmpc_noise &n) {
    UncSource S{};
    S.src = to_block(nullptr);
    S.w = n.w; S.drawn = n.lo != nullptr && n.w > 0;
    S.lo = S.span = S.hi = -1;
    if (S.drawn) {
        S.lo = (int)v.size(); v.insert(v.end(), n.lo, n.lo + n.w);
        S.span = (int)v.size();
        for (int q = 0; q < n.w; q++) v.push_back(n.hi[q] - n.lo[q]);
        S.hi = (int)v.size(); v.insert(v.end(), n.hi, n.hi + n.w);
    } else if (n.w > 0) {
        S.src = to_block(&n.src);
        S.src.w = n.w;                                 // (a NULL source gives zeros whatever src.w says)
    }
    return S;
}

}  // namespace

extern "C" {

int lmpc_scenario_uncertain_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s,
                                  const lmpc_uncertainty *un) {
    const std::string msg = uncertain_problem(nth, nout, observer, s, un);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_scenario_uncertain_check: " + msg);
    return LMPC_OK;
}

int lmpc_simulate_scenario_uncertain_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                            const lmpc_uncertainty *un, double *x, double *xhat, double *uprev,
                                            double *U_traj, double *X_traj, int32_t *flag_min, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const std::string msg = call_problem(h, N, T, s, un, x, xhat, uprev, true);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_uncertain_device: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    const int nx = s->nx, nu = s->nu, nd = s->nd, ny = s->ny, nup = s->nuprev;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, nd, ny, s->plant, s->measurement, s->cost);
    UncStep U{};
    U.process = pack_source(hostC, un->process);
    U.meas = pack_source(hostC, un->measurement);
    U.gw = -1;
    if (un->Gw && un->process.w > 0) {
        U.gw = (int)hostC.size();
        hostC.insert(hostC.end(), un->Gw, un->Gw + (size_t)nx * un->process.w);
    }
    U.n_plants = un->n_plants;
    if (un->n_plants > 0) {                            // the table: n_plants arrays in the layout of s->plant
        K.plant = (int)hostC.size();
        hostC.insert(hostC.end(), un->plants, un->plants + (size_t)un->n_plants * nx * (1 + nx + nu + nd));
    }
    U.plant_index = un->plant_index;
    U.key0 = (uint32_t)(un->seed & 0xffffffffu); U.key1 = (uint32_t)(un->seed >> 32);
    U.goff = (unsigned long long)un->scenario_offset;
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
        A.r.k0 = A.r.H > 0 ? k + 1 : k;
        A.d.k0 = k; A.p.k0 = k;
        A.ym_out = s->Ym_traj ? s->Ym_traj + (size_t)k * N * ny : nullptr;
        A.y_out = s->Y_traj ? s->Y_traj + (size_t)k * N * ny : nullptr;
        A.xhat_out = s->Xhat_traj ? s->Xhat_traj + (size_t)k * N * nx : nullptr;
        A.d_out = s->D_traj ? s->D_traj + (size_t)k * N * nd : nullptr;
        U.step = (uint32_t)(un->step_offset + k);
        U.w_out = un->W_traj ? un->W_traj + (size_t)k * N * nx : nullptr;
        dispatch_nx(nx, [&](auto NX) {
            hipLaunchKernelGGL(uncertain_pre_kernel<decltype(NX)::value>, dim3(grid), dim3(256), sizeof(double) * 256 * (size_t)nx, st, A, K, U);
        });
        HIP_TRY(h, hipGetLastError());
        const uint64_t *wm = (s->warm && k > 0) ? h->simAct : nullptr;
        const int rc = api_launch(h, N, h->simTheta, h->simU, h->simFlag, nullptr, s->warm ? h->simAct : nullptr, wm, st);
        if (rc != LMPC_OK) return rc;
        B.k = k; B.first = k == 0; B.last = k == T - 1;
        B.xtraj_next = X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr;
        B.utraj = U_traj ? U_traj + (size_t)k * N * nu : nullptr;
        dispatch_nx(nx, [&](auto NX) {
            if (wantCost) hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, true>), dim3(grid), dim3(256), 0, st, B, K, U);
            else hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, false>), dim3(grid), dim3(256), 0, st, B, K, U);
        });
        HIP_TRY(h, hipGetLastError());
    }
    return LMPC_OK;
}

int lmpc_simulate_scenario_uncertain(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un,
                                     double *x, double *xhat, double *uprev, double *U_traj, double *X_traj, int32_t *flag_min) {
    if (!h) return LMPC_ERR_BADARG;
    {   // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
        const std::string msg = call_problem(h, N, T, s, un, x, xhat, uprev, false);
        if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_uncertain: " + msg);
    }
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    lmpc_uncertainty du = *un;
    const size_t n = (size_t)N;
    for (lmpc_noise *b : {&du.process, &du.measurement}) {
        const bool read = !b->lo && b->src.src && b->w > 0;
        const size_t cnt = read ? (b->src.stride > 0 ? (n - 1) * (size_t)b->src.stride : 0) + (size_t)b->w * b->src.T : 0;
        b->src.src = read ? static_cast<const double *>(sg.in(b->src.src, sizeof(double) * cnt)) : nullptr;
    }
    du.plant_index = static_cast<const int32_t *>(sg.in(un->plant_index, sizeof(int32_t) * n));
    du.W_traj = (double *)sg.out(un->W_traj, sizeof(double) * T * n * (size_t)s->nx);
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = lmpc_simulate_scenario_uncertain_device(h, N, T, &g.d, &du, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

}  // extern "C"
