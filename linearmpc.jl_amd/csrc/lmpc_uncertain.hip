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

// a Gaussian source: lo = the means, hi = the standard deviations, both required
std::string gaussian_problem(const char *name, const lmpc_noise &n) {
    auto bad = [&](const char *f, const std::string &why) { return std::string(name) + "." + f + ": " + why; };
    if (!n.lo) return bad("lo", "NULL with dist == LMPC_NOISE_GAUSSIAN (the means)");
    if (!n.hi) return bad("hi", "NULL with dist == LMPC_NOISE_GAUSSIAN (the standard deviations)");
    for (int q = 0; q < n.w; q++) {
        if (!std::isfinite(n.lo[q])) return bad("lo", "non-finite mean at component " + std::to_string(q));
        if (!std::isfinite(n.hi[q])) return bad("hi", "non-finite standard deviation at component " + std::to_string(q));
        if (n.hi[q] < 0.0) return bad("hi", "negative standard deviation at component " + std::to_string(q));
    }
    if (n.src.H != 0) return bad("src.H", "a noise block has no preview");
    if (n.src.w < 0) return bad("src.w", "negative width");
    if (n.src.stride < 0) return bad("src.stride", "negative stride");
    return "";
}

std::string noise_problem(const char *name, const lmpc_noise &n) {
    auto bad = [&](const char *f, const std::string &why) { return std::string(name) + "." + f + ": " + why; };
    if (n.w < 0) return bad("w", "negative count");
    if (n.dist != LMPC_NOISE_UNIFORM && n.dist != LMPC_NOISE_GAUSSIAN)
        return bad("dist", "must be LMPC_NOISE_UNIFORM (0) or LMPC_NOISE_GAUSSIAN (1), got " + std::to_string(n.dist));
    if (n.dist == LMPC_NOISE_GAUSSIAN) return gaussian_problem(name, n);
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
    if (S.drawn && n.dist == LMPC_NOISE_GAUSSIAN) {        // the means, then the standard deviations
        S.drawn = UNC_GAUSSIAN;
        S.lo = (int)v.size(); v.insert(v.end(), n.lo, n.lo + n.w);
        S.span = S.hi = (int)v.size(); v.insert(v.end(), n.hi, n.hi + n.w);
    } else if (S.drawn) {
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

// ---- lmpc_noise_draw_*: the e of one (global scenario, global step, stream), all w components, as UncDraws and
// unc_value give them to the loop: one source for the CPU and the GPU.  c = [lo | span | hi] (uniform) or [mean | std].
__host__ __device__ __forceinline__ void noise_draw_record(const double *__restrict__ c, int w, int gaussian, uint32_t k0,
                                                           uint32_t k1, unsigned long long g, uint32_t step, uint32_t stream,
                                                           double *__restrict__ out) {
    for (int j = 0; 2 * j < w; j++) {
        uint32_t r[4] = {(uint32_t)g, (uint32_t)(g >> 32), step, (stream << 16) | (uint32_t)j};
        philox4x32_10(r, k0, k1);
        double a = philox_unit(r[0], r[1]), b = philox_unit(r[2], r[3]);
        if (gaussian) {
            const double ua = a, ub = b;
            nm_gauss_pair(ua, ub, a, b);
        }
        for (int q = 2 * j; q < 2 * j + 2 && q < w; q++) {
            const double v = q & 1 ? b : a;
            if (gaussian) {
                out[q] = nm_gauss_value(c[q], c[w + q], v);
            } else {
                const double e = LMPC_PP_ADD(c[q], LMPC_PP_MUL(v, c[w + q])), hi = c[2 * w + q];
                out[q] = e < hi ? e : hi;
            }
        }
    }
}

// one (scenario, step) per lane: record idx = i * T + k goes to out + idx * w
__global__ __launch_bounds__(256) void noise_draw_kernel(const double *__restrict__ c, int w, int gaussian, uint32_t k0, uint32_t k1,
                                                         unsigned long long goff, uint32_t step0, uint32_t stream, int T,
                                                         long long total, double *__restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long i = idx / T;
    const int k = (int)(idx - i * T);
    noise_draw_record(c, w, gaussian, k0, k1, goff + (unsigned long long)i, step0 + (uint32_t)k, stream, out + idx * w);
}

std::string draw_problem(const lmpc_noise *n, int stream, int64_t N, int32_t step_offset, int T, const double *out) {
    if (!n) return "noise: NULL source";
    const std::string msg = noise_problem("noise", *n);
    if (!msg.empty()) return msg;
    if (!n->lo) return "noise.lo: NULL (a supplied source draws nothing)";
    if (stream != 0 && stream != 1) return "stream: must be 0 (process) or 1 (measurement), got " + std::to_string(stream);
    if (N < 0) return "N: negative";
    if (T < 0) return "T: negative";
    if (step_offset < 0) return "step_offset: negative";
    if ((int64_t)step_offset + T > 2147483647LL) return "step_offset: step_offset + T exceeds 2^31 - 1";
    if (T > 0 && N > (int64_t)0x7fffffff * 256 / T) return "N: N * T exceeds what one launch covers";
    if (N > 0 && T > 0 && n->w > 0 && !out) return "out: NULL";
    return "";
}

// [lo | span | hi] or [mean | std] as noise_draw_record takes them
std::vector<double> draw_constants(const lmpc_noise &n) {
    std::vector<double> c(n.lo, n.lo + n.w);
    if (n.dist == LMPC_NOISE_GAUSSIAN) {
        c.insert(c.end(), n.hi, n.hi + n.w);
    } else {
        for (int q = 0; q < n.w; q++) c.push_back(n.hi[q] - n.lo[q]);
        c.insert(c.end(), n.hi, n.hi + n.w);
    }
    return c;
}

}  // namespace

extern "C" {

int lmpc_noise_draw_host(const lmpc_noise *noise, uint64_t seed, int stream, int64_t scenario_offset, int64_t N,
                         int32_t step_offset, int T, double *out) {
    const std::string msg = draw_problem(noise, stream, N, step_offset, T, out);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_noise_draw_host: " + msg);
    if (N == 0 || T == 0 || noise->w == 0) return LMPC_OK;
    const std::vector<double> c = draw_constants(*noise);
    const int w = noise->w, gaussian = noise->dist == LMPC_NOISE_GAUSSIAN;
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
    for (int64_t i = 0; i < N; i++)
        for (int k = 0; k < T; k++)
            noise_draw_record(c.data(), w, gaussian, k0, k1, (unsigned long long)scenario_offset + (unsigned long long)i,
                              (uint32_t)(step_offset + k), (uint32_t)stream, out + ((size_t)i * T + k) * w);
    return LMPC_OK;
}

int lmpc_noise_draw_device(lmpc_handle *h, const lmpc_noise *noise, uint64_t seed, int stream, int64_t scenario_offset,
                           int64_t N, int32_t step_offset, int T, double *out, void *hip_stream) {
    if (!h) return LMPC_ERR_BADARG;
    const std::string msg = draw_problem(noise, stream, N, step_offset, T, out);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_noise_draw_device: " + msg);
    if (N == 0 || T == 0 || noise->w == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)hip_stream;
    ScnConst K{};
    const std::vector<double> c = draw_constants(*noise);
    { const int rcu = upload_constants(h, c, K, st); if (rcu != LMPC_OK) return rcu; }
    const long long total = (long long)N * T;
    hipLaunchKernelGGL(noise_draw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, K.c, noise->w,
                       (int)(noise->dist == LMPC_NOISE_GAUSSIAN), (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
                       (unsigned long long)scenario_offset, (uint32_t)step_offset, (uint32_t)stream, T, total, out);
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}


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
    // the instantiations that hold the Gaussian sequence serve a run with such a source, and no other
    const bool gauss = U.process.drawn == UNC_GAUSSIAN || U.meas.drawn == UNC_GAUSSIAN;
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
            if (gauss) hipLaunchKernelGGL((uncertain_pre_kernel<decltype(NX)::value, true>), dim3(grid), dim3(256), sizeof(double) * 256 * (size_t)nx, st, A, K, U);
            else hipLaunchKernelGGL(uncertain_pre_kernel<decltype(NX)::value>, dim3(grid), dim3(256), sizeof(double) * 256 * (size_t)nx, st, A, K, U);
        });
        HIP_TRY(h, hipGetLastError());
        const uint64_t *wm = (s->warm && k > 0) ? h->simAct : nullptr;
        const int rc = api_launch(h, N, h->simTheta, h->simU, h->simFlag, nullptr, s->warm ? h->simAct : nullptr, wm, st);
        if (rc != LMPC_OK) return rc;
        B.k = k; B.first = k == 0; B.last = k == T - 1;
        B.xtraj_next = X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr;
        B.utraj = U_traj ? U_traj + (size_t)k * N * nu : nullptr;
        dispatch_nx(nx, [&](auto NX) {
            if (gauss && wantCost) hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, true, true>), dim3(grid), dim3(256), 0, st, B, K, U);
            else if (gauss) hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, false, true>), dim3(grid), dim3(256), 0, st, B, K, U);
            else if (wantCost) hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, true>), dim3(grid), dim3(256), 0, st, B, K, U);
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
