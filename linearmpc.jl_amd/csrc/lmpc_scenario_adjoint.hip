// C ABI of liblmpc_hip.so, the scenario loop's adjoint (include/lmpc_hip.h, "Scenario loop adjoint"): the backward sweep
// of a taped run -- per step one launch of scenario_adjoint_kernel (lmpc_scenario_adjoint_kernel.hpp) and the VJP of
// the differentiable solve (lmpc_sens.hip) on the step's tape slice -- its host-pointer twin, and the host twin that
// runs the same arithmetic without a GPU.  The taped forward run itself is lmpc_scenario.hip's.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_scenario_adjoint_kernel.hpp"
#include "lmpc_scenario_host.hpp"
#include "lmpc_sens_kernel.hpp"

using namespace lmpc;

namespace {

size_t bar_count(const ThetaBlock &b, int64_t N) { return (size_t)b.T * (size_t)N * (size_t)b.w; }

std::string grad_problem(int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape, const lmpc_scenario_grad *g) {
    if (N < 0) return "N: negative";
    if (N > 0x7fffffffLL) return "N: beyond 2^31 - 1";
    if (T < 0) return "T: negative";
    if (!g) return "g: NULL";
    if (N > 0 && T > 0 && (!tape || !tape->active || !tape->flag)) return "tape: NULL";
    if (g->xhat0bar && !s->use_observer) return "xhat0bar: given without use_observer";
    return "";
}

// the records of the sweep's launches, all but what changes from launch to launch (adj_advance)
void adj_fill(ScnAdj &A, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_grad *g, int nth) {
    A.r = to_block(&s->r); A.d = to_block(&s->d); A.p = to_block(&s->p);
    A.rbar = A.r.w > 0 ? g->rbar : nullptr; A.dbar = A.d.w > 0 ? g->dbar : nullptr; A.pbar = A.p.w > 0 ? g->pbar : nullptr;
    A.x0bar = g->x0bar; A.xhat0bar = s->use_observer ? g->xhat0bar : nullptr; A.uprev0bar = s->nuprev > 0 ? g->uprev0bar : nullptr;
    A.status_min = g->status_min;
    A.nx = s->nx; A.nu = s->nu; A.nd = s->nd; A.ny = s->ny; A.nup = s->nuprev; A.nth = nth;
    A.T = T; A.n = (long long)N;
}

// launch number k of the sweep (k = T - 1 down to -1): finishes step k + 1, forms step k
void adj_advance(ScnAdj &A, int64_t N, int T, int k, const lmpc_scenario_grad *g) {
    A.fin = k + 1 < T ? k + 1 : -1;
    A.form = k;
    const int j = A.fin;
    scn_step_columns(A, j);                           // the columns the forward's step j read
    A.xbar_end = g->Xbar ? g->Xbar + (size_t)T * N * A.nx : nullptr;
    A.xbar_fin = (g->Xbar && j >= 0) ? g->Xbar + (size_t)j * N * A.nx : nullptr;
    A.ubar_form = (g->Ubar && k >= 0) ? g->Ubar + (size_t)k * N * A.nu : nullptr;
}

int zero_outputs(lmpc_handle *h, const ScnAdj &A, int64_t N, hipStream_t st) {
    if (A.rbar) HIP_TRY(h, hipMemsetAsync(A.rbar, 0, sizeof(double) * bar_count(A.r, N), st));
    if (A.dbar) HIP_TRY(h, hipMemsetAsync(A.dbar, 0, sizeof(double) * bar_count(A.d, N), st));
    if (A.pbar) HIP_TRY(h, hipMemsetAsync(A.pbar, 0, sizeof(double) * bar_count(A.p, N), st));
    return LMPC_OK;
}

// the sweep itself, on device arrays, once the call has passed its refusals
int sweep(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape, const lmpc_scenario_grad *g,
          hipStream_t st) {
    const int nx = s->nx, nu = s->nu, nup = s->nuprev, nth = h->P.nth;
    const bool obs = s->use_observer != 0;
    // one scratch group: [alpha | beta | gamma | ubar | thbar] and the step's status
    const size_t per = (size_t)2 * nx + nup + nu + nth;
    const size_t need = (size_t)N * per;
    if (need > h->adjDoubles || N > h->adjCap) {
        const int64_t capN = N > h->adjCap ? N : h->adjCap;
        const size_t capD = need > h->adjDoubles ? need : h->adjDoubles;
        h->adjCap = 0; h->adjDoubles = 0;
        HIP_TRY(h, reserve_group(h->adjCap, capN, sized(h->adjState, capD), sized(h->adjStatus, (size_t)capN)));
        h->adjDoubles = capD;
    }
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, s->nd, obs ? s->ny : 0, s->plant, obs ? s->measurement : nullptr, nullptr);
    LMPC_TRY(upload_constants(h, hostC, K, st));
    ScnAdj A;
    adj_fill(A, N, T, s, g, nth);
    double *base = h->adjState;
    A.alpha = base; A.beta = obs ? base + (size_t)N * nx : nullptr; A.gamma = base + (size_t)N * 2 * nx;
    A.ubar = A.gamma + (size_t)N * nup;
    double *thbar = A.ubar + (size_t)N * nu;
    A.thbar = thbar; A.status = h->adjStatus;
    A.plant = K.c + K.plant; A.meas = obs ? K.c + K.meas : nullptr;
    if (obs) {
        const size_t obs_nd = (size_t)h->obsNx * (1 + h->obsNx + h->obsNu + h->obsNd);
        const size_t obs_nm = (size_t)h->obsNy * (1 + h->obsNx + h->obsNd);
        A.obs_dyn = h->obsC; A.obs_meas = h->obsC + obs_nd; A.obs_kt = h->obsC + obs_nd + obs_nm;
    }
    LMPC_TRY(zero_outputs(h, A, N, st));
    const int tw = adj_tile_width(nth), ld = adj_tile_ld(nth);
    const size_t lds = sizeof(double) * kAdjBlock * (size_t)ld;
    const unsigned grid = (unsigned)((N + kAdjBlock - 1) / kAdjBlock);
    const size_t words = (size_t)h->P.words();
    int nxt = 0, listPass = 0;
    if (lds > 48 * 1024) {
        hipError_t ea = hipSuccess;
        dispatch_nx(nx, [&](auto NX) {
            ea = hipFuncSetAttribute((const void *)scenario_adjoint_kernel<decltype(NX)::value>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        });
        HIP_TRY(h, ea);
    }
    for (int k = T - 1; k >= -1; k--) {
        adj_advance(A, N, T, k, g);
        dispatch_nx(nx, [&](auto NX) {
            nxt = decltype(NX)::value;
            hipLaunchKernelGGL(scenario_adjoint_kernel<decltype(NX)::value>, dim3(grid), dim3(kAdjBlock), lds, st, A, tw, ld);
        });
        HIP_TRY(h, hipGetLastError());
        if (k < 0) break;
        LMPC_TRY(sens_vjp_enqueue(h, N, tape->active + (size_t)k * N * words, tape->flag + (size_t)k * N, A.ubar, thbar,
                                  h->adjStatus, st, &listPass));
    }
    const int32_t rec[LMPC_SCENARIO_ADJOINT_INFO_WORDS] = {0, nxt, (int32_t)grid, (int32_t)lds, T, (int32_t)N, listPass, tw};
    h->adjRec.push(rec);
    return LMPC_OK;
}

int refuse(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape, const lmpc_scenario_grad *g,
           const char *who) {
    LMPC_TRY(sens_refuse(h, who));
    const HandleObserver ob(h);
    std::string msg = scenario_problem(h->P.nth, h->P.nout, ob.ptr, s);
    if (msg.empty()) msg = grad_problem(N, T, s, tape, g);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, std::string(who) + ": " + msg);
    return LMPC_OK;
}

}  // namespace

extern "C" {

int lmpc_scenario_vjp_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape,
                             const lmpc_scenario_grad *g, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    LMPC_TRY(refuse(h, N, T, s, tape, g, "lmpc_scenario_vjp_device"));
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    return sweep(h, N, T, s, tape, g, (hipStream_t)stream);
}

int lmpc_scenario_vjp(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape,
                      const lmpc_scenario_grad *g) {
    if (!h) return LMPC_ERR_BADARG;
    LMPC_TRY(refuse(h, N, T, s, tape, g, "lmpc_scenario_vjp"));
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const size_t n = (size_t)N, R = sizeof(double), nx = (size_t)s->nx;
    const ThetaBlock br = to_block(&s->r), bd = to_block(&s->d), bp = to_block(&s->p);
    Staging sg;
    lmpc_scenario_tape dt;
    lmpc_scenario_grad dg;
    dt.active = (uint64_t *)sg.in(tape ? tape->active : nullptr, sizeof(uint64_t) * (size_t)T * n * (size_t)h->P.words());
    dt.flag = (int32_t *)sg.in(tape ? tape->flag : nullptr, sizeof(int32_t) * (size_t)T * n);
    dg.Xbar = (const double *)sg.in(g->Xbar, R * ((size_t)T + 1) * n * nx);
    dg.Ubar = (const double *)sg.in(g->Ubar, R * (size_t)T * n * (size_t)s->nu);
    dg.x0bar = (double *)sg.out(g->x0bar, R * n * nx);
    dg.xhat0bar = (double *)sg.out(g->xhat0bar, R * n * nx);
    dg.uprev0bar = (double *)sg.out(s->nuprev > 0 ? g->uprev0bar : nullptr, R * n * (size_t)s->nuprev);
    dg.rbar = (double *)sg.out(br.w > 0 ? g->rbar : nullptr, R * bar_count(br, N));
    dg.dbar = (double *)sg.out(bd.w > 0 ? g->dbar : nullptr, R * bar_count(bd, N));
    dg.pbar = (double *)sg.out(bp.w > 0 ? g->pbar : nullptr, R * bar_count(bp, N));
    dg.status_min = (int32_t *)sg.out(g->status_min, sizeof(int32_t) * n);
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = sweep(h, N, T, s, &dt, &dg, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

int lmpc_scenario_vjp_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                           const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                           const lmpc_settings *settings, int is_avi, const lmpc_observer *observer, int64_t N, int T,
                           const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape, const lmpc_scenario_grad *g) {
    auto bad = [](int code, const std::string &msg) { g_setup_err = "lmpc_scenario_vjp_host: " + msg; return code; };
    (void)du; (void)dl; (void)x0;
    // the pack's own refusals, those of lmpc_solve_vjp_host
    lmpc_settings st;
    LMPC_TRY(sens_check_pack("lmpc_solve_*_host", n, m, ms, nth, nout, M, Dth, Rout, Xth, sense, true, settings, is_avi, 0, &st));
    std::string msg = scenario_problem(nth, nout, observer, s);
    if (msg.empty()) msg = grad_problem(N, T, s, tape, g);
    if (msg.empty() && s->use_observer && (!observer->plant_dynamics || !observer->measurement_function || !observer->k_transpose))
        msg = "observer: NULL array";
    if (!msg.empty()) return bad(LMPC_ERR_BADARG, msg);
    if (N == 0) return LMPC_OK;
    const int nx = s->nx, nu = s->nu, nup = s->nuprev;
    const bool obs = s->use_observer != 0;
    SensDims d;
    d.m = m; d.nth = nth; d.nout = nout; d.words = (2 * m + 63) / 64;
    const size_t words = (size_t)d.words;
    std::vector<double> C;                               // the derived pack, once for the sweep
    sens_build_pack(n, d, M, nullptr, Dth, Rout, Xth, sense, C);
    const SensView S = sens_view(C.data(), d, st.rho_soft, st.zero_tol);
    std::vector<double> state((size_t)N * ((size_t)2 * nx + nup + nu + nth));
    std::vector<int32_t> status((size_t)N);
    ScnAdj A;
    adj_fill(A, N, T, s, g, nth);
    A.alpha = state.data(); A.beta = obs ? A.alpha + (size_t)N * nx : nullptr; A.gamma = A.alpha + (size_t)N * 2 * nx;
    A.ubar = A.gamma + (size_t)N * nup;
    double *thbar = A.ubar + (size_t)N * nu;
    A.thbar = thbar; A.status = status.data();
    A.plant = s->plant; A.meas = obs ? s->measurement : nullptr;
    if (obs) { A.obs_dyn = observer->plant_dynamics; A.obs_meas = observer->measurement_function; A.obs_kt = observer->k_transpose; }
    auto zero = [&](double *bar, const ThetaBlock &b) {
        if (bar) for (size_t q = 0, cnt = bar_count(b, N); q < cnt; q++) bar[q] = 0.0;
    };
    zero(A.rbar, A.r); zero(A.dbar, A.d); zero(A.pbar, A.p);
    for (int k = T - 1; k >= -1; k--) {
        adj_advance(A, N, T, k, g);
        adj_launch_host(A);
        if (k < 0) break;
        sens_host_points(S, d, false, N, tape->active + (size_t)k * N * words, tape->flag + (size_t)k * N, A.ubar, thbar, status.data());
    }
    return LMPC_OK;
}

int lmpc_scenario_adjoint_launch_info(const lmpc_handle *h, int32_t *out, int max) {
    if (!h || !out || max < 0) return LMPC_ERR_BADARG;
    return h->adjRec.read(out, max);
}

}  // extern "C"
