// Host side of the scenario loops, shared by lmpc_scenario.hip, lmpc_uncertain.hip, lmpc_nonlinear.hip,
// lmpc_offset_free.hip and lmpc_explicit_sim.hip: the refusals that need no device, the run's constants packed into one
// buffer and uploaded into the handle's scratch, the staging of a host-pointer call's descriptor and arrays, and the
// lock-step loop itself (scn_loop: per step the PRE launch, the solve, the POST launch) with what it is set up from.
#pragma once

#include <string>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_scenario_kernels.hpp"

namespace lmpc {

inline int bwidth(const lmpc_block &b) { return b.w * (b.H > 0 ? b.H : 1); }

// every check that needs no device; `obs`: the dimensions lmpc_set_observer was given, or nullptr.  "" = fine,
// otherwise the text, which starts with the offending field's name.  `offset_free`: the check of the offset-free loop
// (lmpc_scenario_offset_free_check) -- the observer is required and na = nx + of->n_offset_free wide, nd counts the
// MEASURED disturbances and every column of theta's d block carries the n_offset_free estimates behind them
inline std::string scenario_problem(int nth, int nout, const lmpc_observer *obs, const lmpc_scenario_sim *s,
                                    const lmpc_offset_free *of = nullptr, bool offset_free = false) {
    if (!s) return "s: NULL descriptor";
    auto bad = [](const char *f, const std::string &why) { return std::string(f) + ": " + why; };
    if (offset_free && !of) return "of: NULL descriptor";
    if (offset_free && of->n_offset_free <= 0) return bad("n_offset_free", "must be >= 1, got " + std::to_string(of->n_offset_free));
    const int ndo = offset_free ? of->n_offset_free : 0;
    if (s->nx < 1 || s->nx > 32) return bad("nx", "1 <= nx <= 32, got " + std::to_string(s->nx));
    if (offset_free && s->nx + ndo > 32)
        return bad("n_offset_free", "nx + n_offset_free <= 32, got " + std::to_string(s->nx) + " + " + std::to_string(ndo));
    if (s->nu != nout || s->nu < 0 || s->nu > 64)
        return bad("nu", "must equal the handle's nout = " + std::to_string(nout) + " (and be <= 64), got " + std::to_string(s->nu));
    if (s->nd < 0 || s->nd > 32) return bad("nd", "0 <= nd <= 32, got " + std::to_string(s->nd));
    if (s->ny < 0 || s->ny > 32) return bad("ny", "0 <= ny <= 32, got " + std::to_string(s->ny));
    if (!s->plant) return bad("plant", "NULL");
    if (s->ny > 0 && !s->measurement) return bad("measurement", "NULL with ny > 0");
    const lmpc_block *bs[4] = {&s->r, &s->d, &s->p, &s->noise};
    const char *bn[4] = {"r", "d", "p", "noise"};
    for (int b = 0; b < 4; b++) {
        if (bs[b]->w < 0) return bad((std::string(bn[b]) + ".w").c_str(), "negative width");
        if (bs[b]->H < 0) return bad((std::string(bn[b]) + ".H").c_str(), "negative preview length");
        if (bs[b]->src && bs[b]->w > 0 && bs[b]->T < 1) return bad((std::string(bn[b]) + ".T").c_str(), "no columns");
        if (bs[b]->stride < 0) return bad((std::string(bn[b]) + ".stride").c_str(), "negative stride");
    }
    if (s->d.w != 0 && s->d.w != s->nd) return bad("d.w", "must be nd = " + std::to_string(s->nd) + " (or 0: no disturbance), got " + std::to_string(s->d.w));
    if (s->noise.w != 0 && s->noise.w != s->ny) return bad("noise.w", "must be ny = " + std::to_string(s->ny) + " (or 0: no noise), got " + std::to_string(s->noise.w));
    if (s->noise.H != 0) return bad("noise.H", "the noise block has no preview");
    if (s->nuprev < 0 || s->nuprev > s->nu) return bad("nuprev", "0 <= nuprev <= nu, got " + std::to_string(s->nuprev));
    if (offset_free && !s->use_observer) return bad("use_observer", "must be non-zero: the offset-free loop runs the handle's observer");
    if (s->use_observer) {
        if (!obs) return bad("use_observer", "lmpc_set_observer has not been called on this handle");
        if (s->ny < 1) return bad("ny", "an observer needs a measurement (ny >= 1)");
        if (offset_free && obs->n_state != s->nx + ndo)
            return bad("n_offset_free", "the observer was set with n_state = " + std::to_string(obs->n_state) + ", the descriptor says nx + n_offset_free = " + std::to_string(s->nx + ndo));
        if (!offset_free && obs->n_state != s->nx) return bad("nx", "the observer was set with n_state = " + std::to_string(obs->n_state) + ", the descriptor says " + std::to_string(s->nx));
        if (obs->n_control != s->nu) return bad("nu", "the observer was set with n_control = " + std::to_string(obs->n_control) + ", the descriptor says " + std::to_string(s->nu));
        if (obs->n_disturbance != s->nd) return bad("nd", "the observer was set with n_disturbance = " + std::to_string(obs->n_disturbance) + ", the descriptor says " + std::to_string(s->nd));
        if (obs->n_measurement != s->ny) return bad("ny", "the observer was set with n_measurement = " + std::to_string(obs->n_measurement) + ", the descriptor says " + std::to_string(s->ny));
    }
    if (offset_free) {
        const int osum = s->nx + bwidth(s->r) + (s->nd + ndo) * (s->d.H > 0 ? s->d.H : 1) + s->nuprev + bwidth(s->p);
        if (osum != nth)
            return bad("nth", "nx + width(r) + (nd + n_offset_free) * max(d.H, 1) + nuprev + width(p) = " + std::to_string(osum) + " must equal the handle's nth = " + std::to_string(nth));
    }
    const int sum = s->nx + bwidth(s->r) + bwidth(s->d) + s->nuprev + bwidth(s->p);
    if (!offset_free && sum != nth)
        return bad("nth", "nx + width(r) + width(d) + nuprev + width(p) = " + std::to_string(sum) + " must equal the handle's nth = " + std::to_string(nth));
    if ((s->Y_traj || s->Ym_traj) && s->ny == 0) return bad(s->Y_traj ? "Y_traj" : "Ym_traj", "asked for with ny = 0");
    if (s->D_traj && s->nd == 0) return bad("D_traj", "asked for with nd = 0");
    if (s->cost_out && !s->cost) return bad("cost_out", "asked for without cost");
    if (s->violation_out && !s->cost) return bad("violation_out", "asked for without cost");
    if (const lmpc_sim_cost *c = s->cost) {
        if (c->ny < 0 || c->ny > 32) return bad("cost.ny", "0 <= ny <= 32, got " + std::to_string(c->ny));
        if (c->nc < 0) return bad("cost.nc", "negative row count");
        if (c->Q && (!c->C || c->ny == 0)) return bad("cost.C", "Q given without C (ny rows)");
        if (c->C && s->r.w > 0 && s->r.w != c->ny) return bad("cost.ny", "must equal r.w = " + std::to_string(s->r.w) + ", got " + std::to_string(c->ny));
        if (c->nc > 0 && (!c->lb || !c->ub)) return bad("cost.lb", "lb and ub are required with nc > 0");
    }
    return "";
}

// the handle's observer as scenario_problem takes it (nullptr: lmpc_set_observer has not been called)
struct HandleObserver {
    lmpc_observer od;
    const lmpc_observer *ptr;
    explicit HandleObserver(const lmpc_handle *h)
        : od{h->obsNx, h->obsNu, h->obsNd, h->obsNy, nullptr, nullptr, nullptr}, ptr(h->obsC ? &od : nullptr) {}
    HandleObserver(const HandleObserver &) = delete;   // ptr points into the object
};

// What every loop's entry point refuses of its call arguments once the descriptors have passed, in two parts (the
// nonlinear loop's `q` stands between them): the sizes and the state ...
inline std::string call_size_problem(int64_t N, int T, const double *x, const lmpc_uncertainty *un = nullptr) {
    if (N < 0) return "N: negative";
    if (T < 0) return "T: negative";
    if (un && (int64_t)un->step_offset + T > 2147483647LL) return "step_offset: step_offset + T exceeds 2^31 - 1";
    if (N > 0 && !x) return "x: NULL";
    return "";
}
// ... and the arrays the descriptor decides about (`device`: a host-pointer twin takes a NULL uprev as zeros)
inline std::string call_array_problem(int64_t N, const lmpc_scenario_sim *s, const double *xhat, const double *uprev, bool device) {
    if (device && N > 0 && s->nuprev > 0 && !uprev) return "uprev: NULL with nuprev > 0";
    if (xhat && !s->use_observer) return "xhat: given without use_observer";
    return "";
}

// the run's constants in one host vector + their offsets; cost may be nullptr
inline ScnConst pack_constants(std::vector<double> &v, int nx, int nu, int nd, int ny, const double *plant, const double *meas,
                        const lmpc_sim_cost *c) {
    ScnConst K{nullptr, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0};
    auto put = [&](const double *src, size_t cnt) -> int {
        if (!src || cnt == 0) return -1;
        const int off = (int)v.size();
        v.insert(v.end(), src, src + cnt);
        return off;
    };
    if (plant) K.plant = put(plant, (size_t)nx * (1 + nx + nu + nd));
    if (meas && ny > 0) K.meas = put(meas, (size_t)ny * (1 + nx + nd));
    if (c) {
        K.nyc = c->C ? c->ny : 0; K.nc = c->nc;
        K.cC = put(c->C, (size_t)c->ny * nx); K.cQ = put(c->Q, (size_t)c->ny * c->ny);
        K.cR = put(c->R, (size_t)nu * nu); K.cRr = put(c->Rr, (size_t)nu * nu); K.cS = put(c->S, (size_t)nx * nu);
        K.cAx = put(c->Ax, (size_t)c->nc * nx); K.cAu = put(c->Au, (size_t)c->nc * nu);
        K.clb = put(c->lb, (size_t)c->nc); K.cub = put(c->ub, (size_t)c->nc);
    }
    if (v.empty()) v.push_back(0.0);
    return K;
}

inline int upload_constants(lmpc_handle *h, const std::vector<double> &v, ScnConst &K, hipStream_t st) {
    HIP_TRY(h, h->scnC.reserve(v.size()));
    HIP_TRY(h, hipMemcpyAsync(h->scnC, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, st));
    K.c = h->scnC;
    return LMPC_OK;
}

// ---- the lock-step loop

inline bool scn_want_cost(const lmpc_scenario_sim *s) { return s->cost && (s->cost_out || s->violation_out); }

// The per-run scratch [observer state | ulast] in buf (grown to fit): stateW doubles per scenario of
// observer state when the caller keeps none (else 0), the previous control of the cost's du term when the run needs it.
struct ScnScratch { double *state, *ulast; };
inline int scn_scratch(lmpc_handle *h, DevBuf<double> &buf, int64_t N, const lmpc_scenario_sim *s, size_t stateW, ScnScratch &out) {
    const size_t ulastW = scn_want_cost(s) && s->cost_out && s->cost->Rr ? (size_t)s->nu : 0;
    const size_t needScr = (size_t)N * (stateW + ulastW);
    HIP_TRY(h, buf.reserve(needScr));
    out.state = stateW ? buf.get() : nullptr;
    out.ulast = ulastW ? buf + (size_t)N * stateW : nullptr;
    return LMPC_OK;
}

// the records of the PRE / POST kernels, all but what changes from step to step (scn_advance); theta, u, flag: the
// solve's batch
inline void scn_fill(const lmpc_handle *h, const lmpc_scenario_sim *s, int64_t N, double *x, double *xhat, double *uprev,
                     int32_t *flag_min, double *theta, const double *u, const int32_t *flag, double *ulast, ScnPre &A, ScnPost &B) {
    const bool obs = s->use_observer != 0, wantCost = scn_want_cost(s);
    const size_t obs_nd = (size_t)h->obsNx * (1 + h->obsNx + h->obsNu + h->obsNd);
    const size_t obs_nm = (size_t)h->obsNy * (1 + h->obsNx + h->obsNd);
    A = ScnPre{};
    A.x = x; A.xhat = obs ? xhat : nullptr; A.uprev = uprev; A.theta = theta;
    A.obs_meas = obs ? h->obsC + obs_nd : nullptr; A.obs_kt = obs ? h->obsC + obs_nd + obs_nm : nullptr;
    A.r = to_block(&s->r); A.d = to_block(&s->d); A.p = to_block(&s->p); A.noise = to_block(&s->noise);
    A.nx = s->nx; A.ny = s->ny; A.nd = s->nd; A.nup = s->nuprev; A.n = (long long)N;
    B = ScnPost{};
    B.x = x; B.xhat = A.xhat; B.uprev = uprev; B.u = u; B.flag = flag;
    B.obs_dyn = obs ? h->obsC : nullptr; B.d = A.d; B.r = A.r;
    B.flag_min = flag_min; B.cost = wantCost ? s->cost_out : nullptr; B.viol = wantCost ? s->violation_out : nullptr;
    B.ulast = ulast; B.nx = s->nx; B.nu = s->nu; B.nd = s->nd; B.nup = s->nuprev; B.n = (long long)N;
}

// The start of a run whose observer is nx wide: the scratch in buf, xhat <- x when the caller keeps no observer state
// (set_state!(mpc, x0), simulation.jl:92; the state then lives in the scratch), X_traj's first slice <- x, the records.
inline int scn_begin(lmpc_handle *h, DevBuf<double> &buf, int64_t N, const lmpc_scenario_sim *s, double *x, double *xhat,
                     double *uprev, double *X_traj, int32_t *flag_min, double *theta, const double *u, const int32_t *flag,
                     hipStream_t st, ScnPre &A, ScnPost &B) {
    const size_t bytes = sizeof(double) * (size_t)N * s->nx;
    ScnScratch scr;
    { const int rc = scn_scratch(h, buf, N, s, s->use_observer && !xhat ? (size_t)s->nx : 0, scr); if (rc != LMPC_OK) return rc; }
    if (scr.state) {
        xhat = scr.state;
        HIP_TRY(h, hipMemcpyAsync(xhat, x, bytes, hipMemcpyDeviceToDevice, st));
    }
    if (X_traj) HIP_TRY(h, hipMemcpyAsync(X_traj, x, bytes, hipMemcpyDeviceToDevice, st));
    scn_fill(h, s, N, x, xhat, uprev, flag_min, theta, u, flag, scr.ulast, A, B);
    return LMPC_OK;
}

// the first trajectory column of step k's r / d / p blocks of theta, for the forward's PRE record and the adjoint's
template <class Rec>
void scn_step_columns(Rec &A, int k) {
    A.r.k0 = A.r.H > 0 ? k + 1 : k;                   // simulation.jl:102 get_preview(rs, k, Np) / rs[:, k]
    A.d.k0 = k; A.p.k0 = k;                           // :103-104 get_preview(ds, k - 1, Np) / ds[:, k]
}

// step k's fields of the two records (ScnPre / ScnPost or the offset-free loop's)
template <class Pre, class Post>
void scn_advance(Pre &A, Post &B, const lmpc_scenario_sim *s, int64_t N, int T, int k, double *U_traj, double *X_traj) {
    const size_t row = (size_t)k * N;
    A.k = k;
    scn_step_columns(A, k);
    A.ym_out = s->Ym_traj ? s->Ym_traj + row * s->ny : nullptr;
    A.y_out = s->Y_traj ? s->Y_traj + row * s->ny : nullptr;
    A.xhat_out = s->Xhat_traj ? s->Xhat_traj + row * s->nx : nullptr;
    A.d_out = s->D_traj ? s->D_traj + row * s->nd : nullptr;
    B.k = k; B.first = k == 0; B.last = k == T - 1;
    B.xtraj_next = X_traj ? X_traj + (row + N) * s->nx : nullptr;
    B.utraj = U_traj ? U_traj + row * s->nu : nullptr;
}

// The loop: per step the records advanced, pre(k) (the PRE launch), solve(k) (LMPC_OK or the code to hand back, its
// text already set), post(k) (the POST launch).  Nothing but enqueues unless solve waits.
template <class Pre, class Post, class FPre, class FSolve, class FPost>
int scn_loop(lmpc_handle *h, const lmpc_scenario_sim *s, int64_t N, int T, double *U_traj, double *X_traj, Pre &A, Post &B,
             FPre &&pre, FSolve &&solve, FPost &&post) {
    for (int k = 0; k < T; k++) {
        scn_advance(A, B, s, N, T, k, U_traj, X_traj);
        pre(k);
        HIP_TRY(h, hipGetLastError());
        { const int rc = solve(k); if (rc != LMPC_OK) return rc; }
        post(k);
        HIP_TRY(h, hipGetLastError());
    }
    return LMPC_OK;
}

// the handle's solve of step k on its closed-loop batch (simTheta -> simU, simFlag); warm start = the previous step's
// final working set, the first step cold (as lmpc_simulate_ref_device)
inline int scn_solve(lmpc_handle *h, const lmpc_scenario_sim *s, int64_t N, int k, hipStream_t st) {
    const uint64_t *wm = (s->warm && k > 0) ? h->simAct : nullptr;
    return api_launch(h, LoopMode{}, N, h->simTheta, h->simU, h->simFlag, nullptr, s->warm ? h->simAct : nullptr, wm, st);
}

// the host-pointer twins: the descriptor's trajectories and outputs and the caller's arrays staged on the device
// (`sg.err` says whether it worked; the caller downloads with sg.download_all())
struct StagedScenario {
    lmpc_scenario_sim d;
    double *x, *xhat, *uprev, *U, *X;
    int32_t *flag_min;
};

inline StagedScenario stage_scenario(Staging &sg, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                     double *uprev, double *U_traj, double *X_traj, int32_t *flag_min) {
    StagedScenario g{*s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    lmpc_scenario_sim &d = g.d;
    const size_t nx = (size_t)s->nx, nu = (size_t)s->nu, nd = (size_t)s->nd, ny = (size_t)s->ny, nup = (size_t)s->nuprev;
    const size_t n = (size_t)N, R = sizeof(double);
    // trajectories: one matrix per scenario (stride apart) or one shared matrix
    for (lmpc_block *b : {&d.r, &d.d, &d.p, &d.noise}) {
        const size_t cnt = (b->stride > 0 ? (n - 1) * (size_t)b->stride : 0) + (size_t)b->w * b->T;
        b->src = b->src && b->w > 0 ? static_cast<const double *>(sg.in(b->src, R * cnt)) : nullptr;
    }
    g.x = (double *)sg.out(x, R * n * nx, true);
    g.xhat = (double *)sg.out(xhat, R * n * nx, true);
    if (nup > 0) g.uprev = (double *)(uprev ? sg.out(uprev, R * n * nup, true) : sg.zeros(R * n * nup));   // NULL = zeros, as in lmpc_simulate
    g.U = (double *)sg.out(U_traj, R * T * n * nu);
    g.X = (double *)sg.out(X_traj, R * (T + 1) * n * nx);
    g.flag_min = (int32_t *)sg.out(flag_min, sizeof(int32_t) * n);
    d.Y_traj = (double *)sg.out(s->Y_traj, R * T * n * ny);
    d.Ym_traj = (double *)sg.out(s->Ym_traj, R * T * n * ny);
    d.Xhat_traj = (double *)sg.out(s->Xhat_traj, R * T * n * nx);
    d.D_traj = (double *)sg.out(s->D_traj, R * T * n * nd);
    d.cost_out = (double *)sg.out(s->cost_out, R * n);
    d.violation_out = (double *)sg.out(s->violation_out, R * n);
    return g;
}

}  // namespace lmpc
