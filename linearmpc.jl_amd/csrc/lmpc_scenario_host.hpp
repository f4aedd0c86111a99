// Host side of the scenario loops, shared by lmpc_scenario.hip and lmpc_explicit_sim.hip: the refusals that need no
// device, the run's constants packed into one buffer and uploaded into the handle's scratch, and the staging of a
// host-pointer call's descriptor and arrays.
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
    if (v.size() > h->scnCCap) {
        hipFree(h->scnC); h->scnC = nullptr; h->scnCCap = 0;
        HIP_TRY(h, hipMalloc(&h->scnC, sizeof(double) * v.size()));
        h->scnCCap = v.size();
    }
    HIP_TRY(h, hipMemcpyAsync(h->scnC, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, st));
    K.c = h->scnC;
    return LMPC_OK;
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
