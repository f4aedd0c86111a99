// Host side of the uncertainty descriptor, shared by lmpc_uncertain.hip and lmpc_nonlinear.hip: its refusals, its
// packing behind the run's constants (UncStep) and its staging for a host-pointer call.
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "lmpc_scenario_host.hpp"
#include "lmpc_uncertain_kernels.hpp"

namespace lmpc {

// a Gaussian source: lo = the means, hi = the standard deviations, both required
inline std::string gaussian_problem(const char *name, const lmpc_noise &n) {
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

inline std::string noise_problem(const char *name, const lmpc_noise &n) {
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
inline std::string uncertain_problem(int nth, int nout, const lmpc_observer *obs, const lmpc_scenario_sim *s, const lmpc_uncertainty *un) {
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

// a drawn source's constants appended to v as the draws take them: [lo | span | hi] with span = hi - lo (uniform) or
// [mean | std] (Gaussian), w entries each; returns where they start
inline int append_draw_constants(std::vector<double> &v, const lmpc_noise &n) {
    const int off = (int)v.size();
    v.insert(v.end(), n.lo, n.lo + n.w);
    if (n.dist != LMPC_NOISE_GAUSSIAN)
        for (int q = 0; q < n.w; q++) v.push_back(n.hi[q] - n.lo[q]);
    v.insert(v.end(), n.hi, n.hi + n.w);
    return off;
}

// a source as the kernels take it; a drawn one's constants go behind the run's constants
inline UncSource pack_source(std::vector<double> &v, const lmpc_noise &n) {
    UncSource S{};
    S.src = to_block(nullptr);
    S.w = n.w; S.drawn = n.lo != nullptr && n.w > 0;
    S.lo = S.span = S.hi = -1;
    if (S.drawn) {
        const bool gaussian = n.dist == LMPC_NOISE_GAUSSIAN;
        if (gaussian) S.drawn = UNC_GAUSSIAN;
        S.lo = append_draw_constants(v, n);
        S.span = S.lo + n.w;
        S.hi = gaussian ? S.span : S.span + n.w;
    } else if (n.w > 0) {
        S.src = to_block(&n.src);
        S.src.w = n.w;                                 // (a NULL source gives zeros whatever src.w says)
    }
    return S;
}

// the uncertainty as one step's launches take it, all but `step` and `w_out`: the two sources and Gw behind the run's
// constants, the keys, the scenario offset (the plant table is the uncertain loop's own)
inline UncStep pack_uncertainty(std::vector<double> &hostC, const lmpc_uncertainty *un, int nx) {
    UncStep U{};
    U.process = pack_source(hostC, un->process);
    U.meas = pack_source(hostC, un->measurement);
    U.gw = -1;
    if (un->Gw && un->process.w > 0) {
        U.gw = (int)hostC.size();
        hostC.insert(hostC.end(), un->Gw, un->Gw + (size_t)nx * un->process.w);
    }
    U.key0 = (uint32_t)(un->seed & 0xffffffffu); U.key1 = (uint32_t)(un->seed >> 32);
    U.goff = (unsigned long long)un->scenario_offset;
    return U;
}

// step k's fields
inline void unc_advance(UncStep &U, const lmpc_uncertainty *un, int64_t N, int nx, int k) {
    U.step = (uint32_t)(un->step_offset + k);
    U.w_out = un->W_traj ? un->W_traj + (size_t)k * N * nx : nullptr;
}

// the instantiations that hold the Gaussian sequence serve a run with such a source, and no other
inline bool unc_gauss(const UncStep &U) { return U.process.drawn == UNC_GAUSSIAN || U.meas.drawn == UNC_GAUSSIAN; }

// the PRE launch of the uncertain and the nonlinear loop
inline void launch_uncertain_pre(int64_t N, const ScnPre &A, const ScnConst &K, const UncStep &U, hipStream_t st) {
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    const size_t lds = sizeof(double) * 256 * (size_t)A.nx;
    dispatch_nx(A.nx, [&](auto NX) {
        if (unc_gauss(U)) hipLaunchKernelGGL((uncertain_pre_kernel<decltype(NX)::value, true>), grid, block, lds, st, A, K, U);
        else hipLaunchKernelGGL(uncertain_pre_kernel<decltype(NX)::value>, grid, block, lds, st, A, K, U);
    });
}

// a host-pointer call's uncertainty with its supplied sources and W_traj staged on the device (plant_index: the
// uncertain loop's own)
inline lmpc_uncertainty stage_uncertainty(Staging &sg, const lmpc_uncertainty *un, int64_t N, int T, int nx) {
    lmpc_uncertainty du = *un;
    const size_t n = (size_t)N;
    for (lmpc_noise *b : {&du.process, &du.measurement}) {
        const bool read = !b->lo && b->src.src && b->w > 0;
        const size_t cnt = read ? (b->src.stride > 0 ? (n - 1) * (size_t)b->src.stride : 0) + (size_t)b->w * b->src.T : 0;
        b->src.src = read ? static_cast<const double *>(sg.in(b->src.src, sizeof(double) * cnt)) : nullptr;
    }
    du.W_traj = (double *)sg.out(un->W_traj, sizeof(double) * T * n * (size_t)nx);
    return du;
}

}  // namespace lmpc
