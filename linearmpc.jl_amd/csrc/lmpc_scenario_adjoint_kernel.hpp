// Backward sweep of the scenario loop (lmpc_scenario_vjp*): the transposed glue of one time step, per scenario.  One copy
// of the arithmetic (AdjLane) serves scenario_adjoint_kernel and the host twin; the contract is stated in
// include/lmpc_hip.h ("Scenario loop adjoint") and restated in numpy in tests/scenario_adjoint_reference.py.  Every sum
// is one chain of explicit fmas in index order, every other operation a single addition.
// Internal to liblmpc_hip.so.
#pragma once

#include <cmath>
#include <cstdint>

#include "lmpc_sim_kernels.hpp"

namespace lmpc {

constexpr int kAdjBlock = 256;              // workgroup: one scenario per lane
constexpr int kAdjTileMax = 32;             // entries of a theta-bar record staged in LDS at a time (two workgroups per CU)

// What one launch of the sweep is told.  It FINISHES step `fin` (items 3 - 6 of the contract, from that step's theta-bar
// and VJP status) and FORMS ubar of step `form` = fin - 1; the first launch only forms (fin = -1, state from Xbar[T] and
// zeros), the last only finishes (form = -1) and writes the gradients of the initial values.
struct ScnAdj {
    double *alpha = nullptr, *beta = nullptr, *gamma = nullptr;     // carried state, N records (beta nullptr: no observer)
    double *ubar = nullptr;                                         // N x nu (out): cotangent of the formed step's solve
    const double *thbar = nullptr;                                  // N x nth: theta-bar of the finished step
    const int32_t *status = nullptr;                                // N: its VJP status
    int32_t *status_min = nullptr;                                  // N or nullptr
    const double *xbar_fin = nullptr, *xbar_end = nullptr, *ubar_form = nullptr;   // slices of Xbar / Ubar or nullptr = zeros
    double *rbar = nullptr, *dbar = nullptr, *pbar = nullptr;       // step-major gradient arrays or nullptr
    double *x0bar = nullptr, *xhat0bar = nullptr, *uprev0bar = nullptr;            // written by the last launch
    const double *plant = nullptr, *meas = nullptr;                 // the TRUE plant's rows [f, F, G, Gd] / [h, C, Dd]
    const double *obs_dyn = nullptr, *obs_meas = nullptr, *obs_kt = nullptr;       // the handle's observer
    ThetaBlock r{nullptr, 0, 0, 1, 0, 0}, d{nullptr, 0, 0, 1, 0, 0}, p{nullptr, 0, 0, 1, 0, 0};   // k0 of the FINISHED step
    int nx = 0, nu = 0, nd = 0, ny = 0, nup = 0, nth = 0;
    int fin = -1, form = -1, T = 0;
    long long n = 0;
};

// One scenario's part of a launch: load, then (fin >= 0) finish_head with the first nx entries of theta-bar and entry()
// for every later one in theta's order, then form (form >= 0), then store.
template <int NXT>
struct AdjLane {
    static constexpr int NXA = NXT > 0 ? NXT : 32;
    double al[NXA], be[NXA];
    int nx;

    __host__ __device__ void load(const ScnAdj &A, long long i) {
        nx = NXT > 0 ? NXT : A.nx;
        if (A.fin < 0) {
            for_nx<NXT>(nx, [&](int c) { al[c] = A.xbar_end ? A.xbar_end[i * nx + c] : 0.0; be[c] = 0.0; });
            for (int l = 0; l < A.nup; l++) A.gamma[i * A.nup + l] = 0.0;
        } else {
            for_nx<NXT>(nx, [&](int c) { al[c] = A.alpha[i * nx + c]; be[c] = A.beta ? A.beta[i * nx + c] : 0.0; });
        }
    }

    // items 3 - 5: xi, eta, the direct use of d, then alpha' and beta'; th(c): entry c < nx of theta-bar
    template <class TH>
    __host__ __device__ void finish_head(const ScnAdj &A, long long i, TH &&th) {
        const bool obs = A.beta != nullptr;
        const int nu = A.nu, nd = A.nd, ny = A.ny;
        const int ps = 1 + nx + nu + nd, ms = 1 + nx + nd;
        double xi[NXA], eta[32];
        for_nx<NXT>(nx, [&](int c) { xi[c] = th(c); });
        if (obs) {
            for_nx<NXT>(nx, [&](int c) {
                double v = xi[c];
                for_nx<NXT>(nx, [&](int a) { v = fma(A.obs_dyn[a * ps + 1 + c], be[a], v); });
                xi[c] = v;
            });
            for (int j = 0; j < ny; j++) {
                double e = 0.0;
                for_nx<NXT>(nx, [&](int c) { e = fma(A.obs_kt[j * nx + c], xi[c], e); });
                eta[j] = e;
            }
        }
        if (A.dbar && A.d.w > 0) {
            const long long row = ((long long)block_col(A.d, A.fin) * A.n + i) * A.d.w;
            for (int q = 0; q < nd; q++) {
                double dl = 0.0;
                for_nx<NXT>(nx, [&](int a) { dl = fma(A.plant[a * ps + 1 + nx + nu + q], al[a], dl); });
                if (obs) {
                    for_nx<NXT>(nx, [&](int a) { dl = fma(A.obs_dyn[a * ps + 1 + nx + nu + q], be[a], dl); });
                    for (int j = 0; j < ny; j++) dl = fma(A.meas[j * ms + 1 + nx + q], eta[j], dl);
                    for (int j = 0; j < ny; j++) dl = fma(-A.obs_meas[j * ms + 1 + nx + q], eta[j], dl);
                }
                A.dbar[row + q] = A.dbar[row + q] + dl;
            }
        }
        double an[NXA], bn[NXA];
        for_nx<NXT>(nx, [&](int c) {
            double v = A.xbar_fin ? A.xbar_fin[i * nx + c] : 0.0;
            for_nx<NXT>(nx, [&](int a) { v = fma(A.plant[a * ps + 1 + c], al[a], v); });
            if (!obs) {
                v = v + xi[c];
            } else {
                for (int j = 0; j < ny; j++) v = fma(A.meas[j * ms + 1 + c], eta[j], v);
                double w = xi[c];
                for (int j = 0; j < ny; j++) w = fma(-A.obs_meas[j * ms + 1 + c], eta[j], w);
                bn[c] = w;
            }
            an[c] = v;
        });
        for_nx<NXT>(nx, [&](int c) { al[c] = an[c]; be[c] = obs ? bn[c] : 0.0; });
        if (A.status_min) {
            const int32_t s = A.status[i];
            A.status_min[i] = (A.fin == A.T - 1 || s < A.status_min[i]) ? s : A.status_min[i];
        }
    }

    // one addition into the gradient column the forward read entry q of block b from
    __host__ __device__ static void add_entry(double *bar, const ThetaBlock &b, long long n, long long i, int q, double v) {
        const long long at = ((long long)block_entry_col(b, q) * n + i) * b.w + block_entry_row(b, q);
        bar[at] = bar[at] + v;
    }

    // item 6: entry e >= nx of theta-bar, in theta's order [r-block; d-block; uprev; p-block]
    __host__ __device__ void entry(const ScnAdj &A, long long i, int e, double v) {
        const int nr = A.r.width(), ndw = A.d.width();
        int q = e - nx;
        if (q < nr) { if (A.rbar) add_entry(A.rbar, A.r, A.n, i, q, v); }
        else if ((q -= nr) < ndw) { if (A.dbar) add_entry(A.dbar, A.d, A.n, i, q, v); }
        else if ((q -= ndw) < A.nup) A.gamma[i * A.nup + q] = v;
        else if (A.pbar) add_entry(A.pbar, A.p, A.n, i, q - A.nup, v);
    }

    // item 1
    __host__ __device__ void form(const ScnAdj &A, long long i) {
        const bool obs = A.beta != nullptr;
        const int nu = A.nu, ps = 1 + nx + nu + A.nd;
        for (int l = 0; l < nu; l++) {
            double v = A.ubar_form ? A.ubar_form[i * nu + l] : 0.0;
            for_nx<NXT>(nx, [&](int a) { v = fma(A.plant[a * ps + 1 + nx + l], al[a], v); });
            if (obs) for_nx<NXT>(nx, [&](int a) { v = fma(A.obs_dyn[a * ps + 1 + nx + l], be[a], v); });
            if (l < A.nup) v = v + A.gamma[i * A.nup + l];
            A.ubar[i * nu + l] = v;
        }
    }

    __host__ __device__ void store(const ScnAdj &A, long long i) {
        const bool obs = A.beta != nullptr;
        if (A.form >= 0) {
            for_nx<NXT>(nx, [&](int c) { A.alpha[i * nx + c] = al[c]; if (obs) A.beta[i * nx + c] = be[c]; });
            return;
        }
        // x0bar = alpha (+ beta where the observer started at x); xhat0bar = beta otherwise
        const bool own = obs && A.xhat0bar != nullptr;
        if (A.x0bar) for_nx<NXT>(nx, [&](int c) { A.x0bar[i * nx + c] = (obs && !own) ? al[c] + be[c] : al[c]; });
        if (own) for_nx<NXT>(nx, [&](int c) { A.xhat0bar[i * nx + c] = be[c]; });
        if (A.uprev0bar) for (int l = 0; l < A.nup; l++) A.uprev0bar[i * A.nup + l] = A.gamma[i * A.nup + l];
        if (A.T == 0 && A.status_min) A.status_min[i] = 1;     // no step: nothing was left undifferentiated
    }
};

// the whole of one launch for scenario i on the host (the device kernel walks the same calls with theta-bar in LDS)
inline void adj_launch_host(const ScnAdj &A) {
    for (long long i = 0; i < A.n; i++) {
        AdjLane<0> L;
        L.load(A, i);
        if (A.fin >= 0) {
            const double *th = A.thbar + i * A.nth;
            L.finish_head(A, i, [&](int c) { return th[c]; });
            for (int e = A.nx; e < A.nth; e++) L.entry(A, i, e, th[e]);
        }
        if (A.form >= 0) L.form(A, i);
        L.store(A, i);
    }
}

// entries of a theta-bar record a workgroup stages at a time, and the (odd) row stride of its tile in LDS
inline int adj_tile_width(int nth) { return nth < kAdjTileMax ? nth : kAdjTileMax; }
inline int adj_tile_ld(int nth) { return adj_tile_width(nth) | 1; }

#if defined(__HIPCC__)
// One scenario per lane.  The finished step's theta-bar (N x nth records, up to 64 doubles wide) is read the way
// scn_form_theta writes theta: the workgroup's tile entry by entry, consecutive lanes on consecutive addresses, through
// LDS; a lane then takes its own row from there.  Records wider than kAdjTileMax go through in column slices of that
// width, so the tile stays below 68 KB and two workgroups share a CU.  Dynamic LDS: 256 * ld doubles.
template <int NXT>
__global__ __launch_bounds__(kAdjBlock) void scenario_adjoint_kernel(ScnAdj A, int tw, int ld) {
    extern __shared__ double adj_lds[];
    const long long base = (long long)blockIdx.x * kAdjBlock;
    const long long i = base + threadIdx.x;
    const bool live = i < A.n;
    AdjLane<NXT> L;
    if (live) L.load(A, i);
    if (A.fin >= 0) {
        const long long left = A.n - base;
        const int rows = left < kAdjBlock ? (int)left : kAdjBlock;
        const double *mine = adj_lds + threadIdx.x * ld;
        for (int c0 = 0; c0 < A.nth; c0 += tw) {
            const int cw = A.nth - c0 < tw ? A.nth - c0 : tw;
            if (c0 > 0) __syncthreads();
            // (row, column) of the element a lane copies, walked in steps of the workgroup: one division per slice
            const int dr = kAdjBlock / cw, dc = kAdjBlock - dr * cw;
            for (int sl = threadIdx.x / cw, e = threadIdx.x - sl * cw; sl < rows; sl += dr) {
                adj_lds[sl * ld + e] = A.thbar[(base + sl) * A.nth + c0 + e];
                e += dc;
                if (e >= cw) { e -= cw; sl++; }
            }
            __syncthreads();
            if (live) {
                if (c0 == 0) L.finish_head(A, i, [&](int c) { return mine[c]; });
                for (int e = c0 > L.nx ? c0 : L.nx; e < c0 + cw; e++) L.entry(A, i, e, mine[e - c0]);
            }
        }
    }
    if (live) {
        if (A.form >= 0) L.form(A, i);
        L.store(A, i);
    }
}
#endif

}  // namespace lmpc
