// Sensitivity of the batched solve: the derivative of x*(theta) on the affine piece the solver reported, per point.
// The arithmetic on K_A -- factor, substitutions, the tail of theta-bar -- stands here once per form for every
// derivative kernel (lmpc_pack_grad_kernel.hpp calls it too): the register form (sens_factor, sens_subst, sens_tail)
// serves the lane kernels and the host twins, the wavefront form (sens_wave_*) spreads the same operations over the
// lanes of a wavefront, in the same order per value.  The arithmetic contract is stated in include/lmpc_hip.h
// ("Differentiable solve") and restated in numpy in tests/sens_reference.py.  Internal to liblmpc_hip.so.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LMPC_SENS_HD __host__ __device__
#else
#define LMPC_SENS_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define LMPC_SENS_UNROLL _Pragma("unroll")
#else
#define LMPC_SENS_UNROLL
#endif

namespace lmpc {

constexpr int kSensMaxSet = 64;             // rows of an active set the kernels hold (one per lane of a wavefront)
constexpr int kSensCaps[] = {5, 8};         // CAP of the sens_lane_kernel instantiations built
constexpr int kSensBlock = 256;             // workgroup of the lane kernel
constexpr int kSensLd = kSensMaxSet + 1;    // row stride of the wavefront kernel's factor in LDS (odd: no bank conflicts down a column)
constexpr size_t kSensStageMax = 48 * 1024; // the derived pack is staged in LDS up to this many bytes
constexpr int kSensStageOutMax = 16;        // results of up to this many doubles per point leave the lane kernel through LDS
constexpr size_t kSensLdsMax = 64 * 1024;   // ... while the workgroup's LDS stays within this

enum : int32_t { SENS_DONE = 1, SENS_FAILED_POINT = 0, SENS_SINGULAR = -1, SENS_TOO_MANY = -7,
                 SENS_QUEUED = 2 };         // (sens_classify's, never a point's status)

// The derived pack, one block of doubles: [G: packed triangle of M M', tri(m)] [P = M Rout', m x nout] [Dth, m x nth]
// [Xth, nout x nth] [soft: 1.0 on SOFT rows, else 0.0, m]
struct SensDims { int m = 0, nth = 0, nout = 0, words = 0; };
LMPC_SENS_HD inline size_t sens_tri(size_t a) { return a * (a + 1) / 2; }
LMPC_SENS_HD inline size_t sens_pack_doubles(const SensDims &d) {
    return sens_tri((size_t)d.m) + (size_t)d.m * d.nout + (size_t)d.m * d.nth + (size_t)d.nout * d.nth + (size_t)d.m;
}
struct SensView {
    const double *G, *P, *Dth, *Xth, *soft;
    int nth, nout;
    double rho, zero_tol;
};
LMPC_SENS_HD inline SensView sens_view(const double *C, const SensDims &d, double rho, double zero_tol) {
    SensView v;
    v.G = C;
    v.P = v.G + sens_tri((size_t)d.m);
    v.Dth = v.P + (size_t)d.m * d.nout;
    v.Xth = v.Dth + (size_t)d.m * d.nth;
    v.soft = v.Xth + (size_t)d.nout * d.nth;
    v.nth = d.nth; v.nout = d.nout; v.rho = rho; v.zero_tol = zero_tol;
    return v;
}

// 64 bits of a mask of `words` words from bit `pos` on (bits beyond the mask read as 0)
LMPC_SENS_HD inline uint64_t sens_bits(const uint64_t *mask, int words, int pos) {
    const int w = pos >> 6, s = pos & 63;
    uint64_t lo = w < words ? mask[w] : 0;
    if (s == 0) return lo;
    const uint64_t hi = w + 1 < words ? mask[w + 1] : 0;
    return (lo >> s) | (hi << (64 - s));
}
// rows 64 rw .. 64 rw + 63 of the active set: a row counts once whether its upper bit (j), its lower bit (m + j) or both are set
LMPC_SENS_HD inline uint64_t sens_rows(const uint64_t *mask, int words, int m, int rw) {
    const int left = m - 64 * rw;
    const uint64_t valid = left >= 64 ? ~0ull : ((1ull << left) - 1);
    return (sens_bits(mask, words, 64 * rw) | sens_bits(mask, words, m + 64 * rw)) & valid;
}
LMPC_SENS_HD inline int sens_popc(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(u);
#else
    return __builtin_popcountll(u);
#endif
}
LMPC_SENS_HD inline int sens_ctz(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)u) - 1;
#else
    return __builtin_ctzll(u);
#endif
}
// |A| and its first CAP rows in ascending order
template <int CAP>
LMPC_SENS_HD inline int sens_active_rows(const uint64_t *mask, int words, int m, int *a) {
    int k = 0;
    for (int rw = 0; 64 * rw < m; rw++) {
        uint64_t u = sens_rows(mask, words, m, rw);
        const int c = sens_popc(u);
        if (k < CAP) {
            int q = k;
            while (u && q < CAP) {
                const int j = sens_ctz(u);
                LMPC_SENS_UNROLL
                for (int i = 0; i < CAP; i++) if (i == q) a[i] = 64 * rw + j;
                q++; u &= u - 1;
            }
        }
        k += c;
    }
    return k;
}

// K_A = L D L' of a set of k <= CAP rows a[0] < a[1] < ..., factored without pivoting in that order: L[i][j], i > j, at
// L[i (i - 1) / 2 + j], and the reciprocals of the pivots.  Every loop of the register form has compile-time bounds and
// predicates on k, so that on the device the factor and the right-hand sides live in registers.
template <int CAP>
struct SensFactor { double L[CAP * (CAP - 1) / 2 + 1], rD[CAP]; };

// SENS_DONE, or SENS_SINGULAR at the first pivot below zero_tol
template <int CAP>
LMPC_SENS_HD inline int sens_factor(const SensView &S, const int *a, int k, SensFactor<CAP> &F) {
    double D[CAP], c[CAP];
    auto &L = F.L;
    auto &rD = F.rD;
    LMPC_SENS_UNROLL
    for (int j = 0; j < CAP; j++) {
        if (j < k) {
            LMPC_SENS_UNROLL
            for (int p = 0; p < j; p++) c[p] = L[j * (j - 1) / 2 + p] * D[p];
            LMPC_SENS_UNROLL
            for (int i = j; i < CAP; i++) {
                if (i < k) {
                    double v = S.G[sens_tri((size_t)a[i]) + a[j]];
                    if (i == j && S.soft[a[j]] != 0.0) v = v + S.rho;
                    LMPC_SENS_UNROLL
                    for (int p = 0; p < j; p++) v = fma(-L[i * (i - 1) / 2 + p], c[p], v);
                    if (i == j) {
                        if (v < S.zero_tol) return SENS_SINGULAR;
                        D[j] = v;
                        rD[j] = 1.0 / v;
                    } else {
                        L[i * (i - 1) / 2 + j] = v * rD[j];
                    }
                }
            }
        }
    }
    return SENS_DONE;
}

// NR right-hand sides side by side, each in the contract's order: L z = w (columns ascending), z = z / D through the
// stored reciprocals, L' y = z (columns descending)
template <int CAP, int NR>
LMPC_SENS_HD inline void sens_subst(const SensFactor<CAP> &F, int k, double (&z)[NR][CAP]) {
    LMPC_SENS_UNROLL
    for (int i = 1; i < CAP; i++) {
        if (i < k) {
            LMPC_SENS_UNROLL
            for (int p = 0; p < i; p++) {
                LMPC_SENS_UNROLL
                for (int r = 0; r < NR; r++) z[r][i] = fma(-F.L[i * (i - 1) / 2 + p], z[r][p], z[r][i]);
            }
        }
    }
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) {
        LMPC_SENS_UNROLL
        for (int r = 0; r < NR; r++) if (i < k) z[r][i] = z[r][i] * F.rD[i];
    }
    LMPC_SENS_UNROLL
    for (int i = CAP - 2; i >= 0; i--) {
        if (i < k) {
            LMPC_SENS_UNROLL
            for (int p = CAP - 1; p > i; p--) {
                LMPC_SENS_UNROLL
                for (int r = 0; r < NR; r++) if (p < k) z[r][i] = fma(-F.L[p * (p - 1) / 2 + i], z[r][p], z[r][i]);
            }
        }
    }
}

// w = P_A xbar, zeros beyond the set
template <int CAP>
LMPC_SENS_HD inline void sens_rhs(const SensView &S, const int *a, int k, const double *xbar, double *w) {
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) w[i] = 0.0;
    for (int q = 0; q < S.nout; q++) {
        const double xb = xbar[q];
        LMPC_SENS_UNROLL
        for (int i = 0; i < CAP; i++) if (i < k) w[i] = fma(S.P[(size_t)a[i] * S.nout + q], xb, w[i]);
    }
}
// row `row` of P xbar, and column t of Xth' xbar
LMPC_SENS_HD inline double sens_p_dot(const SensView &S, int row, const double *xbar) {
    double w = 0.0;
    for (int q = 0; q < S.nout; q++) w = fma(S.P[(size_t)row * S.nout + q], xbar[q], w);
    return w;
}
LMPC_SENS_HD inline double sens_xth_dot(const SensView &S, const double *xbar, int t) {
    double acc = 0.0;
    for (int q = 0; q < S.nout; q++) acc = fma(S.Xth[(size_t)q * S.nth + t], xbar[q], acc);
    return acc;
}
// acc + sum over the set of Dth[a_i][t] y_i
template <int CAP>
LMPC_SENS_HD inline double sens_tail(const SensView &S, const int *a, int k, const double *y, int t, double acc) {
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) if (i < k) acc = fma(S.Dth[(size_t)a[i] * S.nth + t], y[i], acc);
    return acc;
}

// One point with |A| = k <= CAP: the VJP of xbar (JAC false: out = nth values) or the Jacobian (JAC true: out = nout x
// nth, xbar not read).  Returns the status; out is written only with SENS_DONE.
template <int CAP, bool JAC>
LMPC_SENS_HD inline int sens_point(const SensView &S, const int *a, int k, const double *xbar, double *out) {
    SensFactor<CAP> F;
    if (sens_factor<CAP>(S, a, k, F) != SENS_DONE) return SENS_SINGULAR;
    double z[1][CAP];
    const int nrhs = JAC ? S.nout : 1;
    for (int r = 0; r < nrhs; r++) {
        // (the Jacobian's xbar = e_r: the products with its exact zeros and its one are left out)
        if (JAC) {
            LMPC_SENS_UNROLL
            for (int i = 0; i < CAP; i++) z[0][i] = i < k ? S.P[(size_t)a[i] * S.nout + r] : 0.0;
        } else {
            sens_rhs<CAP>(S, a, k, xbar, z[0]);
        }
        sens_subst<CAP, 1>(F, k, z);
        for (int t = 0; t < S.nth; t++)
            out[(size_t)r * S.nth + t] = sens_tail<CAP>(S, a, k, z[0], t, JAC ? S.Xth[(size_t)r * S.nth + t] : sens_xth_dot(S, xbar, t));
    }
    return SENS_DONE;
}

// What becomes of a point at a capacity of `cap` rows: its final status, SENS_QUEUED (left to the wavefront kernel) or
// SENS_DONE (to be solved by the caller)
LMPC_SENS_HD inline int sens_classify(int flag, int k, int cap) {
    if (flag < 1) return SENS_FAILED_POINT;
    if (k > kSensMaxSet) return SENS_TOO_MANY;
    return k > cap ? SENS_QUEUED : SENS_DONE;
}

// What one call's two launches are told
struct SensArgs {
    const double *C = nullptr;          // derived pack (global memory)
    SensDims d{};
    double rho = 0.0, zero_tol = 0.0;
    long long N = 0;
    const uint64_t *active = nullptr;
    const int32_t *flag = nullptr;
    const double *xbar = nullptr;       // VJP only
    double *out = nullptr;              // N x nth (VJP) or N x nout x nth (Jacobian)
    int32_t *status = nullptr;          // may be NULL
    int32_t *list = nullptr, *count = nullptr;
    int cap = 0;                        // points with |A| beyond it go to the list (0 <= cap <= CAP; below CAP: a forced list pass)
    int staged = 0;                     // the derived pack is copied to LDS first
    int stage_out = 0;                  // results of the lane kernel leave through LDS, as whole lines
};

#if defined(__HIPCC__)

// The lane kernels' shared ends.  The derived pack: where it is read from, after the workgroup has copied it to LDS
// if `staged`
__device__ inline const double *sens_stage_pack(const double *C, const SensDims &d, int staged, double *lds) {
    if (!staged) return C;
    const int nd = (int)sens_pack_doubles(d);
    for (int i = threadIdx.x; i < nd; i += blockDim.x) lds[i] = C[i];
    __syncthreads();
    return lds;
}
// ... and the queued points of a wavefront appended to the list with one atomic (ballot + mbcnt)
__device__ inline void sens_append(bool queued, long long p, int32_t *list, int32_t *count) {
    const unsigned long long q = __ballot(queued);
    if (!q) return;
    const int leader = __ffsll(q) - 1;
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(q >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)q, 0u));
    int slot = 0;
    if ((int)__lane_id() == leader) slot = atomicAdd(count, (int)__popcll(q));
    slot = __shfl(slot, leader);
    if (queued) list[slot + (int)below] = (int32_t)p;
}

// The wavefront form: one listed point per wavefront (a workgroup is one wavefront), position i of the set on lane i.
// K_A is gathered into LDS and factored in place, left-looking: at column j lane i forms its entry with the sum over
// the columns before in ascending order, reading row j and the pivots as LDS broadcasts; the pivot of the column goes
// round by readlane.  The substitutions run column by column with the column's value broadcast by readlane, so that
// every lane accumulates in the contract's order.
struct alignas(16) SensWaveLds {
    double Lm[kSensMaxSet * kSensLd];       // the factor, row i at Lm[i * kSensLd]
    double Ds[kSensMaxSet], ys[kSensMaxSet];
    int idx[kSensMaxSet];                   // the set's rows
};
static_assert(sizeof(SensWaveLds) == 34560, "four one-wavefront workgroups per CU");

// |A| of the point, and the row at position `lane` of the set (0 beyond it)
__device__ inline int sens_wave_rows(const uint64_t *mask, const SensDims &d, int lane, int *mine) {
    int k = 0;
    *mine = 0;
    for (int rw = 0; 64 * rw < d.m; rw++) {
        uint64_t u = sens_rows(mask, d.words, d.m, rw);
        while (u) {
            if (k == lane) *mine = 64 * rw + sens_ctz(u);
            k++; u &= u - 1;
        }
    }
    return k;
}

// Gather and factor of a set of k <= 64 rows; false at the first pivot below zero_tol.  *rD: the reciprocal of the
// lane's pivot (0 beyond the set).
__device__ inline bool sens_wave_factor(SensWaveLds &W, const SensView &S, int lane, int mine, int k, double *rD) {
    const bool in = lane < k;
    __syncthreads();
    W.idx[lane] = mine;
    __syncthreads();
    if (in)
        for (int j = 0; j <= lane; j++) {
            double v = S.G[sens_tri((size_t)mine) + W.idx[j]];
            if (j == lane && S.soft[mine] != 0.0) v = v + S.rho;
            W.Lm[lane * kSensLd + j] = v;
        }
    __syncthreads();
    for (int j = 0; j < k; j++) {
        double v = 0.0;
        if (in && lane >= j) {
            v = W.Lm[lane * kSensLd + j];
            for (int q = 0; q < j; q++) {
                const double c = W.Lm[j * kSensLd + q] * W.Ds[q];
                v = fma(-W.Lm[lane * kSensLd + q], c, v);
            }
        }
        const double dj = __shfl(v, j);
        if (dj < S.zero_tol) return false;
        const double r = 1.0 / dj;
        if (lane == j) W.Ds[j] = dj;
        if (in && lane > j) W.Lm[lane * kSensLd + j] = v * r;
        __syncthreads();
    }
    *rD = in ? 1.0 / W.Ds[lane] : 0.0;
    return true;
}

// NR right-hand sides side by side, the lane's value of each in z
template <int NR>
__device__ inline void sens_wave_subst(const SensWaveLds &W, int lane, int k, double rD, double (&z)[NR]) {
    for (int q = 0; q + 1 < k; q++) {
        double zq[NR];
        for (int r = 0; r < NR; r++) zq[r] = __shfl(z[r], q);
        if (lane < k && lane > q)
            for (int r = 0; r < NR; r++) z[r] = fma(-W.Lm[lane * kSensLd + q], zq[r], z[r]);
    }
    for (int r = 0; r < NR; r++) z[r] = z[r] * rD;
    for (int q = k - 1; q >= 1; q--) {
        double yq[NR];
        for (int r = 0; r < NR; r++) yq[r] = __shfl(z[r], q);
        if (lane < q)
            for (int r = 0; r < NR; r++) z[r] = fma(-W.Lm[q * kSensLd + lane], yq[r], z[r]);
    }
}

// out[t] = (JAC ? Xth[r][t] : column t of Xth' xb) + sum over the set of Dth[a_i][t] y_i, t over the lanes; y: the
// lane's value
template <bool JAC>
__device__ inline void sens_wave_tail(SensWaveLds &W, const SensView &S, int lane, int k, double y, const double *xb, int r, double *out) {
    __syncthreads();
    W.ys[lane] = y;
    __syncthreads();
    for (int t = lane; t < S.nth; t += 64) {
        double acc = JAC ? S.Xth[(size_t)r * S.nth + t] : sens_xth_dot(S, xb, t);
        for (int i = 0; i < k; i++) acc = fma(S.Dth[(size_t)W.idx[i] * S.nth + t], W.ys[i], acc);
        out[t] = acc;
    }
}

#endif  // __HIPCC__

#if defined(__HIPCC__) && defined(LMPC_SENS_KERNELS)

// One point per lane.  Points with |A| <= cap are finished here, in registers; failed points and sets beyond the 64
// rows get zeros and their status; the rest is appended to `list`.
template <int CAP, bool JAC>
__global__ __launch_bounds__(kSensBlock) void sens_lane_kernel(SensArgs A) {
    extern __shared__ double sens_lds[];
    const SensDims d = A.d;
    const SensView S = sens_view(sens_stage_pack(A.C, d, A.staged, sens_lds), d, A.rho, A.zero_tol);
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = JAC ? (size_t)d.nout * d.nth : (size_t)d.nth;
    int a[CAP];
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) a[i] = 0;
    bool queued = false;
    // short results go through LDS and leave as whole lines (a lane's own `per` doubles lie `per` apart in memory: stored
    // from the lanes they would touch every line of the workgroup's block once per value)
    double *const tile = sens_lds + (A.staged ? sens_pack_doubles(d) : 0);
    double *const mine = A.stage_out ? tile + (size_t)threadIdx.x * per : A.out + (size_t)p * per;
    if (p < A.N) {
        const int k = sens_active_rows<CAP>(A.active + (size_t)p * d.words, d.words, d.m, a);
        int st = sens_classify(A.flag[p], k, A.cap);
        queued = st == SENS_QUEUED;
        if (st == SENS_DONE) st = sens_point<CAP, JAC>(S, a, k, JAC ? nullptr : A.xbar + (size_t)p * d.nout, mine);
        if (!queued) {
            if (st != SENS_DONE)
                for (size_t i = 0; i < per; i++) mine[i] = 0.0;
            if (A.status) A.status[p] = st;
        }
    }
    if (A.stage_out) {
        // (a queued point's row is the wavefront kernel's to write)
        int *const skip = reinterpret_cast<int *>(tile + (size_t)blockDim.x * per);
        skip[threadIdx.x] = queued;
        __syncthreads();
        const long long base = (long long)blockIdx.x * blockDim.x;
        const long long left = A.N - base;
        const int nb = left < (long long)blockDim.x ? (int)left : (int)blockDim.x;
        const int total = nb * (int)per;
        for (int i = threadIdx.x; i < total; i += blockDim.x)
            if (!skip[i / (int)per]) A.out[(size_t)base * per + i] = tile[i];
    }
    sens_append(queued, p, A.list, A.count);
}

// The listed points, by a persistent grid that reads the list's length on the device
template <bool JAC>
__global__ __launch_bounds__(64) void sens_wave_kernel(SensArgs A) {
    __shared__ SensWaveLds W;
    const SensDims d = A.d;
    const SensView S = sens_view(A.C, d, A.rho, A.zero_tol);
    const int lane = threadIdx.x;
    const size_t per = JAC ? (size_t)d.nout * d.nth : (size_t)d.nth;
    const int cnt = *A.count;
    for (int e = blockIdx.x; e < cnt; e += gridDim.x) {
        const long long p = A.list[e];
        int mine;
        const int k = sens_wave_rows(A.active + (size_t)p * d.words, d, lane, &mine);
        double *out = A.out + (size_t)p * per;
        double rD = 0.0;
        // (a set beyond the 64 rows is never listed; refused so that no lane index can leave them)
        const int st = k > kSensMaxSet ? SENS_TOO_MANY : sens_wave_factor(W, S, lane, mine, k, &rD) ? SENS_DONE : SENS_SINGULAR;
        if (A.status && lane == 0) A.status[p] = st;
        if (st != SENS_DONE) {
            for (size_t i = lane; i < per; i += 64) out[i] = 0.0;
            continue;
        }
        const double *xb = JAC ? nullptr : A.xbar + (size_t)p * d.nout;
        const int nrhs = JAC ? d.nout : 1;
        for (int r = 0; r < nrhs; r++) {
            double z[1] = {0.0};
            if (lane < k) z[0] = JAC ? S.P[(size_t)mine * d.nout + r] : sens_p_dot(S, mine, xb);
            sens_wave_subst<1>(W, lane, k, rD, z);
            sens_wave_tail<JAC>(W, S, lane, k, z[0], xb, r, out + (size_t)r * d.nth);
        }
    }
}

#endif  // __HIPCC__ && LMPC_SENS_KERNELS

}  // namespace lmpc
