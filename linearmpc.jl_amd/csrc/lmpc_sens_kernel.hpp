// Sensitivity of the batched solve: the derivative of x*(theta) on the affine piece the solver reported, per point.
// One copy of the per-point arithmetic (sens_point) serves the lane kernel and the host twin; the wavefront kernel
// spreads the same operations over the lanes of a wavefront, in the same order per value.  The arithmetic contract is
// stated in include/lmpc_hip.h ("Differentiable solve") and restated in numpy in tests/sens_reference.py.
// Internal to liblmpc_hip.so.
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

enum : int32_t { SENS_DONE = 1, SENS_FAILED_POINT = 0, SENS_SINGULAR = -1, SENS_TOO_MANY = -7 };

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

// One point with |A| = k <= CAP, rows a[0] < a[1] < ...: factor K_A = L D L' without pivoting in that order, then the
// VJP of xbar (JAC false: out = nth values) or the Jacobian (JAC true: out = nout x nth, xbar not read).  Returns the
// status; out is written only with SENS_DONE.  Every loop has compile-time bounds and predicates on k, so that on the
// device the factor lives in registers.
template <int CAP, bool JAC>
LMPC_SENS_HD inline int sens_point(const SensView &S, const int *a, int k, const double *xbar, double *out) {
    constexpr int NL = CAP * (CAP - 1) / 2 + 1;
    double L[NL], D[CAP], rD[CAP], c[CAP], z[CAP];
    // L[i][j], i > j, at L[i (i - 1) / 2 + j]
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
    const int nrhs = JAC ? S.nout : 1;
    for (int r = 0; r < nrhs; r++) {
        // w = P_A xbar (the Jacobian's xbar = e_r: the products with its exact zeros and its one are left out)
        if (JAC) {
            LMPC_SENS_UNROLL
            for (int i = 0; i < CAP; i++) z[i] = i < k ? S.P[(size_t)a[i] * S.nout + r] : 0.0;
        } else {
            LMPC_SENS_UNROLL
            for (int i = 0; i < CAP; i++) z[i] = 0.0;
            for (int q = 0; q < S.nout; q++) {
                const double xb = xbar[q];
                LMPC_SENS_UNROLL
                for (int i = 0; i < CAP; i++) if (i < k) z[i] = fma(S.P[(size_t)a[i] * S.nout + q], xb, z[i]);
            }
        }
        // L z = w (columns ascending), z = z / D through the stored reciprocals, L' y = z (columns descending)
        LMPC_SENS_UNROLL
        for (int i = 1; i < CAP; i++) {
            if (i < k) {
                LMPC_SENS_UNROLL
                for (int p = 0; p < i; p++) z[i] = fma(-L[i * (i - 1) / 2 + p], z[p], z[i]);
            }
        }
        LMPC_SENS_UNROLL
        for (int i = 0; i < CAP; i++) if (i < k) z[i] = z[i] * rD[i];
        LMPC_SENS_UNROLL
        for (int i = CAP - 2; i >= 0; i--) {
            if (i < k) {
                LMPC_SENS_UNROLL
                for (int p = CAP - 1; p > i; p--) if (p < k) z[i] = fma(-L[p * (p - 1) / 2 + i], z[p], z[i]);
            }
        }
        for (int t = 0; t < S.nth; t++) {
            double acc;
            if (JAC) {
                acc = S.Xth[(size_t)r * S.nth + t];
            } else {
                acc = 0.0;
                for (int q = 0; q < S.nout; q++) acc = fma(S.Xth[(size_t)q * S.nth + t], xbar[q], acc);
            }
            LMPC_SENS_UNROLL
            for (int i = 0; i < CAP; i++) if (i < k) acc = fma(S.Dth[(size_t)a[i] * S.nth + t], z[i], acc);
            out[(size_t)r * S.nth + t] = acc;
        }
    }
    return SENS_DONE;
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

#if defined(__HIPCC__) && defined(LMPC_SENS_KERNELS)

// One point per lane.  Points with |A| <= cap are finished here, in registers; failed points and sets beyond the 64
// rows get zeros and their status; the rest is appended to `list` with one atomic per wavefront (ballot + mbcnt).
template <int CAP, bool JAC>
__global__ __launch_bounds__(kSensBlock) void sens_lane_kernel(SensArgs A) {
    extern __shared__ double sens_lds[];
    const SensDims d = A.d;
    if (A.staged) {
        const int nd = (int)sens_pack_doubles(d);
        for (int i = threadIdx.x; i < nd; i += blockDim.x) sens_lds[i] = A.C[i];
        __syncthreads();
    }
    const SensView S = sens_view(A.staged ? sens_lds : A.C, d, A.rho, A.zero_tol);
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < A.N;
    const size_t per = JAC ? (size_t)d.nout * d.nth : (size_t)d.nth;
    int a[CAP];
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) a[i] = 0;
    int st = SENS_FAILED_POINT, k = 0;
    bool queued = false;
    // short results go through LDS and leave as whole lines (a lane's own `per` doubles lie `per` apart in memory: stored
    // from the lanes they would touch every line of the workgroup's block once per value)
    double *const tile = sens_lds + (A.staged ? sens_pack_doubles(d) : 0);
    double *const mine = A.stage_out ? tile + (size_t)threadIdx.x * per : A.out + (size_t)p * per;
    if (live) {
        k = sens_active_rows<CAP>(A.active + (size_t)p * d.words, d.words, d.m, a);
        if (A.flag[p] < 1) st = SENS_FAILED_POINT;
        else if (k > kSensMaxSet) st = SENS_TOO_MANY;
        else if (k > A.cap) queued = true;
        else st = sens_point<CAP, JAC>(S, a, k, JAC ? nullptr : A.xbar + (size_t)p * d.nout, mine);
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
    const unsigned long long q = __ballot(queued);
    if (q) {
        const int leader = __ffsll(q) - 1;
        const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(q >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)q, 0u));
        int slot = 0;
        if ((int)__lane_id() == leader) slot = atomicAdd(A.count, (int)__popcll(q));
        slot = __shfl(slot, leader);
        if (queued) A.list[slot + (int)below] = (int32_t)p;
    }
}

// One listed point per wavefront (a workgroup is one wavefront), position i of the set on lane i; a persistent grid that
// reads the list's length on the device.  K_A is gathered into LDS and factored in place, left-looking: at column j
// lane i forms its entry with the sum over the columns before in ascending order, reading row j and the pivots as LDS
// broadcasts; the pivot of the column goes round by readlane.  The substitutions run column by column with the
// column's value broadcast by readlane, so that every lane accumulates in the contract's order.
template <bool JAC>
__global__ __launch_bounds__(64) void sens_wave_kernel(SensArgs A) {
    __shared__ double Lm[kSensMaxSet * kSensLd];
    __shared__ double Ds[kSensMaxSet], ys[kSensMaxSet];
    __shared__ int idx[kSensMaxSet];
    const SensDims d = A.d;
    const SensView S = sens_view(A.C, d, A.rho, A.zero_tol);
    const int lane = threadIdx.x;
    const size_t per = JAC ? (size_t)d.nout * d.nth : (size_t)d.nth;
    const int cnt = *A.count;
    for (int e = blockIdx.x; e < cnt; e += gridDim.x) {
        const long long p = A.list[e];
        const uint64_t *mask = A.active + (size_t)p * d.words;
        int mine = 0, k = 0;
        for (int rw = 0; 64 * rw < d.m; rw++) {
            uint64_t u = sens_rows(mask, d.words, d.m, rw);
            while (u) {
                if (k == lane) mine = 64 * rw + sens_ctz(u);
                k++; u &= u - 1;
            }
        }
        double *out = A.out + (size_t)p * per;
        if (k > kSensMaxSet) {          // (never listed; kept so that no lane index can leave the 64 rows)
            for (size_t i = lane; i < per; i += 64) out[i] = 0.0;
            if (A.status && lane == 0) A.status[p] = SENS_TOO_MANY;
            continue;
        }
        const bool in = lane < k;
        __syncthreads();
        idx[lane] = mine;
        __syncthreads();
        if (in)
            for (int j = 0; j <= lane; j++) {
                double v = S.G[sens_tri((size_t)mine) + idx[j]];
                if (j == lane && S.soft[mine] != 0.0) v = v + S.rho;
                Lm[lane * kSensLd + j] = v;
            }
        __syncthreads();
        bool ok = true;
        for (int j = 0; j < k; j++) {
            double v = 0.0;
            if (in && lane >= j) {
                v = Lm[lane * kSensLd + j];
                for (int q = 0; q < j; q++) {
                    const double c = Lm[j * kSensLd + q] * Ds[q];
                    v = fma(-Lm[lane * kSensLd + q], c, v);
                }
            }
            const double dj = __shfl(v, j);
            if (dj < S.zero_tol) { ok = false; break; }
            const double r = 1.0 / dj;
            if (lane == j) Ds[j] = dj;
            if (in && lane > j) Lm[lane * kSensLd + j] = v * r;
            __syncthreads();
        }
        if (!ok) {
            for (size_t i = lane; i < per; i += 64) out[i] = 0.0;
            if (A.status && lane == 0) A.status[p] = SENS_SINGULAR;
            continue;
        }
        const double rD = in ? 1.0 / Ds[lane] : 0.0;
        const double *xb = JAC ? nullptr : A.xbar + (size_t)p * d.nout;
        const int nrhs = JAC ? d.nout : 1;
        for (int r = 0; r < nrhs; r++) {
            double z = 0.0;
            if (in) {
                if (JAC) z = S.P[(size_t)mine * d.nout + r];
                else
                    for (int q = 0; q < d.nout; q++) z = fma(S.P[(size_t)mine * d.nout + q], xb[q], z);
            }
            for (int q = 0; q + 1 < k; q++) {
                const double zq = __shfl(z, q);
                if (in && lane > q) z = fma(-Lm[lane * kSensLd + q], zq, z);
            }
            z = z * rD;
            for (int q = k - 1; q >= 1; q--) {
                const double yq = __shfl(z, q);
                if (lane < q) z = fma(-Lm[q * kSensLd + lane], yq, z);
            }
            __syncthreads();
            ys[lane] = z;
            __syncthreads();
            for (int t = lane; t < d.nth; t += 64) {
                double acc;
                if (JAC) {
                    acc = S.Xth[(size_t)r * d.nth + t];
                } else {
                    acc = 0.0;
                    for (int q = 0; q < d.nout; q++) acc = fma(S.Xth[(size_t)q * d.nth + t], xb[q], acc);
                }
                for (int i = 0; i < k; i++) acc = fma(S.Dth[(size_t)idx[i] * d.nth + t], ys[i], acc);
                out[(size_t)r * d.nth + t] = acc;
            }
        }
        if (A.status && lane == 0) A.status[p] = SENS_DONE;
    }
}

#endif  // __HIPCC__ && LMPC_SENS_KERNELS

}  // namespace lmpc
