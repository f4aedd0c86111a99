// Gradient of the batched solve with respect to the pack (M, du, dl, Dth, Rout, x0, Xth), summed over the batch.
// Stage 1 (pack_grad_lane_kernel / pack_grad_wave_kernel) solves two right-hand sides on the factor of K_A per point
// and leaves the record [lambda | y]; stage 2 (pack_grad_reduce_kernel) forms every point's contributions, one point
// per lane, and sums the 64 points of a wavefront in the contract's pairing; pack_grad_tree_kernel sums the partials
// pairwise.  The arithmetic contract is stated in include/lmpc_hip.h ("Gradient with respect to the pack") and
// restated in numpy in tests/pack_grad_reference.py.  The factor and the substitutions are those of
// lmpc_sens_kernel.hpp, operation for operation.  Internal to liblmpc_hip.so.
#pragma once

#include "lmpc_sens_kernel.hpp"

namespace lmpc {

constexpr int kPackGradBlock = 256;                 // workgroup of the lane, reduce and tree kernels
constexpr int kPackGradFan = 32;                    // partials one thread of the tree kernel sums per launch
constexpr int kPackGradSlabMin = 8, kPackGradSlabMax = 20;     // log2 of the points of a slab
constexpr size_t kPackGradBudget = 64u << 20;       // bytes of records + partials the default slab stays within
constexpr size_t kPackGradStageMax = 48 * 1024;     // M and Rout are staged in LDS by the reduce kernel up to this many bytes

// The sums in the order the reduce kernel emits them (one partial = pack_grad_doubles values):
//   per column c of M:  Rout-bar[q][c] (q = 0 .. nout - 1), M-bar[j][c] (j = 0 .. m - 1)
//   per row j:          du-bar[j], dl-bar[j], Dth-bar[j][t] (t = 0 .. nth - 1)
//   per output q:       x0-bar[q], Xth-bar[q][t]
struct PackGradDims { int n = 0, m = 0, nth = 0, nout = 0; };
LMPC_SENS_HD inline size_t pack_grad_doubles(const PackGradDims &d) {
    return (size_t)d.n * (d.nout + d.m) + (size_t)d.m * (2 + d.nth) + (size_t)d.nout * (1 + d.nth);
}
enum { PG_M = 0, PG_DU, PG_DL, PG_DTH, PG_ROUT, PG_X0, PG_XTH, PG_ARRAYS };
struct PackGradOut { double *p[PG_ARRAYS] = {}; };
// emitted position e -> output array and row-major index in it
LMPC_SENS_HD inline int pack_grad_locate(const PackGradDims &d, size_t e, size_t *idx) {
    const size_t perc = (size_t)d.nout + d.m, nc = (size_t)d.n * perc;
    if (e < nc) {
        const size_t c = e / perc, r = e % perc;
        if (r < (size_t)d.nout) { *idx = r * d.n + c; return PG_ROUT; }
        *idx = (r - d.nout) * d.n + c;
        return PG_M;
    }
    e -= nc;
    const size_t perj = 2 + (size_t)d.nth, nj = (size_t)d.m * perj;
    if (e < nj) {
        const size_t j = e / perj, r = e % perj;
        if (r == 0) { *idx = j; return PG_DU; }
        if (r == 1) { *idx = j; return PG_DL; }
        *idx = j * d.nth + (r - 2);
        return PG_DTH;
    }
    e -= nj;
    const size_t perq = 1 + (size_t)d.nth, q = e / perq, r = e % perq;
    if (r == 0) { *idx = q; return PG_X0; }
    *idx = q * d.nth + (r - 1);
    return PG_XTH;
}

// 1 if row j is active at its upper side (a row with both bits counts as upper)
LMPC_SENS_HD inline int pack_grad_upper(const uint64_t *mask, int j) { return (int)((mask[j >> 6] >> (j & 63)) & 1); }

// One point with |A| = k <= CAP: the factor of sens_point, then lambda = K_A^-1 d and y = K_A^-1 (P_A xbar) by the same
// forward, diagonal and backward order, and thbar (where asked for) as sens_point forms it.  lam and y are written for
// i < k only with SENS_DONE.
template <int CAP>
LMPC_SENS_HD inline int pack_grad_point(const SensView &S, const double *du, const double *dl, const uint64_t *mask, const int *a,
                                        int k, const double *theta, const double *xbar, double *lam, double *y, double *thbar) {
    constexpr int NL = CAP * (CAP - 1) / 2 + 1;
    double L[NL], D[CAP], rD[CAP], c[CAP];
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
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) {
        y[i] = 0.0;
        lam[i] = 0.0;
        if (i < k) {
            double acc = pack_grad_upper(mask, a[i]) ? du[a[i]] : dl[a[i]];
            for (int t = 0; t < S.nth; t++) acc = fma(S.Dth[(size_t)a[i] * S.nth + t], theta[t], acc);
            lam[i] = acc;
        }
    }
    for (int q = 0; q < S.nout; q++) {
        const double xb = xbar[q];
        LMPC_SENS_UNROLL
        for (int i = 0; i < CAP; i++) if (i < k) y[i] = fma(S.P[(size_t)a[i] * S.nout + q], xb, y[i]);
    }
    LMPC_SENS_UNROLL
    for (int i = 1; i < CAP; i++) {
        if (i < k) {
            LMPC_SENS_UNROLL
            for (int p = 0; p < i; p++) {
                y[i] = fma(-L[i * (i - 1) / 2 + p], y[p], y[i]);
                lam[i] = fma(-L[i * (i - 1) / 2 + p], lam[p], lam[i]);
            }
        }
    }
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) if (i < k) { y[i] = y[i] * rD[i]; lam[i] = lam[i] * rD[i]; }
    LMPC_SENS_UNROLL
    for (int i = CAP - 2; i >= 0; i--) {
        if (i < k) {
            LMPC_SENS_UNROLL
            for (int p = CAP - 1; p > i; p--)
                if (p < k) {
                    y[i] = fma(-L[p * (p - 1) / 2 + i], y[p], y[i]);
                    lam[i] = fma(-L[p * (p - 1) / 2 + i], lam[p], lam[i]);
                }
        }
    }
    if (thbar)
        for (int t = 0; t < S.nth; t++) {
            double acc = 0.0;
            for (int q = 0; q < S.nout; q++) acc = fma(S.Xth[(size_t)q * S.nth + t], xbar[q], acc);
            LMPC_SENS_UNROLL
            for (int i = 0; i < CAP; i++) if (i < k) acc = fma(S.Dth[(size_t)a[i] * S.nth + t], y[i], acc);
            thbar[t] = acc;
        }
    return SENS_DONE;
}

// What the launches of one slab are told.  Every per-point pointer is the slab's own (the caller's arrays offset to its
// first point); N = the slab's points.
struct PackGradArgs {
    const double *C = nullptr;          // derived pack of the sens kernels
    SensDims d{};
    double rho = 0.0, zero_tol = 0.0;
    const double *K = nullptr;          // [M, m x n][Rout, nout x n][du, m][dl, m]
    int n = 0;
    long long N = 0;
    const uint64_t *active = nullptr;
    const int32_t *flag = nullptr;
    const double *theta = nullptr, *xbar = nullptr;
    double *thbar = nullptr;            // may be NULL
    int32_t *status = nullptr;          // may be NULL
    int32_t *st = nullptr;              // the slab's statuses (scratch)
    double *rec = nullptr;              // per point [lambda, recK][y, recK] in set order (scratch)
    int recK = 0;
    int32_t *list = nullptr, *count = nullptr;
    int cap = 0;                        // points with |A| beyond it go to the list
    int staged = 0;                     // lane kernel: the derived pack is copied to LDS first
    int stagedM = 0;                    // reduce kernel: a workgroup's columns of M and Rout are copied to LDS first
    int colChunk = 0;                   // reduce kernel: columns of M per blockIdx.y (the last blockIdx.y: the rows' and outputs' sums)
    double *part = nullptr;             // one partial per 64 points (scratch)
};

#if defined(__HIPCC__) && defined(LMPC_PACK_GRAD_KERNELS)

// One point per lane, as sens_lane_kernel: finished here for |A| <= cap, else queued for the wavefront kernel.
template <int CAP>
__global__ __launch_bounds__(kPackGradBlock) void pack_grad_lane_kernel(PackGradArgs A) {
    extern __shared__ double pack_grad_lds[];
    const SensDims d = A.d;
    if (A.staged) {
        const int nd = (int)sens_pack_doubles(d);
        for (int i = threadIdx.x; i < nd; i += blockDim.x) pack_grad_lds[i] = A.C[i];
        __syncthreads();
    }
    const SensView S = sens_view(A.staged ? pack_grad_lds : A.C, d, A.rho, A.zero_tol);
    const double *du = A.K + (size_t)(d.m + d.nout) * A.n, *dl = du + d.m;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int a[CAP];
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) a[i] = 0;
    bool queued = false;
    if (p < A.N) {
        const uint64_t *mask = A.active + (size_t)p * d.words;
        const int k = sens_active_rows<CAP>(mask, d.words, d.m, a);
        double lam[CAP], y[CAP];
        double *tb = A.thbar ? A.thbar + (size_t)p * d.nth : nullptr;
        int st = SENS_FAILED_POINT;
        if (A.flag[p] < 1) st = SENS_FAILED_POINT;
        else if (k > kSensMaxSet) st = SENS_TOO_MANY;
        else if (k > A.cap) queued = true;
        else st = pack_grad_point<CAP>(S, du, dl, mask, a, k, A.theta + (size_t)p * d.nth, A.xbar + (size_t)p * d.nout, lam, y, tb);
        if (!queued) {
            if (st == SENS_DONE) {
                double *r = A.rec + (size_t)p * 2 * A.recK;
                LMPC_SENS_UNROLL
                for (int i = 0; i < CAP; i++) if (i < k) { r[i] = lam[i]; r[A.recK + i] = y[i]; }
            } else if (tb) {
                for (int t = 0; t < d.nth; t++) tb[t] = 0.0;
            }
            A.st[p] = st;
            if (A.status) A.status[p] = st;
        }
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

// One listed point per wavefront, as sens_wave_kernel (same factor, same order per value), with the two right-hand
// sides substituted side by side.
__global__ __launch_bounds__(64) void pack_grad_wave_kernel(PackGradArgs A) {
    __shared__ double Lm[kSensMaxSet * kSensLd];
    __shared__ double Ds[kSensMaxSet], ys[kSensMaxSet];
    __shared__ int idx[kSensMaxSet];
    const SensDims d = A.d;
    const SensView S = sens_view(A.C, d, A.rho, A.zero_tol);
    const double *du = A.K + (size_t)(d.m + d.nout) * A.n, *dl = du + d.m;
    const int lane = threadIdx.x;
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
        double *tb = A.thbar ? A.thbar + (size_t)p * d.nth : nullptr;
        int st = SENS_DONE;
        if (k > kSensMaxSet) st = SENS_TOO_MANY;     // (never listed; kept so that no lane index can leave the 64 rows)
        const bool in = lane < k && st == SENS_DONE;
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
        for (int j = 0; st == SENS_DONE && j < k; j++) {
            double v = 0.0;
            if (in && lane >= j) {
                v = Lm[lane * kSensLd + j];
                for (int q = 0; q < j; q++) {
                    const double c = Lm[j * kSensLd + q] * Ds[q];
                    v = fma(-Lm[lane * kSensLd + q], c, v);
                }
            }
            const double dj = __shfl(v, j);
            if (dj < S.zero_tol) { st = SENS_SINGULAR; break; }
            const double r = 1.0 / dj;
            if (lane == j) Ds[j] = dj;
            if (in && lane > j) Lm[lane * kSensLd + j] = v * r;
            __syncthreads();
        }
        if (st != SENS_DONE) {
            if (tb) for (int t = lane; t < d.nth; t += 64) tb[t] = 0.0;
            if (lane == 0) { A.st[p] = st; if (A.status) A.status[p] = st; }
            continue;
        }
        const double rD = in ? 1.0 / Ds[lane] : 0.0;
        const double *xb = A.xbar + (size_t)p * d.nout, *th = A.theta + (size_t)p * d.nth;
        double z = 0.0, l = 0.0;
        if (in) {
            for (int q = 0; q < d.nout; q++) z = fma(S.P[(size_t)mine * d.nout + q], xb[q], z);
            l = pack_grad_upper(mask, mine) ? du[mine] : dl[mine];
            for (int t = 0; t < d.nth; t++) l = fma(S.Dth[(size_t)mine * d.nth + t], th[t], l);
        }
        for (int q = 0; q + 1 < k; q++) {
            const double zq = __shfl(z, q), lq = __shfl(l, q);
            if (in && lane > q) { z = fma(-Lm[lane * kSensLd + q], zq, z); l = fma(-Lm[lane * kSensLd + q], lq, l); }
        }
        z = z * rD;
        l = l * rD;
        for (int q = k - 1; q >= 1; q--) {
            const double yq = __shfl(z, q), lq = __shfl(l, q);
            if (lane < q) { z = fma(-Lm[q * kSensLd + lane], yq, z); l = fma(-Lm[q * kSensLd + lane], lq, l); }
        }
        if (in) {
            double *r = A.rec + (size_t)p * 2 * A.recK;
            r[lane] = l;
            r[A.recK + lane] = z;
        }
        if (tb) {
            __syncthreads();
            ys[lane] = z;
            __syncthreads();
            for (int t = lane; t < d.nth; t += 64) {
                double acc = 0.0;
                for (int q = 0; q < d.nout; q++) acc = fma(S.Xth[(size_t)q * d.nth + t], xb[q], acc);
                for (int i = 0; i < k; i++) acc = fma(S.Dth[(size_t)idx[i] * d.nth + t], ys[i], acc);
                tb[t] = acc;
            }
        }
        if (lane == 0) { A.st[p] = SENS_DONE; if (A.status) A.status[p] = SENS_DONE; }
    }
}

// the 64 leaves of a wavefront summed by the balanced tree (lane i with i ^ 1, then pairs with pairs, ...): every lane
// ends with the root, the two operands of an addition being the same on both sides of a pair
__device__ inline double pack_grad_sum64(double v) {
    for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s);
    return v;
}

// The sums of one wavefront leave in their order from position lo on: lane (e mod 64) keeps sum e and every 64 sums one
// line is stored (of the first line only the positions from lo on).
struct PackGradEmit {
    double *dst;
    size_t lo, e;
    double keep;
    int lane;
    __device__ void put(double v) {
        if ((int)(e & 63) == lane) keep = v;
        e++;
        if ((e & 63) == 0 && e - 64 + lane >= lo) dst[e - 64 + lane] = keep;
    }
    __device__ void flush() {
        const size_t r = e & 63;
        if ((size_t)lane < r && e - r + lane >= lo) dst[e - r + lane] = keep;
    }
};

// One point per lane, one 64-aligned block of points per wavefront: the contributions of the block, summed over its 64
// points, into the wavefront's partial.  blockIdx.y < gridDim.y - 1 takes colChunk columns of M (their Rout-bar and M-bar
// sums), the last blockIdx.y the sums per row and per output, so that a slab of few points still fills the device.
// A row no lane holds costs one ballot.
__global__ __launch_bounds__(kPackGradBlock) void pack_grad_reduce_kernel(PackGradArgs A) {
    extern __shared__ double pack_grad_lds[];
    const int n = A.n, m = A.d.m, nth = A.d.nth, nout = A.d.nout, words = A.d.words;
    const bool columns = blockIdx.y + 1 < gridDim.y;
    const int c0 = columns ? (int)blockIdx.y * A.colChunk : n, c1 = columns && c0 + A.colChunk < n ? c0 + A.colChunk : n;
    // entry (row r, column c) of [M; Rout] at MR[r * ldm + c - c0]: global memory, or the chunk's columns staged in LDS
    // (the last blockIdx.y reads neither array and stages nothing)
    const double *MR = A.K + c0;
    int ldm = n;
    if (A.stagedM && columns) {
        const int wd = c1 - c0, nd = (m + nout) * wd;
        for (int i = threadIdx.x; i < nd; i += blockDim.x) pack_grad_lds[i] = A.K[(size_t)(i / wd) * n + c0 + i % wd];
        __syncthreads();
        MR = pack_grad_lds;
        ldm = wd;
    }
    const double *M = MR, *Rout = MR + (size_t)m * ldm;
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long wave = p >> 6;
    if (wave * 64 >= A.N) return;
    const bool ok = p < A.N && A.st[p] == SENS_DONE;
    const long long pc = ok ? p : 0;                    // (a lane without a point reads nothing)
    const uint64_t *mask = A.active + (size_t)pc * words;
    const double *lam = A.rec + (size_t)pc * 2 * A.recK, *y = lam + A.recK;
    const double *xb = A.xbar + (size_t)pc * nout, *th = A.theta + (size_t)pc * nth;
    PackGradDims gd;
    gd.n = n; gd.m = m; gd.nth = nth; gd.nout = nout;
    const int nrw = (m + 63) / 64;
    const size_t e0 = (size_t)c0 * (nout + m);
    PackGradEmit E{A.part + (size_t)wave * pack_grad_doubles(gd), e0, e0, 0.0, lane};
    for (int c = c0; c < c1; c++) {
        double v = 0.0, w = 0.0, vb = 0.0;
        if (ok) {
            int i = 0;
            for (int rw = 0; rw < nrw; rw++) {
                uint64_t u = sens_rows(mask, words, m, rw);
                while (u) {
                    const double mjc = M[(size_t)(64 * rw + sens_ctz(u)) * ldm + c - c0];
                    v = fma(mjc, lam[i], v);
                    w = fma(mjc, y[i], w);
                    i++; u &= u - 1;
                }
            }
            for (int q = 0; q < nout; q++) vb = fma(Rout[(size_t)q * ldm + c - c0], xb[q], vb);
        }
        const double g = vb - w;
        for (int q = 0; q < nout; q++) E.put(pack_grad_sum64(ok ? xb[q] * v : 0.0));
        int base = 0;
        for (int rw = 0; rw < nrw; rw++) {
            const uint64_t u = ok ? sens_rows(mask, words, m, rw) : 0;
            const int nj = m - 64 * rw < 64 ? m - 64 * rw : 64;
            for (int jj = 0; jj < nj; jj++) {
                const bool has = (u >> jj) & 1;
                if (__ballot(has) == 0) { E.put(0.0); continue; }
                double cv = 0.0;
                if (has) {
                    const int i = base + sens_popc(u & ((1ull << jj) - 1));
                    cv = fma(lam[i], g, -(y[i] * v));
                }
                E.put(pack_grad_sum64(cv));
            }
            base += sens_popc(u);
        }
    }
    if (columns) { E.flush(); return; }
    int base = 0;
    for (int rw = 0; rw < nrw; rw++) {
        const uint64_t u = ok ? sens_rows(mask, words, m, rw) : 0;
        const int nj = m - 64 * rw < 64 ? m - 64 * rw : 64;
        for (int jj = 0; jj < nj; jj++) {
            const bool has = (u >> jj) & 1;
            if (__ballot(has) == 0) {
                for (int t = 0; t < 2 + nth; t++) E.put(0.0);
                continue;
            }
            double yi = 0.0;
            bool up = false;
            if (has) {
                yi = y[base + sens_popc(u & ((1ull << jj) - 1))];
                up = pack_grad_upper(mask, 64 * rw + jj) != 0;
            }
            E.put(pack_grad_sum64(has && up ? yi : 0.0));
            E.put(pack_grad_sum64(has && !up ? yi : 0.0));
            for (int t = 0; t < nth; t++) E.put(pack_grad_sum64(has ? yi * th[t] : 0.0));
        }
        base += sens_popc(u);
    }
    for (int q = 0; q < nout; q++) {
        const double xq = ok ? xb[q] : 0.0;
        E.put(pack_grad_sum64(xq));
        for (int t = 0; t < nth; t++) E.put(pack_grad_sum64(ok ? xq * th[t] : 0.0));
    }
    E.flush();
}

// One level group of the tree per thread and value: items lie `step` partials apart, a thread sums `fan` of them (a power
// of two, groups aligned to it) pairwise in place -- neighbours, then pairs of neighbours, ... -- and an absent item is
// the +0.0 of the contract, left out.  The last launch of a tree (one group) stores the root: into dst, or (final)
// into the caller's arrays.  The items are those an EARLIER launch wrote.
__global__ __launch_bounds__(kPackGradBlock) void pack_grad_tree_kernel(double *items, PackGradDims gd, long long count,
                                                                        long long step, double *dst, PackGradOut out, int final) {
    const size_t G = pack_grad_doubles(gd);
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const long long groups = (count + kPackGradFan - 1) / kPackGradFan;
    if (tid >= G * (size_t)groups) return;
    const size_t g = tid % G;
    const long long base = (long long)(tid / G) * kPackGradFan;
    const int lim = count - base < kPackGradFan ? (int)(count - base) : kPackGradFan;
    const size_t stride = (size_t)step * G;
    double *it = items + (size_t)base * stride + g;
    for (int s = 1; s < lim; s <<= 1)
        for (int i = 0; i + s < lim; i += 2 * s) it[(size_t)i * stride] = it[(size_t)i * stride] + it[(size_t)(i + s) * stride];
    if (groups != 1) return;
    if (final) {
        size_t idx = 0;
        const int which = pack_grad_locate(gd, g, &idx);
        if (out.p[which]) out.p[which][idx] = it[0];
    } else if (dst) {
        dst[g] = it[0];
    }
}

#endif  // __HIPCC__ && LMPC_PACK_GRAD_KERNELS

}  // namespace lmpc
