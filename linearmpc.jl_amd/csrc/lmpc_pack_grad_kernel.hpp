// Gradient of the batched solve with respect to the pack (M, du, dl, Dth, Rout, x0, Xth), summed over the batch.
// Stage 1 (pack_grad_lane_kernel / pack_grad_wave_kernel) solves two right-hand sides on the factor of K_A per point
// and leaves the record [lambda | y]; stage 2 (pack_grad_reduce_kernel) forms every point's contributions, one point
// per lane, and sums the 64 points of a wavefront in the contract's pairing; pack_grad_tree_kernel sums the partials
// pairwise.  The arithmetic contract is stated in include/lmpc_hip.h ("Gradient with respect to the pack") and
// restated in numpy in tests/pack_grad_reference.py.  The factor, the substitutions and the lane kernel's ends are
// lmpc_sens_kernel.hpp's, called from here.  Internal to liblmpc_hip.so.
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

// One point with |A| = k <= CAP: on the factor of sens_point, y = K_A^-1 (P_A xbar) and lambda = K_A^-1 d side by side,
// and thbar (where asked for) as sens_point forms it.  lam and y are written for i < k only with SENS_DONE.
template <int CAP>
LMPC_SENS_HD inline int pack_grad_point(const SensView &S, const double *du, const double *dl, const uint64_t *mask, const int *a,
                                        int k, const double *theta, const double *xbar, double *lam, double *y, double *thbar) {
    SensFactor<CAP> F;
    if (sens_factor<CAP>(S, a, k, F) != SENS_DONE) return SENS_SINGULAR;
    double z[2][CAP];       // y, lambda
    sens_rhs<CAP>(S, a, k, xbar, z[0]);
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) {
        z[1][i] = 0.0;
        if (i < k) {
            double acc = pack_grad_upper(mask, a[i]) ? du[a[i]] : dl[a[i]];
            for (int t = 0; t < S.nth; t++) acc = fma(S.Dth[(size_t)a[i] * S.nth + t], theta[t], acc);
            z[1][i] = acc;
        }
    }
    sens_subst<CAP, 2>(F, k, z);
    LMPC_SENS_UNROLL
    for (int i = 0; i < CAP; i++) if (i < k) { y[i] = z[0][i]; lam[i] = z[1][i]; }
    if (thbar)
        for (int t = 0; t < S.nth; t++) thbar[t] = sens_tail<CAP>(S, a, k, z[0], t, sens_xth_dot(S, xbar, t));
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
    const SensView S = sens_view(sens_stage_pack(A.C, d, A.staged, pack_grad_lds), d, A.rho, A.zero_tol);
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
        int st = sens_classify(A.flag[p], k, A.cap);
        queued = st == SENS_QUEUED;
        if (st == SENS_DONE)
            st = pack_grad_point<CAP>(S, du, dl, mask, a, k, A.theta + (size_t)p * d.nth, A.xbar + (size_t)p * d.nout, lam, y, tb);
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
    sens_append(queued, p, A.list, A.count);
}

// One listed point per wavefront, as sens_wave_kernel, with the two right-hand sides substituted side by side.
__global__ __launch_bounds__(64) void pack_grad_wave_kernel(PackGradArgs A) {
    __shared__ SensWaveLds W;
    const SensDims d = A.d;
    const SensView S = sens_view(A.C, d, A.rho, A.zero_tol);
    const double *du = A.K + (size_t)(d.m + d.nout) * A.n, *dl = du + d.m;
    const int lane = threadIdx.x;
    const int cnt = *A.count;
    for (int e = blockIdx.x; e < cnt; e += gridDim.x) {
        const long long p = A.list[e];
        const uint64_t *mask = A.active + (size_t)p * d.words;
        int mine;
        const int k = sens_wave_rows(mask, d, lane, &mine);
        double *tb = A.thbar ? A.thbar + (size_t)p * d.nth : nullptr;
        double rD = 0.0;
        // (a set beyond the 64 rows is never listed; refused so that no lane index can leave them)
        const int st = k > kSensMaxSet ? SENS_TOO_MANY : sens_wave_factor(W, S, lane, mine, k, &rD) ? SENS_DONE : SENS_SINGULAR;
        if (lane == 0) { A.st[p] = st; if (A.status) A.status[p] = st; }
        if (st != SENS_DONE) {
            if (tb) for (int t = lane; t < d.nth; t += 64) tb[t] = 0.0;
            continue;
        }
        const double *xb = A.xbar + (size_t)p * d.nout, *th = A.theta + (size_t)p * d.nth;
        double z[2] = {0.0, 0.0};       // y, lambda
        if (lane < k) {
            z[0] = sens_p_dot(S, mine, xb);
            z[1] = pack_grad_upper(mask, mine) ? du[mine] : dl[mine];
            for (int t = 0; t < d.nth; t++) z[1] = fma(S.Dth[(size_t)mine * d.nth + t], th[t], z[1]);
        }
        sens_wave_subst<2>(W, lane, k, rD, z);
        if (lane < k) {
            double *r = A.rec + (size_t)p * 2 * A.recK;
            r[lane] = z[1];
            r[A.recK + lane] = z[0];
        }
        if (tb) sens_wave_tail<false>(W, S, lane, k, z[0], xb, 0, tb);
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
