// Explicit MPC: the serialised controller (blob layout) and its point evaluation, shared by the host builder
// (lmpc_explicit.cpp: lmpc_explicit_locate_host) and the GPU kernel below (lmpc_explicit.hip), so that both run the
// same arithmetic -- explicit fmas in the same order, bit for bit the same answer on either side.
//
// Blob (one contiguous allocation, every section 8-byte aligned, offsets in bytes from the start):
//   int64 head[16]           kHead* below
//   int32 nodes[nodes][4]    inner node {row, left, right, 0}: go left if a_row . theta <= b_row;
//                            leaf       {-1, first, count, 0}: candidates leafidx[first .. first + count)
//   int32 leafidx[]          region indices, most frequent first within a leaf
//   int32 regions[R][8]      {row0, nrows, law, soft, nsoft, nsoftrows, 0, 0}: rows row0 .. row0 + nrows of `rows` (the
//                            first nsoftrows of them bounds of inactive SOFT rows, for inspection), the output
//                            law at record `law` of `laws` (nout records), the soft multipliers' law at record `soft`
//                            of `soft` (nsoft records)
//   double rows[][nth + 1]   halfspace a . theta <= b as (a, b)
//   double laws[][nth + 1]   output k = F_k . theta + g_k as (F_k, g_k)
//   double soft[][nth + 1]   multiplier of an active SOFT row = L_i . theta + l_i as (L_i, l_i)
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define LMPC_EXP_HD __host__ __device__
#else
#define LMPC_EXP_HD
#endif

namespace lmpc {

constexpr int kExplicitMaxNth = 32;

enum : int {
    kHeadNth = 0, kHeadNout, kHeadRegions, kHeadNodes, kHeadLeafIdx, kHeadRows, kHeadOffNodes, kHeadOffLeafIdx,
    kHeadOffRegions, kHeadOffRows, kHeadOffLaws, kHeadOffSoft, kHeadBytes, kHeadSoftRows, kHeadWords = 16
};

struct ExplicitView {
    const int32_t *nodes, *leafidx, *regions;
    const double *rows, *laws, *soft;
    int nth, nout;
    double primal_tol, band, rho_soft;
};

// `base`: where the blob lives (host copy or device copy); `head`: its header, read on the host
inline ExplicitView explicit_view(const void *base, const int64_t *head, double primal_tol, double band, double rho_soft) {
    const char *b = static_cast<const char *>(base);
    ExplicitView v;
    v.nodes = reinterpret_cast<const int32_t *>(b + head[kHeadOffNodes]);
    v.leafidx = reinterpret_cast<const int32_t *>(b + head[kHeadOffLeafIdx]);
    v.regions = reinterpret_cast<const int32_t *>(b + head[kHeadOffRegions]);
    v.rows = reinterpret_cast<const double *>(b + head[kHeadOffRows]);
    v.laws = reinterpret_cast<const double *>(b + head[kHeadOffLaws]);
    v.soft = reinterpret_cast<const double *>(b + head[kHeadOffSoft]);
    v.nth = (int)head[kHeadNth];
    v.nout = (int)head[kHeadNout];
    v.primal_tol = primal_tol; v.band = band; v.rho_soft = rho_soft;
    return v;
}

// a . theta > b ?  (the dot product as a chain of fmas from 0, then one comparison)
template <int NT>
LMPC_EXP_HD inline bool explicit_row_violated(const double *row, const double *th, int nth) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NT; k++)
        if (k < nth) acc = fma(row[k], th[k], acc);
    return acc > row[nth];
}

// F . theta + g as a chain of fmas from g
template <int NT>
LMPC_EXP_HD inline double explicit_affine(const double *rec, const double *th, int nth) {
    double acc = rec[nth];
#pragma unroll
    for (int k = 0; k < NT; k++)
        if (k < nth) acc = fma(rec[k], th[k], acc);
    return acc;
}

// Point location: tree walk, then the leaf's candidates in order, each left at its first violated row.
// Returns the region (or -1) and, through *flag, 1 / 2 (soft slack rho * sum lambda_soft^2 above primal_tol, the
// solver's rule).  A point whose soft slack lies within the relative band around primal_tol is returned as -1: the
// implicit solve decides its flag.  *rows_checked (may be NULL): tree nodes plus halfspace rows evaluated.
template <int NT>
LMPC_EXP_HD inline int explicit_locate(const ExplicitView &v, const double *th, int *flag, int *rows_checked) {
    const int nth = v.nth, stride = nth + 1;
    int node = 0;
    int checked = 0;
    while (v.nodes[4 * node] >= 0) {
        const int row = v.nodes[4 * node];
        checked++;
        node = explicit_row_violated<NT>(v.rows + (int64_t)row * stride, th, nth) ? v.nodes[4 * node + 2]
                                                                                    : v.nodes[4 * node + 1];
    }
    const int first = v.nodes[4 * node + 1], cnt = v.nodes[4 * node + 2];
    int found = -1;
    for (int c = 0; c < cnt && found < 0; c++) {
        const int r = v.leafidx[first + c];
        const int32_t *rec = v.regions + 8 * r;
        const double *row = v.rows + (int64_t)rec[0] * stride;
        bool inside = true;
        for (int i = 0; i < rec[1]; i++) {
            checked++;
            const double *ri = row + (int64_t)i * stride;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < NT; k++)
                if (k < nth) acc = fma(ri[k], th[k], acc);
            if (acc > ri[nth]) { inside = false; break; }
        }
        if (inside) found = r;
    }
    if (rows_checked) *rows_checked = checked;
    *flag = 0;
    if (found < 0) return -1;
    const int32_t *rec = v.regions + 8 * found;
    double s = 0.0;
    for (int i = 0; i < rec[4]; i++) {
        const double l = explicit_affine<NT>(v.soft + ((int64_t)rec[3] + i) * stride, th, nth);
        s = fma(l * l, v.rho_soft, s);
    }
    if (rec[4] > 0 && fabs(s - v.primal_tol) <= v.band * v.primal_tol) return -1;
    *flag = s > v.primal_tol ? 2 : 1;
    return found;
}

#if defined(__HIP__) && defined(LMPC_EXPLICIT_KERNELS)
// One point per lane.  The block's theta records are staged through LDS with coalesced loads (nth doubles per
// record), each lane copies its own into registers, locates it and evaluates the law.  Unlocated points get
// region = -1 and are appended to `list` with one atomic per wavefront (ballot + mbcnt); their x / exitflag are left
// to the implicit solve.  Every store is a vector store.
template <int NT>
__global__ __launch_bounds__(256) void explicit_eval_kernel(ExplicitView v, int64_t N, const double *__restrict__ theta,
                                                            double *__restrict__ x, int32_t *__restrict__ exitflag,
                                                            int32_t *__restrict__ region, int32_t *__restrict__ list,
                                                            int32_t *__restrict__ count) {
    extern __shared__ double sth[];
    const int nth = v.nth;
    const int64_t base = (int64_t)blockIdx.x * blockDim.x;
    const int64_t left = N - base;
    const int nb = left < (int64_t)blockDim.x ? (int)left : (int)blockDim.x;
    for (int i = threadIdx.x; i < nb * nth; i += blockDim.x) sth[i] = theta[base * nth + i];
    __syncthreads();
    const bool live = (int)threadIdx.x < nb;
    const int64_t p = base + threadIdx.x;
    double th[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) th[k] = (live && k < nth) ? sth[threadIdx.x * nth + k] : 0.0;
    int flag = 0, r = -1;
    if (live) r = explicit_locate<NT>(v, th, &flag, nullptr);
    if (live && r >= 0) {
        const double *law = v.laws + (int64_t)v.regions[8 * r + 2] * (nth + 1);
        for (int k = 0; k < v.nout; k++) x[p * v.nout + k] = explicit_affine<NT>(law + (int64_t)k * (nth + 1), th, nth);
        exitflag[p] = flag;
    }
    if (live) region[p] = r;
    const unsigned long long miss = __ballot(live && r < 0);
    if (miss) {
        const int leader = __ffsll((unsigned long long)miss) - 1;
        const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(miss >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)miss, 0u));
        int slot = 0;
        if ((int)__lane_id() == leader) slot = atomicAdd(count, (int)__popcll(miss));
        slot = __shfl(slot, leader);
        if (live && r < 0) list[slot + (int)below] = (int32_t)p;
    }
}

// fallback plumbing: theta of the listed points into a dense batch, and that batch's answers back to their indices
__global__ void explicit_gather_kernel(int64_t n, int nth, const int32_t *__restrict__ list, const double *__restrict__ theta,
                                       double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t src = list[i];
    for (int k = 0; k < nth; k++) out[i * nth + k] = theta[src * nth + k];
}

__global__ void explicit_scatter_kernel(int64_t n, int nout, const int32_t *__restrict__ list, const double *__restrict__ xs,
                                        const int32_t *__restrict__ fs, double *__restrict__ x, int32_t *__restrict__ exitflag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t dst = list[i];
    for (int k = 0; k < nout; k++) x[dst * nout + k] = xs[i * nout + k];
    exitflag[dst] = fs[i];
}
#endif

}  // namespace lmpc
