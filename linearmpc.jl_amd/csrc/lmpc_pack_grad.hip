// Gradient of the batched solve with respect to the pack (include/lmpc_hip.h, "Gradient with respect to the pack"):
// the slab loop over the kernels of lmpc_pack_grad_kernel.hpp, its scratch, the host-pointer wrapper and the host twin
// that runs the same arithmetic without a GPU.
#define LMPC_PACK_GRAD_KERNELS 1
#include "lmpc_internal.hpp"
#include "lmpc_pack_grad_kernel.hpp"

#include <cstring>

namespace lmpc {
namespace {

PackGradDims pg_dims(const lmpc_handle *h) {
    PackGradDims g;
    g.n = h->P.n; g.m = h->P.m; g.nth = h->P.nth; g.nout = h->P.nout;
    return g;
}
int pg_rec_rows(int m) { return m < kSensMaxSet ? (m > 0 ? m : 1) : kSensMaxSet; }

// log2 of the slab: the option, or the largest whose records, statuses and partials stay within the budget
int pg_slab_log(const lmpc_handle *h) {
    if (h->packGradSlab) return h->packGradSlab;
    const size_t per = 16 * (size_t)pg_rec_rows(h->P.m) + sizeof(int32_t) + sizeof(double) * pack_grad_doubles(pg_dims(h)) / 64 + 1;
    int s = kPackGradSlabMin;
    while (s < kPackGradSlabMax && (per << (s + 1)) <= kPackGradBudget) s++;
    return s;
}

int pg_ensure(lmpc_handle *h, int64_t N, size_t *bytes) {
    const PackGradDims g = pg_dims(h);
    const size_t G = pack_grad_doubles(g);
    const int slog = pg_slab_log(h);
    const int64_t slab = (int64_t)1 << slog;
    const int64_t pts = N < slab ? (N + 63) / 64 * 64 : slab;
    LMPC_TRY(sens_ensure(h, pts));
    if (!h->pgK) {
        std::vector<double> K;
        K.insert(K.end(), h->P.M.begin(), h->P.M.end());
        K.insert(K.end(), h->P.Rout.begin(), h->P.Rout.end());
        K.insert(K.end(), h->P.du0.begin(), h->P.du0.end());
        K.insert(K.end(), h->P.dl0.begin(), h->P.dl0.end());
        HIP_TRY(h, h->pgK.reserve(K.size()));
        const hipError_t e = hipMemcpy(h->pgK, K.data(), sizeof(double) * K.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            h->pgK.reset();
            return fail(h, LMPC_ERR_HIP, std::string("hipMemcpy of the pack gradient's constants: ") + hipGetErrorString(e));
        }
    }
    if (slog != h->pgSlabLog) h->pgCap = 0;
    const size_t nslab = (size_t)((N + slab - 1) / slab);
    HIP_TRY(h, reserve_group(h->pgCap, N, sized(h->pgRec, (size_t)pts * 2 * pg_rec_rows(g.m)), sized(h->pgSt, (size_t)pts),
                             sized(h->pgPart, (size_t)(pts / 64) * G), sized(h->pgSum, nslab * G)));
    h->pgSlabLog = slog;
    if (bytes)
        *bytes = sizeof(double) * (h->pgK.size() + h->pgRec.size() + h->pgPart.size() + h->pgSum.size()) + sizeof(int32_t) * h->pgSt.size();
    return LMPC_OK;
}

template <int CAP>
void pg_launch_lane(const PackGradArgs &A, unsigned grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((pack_grad_lane_kernel<CAP>), dim3(grid), dim3(kPackGradBlock), lds, st, A);
}

// the tree over `count` items of G doubles, `items` written by earlier launches; the root into dst or the caller's arrays
int pg_tree(lmpc_handle *h, double *items, const PackGradDims &g, long long count, double *dst, const PackGradOut &out, int final,
            hipStream_t st, int *launches) {
    const size_t G = pack_grad_doubles(g);
    long long step = 1;
    for (;;) {
        const long long groups = (count + kPackGradFan - 1) / kPackGradFan;
        const size_t threads = G * (size_t)groups;
        hipLaunchKernelGGL(pack_grad_tree_kernel, dim3((unsigned)((threads + kPackGradBlock - 1) / kPackGradBlock)), dim3(kPackGradBlock),
                           0, st, items, g, count, step, dst, out, final);
        HIP_TRY(h, hipGetLastError());
        (*launches)++;
        if (groups == 1) return LMPC_OK;
        step *= kPackGradFan;
        count = groups;
    }
}

int pg_launch(lmpc_handle *h, int64_t N, const double *theta, const uint64_t *active, const int32_t *flag, const double *xbar,
              const PackGradOut &out, double *thbar, int32_t *status, hipStream_t st) {
    size_t scratch = 0;
    LMPC_TRY(pg_ensure(h, N, &scratch));
    const PackGradDims g = pg_dims(h);
    const size_t G = pack_grad_doubles(g);
    PackGradArgs A;
    A.C = h->dSens;
    A.d.m = g.m; A.d.nth = g.nth; A.d.nout = g.nout; A.d.words = h->P.words();
    A.rho = h->S.rho_soft; A.zero_tol = h->S.zero_tol;
    A.K = h->pgK; A.n = g.n;
    A.st = h->pgSt; A.rec = h->pgRec; A.recK = pg_rec_rows(g.m);
    A.list = h->dSensList; A.count = h->dSensCnt;
    A.part = h->pgPart;
    const int CAP = sens_cap_of(h);                      // the lane capacity the VJP picks
    A.cap = h->sensForceList ? 0 : CAP;
    const size_t cbytes = sizeof(double) * sens_pack_doubles(A.d);
    A.staged = cbytes <= kSensStageMax;
    const size_t mbytes = sizeof(double) * (size_t)(g.m + g.nout) * g.n;
    A.stagedM = mbytes <= kPackGradStageMax;
    const size_t lds1 = A.staged ? cbytes : 0;
    size_t lds2first = 0;
    const bool pass2 = g.m > A.cap;
    const int slog = h->pgSlabLog;
    const int64_t slab = (int64_t)1 << slog;
    const int64_t nslab = (N + slab - 1) / slab;
    bool sums = false;                                   // no output array asked for: stage 1 alone (thbar and status)
    for (int q = 0; q < PG_ARRAYS; q++) sums = sums || out.p[q] != nullptr;
    unsigned grid1 = 0, gridw = 0, gridr = 0;
    int trees = 0, chunks1 = 0;
    for (int64_t s = 0; s < nslab; s++) {
        const int64_t p0 = s * slab, ns = N - p0 < slab ? N - p0 : slab;
        A.N = ns;
        A.active = active + (size_t)p0 * A.d.words;
        A.flag = flag + p0;
        A.theta = theta + (size_t)p0 * g.nth;
        A.xbar = xbar + (size_t)p0 * g.nout;
        A.thbar = thbar ? thbar + (size_t)p0 * g.nth : nullptr;
        A.status = status ? status + p0 : nullptr;
        const unsigned grid = (unsigned)((ns + kPackGradBlock - 1) / kPackGradBlock);
        HIP_TRY(h, hipMemsetAsync(A.count, 0, sizeof(int32_t), st));
        if (CAP == 5) pg_launch_lane<5>(A, grid, lds1, st);
        else pg_launch_lane<8>(A, grid, lds1, st);
        HIP_TRY(h, hipGetLastError());
        const unsigned gw = sens_wave_grid(h, ns);
        if (pass2) {
            hipLaunchKernelGGL(pack_grad_wave_kernel, dim3(gw), dim3(64), 0, st, A);
            HIP_TRY(h, hipGetLastError());
        }
        if (s == 0) { grid1 = grid; gridw = gw; }
        if (!sums) continue;
        // the columns of M are split over blockIdx.y until the grid holds two workgroups per CU
        int ny = (int)((2u * (unsigned)h->numCU + grid - 1) / grid);
        ny = ny < 1 ? 1 : ny > g.n ? g.n : ny;
        A.colChunk = (g.n + ny - 1) / ny;
        ny = (g.n + A.colChunk - 1) / A.colChunk;
        const size_t lds2 = A.stagedM ? sizeof(double) * (size_t)(g.m + g.nout) * A.colChunk : 0;      // the chunk's columns
        hipLaunchKernelGGL(pack_grad_reduce_kernel, dim3(grid, (unsigned)ny + 1), dim3(kPackGradBlock), lds2, st, A);
        HIP_TRY(h, hipGetLastError());
        LMPC_TRY(pg_tree(h, h->pgPart, g, (ns + 63) / 64, h->pgSum + (size_t)s * G, PackGradOut{}, 0, st, &trees));
        if (s == 0) { gridr = grid; chunks1 = ny; lds2first = lds2; }
    }
    if (sums) LMPC_TRY(pg_tree(h, h->pgSum, g, nslab, nullptr, out, 1, st, &trees));
    const int32_t rec[LMPC_PACK_GRAD_INFO_WORDS] = {0, CAP, A.cap, (int32_t)grid1, (int32_t)lds1, A.staged + 2 * A.stagedM, pass2 ? 1 : 0,
                                                    pass2 ? (int32_t)gridw : 0, (int32_t)gridr, (int32_t)lds2first, slog, (int32_t)nslab, trees,
                                                    (int32_t)((scratch + 1023) / 1024), (int32_t)G, (int32_t)N, chunks1};
    h->packGradRec.push(rec);
    return LMPC_OK;
}

int pg_checks(lmpc_handle *h, int64_t N, const char *who) {
    if (!h || N < 0 || N > 0x7fffffffLL) return LMPC_ERR_BADARG;
    return sens_refuse(h, who);
}

// the point's contributions into the dense vector c (output arrays one after the other, each row-major), zeros elsewhere
void pg_contrib(const PackGradDims &g, const double *M, const double *Rout, const uint64_t *mask, const int *a, int k,
                const double *lam, const double *y, const double *theta, const double *xbar, const size_t *off, double *c) {
    for (int col = 0; col < g.n; col++) {
        double v = 0.0, w = 0.0, vb = 0.0;
        for (int i = 0; i < k; i++) {
            const double mjc = M[(size_t)a[i] * g.n + col];
            v = std::fma(mjc, lam[i], v);
            w = std::fma(mjc, y[i], w);
        }
        for (int q = 0; q < g.nout; q++) vb = std::fma(Rout[(size_t)q * g.n + col], xbar[q], vb);
        const double gc = vb - w;
        for (int q = 0; q < g.nout; q++) c[off[PG_ROUT] + (size_t)q * g.n + col] = xbar[q] * v;
        for (int i = 0; i < k; i++) c[off[PG_M] + (size_t)a[i] * g.n + col] = std::fma(lam[i], gc, -(y[i] * v));
    }
    for (int i = 0; i < k; i++) {
        c[off[pack_grad_upper(mask, a[i]) ? PG_DU : PG_DL] + a[i]] = y[i];
        for (int t = 0; t < g.nth; t++) c[off[PG_DTH] + (size_t)a[i] * g.nth + t] = y[i] * theta[t];
    }
    for (int q = 0; q < g.nout; q++) {
        c[off[PG_X0] + q] = xbar[q];
        for (int t = 0; t < g.nth; t++) c[off[PG_XTH] + (size_t)q * g.nth + t] = xbar[q] * theta[t];
    }
}

}  // namespace

int pack_grad_reserve(lmpc_handle *h, int64_t N) {
    return sens_no_derivative(h, nullptr) ? LMPC_OK : pg_ensure(h, N, nullptr);
}

}  // namespace lmpc

using namespace lmpc;

extern "C" {

int lmpc_solve_pack_vjp_device(lmpc_handle *h, int64_t N, const double *theta, const uint64_t *active, const int32_t *exitflag,
                               const double *xbar, double *Mbar, double *dubar, double *dlbar, double *Dthbar, double *Routbar,
                               double *x0bar, double *Xthbar, double *thbar, int32_t *status, void *stream) {
    LMPC_TRY(pg_checks(h, N, "lmpc_solve_pack_vjp_device"));
    if (N == 0) return LMPC_OK;
    if (!theta || !active || !exitflag || !xbar) return fail(h, LMPC_ERR_BADARG, "lmpc_solve_pack_vjp_device: a required array is NULL");
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    PackGradOut out;
    out.p[PG_M] = Mbar; out.p[PG_DU] = dubar; out.p[PG_DL] = dlbar; out.p[PG_DTH] = Dthbar; out.p[PG_ROUT] = Routbar;
    out.p[PG_X0] = x0bar; out.p[PG_XTH] = Xthbar;
    return pg_launch(h, N, theta, active, exitflag, xbar, out, thbar, status, (hipStream_t)stream);
}

int lmpc_solve_pack_vjp(lmpc_handle *h, int64_t N, const double *theta, const uint64_t *active, const int32_t *exitflag,
                        const double *xbar, double *Mbar, double *dubar, double *dlbar, double *Dthbar, double *Routbar,
                        double *x0bar, double *Xthbar, double *thbar, int32_t *status) {
    LMPC_TRY(pg_checks(h, N, "lmpc_solve_pack_vjp"));
    if (N == 0) return LMPC_OK;
    if (!theta || !active || !exitflag || !xbar) return fail(h, LMPC_ERR_BADARG, "lmpc_solve_pack_vjp: a required array is NULL");
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const int n = h->P.n, m = h->P.m, nth = h->P.nth, nout = h->P.nout, words = h->P.words();
    Staging s;
    const double *dT = static_cast<const double *>(s.in(theta, sizeof(double) * (size_t)N * nth));
    const uint64_t *dA = static_cast<const uint64_t *>(s.in(active, sizeof(uint64_t) * (size_t)N * words));
    const int32_t *dF = static_cast<const int32_t *>(s.in(exitflag, sizeof(int32_t) * (size_t)N));
    const double *dX = static_cast<const double *>(s.in(xbar, sizeof(double) * (size_t)N * nout));
    PackGradOut out;
    out.p[PG_M] = static_cast<double *>(s.out(Mbar, sizeof(double) * (size_t)m * n));
    out.p[PG_DU] = static_cast<double *>(s.out(dubar, sizeof(double) * (size_t)m));
    out.p[PG_DL] = static_cast<double *>(s.out(dlbar, sizeof(double) * (size_t)m));
    out.p[PG_DTH] = static_cast<double *>(s.out(Dthbar, sizeof(double) * (size_t)m * nth));
    out.p[PG_ROUT] = static_cast<double *>(s.out(Routbar, sizeof(double) * (size_t)nout * n));
    out.p[PG_X0] = static_cast<double *>(s.out(x0bar, sizeof(double) * (size_t)nout));
    out.p[PG_XTH] = static_cast<double *>(s.out(Xthbar, sizeof(double) * (size_t)nout * nth));
    double *dTb = static_cast<double *>(s.out(thbar, sizeof(double) * (size_t)N * nth));
    int32_t *dS = static_cast<int32_t *>(s.out(status, sizeof(int32_t) * (size_t)N));
    if (s.err != hipSuccess) return s.fail(h);
    LMPC_TRY(pg_launch(h, N, dT, dA, dF, dX, out, dTb, dS, nullptr));
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    if (!s.download_all()) return s.fail(h);
    return LMPC_OK;
}

int lmpc_solve_pack_vjp_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                             const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                             const lmpc_settings *s, int is_avi, int64_t N, const double *theta, const uint64_t *active,
                             const int32_t *exitflag, const double *xbar, double *Mbar, double *dubar, double *dlbar,
                             double *Dthbar, double *Routbar, double *x0bar, double *Xthbar, double *thbar, int32_t *status) {
    (void)x0;
    lmpc_settings st;
    LMPC_TRY(sens_check_pack("lmpc_solve_pack_vjp_host", n, m, ms, nth, nout, M, Dth, Rout, Xth, sense, du && dl, s, is_avi, N, &st));
    PackGradDims g;
    g.n = n; g.m = m; g.nth = nth; g.nout = nout;
    double *outs[PG_ARRAYS] = {Mbar, dubar, dlbar, Dthbar, Routbar, x0bar, Xthbar};
    const size_t len[PG_ARRAYS] = {(size_t)m * n, (size_t)m, (size_t)m, (size_t)m * nth, (size_t)nout * n, (size_t)nout, (size_t)nout * nth};
    size_t off[PG_ARRAYS + 1] = {0};
    for (int q = 0; q < PG_ARRAYS; q++) off[q + 1] = off[q] + len[q];
    const size_t G = off[PG_ARRAYS];
    for (int q = 0; q < PG_ARRAYS; q++)
        if (outs[q]) std::memset(outs[q], 0, sizeof(double) * len[q]);
    if (N == 0) return LMPC_OK;
    if (!theta || !active || !exitflag || !xbar) {
        g_setup_err = "lmpc_solve_pack_vjp_host: a required array is NULL";
        return LMPC_ERR_BADARG;
    }
    const int words = (2 * m + 63) / 64;
    SensDims d;
    d.m = m; d.nth = nth; d.nout = nout; d.words = words;
    std::vector<double> C;
    sens_build_pack(n, d, M, nullptr, Dth, Rout, Xth, sense, C);
    const SensView S = sens_view(C.data(), d, st.rho_soft, st.zero_tol);
    // the balanced tree as a binary counter: level[l] holds the sum of a finished block of 2^l points
    std::vector<std::vector<double>> level;
    std::vector<char> has;
    std::vector<double> cur(G), lam(kSensMaxSet), y(kSensMaxSet), tb((size_t)nth);
    int a[kSensMaxSet] = {};
    for (int64_t p = 0; p < N; p++) {
        const uint64_t *mask = active + (size_t)p * words;
        const int k = sens_active_rows<kSensMaxSet>(mask, words, m, a);
        int stp = sens_classify(exitflag[p], k, kSensMaxSet);
        if (stp == SENS_DONE)
            stp = pack_grad_point<kSensMaxSet>(S, du, dl, mask, a, k, theta + (size_t)p * nth, xbar + (size_t)p * nout, lam.data(),
                                               y.data(), tb.data());
        if (status) status[p] = stp;
        if (thbar)
            for (int t = 0; t < nth; t++) thbar[(size_t)p * nth + t] = stp == SENS_DONE ? tb[t] : 0.0;
        std::fill(cur.begin(), cur.end(), 0.0);
        if (stp == SENS_DONE) pg_contrib(g, M, Rout, mask, a, k, lam.data(), y.data(), theta + (size_t)p * nth, xbar + (size_t)p * nout, off, cur.data());
        size_t l = 0;
        for (; l < has.size() && has[l]; l++) {
            for (size_t e = 0; e < G; e++) cur[e] = level[l][e] + cur[e];
            has[l] = 0;
        }
        if (l == has.size()) { level.emplace_back(G); has.push_back(0); }
        level[l] = cur;
        has[l] = 1;
    }
    // the absent points up to the next power of two are +0.0: a finished block moves up unchanged until it meets one to its left
    bool any = false;
    for (size_t l = 0; l < has.size(); l++) {
        if (!has[l]) continue;
        if (any) for (size_t e = 0; e < G; e++) cur[e] = level[l][e] + cur[e];
        else cur = level[l];
        any = true;
    }
    for (int q = 0; q < PG_ARRAYS; q++)
        if (outs[q] && len[q]) std::memcpy(outs[q], cur.data() + off[q], sizeof(double) * len[q]);
    return LMPC_OK;
}

int lmpc_pack_grad_launch_info(const lmpc_handle *h, int32_t *out, int max) {
    if (!h || !out || max < 0) return LMPC_ERR_BADARG;
    return h->packGradRec.read(out, max);
}

}  // extern "C"
