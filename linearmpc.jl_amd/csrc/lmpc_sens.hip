// Differentiable batched solve (include/lmpc_hip.h, "Differentiable solve"): VJP and Jacobian of x*(theta) per point
// from the optimal active set -- derived pack, dispatch of the two kernels (lmpc_sens_kernel.hpp), the host-pointer
// wrappers and the host twins that run the same arithmetic without a GPU.
#define LMPC_SENS_KERNELS 1
#include "lmpc_internal.hpp"
#include "lmpc_sens_kernel.hpp"

#include <cstring>

namespace lmpc {
namespace {

// [G | P | Dth | Xth | soft] (lmpc_sens_kernel.hpp).  G: the pack's own triangle, or (G == nullptr) accumulated here by
// the same chain as finish_pack; P = M Rout' with the fma chain over the n columns in order.
void sens_build_pack(int n, const SensDims &d, const double *M, const double *G, const double *Dth, const double *Rout,
                     const double *Xth, const int32_t *sense, std::vector<double> &C) {
    C.assign(sens_pack_doubles(d), 0.0);
    double *g = C.data(), *p = g + sens_tri((size_t)d.m), *dt = p + (size_t)d.m * d.nout, *xt = dt + (size_t)d.m * d.nth,
           *so = xt + (size_t)d.nout * d.nth;
    for (int a = 0; a < d.m; a++)
        for (int b = 0; b <= a; b++) {
            if (G) { g[sens_tri((size_t)a) + b] = G[sens_tri((size_t)a) + b]; continue; }
            double acc = 0.0;
            for (int k = 0; k < n; k++) acc = std::fma(M[(size_t)a * n + k], M[(size_t)b * n + k], acc);
            g[sens_tri((size_t)a) + b] = acc;
        }
    for (int a = 0; a < d.m; a++)
        for (int q = 0; q < d.nout; q++) {
            double acc = 0.0;
            for (int k = 0; k < n; k++) acc = std::fma(M[(size_t)a * n + k], Rout[(size_t)q * n + k], acc);
            p[(size_t)a * d.nout + q] = acc;
        }
    if (d.m > 0) std::memcpy(dt, Dth, sizeof(double) * (size_t)d.m * d.nth);
    std::memcpy(xt, Xth, sizeof(double) * (size_t)d.nout * d.nth);
    for (int a = 0; a < d.m; a++) so[a] = (sense[a] & SENSE_SOFT) ? 1.0 : 0.0;
}

int sens_refuse(lmpc_handle *h, const char *who) {
    if (h->avi || h->P.avi || h->P.prox)
        return fail(h, LMPC_ERR_UNSUPPORTED, std::string(who) + ": variational and proximal-point handles have no derivative here");
    for (int32_t s : h->P.sense)
        if (s & SENSE_BINARY) return fail(h, LMPC_ERR_UNSUPPORTED, std::string(who) + ": BINARY rows have no derivative");
    if (h->P.nth == 0) return fail(h, LMPC_ERR_BADARG, std::string(who) + ": the problem has no parameter (nth = 0)");
    return LMPC_OK;
}

SensDims sens_dims(const lmpc_handle *h) {
    SensDims d;
    d.m = h->P.m; d.nth = h->P.nth; d.nout = h->P.nout; d.words = h->P.words();
    return d;
}

int sens_cap_of(const lmpc_handle *h) {
    if (h->sensCap == 5 || h->sensCap == 8) return h->sensCap;
    const int reach = h->P.n + h->P.nsoft < h->P.m ? h->P.n + h->P.nsoft : h->P.m;      // rows a set of this problem reaches
    return reach <= 5 ? 5 : 8;
}

template <int CAP, bool JAC>
void sens_launch_lane(const SensArgs &A, unsigned grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((sens_lane_kernel<CAP, JAC>), dim3(grid), dim3(kSensBlock), lds, st, A);
}

template <bool JAC>
int sens_launch(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar, double *out,
                int32_t *status, hipStream_t st) {
    LMPC_TRY(sens_ensure(h, N));
    SensArgs A;
    A.C = h->dSens; A.d = sens_dims(h);
    A.rho = h->S.rho_soft; A.zero_tol = h->S.zero_tol;
    A.N = N; A.active = active; A.flag = flag; A.xbar = xbar; A.out = out; A.status = status;
    A.list = h->dSensList; A.count = h->dSensCnt;
    const int CAP = sens_cap_of(h);
    A.cap = h->sensForceList ? 0 : CAP;
    const size_t bytes = sizeof(double) * sens_pack_doubles(A.d);
    A.staged = bytes <= kSensStageMax;
    const size_t per = JAC ? (size_t)A.d.nout * A.d.nth : (size_t)A.d.nth;
    const size_t tile = kSensBlock * (sizeof(double) * per + sizeof(int));
    A.stage_out = per <= (size_t)kSensStageOutMax && (A.staged ? bytes : 0) + tile <= kSensLdsMax;
    const size_t lds = (A.staged ? bytes : 0) + (A.stage_out ? tile : 0);
    const unsigned grid = (unsigned)((N + kSensBlock - 1) / kSensBlock);
    const bool pass2 = A.d.m > A.cap;                    // a set beyond `cap` rows exists only then
    HIP_TRY(h, hipMemsetAsync(A.count, 0, sizeof(int32_t), st));
    if (CAP == 5) sens_launch_lane<5, JAC>(A, grid, lds, st);
    else sens_launch_lane<8, JAC>(A, grid, lds, st);
    HIP_TRY(h, hipGetLastError());
    const long long resident = 4LL * h->numCU;           // (34.6 KB of LDS per one-wavefront workgroup: four per CU)
    const unsigned gridw = (unsigned)(N < resident ? N : resident);
    if (pass2) {
        hipLaunchKernelGGL((sens_wave_kernel<JAC>), dim3(gridw), dim3(64), 0, st, A);
        HIP_TRY(h, hipGetLastError());
    }
    const int32_t rec[LMPC_SENS_INFO_WORDS] = {0, JAC ? 1 : 0, CAP, A.cap, (int32_t)grid, kSensBlock, (int32_t)lds, A.staged + 2 * A.stage_out,
                                               pass2 ? 1 : 0, pass2 ? (int32_t)gridw : 0,
                                               pass2 ? (int32_t)(sizeof(double) * (kSensMaxSet * kSensLd + 2 * kSensMaxSet) + sizeof(int) * kSensMaxSet) : 0,
                                               (int32_t)N};
    h->sensRec.push(rec);
    return LMPC_OK;
}

int sens_device(lmpc_handle *h, bool jac, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar,
                double *out, int32_t *status, void *stream, const char *who) {
    if (!h || N < 0 || N > 0x7fffffffLL) return LMPC_ERR_BADARG;
    LMPC_TRY(sens_refuse(h, who));
    if (N == 0) return LMPC_OK;
    if (!active || !flag || !out || (!jac && !xbar)) return fail(h, LMPC_ERR_BADARG, std::string(who) + ": a required array is NULL");
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    return jac ? sens_launch<true>(h, N, active, flag, xbar, out, status, st)
               : sens_launch<false>(h, N, active, flag, xbar, out, status, st);
}

int sens_host_ptrs(lmpc_handle *h, bool jac, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar,
                   double *out, int32_t *status, const char *who) {
    if (!h || N < 0 || N > 0x7fffffffLL) return LMPC_ERR_BADARG;
    LMPC_TRY(sens_refuse(h, who));
    if (N == 0) return LMPC_OK;
    if (!active || !flag || !out || (!jac && !xbar)) return fail(h, LMPC_ERR_BADARG, std::string(who) + ": a required array is NULL");
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const SensDims d = sens_dims(h);
    const size_t per = jac ? (size_t)d.nout * d.nth : (size_t)d.nth;
    Staging s;
    const uint64_t *dA = static_cast<const uint64_t *>(s.in(active, sizeof(uint64_t) * (size_t)N * d.words));
    const int32_t *dF = static_cast<const int32_t *>(s.in(flag, sizeof(int32_t) * (size_t)N));
    const double *dX = jac ? nullptr : static_cast<const double *>(s.in(xbar, sizeof(double) * (size_t)N * d.nout));
    double *dO = static_cast<double *>(s.out(out, sizeof(double) * (size_t)N * per));
    int32_t *dS = static_cast<int32_t *>(s.out(status, sizeof(int32_t) * (size_t)N));
    if (s.err != hipSuccess) return s.fail(h);
    const int rc = jac ? sens_launch<true>(h, N, dA, dF, dX, dO, dS, nullptr) : sens_launch<false>(h, N, dA, dF, dX, dO, dS, nullptr);
    if (rc != LMPC_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    if (!s.download_all()) return s.fail(h);
    return LMPC_OK;
}

// the kernels' arithmetic on the CPU from a raw pack: every set up to the 64 rows goes through sens_point
int sens_host(bool jac, int n, int m, int ms, int nth, int nout, const double *M, const double *Dth, const double *Rout,
              const double *Xth, const int32_t *sense, const lmpc_settings *s, int is_avi, int64_t N, const uint64_t *active,
              const int32_t *flag, const double *xbar, double *out, int32_t *status) {
    auto bad = [](int code, const char *msg) { g_setup_err = msg; return code; };
    if (n <= 0 || m < 0 || ms < 0 || ms > m || nth < 0 || nout <= 0 || nout > n || N < 0 || !Rout || (m > 0 && (!M || !sense)))
        return bad(LMPC_ERR_BADARG, "lmpc_solve_*_host: inconsistent dimensions or a NULL pack array");
    lmpc_settings st;
    if (s) st = *s; else lmpc_default_settings(&st);
    if (is_avi || st.eps_prox > 0.0)
        return bad(LMPC_ERR_UNSUPPORTED, "lmpc_solve_*_host: variational and proximal-point problems have no derivative here");
    for (int j = 0; j < m; j++)
        if (sense[j] & SENSE_BINARY) return bad(LMPC_ERR_UNSUPPORTED, "lmpc_solve_*_host: BINARY rows have no derivative");
    if (nth == 0) return bad(LMPC_ERR_BADARG, "lmpc_solve_*_host: the problem has no parameter (nth = 0)");
    if (!Xth || (m > 0 && !Dth)) return bad(LMPC_ERR_BADARG, "lmpc_solve_*_host: a NULL pack array");
    if (N == 0) return LMPC_OK;
    if (!active || !flag || !out || (!jac && !xbar)) return bad(LMPC_ERR_BADARG, "lmpc_solve_*_host: a required array is NULL");
    SensDims d;
    d.m = m; d.nth = nth; d.nout = nout; d.words = (2 * m + 63) / 64;
    std::vector<double> C;
    sens_build_pack(n, d, M, nullptr, Dth, Rout, Xth, sense, C);
    const SensView S = sens_view(C.data(), d, st.rho_soft, st.zero_tol);
    const size_t per = jac ? (size_t)nout * nth : (size_t)nth;
    int a[kSensMaxSet] = {};
    for (int64_t p = 0; p < N; p++) {
        const int k = sens_active_rows<kSensMaxSet>(active + (size_t)p * d.words, d.words, m, a);
        double *o = out + (size_t)p * per;
        int stp;
        if (flag[p] < 1) stp = SENS_FAILED_POINT;
        else if (k > kSensMaxSet) stp = SENS_TOO_MANY;
        else stp = jac ? sens_point<kSensMaxSet, true>(S, a, k, nullptr, o)
                       : sens_point<kSensMaxSet, false>(S, a, k, xbar + (size_t)p * nout, o);
        if (stp != SENS_DONE)
            for (size_t i = 0; i < per; i++) o[i] = 0.0;
        if (status) status[p] = stp;
    }
    return LMPC_OK;
}

}  // namespace

int sens_ensure(lmpc_handle *h, int64_t N) {
    if (!h->dSens) {
        std::vector<double> C;
        sens_build_pack(h->P.n, sens_dims(h), h->P.M.data(), h->P.G.data(), h->P.Dth.data(), h->P.Rout.data(), h->P.Xth.data(),
                        h->P.sense.data(), C);
        HIP_TRY(h, h->dSens.reserve(C.size()));
        const hipError_t e = hipMemcpy(h->dSens, C.data(), sizeof(double) * C.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            h->dSens.reset();
            return fail(h, LMPC_ERR_HIP, std::string("hipMemcpy of the derived pack: ") + hipGetErrorString(e));
        }
    }
    HIP_TRY(h, reserve_group(h->sensListCap, N, sized(h->dSensList, (size_t)N), sized(h->dSensCnt, 2)));
    return LMPC_OK;
}

int sens_refusal(lmpc_handle *h, const char *who) { return sens_refuse(h, who); }

void sens_derived_pack(int n, int m, int nth, int nout, const double *M, const double *G, const double *Dth, const double *Rout,
                       const double *Xth, const int32_t *sense, std::vector<double> &C) {
    SensDims d;
    d.m = m; d.nth = nth; d.nout = nout; d.words = (2 * m + 63) / 64;
    sens_build_pack(n, d, M, G, Dth, Rout, Xth, sense, C);
}

int sens_vjp_enqueue(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar, double *thbar,
                     int32_t *status, hipStream_t st, int *list_pass) {
    // (a sweep's VJPs are not the caller's derivative calls: lmpc_sens_launch_info keeps showing those)
    const auto kept = h->sensRec;
    const int rc = sens_launch<false>(h, N, active, flag, xbar, thbar, status, st);
    if (rc == LMPC_OK && list_pass) *list_pass = h->sensRec.newest()[8];
    h->sensRec = kept;
    return rc;
}

int sens_reserve(lmpc_handle *h, int64_t N) {
    if (h->avi || h->P.avi || h->P.prox || h->P.nth == 0) return LMPC_OK;
    for (int32_t s : h->P.sense) if (s & SENSE_BINARY) return LMPC_OK;
    return sens_ensure(h, N);
}

}  // namespace lmpc

using namespace lmpc;

extern "C" {

int lmpc_solve_vjp_device(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, const double *xbar,
                          double *thbar, int32_t *status, void *stream) {
    return sens_device(h, false, N, active, exitflag, xbar, thbar, status, stream, "lmpc_solve_vjp_device");
}

int lmpc_solve_jacobian_device(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, double *J,
                               int32_t *status, void *stream) {
    return sens_device(h, true, N, active, exitflag, nullptr, J, status, stream, "lmpc_solve_jacobian_device");
}

int lmpc_solve_vjp(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, const double *xbar, double *thbar,
                   int32_t *status) {
    return sens_host_ptrs(h, false, N, active, exitflag, xbar, thbar, status, "lmpc_solve_vjp");
}

int lmpc_solve_jacobian(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, double *J, int32_t *status) {
    return sens_host_ptrs(h, true, N, active, exitflag, nullptr, J, status, "lmpc_solve_jacobian");
}

int lmpc_solve_vjp_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                        const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                        const lmpc_settings *s, int is_avi, int64_t N, const uint64_t *active, const int32_t *exitflag,
                        const double *xbar, double *thbar, int32_t *status) {
    (void)du; (void)dl; (void)x0;
    return sens_host(false, n, m, ms, nth, nout, M, Dth, Rout, Xth, sense, s, is_avi, N, active, exitflag, xbar, thbar, status);
}

int lmpc_solve_jacobian_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                             const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                             const lmpc_settings *s, int is_avi, int64_t N, const uint64_t *active, const int32_t *exitflag,
                             double *J, int32_t *status) {
    (void)du; (void)dl; (void)x0;
    return sens_host(true, n, m, ms, nth, nout, M, Dth, Rout, Xth, sense, s, is_avi, N, active, exitflag, nullptr, J, status);
}

int lmpc_sens_launch_info(const lmpc_handle *h, int32_t *out, int max) {
    if (!h || !out || max < 0) return LMPC_ERR_BADARG;
    return h->sensRec.read(out, max);
}

}  // extern "C"
