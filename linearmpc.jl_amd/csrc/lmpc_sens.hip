// Differentiable batched solve (include/lmpc_hip.h, "Differentiable solve"): VJP and Jacobian of x*(theta) per point
// from the optimal active set -- derived pack, dispatch of the two kernels (lmpc_sens_kernel.hpp), the host-pointer
// wrappers and the host twins that run the same arithmetic without a GPU.
#define LMPC_SENS_KERNELS 1
#include "lmpc_internal.hpp"
#include "lmpc_sens_kernel.hpp"

#include <cstring>

namespace lmpc {
namespace {

SensDims sens_dims(int m, int nth, int nout) {
    SensDims d;
    d.m = m; d.nth = nth; d.nout = nout; d.words = (2 * m + 63) / 64;
    return d;
}

template <int CAP, bool JAC>
void sens_launch_lane(const SensArgs &A, unsigned grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((sens_lane_kernel<CAP, JAC>), dim3(grid), dim3(kSensBlock), lds, st, A);
}

// the launches of one call; rec: their record, for the caller to keep
template <bool JAC>
int sens_launch(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar, double *out,
                int32_t *status, hipStream_t st, int32_t (&rec)[LMPC_SENS_INFO_WORDS]) {
    LMPC_TRY(sens_ensure(h, N));
    SensArgs A;
    A.C = h->dSens; A.d = sens_dims(h->P.m, h->P.nth, h->P.nout);
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
    const unsigned gridw = sens_wave_grid(h, N);
    if (pass2) {
        hipLaunchKernelGGL((sens_wave_kernel<JAC>), dim3(gridw), dim3(64), 0, st, A);
        HIP_TRY(h, hipGetLastError());
    }
    const int32_t r[LMPC_SENS_INFO_WORDS] = {0, JAC ? 1 : 0, CAP, A.cap, (int32_t)grid, kSensBlock, (int32_t)lds, A.staged + 2 * A.stage_out,
                                             pass2 ? 1 : 0, pass2 ? (int32_t)gridw : 0, pass2 ? (int32_t)sizeof(SensWaveLds) : 0, (int32_t)N};
    std::memcpy(rec, r, sizeof(r));
    return LMPC_OK;
}

// a public call on device arrays (enqueued on `stream`) or on host arrays (staged, run and copied back)
int sens_call(lmpc_handle *h, bool jac, bool host, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar,
              double *out, int32_t *status, void *stream, const char *who) {
    if (!h || N < 0 || N > 0x7fffffffLL) return LMPC_ERR_BADARG;
    LMPC_TRY(sens_refuse(h, who));
    if (N == 0) return LMPC_OK;
    if (!active || !flag || !out || (!jac && !xbar)) return fail(h, LMPC_ERR_BADARG, std::string(who) + ": a required array is NULL");
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging s;
    if (host) {
        const SensDims d = sens_dims(h->P.m, h->P.nth, h->P.nout);
        const size_t per = jac ? (size_t)d.nout * d.nth : (size_t)d.nth;
        active = static_cast<const uint64_t *>(s.in(active, sizeof(uint64_t) * (size_t)N * d.words));
        flag = static_cast<const int32_t *>(s.in(flag, sizeof(int32_t) * (size_t)N));
        xbar = jac ? nullptr : static_cast<const double *>(s.in(xbar, sizeof(double) * (size_t)N * d.nout));
        out = static_cast<double *>(s.out(out, sizeof(double) * (size_t)N * per));
        status = static_cast<int32_t *>(s.out(status, sizeof(int32_t) * (size_t)N));
        if (s.err != hipSuccess) return s.fail(h);
    }
    hipStream_t st = host ? nullptr : (hipStream_t)stream;
    int32_t rec[LMPC_SENS_INFO_WORDS];
    LMPC_TRY(jac ? sens_launch<true>(h, N, active, flag, xbar, out, status, st, rec)
                 : sens_launch<false>(h, N, active, flag, xbar, out, status, st, rec));
    h->sensRec.push(rec);
    if (!host) return LMPC_OK;
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    if (!s.download_all()) return s.fail(h);
    return LMPC_OK;
}

// lmpc_solve_vjp_host / lmpc_solve_jacobian_host
int sens_host(bool jac, int n, int m, int ms, int nth, int nout, const double *M, const double *Dth, const double *Rout,
              const double *Xth, const int32_t *sense, const lmpc_settings *s, int is_avi, int64_t N, const uint64_t *active,
              const int32_t *flag, const double *xbar, double *out, int32_t *status) {
    lmpc_settings st;
    LMPC_TRY(sens_check_pack("lmpc_solve_*_host", n, m, ms, nth, nout, M, Dth, Rout, Xth, sense, true, s, is_avi, N, &st));
    if (N == 0) return LMPC_OK;
    if (!active || !flag || !out || (!jac && !xbar)) {
        g_setup_err = "lmpc_solve_*_host: a required array is NULL";
        return LMPC_ERR_BADARG;
    }
    const SensDims d = sens_dims(m, nth, nout);
    std::vector<double> C;
    sens_build_pack(n, d, M, nullptr, Dth, Rout, Xth, sense, C);
    sens_host_points(sens_view(C.data(), d, st.rho_soft, st.zero_tol), d, jac, N, active, flag, xbar, out, status);
    return LMPC_OK;
}

}  // namespace

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

const char *sens_no_derivative(const lmpc_handle *h, int *code) {
    int c = LMPC_ERR_UNSUPPORTED;
    const char *why = nullptr;
    if (h->avi || h->P.avi || h->P.prox) why = ": variational and proximal-point handles have no derivative here";
    for (int32_t s : h->P.sense)
        if (!why && (s & SENSE_BINARY)) why = ": BINARY rows have no derivative";
    if (!why && h->P.nth == 0) { why = ": the problem has no parameter (nth = 0)"; c = LMPC_ERR_BADARG; }
    if (code) *code = c;
    return why;
}

int sens_refuse(lmpc_handle *h, const char *who) {
    int code = LMPC_OK;
    if (const char *why = sens_no_derivative(h, &code)) return fail(h, code, std::string(who) + why);
    return LMPC_OK;
}

int sens_check_pack(const char *who, int n, int m, int ms, int nth, int nout, const double *M, const double *Dth, const double *Rout,
                    const double *Xth, const int32_t *sense, bool bounds, const lmpc_settings *s, int is_avi, int64_t N,
                    lmpc_settings *st) {
    auto bad = [who](int code, const char *msg) { g_setup_err = std::string(who) + msg; return code; };
    if (n <= 0 || m < 0 || ms < 0 || ms > m || nth < 0 || nout <= 0 || nout > n || N < 0 || !Rout || (m > 0 && (!M || !sense)))
        return bad(LMPC_ERR_BADARG, ": inconsistent dimensions or a NULL pack array");
    if (s) *st = *s; else lmpc_default_settings(st);
    if (is_avi || st->eps_prox > 0.0) return bad(LMPC_ERR_UNSUPPORTED, ": variational and proximal-point problems have no derivative here");
    for (int j = 0; j < m; j++)
        if (sense[j] & SENSE_BINARY) return bad(LMPC_ERR_UNSUPPORTED, ": BINARY rows have no derivative");
    if (nth == 0) return bad(LMPC_ERR_BADARG, ": the problem has no parameter (nth = 0)");
    if (!Xth || (m > 0 && (!Dth || !bounds))) return bad(LMPC_ERR_BADARG, ": a NULL pack array");
    return LMPC_OK;
}

void sens_host_points(const SensView &S, const SensDims &d, bool jac, int64_t N, const uint64_t *active, const int32_t *flag,
                      const double *xbar, double *out, int32_t *status) {
    const size_t per = jac ? (size_t)d.nout * d.nth : (size_t)d.nth;
    int a[kSensMaxSet] = {};
    for (int64_t p = 0; p < N; p++) {
        const int k = sens_active_rows<kSensMaxSet>(active + (size_t)p * d.words, d.words, d.m, a);
        double *o = out + (size_t)p * per;
        int stp = sens_classify(flag[p], k, kSensMaxSet);
        if (stp == SENS_DONE)
            stp = jac ? sens_point<kSensMaxSet, true>(S, a, k, nullptr, o)
                      : sens_point<kSensMaxSet, false>(S, a, k, xbar + (size_t)p * d.nout, o);
        if (stp != SENS_DONE)
            for (size_t i = 0; i < per; i++) o[i] = 0.0;
        if (status) status[p] = stp;
    }
}

int sens_cap_of(const lmpc_handle *h) {
    if (h->sensCap == 5 || h->sensCap == 8) return h->sensCap;
    const int reach = h->P.n + h->P.nsoft < h->P.m ? h->P.n + h->P.nsoft : h->P.m;      // rows a set of this problem reaches
    return reach <= 5 ? 5 : 8;
}

unsigned sens_wave_grid(const lmpc_handle *h, int64_t N) {
    const int64_t resident = 4LL * h->numCU;            // (sizeof(SensWaveLds) per one-wavefront workgroup: four per CU)
    return (unsigned)(N < resident ? N : resident);
}

int sens_ensure(lmpc_handle *h, int64_t N) {
    if (!h->dSens) {
        std::vector<double> C;
        sens_build_pack(h->P.n, sens_dims(h->P.m, h->P.nth, h->P.nout), h->P.M.data(), h->P.G.data(), h->P.Dth.data(), h->P.Rout.data(),
                        h->P.Xth.data(), h->P.sense.data(), C);
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

int sens_vjp_enqueue(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar, double *thbar,
                     int32_t *status, hipStream_t st, int *list_pass) {
    // (a sweep's VJPs are not the caller's derivative calls: their records are not kept, and lmpc_sens_launch_info
    // keeps showing those)
    int32_t rec[LMPC_SENS_INFO_WORDS];
    LMPC_TRY(sens_launch<false>(h, N, active, flag, xbar, thbar, status, st, rec));
    if (list_pass) *list_pass = rec[8];
    return LMPC_OK;
}

int sens_reserve(lmpc_handle *h, int64_t N) { return sens_no_derivative(h, nullptr) ? LMPC_OK : sens_ensure(h, N); }

}  // namespace lmpc

using namespace lmpc;

extern "C" {

int lmpc_solve_vjp_device(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, const double *xbar,
                          double *thbar, int32_t *status, void *stream) {
    return sens_call(h, false, false, N, active, exitflag, xbar, thbar, status, stream, "lmpc_solve_vjp_device");
}

int lmpc_solve_jacobian_device(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, double *J,
                               int32_t *status, void *stream) {
    return sens_call(h, true, false, N, active, exitflag, nullptr, J, status, stream, "lmpc_solve_jacobian_device");
}

int lmpc_solve_vjp(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, const double *xbar, double *thbar,
                   int32_t *status) {
    return sens_call(h, false, true, N, active, exitflag, xbar, thbar, status, nullptr, "lmpc_solve_vjp");
}

int lmpc_solve_jacobian(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, double *J, int32_t *status) {
    return sens_call(h, true, true, N, active, exitflag, nullptr, J, status, nullptr, "lmpc_solve_jacobian");
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
