// Explicit MPC, device half (include/lmpc_hip.h, "Explicit MPC"): the build from a handle's pack with the one upload
// of the table, the evaluation kernel's launch and the fallback of unlocated points to the handle's implicit solve.
#include <hip/hip_runtime.h>

#include <cstring>

#define LMPC_EXPLICIT_KERNELS 1       // the kernels of lmpc_explicit_kernel.hpp live in this translation unit
#include "lmpc_explicit.hpp"
#include "lmpc_explicit_kernel.hpp"
#include "lmpc_internal.hpp"

namespace {

constexpr int kBlock = 256;

int reserve(lmpc_explicit *e, int64_t N) {
    EXP_TRY(e, e->dCount.reserve(1));
    EXP_TRY(e, e->hCount.reserve(1));
    const size_t n = (size_t)N;
    EXP_TRY(e, lmpc::reserve_group(e->cap, N, lmpc::sized(e->dList, n), lmpc::sized(e->dTheta, n * (e->nth > 0 ? e->nth : 1)),
                                   lmpc::sized(e->dX, n * e->nout), lmpc::sized(e->dFlag, n)));
    return LMPC_OK;
}

template <int NT>
void launch_eval(const lmpc::ExplicitView &v, int64_t N, const double *theta, double *x, int32_t *flag, int32_t *region,
                 int32_t *list, int32_t *count, hipStream_t st) {
    const unsigned grid = (unsigned)((N + kBlock - 1) / kBlock);
    const size_t lds = sizeof(double) * kBlock * (size_t)v.nth;
    hipLaunchKernelGGL(lmpc::explicit_eval_kernel<NT>, dim3(grid), dim3(kBlock), lds, st, v, N, theta, x, flag, region,
                       list, count);
}

}  // namespace

namespace lmpc {
int explicit_reserve(lmpc_explicit *e, int64_t N) { return reserve(e, N); }
}  // namespace lmpc

extern "C" {

int lmpc_explicit_build(lmpc_explicit **out, lmpc_handle *h, int64_t N, const double *theta, const uint64_t *active,
                        const int32_t *exitflag, const lmpc_explicit_opts *opts) {
    if (!out) return LMPC_ERR_BADARG;
    *out = nullptr;
    if (!h) return LMPC_ERR_BADARG;
    const lmpc::HostPack &P = h->P;
    lmpc_explicit_opts o;
    if (opts) o = *opts; else lmpc_explicit_default_opts(&o);
    lmpc_explicit *e = new lmpc_explicit();
    int rc = lmpc::explicit_build_pack(e, P.n, P.m, P.ms, P.nth, P.nout, P.M.data(), P.du0.data(), P.dl0.data(),
                                       P.Dth.data(), P.Rout.data(), P.x0.data(), P.Xth.data(), P.sense.data(), h->S,
                                       (P.avi && !P.prox) ? 1 : 0, N, theta, active, exitflag, o);
    if (rc == LMPC_OK) {
        lmpc::DeviceScope scope;
        hipError_t he = scope.enter(h->device);
        if (he == hipSuccess) he = e->dBlob.reserve(e->blob.size());
        if (he == hipSuccess) he = hipMemcpy(e->dBlob, e->blob.data(), sizeof(uint64_t) * e->blob.size(), hipMemcpyHostToDevice);
        if (he != hipSuccess) {
            e->err = std::string("lmpc_explicit_build: upload of the table: ") + hipGetErrorString(he);
            rc = he == hipErrorNoDevice ? LMPC_ERR_NOGPU : LMPC_ERR_HIP;
        }
    }
    if (rc != LMPC_OK) {
        g_setup_err = e->err;
        lmpc_explicit_free(e);
        return rc;
    }
    e->h = h;
    e->device = h->device;
    *out = e;
    return LMPC_OK;
}

int lmpc_explicit_eval_device(lmpc_explicit *e, int64_t N, const double *theta, double *x, int32_t *exitflag,
                              int32_t *region, void *stream) {
    if (!e) return LMPC_ERR_BADARG;
    if (!e->h || !e->dBlob) return efail(e, LMPC_ERR_BADARG, "lmpc_explicit_eval_device: built without a handle (lmpc_explicit_build_ldp)");
    if (N < 0 || N > 0x7fffffffLL || (N > 0 && (!x || !exitflag || (e->nth > 0 && !theta))))
        return efail(e, LMPC_ERR_BADARG, "lmpc_explicit_eval_device: NULL array or N outside [0, 2^31 - 1]");
    if (N == 0) return LMPC_OK;
    lmpc::DeviceScope scope;
    EXP_TRY(e, scope.enter(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = reserve(e, N);
    if (rc != LMPC_OK) return rc;
    int32_t *reg = region ? region : e->dFlag;          // (the fallback's flags reuse this buffer only after the kernel)
    const int64_t *head = reinterpret_cast<const int64_t *>(e->blob.data());
    const lmpc::ExplicitView v = lmpc::explicit_view(e->dBlob, head, e->primal_tol, e->band, e->rho_soft);
    EXP_TRY(e, hipMemsetAsync(e->dCount, 0, sizeof(int32_t), st));
    if (e->nth <= 8) launch_eval<8>(v, N, theta, x, exitflag, reg, e->dList, e->dCount, st);
    else if (e->nth <= 16) launch_eval<16>(v, N, theta, x, exitflag, reg, e->dList, e->dCount, st);
    else launch_eval<32>(v, N, theta, x, exitflag, reg, e->dList, e->dCount, st);
    EXP_TRY(e, hipGetLastError());
    // the one synchronisation: how many points the implicit path takes
    EXP_TRY(e, hipMemcpyAsync(e->hCount, e->dCount, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EXP_TRY(e, hipStreamSynchronize(st));
    const int64_t cnt = *e->hCount;
    if (cnt < 0 || cnt > N) return efail(e, LMPC_ERR_HIP, "lmpc_explicit_eval_device: unlocated count out of range");
    if (cnt == 0) return LMPC_OK;
    if (e->nth > 0) {
        hipLaunchKernelGGL(lmpc::explicit_gather_kernel, dim3((unsigned)((cnt + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           cnt, e->nth, e->dList, theta, e->dTheta);
        EXP_TRY(e, hipGetLastError());
    }
    rc = lmpc_solve_batch_device(e->h, cnt, e->dTheta, e->dX, e->dFlag, nullptr, nullptr, nullptr, stream);
    if (rc != LMPC_OK) return efail(e, rc, std::string("lmpc_explicit_eval_device: implicit solve: ") + lmpc_last_error(e->h));
    hipLaunchKernelGGL(lmpc::explicit_scatter_kernel, dim3((unsigned)((cnt + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       cnt, e->nout, e->dList, e->dX, e->dFlag, x, exitflag);
    EXP_TRY(e, hipGetLastError());
    return LMPC_OK;
}

int lmpc_explicit_eval(lmpc_explicit *e, int64_t N, const double *theta, double *x, int32_t *exitflag, int32_t *region) {
    if (!e) return LMPC_ERR_BADARG;
    if (N < 0 || (N > 0 && (!x || !exitflag || (e->nth > 0 && !theta))))
        return efail(e, LMPC_ERR_BADARG, "lmpc_explicit_eval: NULL array or negative N");
    if (N == 0) return LMPC_OK;
    if (!e->h) return efail(e, LMPC_ERR_BADARG, "lmpc_explicit_eval: built without a handle (lmpc_explicit_build_ldp)");
    lmpc::DeviceScope scope;
    EXP_TRY(e, scope.enter(e->device));
    const size_t n = (size_t)N, nth = (size_t)e->nth, nout = (size_t)e->nout;
    lmpc::DevBuf<double> dth, dx;
    lmpc::DevBuf<int32_t> df, dr;
    hipError_t he = dth.reserve(n * (nth > 0 ? nth : 1));
    if (he == hipSuccess) he = dx.reserve(n * nout);
    if (he == hipSuccess) he = df.reserve(n);
    if (he == hipSuccess) he = dr.reserve(n);
    if (he == hipSuccess && nth > 0) he = hipMemcpy(dth, theta, sizeof(double) * n * nth, hipMemcpyHostToDevice);
    int rc = LMPC_OK;
    if (he == hipSuccess) rc = lmpc_explicit_eval_device(e, N, dth, dx, df, dr, nullptr);
    if (he == hipSuccess && rc == LMPC_OK) he = hipStreamSynchronize(nullptr);
    if (he == hipSuccess && rc == LMPC_OK) he = hipMemcpy(x, dx, sizeof(double) * n * nout, hipMemcpyDeviceToHost);
    if (he == hipSuccess && rc == LMPC_OK) he = hipMemcpy(exitflag, df, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (he == hipSuccess && rc == LMPC_OK && region) he = hipMemcpy(region, dr, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (rc != LMPC_OK) return rc;
    if (he != hipSuccess) return efail(e, LMPC_ERR_HIP, std::string("lmpc_explicit_eval: ") + hipGetErrorString(he));
    return lmpc_check(e->h) == LMPC_OK ? LMPC_OK : efail(e, LMPC_ERR_HIP, std::string("lmpc_explicit_eval: ") + lmpc_last_error(e->h));
}

void lmpc_explicit_free(lmpc_explicit *e) {
    if (!e) return;
    lmpc::DeviceScope scope;
    if (e->dBlob || e->dCount || e->dList) {
        (void)scope.enter(e->device >= 0 ? e->device : 0);
        (void)hipDeviceSynchronize();
    }
    delete e;
}

}  // extern "C"
