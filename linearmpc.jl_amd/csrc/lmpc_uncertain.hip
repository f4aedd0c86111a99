// C ABI of liblmpc_hip.so, the scenario loop under uncertainty (lmpc_simulate_scenario_uncertain*): lmpc_scenario.hip's
// loop with additive process noise on the state, additive measurement noise -- both supplied or drawn on the device --
// and a table of plant variants.  Per step a PRE kernel, the handle's solve (api_launch), a POST kernel
// (lmpc_uncertain_kernels.hpp); nothing but enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_uncertain_host.hpp"

using namespace lmpc;

namespace {

std::string call_problem(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un, const double *x,
                         const double *xhat, const double *uprev, bool device) {
    const HandleObserver ob(h);
    std::string msg = uncertain_problem(h->P.nth, h->P.nout, ob.ptr, s, un);
    if (msg.empty()) msg = call_size_problem(N, T, x, un);
    if (msg.empty()) msg = call_array_problem(N, s, xhat, uprev, device);
    return msg;
}

// the run itself, on device arrays, once the call has passed its refusals
int run(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un, double *x, double *xhat,
        double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, hipStream_t st) {
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    const int nx = s->nx, nu = s->nu, nd = s->nd;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, nd, s->ny, s->plant, s->measurement, s->cost);
    UncStep U = pack_uncertainty(hostC, un, nx);
    U.n_plants = un->n_plants;
    if (un->n_plants > 0) {                            // the table: n_plants arrays in the layout of s->plant
        K.plant = (int)hostC.size();
        hostC.insert(hostC.end(), un->plants, un->plants + (size_t)un->n_plants * nx * (1 + nx + nu + nd));
    }
    U.plant_index = un->plant_index;
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    ScnPre A; ScnPost B;
    { const int rcb = scn_begin(h, h->scnScr, N, s, x, xhat, uprev, X_traj, flag_min, h->simTheta, h->simU, h->simFlag, st, A, B);
      if (rcb != LMPC_OK) return rcb; }
    const bool gauss = unc_gauss(U), wantCost = scn_want_cost(s);
    const unsigned grid = (unsigned)((N + 255) / 256);
    return scn_loop(h, s, N, T, U_traj, X_traj, A, B,
        [&](int k) {
            unc_advance(U, un, N, nx, k);
            launch_uncertain_pre(N, A, K, U, st);
        },
        [&](int k) { return scn_solve(h, s, N, k, st); },
        [&](int) {
            dispatch_nx(nx, [&](auto NX) {
                if (gauss && wantCost) hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, true, true>), dim3(grid), dim3(256), 0, st, B, K, U);
                else if (gauss) hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, false, true>), dim3(grid), dim3(256), 0, st, B, K, U);
                else if (wantCost) hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, true>), dim3(grid), dim3(256), 0, st, B, K, U);
                else hipLaunchKernelGGL((uncertain_post_kernel<decltype(NX)::value, false>), dim3(grid), dim3(256), 0, st, B, K, U);
            });
        });
}

// ---- lmpc_noise_draw_*: the e of one (global scenario, global step, stream), all w components, as UncDraws and
// unc_value give them to the loop: one source for the CPU and the GPU.  c = [lo | span | hi] (uniform) or [mean | std].
__host__ __device__ __forceinline__ void noise_draw_record(const double *__restrict__ c, int w, int gaussian, uint32_t k0,
                                                           uint32_t k1, unsigned long long g, uint32_t step, uint32_t stream,
                                                           double *__restrict__ out) {
    for (int j = 0; 2 * j < w; j++) {
        uint32_t r[4] = {(uint32_t)g, (uint32_t)(g >> 32), step, (stream << 16) | (uint32_t)j};
        philox4x32_10(r, k0, k1);
        double a = philox_unit(r[0], r[1]), b = philox_unit(r[2], r[3]);
        if (gaussian) {
            const double ua = a, ub = b;
            nm_gauss_pair(ua, ub, a, b);
        }
        for (int q = 2 * j; q < 2 * j + 2 && q < w; q++) {
            const double v = q & 1 ? b : a;
            if (gaussian) {
                out[q] = nm_gauss_value(c[q], c[w + q], v);
            } else {
                const double e = LMPC_PP_ADD(c[q], LMPC_PP_MUL(v, c[w + q])), hi = c[2 * w + q];
                out[q] = e < hi ? e : hi;
            }
        }
    }
}

// one (scenario, step) per lane: record idx = i * T + k goes to out + idx * w
__global__ __launch_bounds__(256) void noise_draw_kernel(const double *__restrict__ c, int w, int gaussian, uint32_t k0, uint32_t k1,
                                                         unsigned long long goff, uint32_t step0, uint32_t stream, int T,
                                                         long long total, double *__restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long i = idx / T;
    const int k = (int)(idx - i * T);
    noise_draw_record(c, w, gaussian, k0, k1, goff + (unsigned long long)i, step0 + (uint32_t)k, stream, out + idx * w);
}

std::string draw_problem(const lmpc_noise *n, int stream, int64_t N, int32_t step_offset, int T, const double *out) {
    if (!n) return "noise: NULL source";
    const std::string msg = noise_problem("noise", *n);
    if (!msg.empty()) return msg;
    if (!n->lo) return "noise.lo: NULL (a supplied source draws nothing)";
    if (stream != 0 && stream != 1) return "stream: must be 0 (process) or 1 (measurement), got " + std::to_string(stream);
    if (N < 0) return "N: negative";
    if (T < 0) return "T: negative";
    if (step_offset < 0) return "step_offset: negative";
    if ((int64_t)step_offset + T > 2147483647LL) return "step_offset: step_offset + T exceeds 2^31 - 1";
    if (T > 0 && N > (int64_t)0x7fffffff * 256 / T) return "N: N * T exceeds what one launch covers";
    if (N > 0 && T > 0 && n->w > 0 && !out) return "out: NULL";
    return "";
}

// [lo | span | hi] or [mean | std] as noise_draw_record takes them
std::vector<double> draw_constants(const lmpc_noise &n) {
    std::vector<double> c;
    append_draw_constants(c, n);
    return c;
}

}  // namespace

extern "C" {

int lmpc_noise_draw_host(const lmpc_noise *noise, uint64_t seed, int stream, int64_t scenario_offset, int64_t N,
                         int32_t step_offset, int T, double *out) {
    const std::string msg = draw_problem(noise, stream, N, step_offset, T, out);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_noise_draw_host: " + msg);
    if (N == 0 || T == 0 || noise->w == 0) return LMPC_OK;
    const std::vector<double> c = draw_constants(*noise);
    const int w = noise->w, gaussian = noise->dist == LMPC_NOISE_GAUSSIAN;
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
    for (int64_t i = 0; i < N; i++)
        for (int k = 0; k < T; k++)
            noise_draw_record(c.data(), w, gaussian, k0, k1, (unsigned long long)scenario_offset + (unsigned long long)i,
                              (uint32_t)(step_offset + k), (uint32_t)stream, out + ((size_t)i * T + k) * w);
    return LMPC_OK;
}

int lmpc_noise_draw_device(lmpc_handle *h, const lmpc_noise *noise, uint64_t seed, int stream, int64_t scenario_offset,
                           int64_t N, int32_t step_offset, int T, double *out, void *hip_stream) {
    if (!h) return LMPC_ERR_BADARG;
    const std::string msg = draw_problem(noise, stream, N, step_offset, T, out);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_noise_draw_device: " + msg);
    if (N == 0 || T == 0 || noise->w == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)hip_stream;
    ScnConst K{};
    const std::vector<double> c = draw_constants(*noise);
    { const int rcu = upload_constants(h, c, K, st); if (rcu != LMPC_OK) return rcu; }
    const long long total = (long long)N * T;
    hipLaunchKernelGGL(noise_draw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, K.c, noise->w,
                       (int)(noise->dist == LMPC_NOISE_GAUSSIAN), (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
                       (unsigned long long)scenario_offset, (uint32_t)step_offset, (uint32_t)stream, T, total, out);
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}


int lmpc_scenario_uncertain_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s,
                                  const lmpc_uncertainty *un) {
    const std::string msg = uncertain_problem(nth, nout, observer, s, un);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_scenario_uncertain_check: " + msg);
    return LMPC_OK;
}

int lmpc_simulate_scenario_uncertain_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                            const lmpc_uncertainty *un, double *x, double *xhat, double *uprev,
                                            double *U_traj, double *X_traj, int32_t *flag_min, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const std::string msg = call_problem(h, N, T, s, un, x, xhat, uprev, true);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_uncertain_device: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    return run(h, N, T, s, un, x, xhat, uprev, U_traj, X_traj, flag_min, (hipStream_t)stream);
}

int lmpc_simulate_scenario_uncertain(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un,
                                     double *x, double *xhat, double *uprev, double *U_traj, double *X_traj, int32_t *flag_min) {
    if (!h) return LMPC_ERR_BADARG;
    // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
    const std::string msg = call_problem(h, N, T, s, un, x, xhat, uprev, false);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_uncertain: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    lmpc_uncertainty du = stage_uncertainty(sg, un, N, T, s->nx);
    du.plant_index = static_cast<const int32_t *>(sg.in(un->plant_index, sizeof(int32_t) * (size_t)N));
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = run(h, N, T, &g.d, &du, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

}  // extern "C"
