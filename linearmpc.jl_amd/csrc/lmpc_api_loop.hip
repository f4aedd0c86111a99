// C ABI of liblmpc_hip.so, second unit (round 5: split off lmpc_api.hip): everything that runs a LOOP around the batched solve
// on the device -- closed-loop simulation (lmpc_simulate*), the generated controller's entry points
// (lmpc_set_parameter_layout, lmpc_compute_control*, lmpc_form_parameter_device) and the generated observer
// (lmpc_set_observer, lmpc_predict_state*, lmpc_correct_state*).  Setup, the plain solves, options and the launch
// policy stay in lmpc_api.hip; this unit reaches them through the api_* functions of lmpc_internal.hpp.
// What a loop wants of a launch -- lmpc_simulate_device: the fused plant step, the scenario-asynchronous rounds, the kept
// factors, no profiling inside the rounds; lmpc_compute_control_device: the gather -- it says in a LoopMode on its own
// stack, an argument of api_launch.  Nothing of it is written to the handle, so there is nothing to take back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_lane_kernel.hpp"
#include "lmpc_sim_kernels.hpp"

using namespace lmpc;

namespace lmpc {
// this unit's code object onto the device without a launch (setup; see preload_code in lmpc_api.hip)
void loop_preload() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, (const void *)form_theta_kernel<double>);
    (void)hipGetLastError();
}
}  // namespace lmpc

namespace {
// host-pointer closed loop in either precision: device copies of the caller's arrays around lmpc_simulate_device /
// lmpc_simulate_f32_device.  uprev == NULL: zeros, and nothing copied back.  The binary64 loop only enqueues, so the
// device is synchronised before the results are read; the binary32 one leaves that to the blocking copies.
template <typename R>
int simulate_host(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev, const double *F, const double *G, R *x,
                  const R *r, R *uprev, R *U_traj, R *X_traj, int32_t *flag_min, int warm) {
    if (!h) return LMPC_ERR_BADARG;
    if (N <= 0 || T <= 0) return N < 0 || T < 0 ? LMPC_ERR_BADARG : LMPC_OK;
    LMPC_ENTER_DEVICE(h);
    const size_t n = (size_t)N, nu = (size_t)h->P.nout;
    Staging sg;
    R *dx = static_cast<R *>(sg.out(x, sizeof(R) * n * nx, true));
    R *dr = nr > 0 ? static_cast<R *>(sg.in(r, sizeof(R) * n * nr)) : nullptr, *du = nullptr;
    if (nuprev > 0) du = static_cast<R *>(uprev ? sg.out(uprev, sizeof(R) * n * nuprev, true) : sg.zeros(sizeof(R) * n * nuprev));
    R *dU = static_cast<R *>(sg.out(U_traj, sizeof(R) * T * n * nu));
    R *dX = static_cast<R *>(sg.out(X_traj, sizeof(R) * (T + 1) * n * nx));
    int32_t *df = static_cast<int32_t *>(sg.out(flag_min, sizeof(int32_t) * n));
    if (sg.err != hipSuccess) return sg.fail(h);
    int rc;
    if constexpr (std::is_same<R, double>::value) {
        rc = lmpc_simulate_device(h, N, T, nx, nr, nuprev, F, G, dx, dr, du, dU, dX, df, warm, nullptr);
        if (rc == LMPC_OK) sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    } else {
        rc = lmpc_simulate_f32_device(h, N, T, nx, nr, nuprev, F, G, dx, dr, du, dU, dX, df, warm, nullptr);
    }
    if (rc == LMPC_OK && !(sg.err == hipSuccess && sg.download_all())) return sg.fail(h);
    return rc;
}
}  // namespace

extern "C" {

// per-scenario kept closed-loop state of the wavefront path (working set + factorisation, lmpc_wave_kernel.hpp): makes
// room for N scenarios if the device has it to spare and marks every state "nothing kept"; *keep: whether room was made
static int ensure_keep(lmpc_handle *h, int64_t N, hipStream_t st, bool *keep) {
    const size_t keepR = (size_t)h->W.keepStride, keepI = 5 * 64;
    if (N > h->keepCap) {
        h->dKeepR.reset(); h->dKeepI.reset(); h->keepCap = 0;
        // (17 GB for 1e6 scenarios at capacity 64: only while it is at most half of what the device has free --
        // beyond that the loop runs on masks rather than crowding out the caller)
        size_t freeB = 0, totalB = 0;
        const size_t needB = (sizeof(double) * keepR + sizeof(int32_t) * keepI) * (size_t)N;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { freeB = 0; (void)hipGetLastError(); }
        // (no room, or an allocation that fails all the same: the group stays empty and the loop runs without it)
        if (needB > freeB / 2 ||
            reserve_group(h->keepCap, N, sized(h->dKeepR, sizeof(double) * keepR * (size_t)N),
                          sized(h->dKeepI, keepI * (size_t)N)) != hipSuccess)
            (void)hipGetLastError();
    }
    if (N <= h->keepCap) {
        // nothing kept yet: the size word of every scenario's state to -1
        HIP_TRY(h, hipMemset2DAsync(h->dKeepI + 256, sizeof(int32_t) * keepI, 0xFF, sizeof(int32_t), (size_t)N, st));
        *keep = true;
    }
    return LMPC_OK;
}

int lmpc_simulate_device(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev, const double *F,
                         const double *G, double *x, const double *r, double *uprev, double *U_traj,
                         double *X_traj, int32_t *flag_min, int warm, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const int nu = h->P.nout;
    if (N < 0 || T < 0 || nx <= 0 || nx > 32 || nr < 0 || nuprev < 0 || nuprev > nu || !F || !G || (N > 0 && !x) ||
        (nuprev > 0 && N > 0 && !uprev) || nx + nr + nuprev != h->P.nth)
        return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_device: theta = [x; r; uprev] must match the handle "
                                        "(nx + nr + nuprev == nth, nout == nu, nx <= 32)");
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    HIP_TRY(h, hipMemcpyAsync(h->simFG, F, sizeof(double) * nx * nx, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->simFG + nx * nx, G, sizeof(double) * nx * nu, hipMemcpyHostToDevice, st));
    if (X_traj) HIP_TRY(h, hipMemcpyAsync(X_traj, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    const unsigned grid = (unsigned)((N + 255) / 256);
    if (h->useWave && !h->avi && !h->waveProbed && N >= 4 * kProbe) {
        // fresh handle: the working-set sizes of the first step's problems decide how the loop's launches are shaped
        // (wave_probe) -- on the records of the leading scenarios, formed here and formed again with all the others below
        hipLaunchKernelGGL(form_theta_kernel<double>, dim3((unsigned)((kProbe + 255) / 256)), dim3(256), 0, st, h->simTheta, x, r,
                           uprev, nx, nr, nuprev, (long long)kProbe);
        HIP_TRY(h, hipGetLastError());
        const int rcp = api_wave_probe(h, h->simTheta, N, st);
        if (rcp != LMPC_OK) return rcp;
    }
    // theta = [x; r; uprev] is formed once; from then on every scenario's state lives in its record
    // (the scenario-asynchronous loop forms it in its first streaming pass)
    // (round 3: also on the wavefront-kernel path -- soft rows, many rows: the same streaming half on the handle's
    // screening pack, the wavefront kernel as the iterating half; binary64, no branch and bound)
    const size_t simLds = sizeof(double) * ((((size_t)h->P.m + 7) & ~(size_t)7) * (h->L.nthp + 2) + (size_t)kMaxSimU * h->L.nthp + kMaxSimU + 64 + 8 * kMaxSimU);
    // It is OPT-IN there ("sim_async" 2): measured on the benchmark class (pendulum N = 50, 2e5 scenarios x 100 steps,
    // tools/sim_bench.py) the rounds lose to the lock-step loop -- 4.9e8 against 5.3e8 scenario-steps/s from
    // closed-loop-visited starts, 1.17e9 against 1.31e9 with 90 % of the scenarios at rest: what costs the time is the
    // wavefront kernel on the transient's problems, which both loops run, and a round adds a launch and a host round
    // trip where the lock-step loop adds a 25 us screening pass.
    // (end of round 3: with RUN-AHEAD -- a scenario's consecutive steps that need iterations stay inside the wavefront
    // kernel, warm on the factor as it stands in LDS -- the rounds win on every workload but the six-slot problems:
    // 1.28e9 against 8.7e8 on that benchmark, 2.7e9 against 2.1e9 with 90 % at rest, 1.6e9 against 1.2e9 at 1e6
    // scenarios.  Default from then on whenever run-ahead applies: warm with "sim_keep_factor" 1, or cold.)
    const bool runAhead = h->simRunAhead && (!warm || h->simKeep) && (h->P.m + 63) / 64 <= kWaveRunAheadSlots;
    const bool waveAsync = h->useWave && (h->simAsync >= 2 || (h->simAsync >= 1 && runAhead)) && !h->bnb && nu <= kMaxSimU &&
                           nx <= 8 && h->P.nth <= 16 && api_wave_screens(h, N) && simLds <= 48 * 1024;
    const bool asyncLoop = waveAsync ||
                           (!h->useWave && h->simFused && h->simAsync && nu <= kMaxSimU && nx <= 8 && h->P.nth <= 16 && api_will_screen(h, N));
    if (!asyncLoop)
        hipLaunchKernelGGL(form_theta_kernel<double>, dim3(grid), dim3(256), 0, st, h->simTheta, x, r, uprev, nx, nr,
                           nuprev, (long long)N);
    // Lane / screening kernels: the kernel that finishes a problem also advances its scenario and
    // writes the next step's record into the other theta buffer (SimFuse) -- a closed-loop step is
    // the solve's two launches and nothing else
    // Scenario-asynchronous loop (lmpc_simrun_kernel.hpp): scenarios are independent, so each one runs ahead
    // in registers through its unconstrained steps and only the steps that need iterations go through the
    // iterating kernel, one round per such step.  The host reads the work-list counters after every
    // streaming pass (one stream synchronisation per round) and stops when nothing is queued any more.
    LoopMode mode;
    // the records back into the caller's x and uprev: the last thing each of the three fused loops enqueues
    auto unpack = [&](const double *records) -> int {
        hipLaunchKernelGGL(unpack_theta_kernel, dim3(grid), dim3(256), 0, st, records, x, nuprev > 0 ? uprev : nullptr, nx, nr,
                           nuprev, (long long)N);
        HIP_TRY(h, hipGetLastError());
        return LMPC_OK;
    };
    if (asyncLoop) {
        AsyncRound ar;
        ar.x = x; ar.r = r; ar.up = nuprev > 0 ? uprev : nullptr;
        HIP_TRY(h, hipMemcpyAsync(h->dC + h->L.oFG, F, sizeof(double) * nx * nx, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(h->dC + h->L.oFG + nx * nx, G, sizeof(double) * nx * nu, hipMemcpyHostToDevice, st));
        HIP_TRY(h, h->simK.reserve((size_t)h->simCap));
        HIP_TRY(h, hipMemsetAsync(h->simK, 0, sizeof(int32_t) * (size_t)N, st));
        if (warm) HIP_TRY(h, hipMemsetAsync(h->simAct, 0, sizeof(uint64_t) * (size_t)N * (size_t)h->P.words(), st));   // first step is cold
        mode.round = &ar;
        mode.prof = false;
        ar.T = T;
        mode.sim = SimFuse{h->simFG, h->simTheta, flag_min, nullptr, nx, nu, nr, nuprev, 0, h->simK, U_traj, X_traj,
                           (long long)N};
        mode.raWarm = warm != 0;
        // (asked with raWarm set but mode.waveSim still empty and nothing kept: a plain call's answer.  It has to be -- with
        // the run-ahead loop filled in, "two passes?" is answered "no" for want of the keep a "yes" is about to make room for)
        if (h->useWave && runAhead && warm && T > 1 && wave_first_pass_cap(h, wave_args(h, mode), N) > 0) {
            // (a first pass at a smaller capacity is in sight: it writes every scenario's state out after each step, so
            // that a step which outgrows it restarts exactly where the step-synchronous loop would)
            const int rck = ensure_keep(h, N, st, &mode.keep);
            if (rck != LMPC_OK) return rck;
        }
        if (h->useWave) mode.waveSim = WaveSim{h->simFG, h->simK, U_traj, X_traj, flag_min, nx, nu, nr, nuprev, (long long)N, -1, runAhead ? T : 0};
        constexpr int kBurst = 2;   // steps a scenario of a (short) work list may run ahead before it is parked
        std::vector<int32_t> hc(3 * kCountSetWords);
        uint64_t *masks = warm ? h->simAct : nullptr;
        int rc = LMPC_OK;
        ar.cap = T + 1;
        const bool dbg = std::getenv("LMPC_DEBUG_SIM") != nullptr;
        // pass 0 runs every scenario up to its first step that needs iterations; then: solve that step for the
        // listed scenarios, let them run ahead a little (most meet the next such step at once: the transient),
        // park the ones that broke free; when the list has drained, run the parked ones on, compacted.
        bool drained = false;
        for (int pass = 0; pass <= 2 * T + 4 && rc == LMPC_OK; pass++) {
            ar.phase = 1;
            rc = api_launch(h, mode, N, h->simTheta, nullptr, nullptr, nullptr, masks, masks, st);
            if (rc != LMPC_OK) break;
            if (hipMemcpyAsync(hc.data(), h->dCount, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { rc = fail(h, LMPC_ERR_HIP, "lmpc_simulate: reading the work-list counters"); break; }
            const int32_t *hq = hc.data() + (ar.cntNow - h->dCount), *hp = count_set(hc.data(), 2);     // queued now, parked
            long long queued = 0, longest = 0, parked = 0, plongest = 0;
            for (int sh = 0; sh < kShards; sh++) {
                const long long q = hq[sh * kCountStride], pk = ar.resetPark ? 0 : hp[sh * kCountStride];
                queued += q; parked += pk;
                longest = q > longest ? q : longest;
                plongest = pk > plongest ? pk : plongest;
            }
            if (dbg) std::fprintf(stderr, "lmpc sim pass %d: %lld scenarios queued, %lld parked\n", pass, queued, parked);
            ar.resetPark = false;
            if (queued > 0) {
                ar.phase = 2;
                rc = api_launch(h, mode, N, h->simTheta, nullptr, nullptr, nullptr, masks, masks, st);
                ar.listIn = ar.listOut; ar.cntIn = ar.cntNow; ar.maxIn = longest;
                ar.cap = kBurst;
                // a few more rounds without asking: a list never grows from one round to the next, so the grid of
                // `longest` covers them, and a round on an empty list costs less than the host round trip it saves
                for (int e = 0; e < h->simBlind && rc == LMPC_OK; e++) {
                    ar.phase = 1;
                    rc = api_launch(h, mode, N, h->simTheta, nullptr, nullptr, nullptr, masks, masks, st);
                    if (rc != LMPC_OK) break;
                    ar.phase = 2;
                    rc = api_launch(h, mode, N, h->simTheta, nullptr, nullptr, nullptr, masks, masks, st);
                    ar.listIn = ar.listOut; ar.cntIn = ar.cntNow;
                }
            } else if (parked > 0) {
                // no iterating kernel ran, so nobody cleared the counter set the next pass writes
                if (hipMemsetAsync(h->dCount, 0, sizeof(int32_t) * 2 * kCountSetWords, st) != hipSuccess) { rc = fail(h, LMPC_ERR_HIP, "lmpc_simulate: clearing the work-list counters"); break; }
                ar.listIn = h->dList3; ar.cntIn = count_set(h->dCount.get(), 2); ar.maxIn = plongest;
                ar.cap = T + 1;
                ar.resetPark = true;
            } else {
                drained = true;
                break;
            }
        }
        // the pass cap is generous (every scenario needs at most T rounds), but running into it with scenarios
        // still queued or parked must not look like success: their states and trajectory slots are unfinished
        if (rc == LMPC_OK && !drained)
            rc = fail(h, LMPC_ERR_HIP, "lmpc_simulate: the scenario-asynchronous loop hit its pass limit with scenarios "
                                       "still queued (lmpc_set_option(\"sim_async\", 0) runs the step-synchronous loop)");
        // the last streaming pass queued nothing, so no iterating kernel cleared the other counter set
        if (h->dCount) { hipMemsetAsync(h->dCount, 0, sizeof(int32_t) * 3 * kCountSetWords, st); h->countSet = 0; }
        return rc != LMPC_OK ? rc : unpack(h->simTheta);
    }
    if (!h->useWave && h->simFused && nu <= kMaxSimU) {
        HIP_TRY(h, hipMemcpyAsync(h->dC + h->L.oFG, F, sizeof(double) * nx * nx, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(h->dC + h->L.oFG + nx * nx, G, sizeof(double) * nx * nu, hipMemcpyHostToDevice, st));
        HIP_TRY(h, h->simTheta2.reserve((size_t)h->simCap * h->P.nth));
        double *cur = h->simTheta, *nxt = h->simTheta2;
        int rc = LMPC_OK;
        for (int k = 0; k < T && rc == LMPC_OK; k++) {
            mode.sim = SimFuse{h->simFG, nxt, flag_min, X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr,
                               nx, nu, nr, nuprev, k == 0 ? 1 : 0};
            const uint64_t *wm = (warm && k > 0) ? h->simAct : nullptr;
            // no input trajectory asked for: the kernels write neither u nor the per-step flags
            rc = api_launch(h, mode, N, cur, U_traj ? U_traj + (size_t)k * N * nu : nullptr, nullptr, nullptr,
                        warm ? h->simAct : nullptr, wm, st);
            std::swap(cur, nxt);
        }
        return rc != LMPC_OK ? rc : unpack(cur);
    }
    // Wavefront path, warm: every scenario's final working set stays on the device WITH its factorisation, in its
    // order (2 x 64 + cap (cap - 1) / 2 reals and 320 ints per scenario: 17 KB at cap 64), so that a warm step
    // starts from the factor as it stands -- what DAQP_WARMSTART means in libdaqp, whose workspace is simply not
    // cleared between two calls (codegen/mpc_update_qp.c:44-54) -- instead of re-appending the rows of the mask one
    // by one.  Option "sim_keep_factor" 0 (or no memory for it): the mask-based warm start of the other paths.
    if (h->useWave && !h->avi && warm && !h->bnb && h->simKeep && T > 1) {
        const int rck = ensure_keep(h, N, st, &mode.keep);
        if (rck != LMPC_OK) return rck;
    }
    // Wavefront path with its screening pass in front: the plant step is fused into the three kernels of a step like
    // on the lane path -- the screening pass advances the scenarios it finishes (SimFuse), the wavefront kernel and its
    // slow path advance theirs in place (WaveSim with the step number) -- so a step is those launches and nothing
    // else: no plant kernel (16 us at 2e5 scenarios), no input / flag arrays in between.
    if (h->useWave && h->simFused && !h->bnb && nu <= kMaxSimU && nx <= 8 && api_wave_screens(h, N)) {
        HIP_TRY(h, hipMemcpyAsync(h->dC + h->L.oFG, F, sizeof(double) * nx * nx, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(h->dC + h->L.oFG + nx * nx, G, sizeof(double) * nx * nu, hipMemcpyHostToDevice, st));
        int rc = LMPC_OK;
        for (int k = 0; k < T && rc == LMPC_OK; k++) {
            mode.sim = SimFuse{h->simFG, h->simTheta, flag_min, X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr,
                               nx, nu, nr, nuprev, k == 0 ? 1 : 0};
            mode.waveSim = WaveSim{h->simFG, nullptr, nullptr, X_traj, flag_min, nx, nu, nr, nuprev, (long long)N, k};
            const uint64_t *wm = (warm && k > 0) ? h->simAct : nullptr;
            rc = api_launch(h, mode, N, h->simTheta, U_traj ? U_traj + (size_t)k * N * nu : nullptr, nullptr, nullptr,
                        warm ? h->simAct : nullptr, wm, st);
        }
        return rc != LMPC_OK ? rc : unpack(h->simTheta);
    }
    for (int k = 0; k < T; k++) {
        // warm start = previous step's final working set (reference codegen DAQP_WARMSTART,
        // codegen/mpc_update_qp.c:44-47); the first step is always cold
        const uint64_t *wm = (warm && k > 0) ? h->simAct : nullptr;
        int rc = api_launch(h, mode, N, h->simTheta, h->simU, h->simFlag, nullptr, warm ? h->simAct : nullptr, wm, st);
        if (rc != LMPC_OK) return rc;
        const bool last = k == T - 1;
        hipLaunchKernelGGL(plant_theta_kernel<double>, dim3(grid), dim3(256), 0, st, h->simTheta, h->P.nth, nr, h->simU,
                           h->simFlag, h->simFG, nx, nu, nuprev,
                           X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr,
                           U_traj ? U_traj + (size_t)k * N * nu : nullptr, flag_min, k == 0 ? 1 : 0,
                           last ? x : nullptr, (last && nuprev > 0) ? uprev : nullptr, (long long)N);
        if (hipGetLastError() != hipSuccess) return fail(h, LMPC_ERR_HIP, "lmpc_simulate_device: plant step launch");
    }
    return LMPC_OK;
}

int lmpc_simulate_f32_device(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev, const double *F,
                             const double *G, float *x, const float *r, float *uprev, float *U_traj,
                             float *X_traj, int32_t *flag_min, int warm, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const int nu = h->P.nout;
    if (N < 0 || T < 0 || nx <= 0 || nx > 32 || nr < 0 || nuprev < 0 || nuprev > nu || nu > 64 || !F || !G ||
        (N > 0 && !x) || (nuprev > 0 && N > 0 && !uprev) || nx + nr + nuprev != h->P.nth)
        return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_f32_device: theta = [x; r; uprev] must match the handle "
                                        "(nx + nr + nuprev == nth, nout == nu, nx <= 32)");
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    int rc = api_ensure_f32(h);
    if (rc != LMPC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    float *dTh = h->simTheta.as<float>(), *dU = h->simU.as<float>(),
          *dFG = h->simFG.as<float>();
    std::vector<float> fg((size_t)nx * nx + (size_t)nx * nu);       // the plant rounded to binary32, like the pack
    for (int i = 0; i < nx * nx; i++) fg[i] = (float)F[i];
    for (int i = 0; i < nx * nu; i++) fg[(size_t)nx * nx + i] = (float)G[i];
    HIP_TRY(h, hipMemcpy(dFG, fg.data(), sizeof(float) * fg.size(), hipMemcpyHostToDevice));
    if (X_traj) HIP_TRY(h, hipMemcpyAsync(X_traj, x, sizeof(float) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    const unsigned grid = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(form_theta_kernel<float>, dim3(grid), dim3(256), 0, st, dTh, x, r, uprev, nx, nr, nuprev,
                       (long long)N);
    for (int k = 0; k < T; k++) {
        const uint64_t *wm = (warm && k > 0 && !h->bnb) ? h->simAct : nullptr;
        rc = api_launch_wave_f32(h, h->dCwf, N, dTh, dU, h->simFlag, nullptr, (warm && !h->bnb) ? h->simAct : nullptr,
                                  wm, st);
        if (rc != LMPC_OK) return rc;
        const bool last = k == T - 1;
        hipLaunchKernelGGL(plant_theta_kernel<float>, dim3(grid), dim3(256), 0, st, dTh, h->P.nth, nr, dU, h->simFlag,
                           dFG, nx, nu, nuprev, X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr,
                           U_traj ? U_traj + (size_t)k * N * nu : nullptr, flag_min, k == 0 ? 1 : 0,
                           last ? x : nullptr, (last && nuprev > 0) ? uprev : nullptr, (long long)N);
        HIP_TRY(h, hipGetLastError());
    }
    return LMPC_OK;
}

int lmpc_form_parameter_device(lmpc_handle *h, int64_t N, double *theta, const double *x, int nx,
                               const lmpc_block *r, const lmpc_block *d, const double *uprev, int nuprev,
                               const lmpc_block *p, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const ThetaBlock br = to_block(r), bd = to_block(d), bp = to_block(p);
    if (N < 0 || nx < 0 || nuprev < 0 || br.w < 0 || bd.w < 0 || bp.w < 0 || br.H < 0 || bd.H < 0 || bp.H < 0 ||
        (N > 0 && (!theta || (nx > 0 && !x))))
        return fail(h, LMPC_ERR_BADARG, "lmpc_form_parameter_device: NULL array or negative size");
    if (nx + br.width() + bd.width() + nuprev + bp.width() != h->P.nth)
        return fail(h, LMPC_ERR_BADARG, "lmpc_form_parameter_device: blocks do not add up to the handle's nth = " +
                                            std::to_string(h->P.nth));
    if (N == 0 || h->P.nth == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const long long total = (long long)N * h->P.nth;
    hipLaunchKernelGGL(form_parameter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       theta, x, nx, br, bd, uprev, nuprev, bp, (long long)N);
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}

int lmpc_simulate_ref_device(lmpc_handle *h, int64_t N, int T, int nx, const lmpc_block *r, int nuprev,
                             const double *F, const double *G, double *x, double *uprev, double *U_traj,
                             double *X_traj, int32_t *flag_min, int warm, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const int nu = h->P.nout;
    ThetaBlock br = to_block(r);
    if (N < 0 || T < 0 || nx <= 0 || nx > 32 || nuprev < 0 || nuprev > nu || !F || !G || (N > 0 && !x) ||
        (nuprev > 0 && N > 0 && !uprev) || br.w < 0 || br.H < 0 || nx + br.width() + nuprev != h->P.nth)
        return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_ref_device: theta = [x; r-block; uprev] must match the handle "
                                        "(nx + width(r) + nuprev == nth, nout == nu, nx <= 32)");
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    HIP_TRY(h, hipMemcpyAsync(h->simFG, F, sizeof(double) * nx * nx, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->simFG + nx * nx, G, sizeof(double) * nx * nu, hipMemcpyHostToDevice, st));
    if (X_traj) HIP_TRY(h, hipMemcpyAsync(X_traj, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    const unsigned grid = (unsigned)((N + 255) / 256);
    const long long total = (long long)N * h->P.nth;
    const ThetaBlock none{nullptr, 0, 0, 1, 0, 0};
    for (int k = 0; k < T; k++) {
        br.k0 = br.H > 0 ? k + 1 : k;                 // simulation.jl:101 get_preview(rs, k, Np) / rs[:,k]
        hipLaunchKernelGGL(form_parameter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           h->simTheta, x, nx, br, none, uprev, nuprev, none, (long long)N);
        const uint64_t *wm = (warm && k > 0) ? h->simAct : nullptr;
        int rc = api_launch(h, LoopMode{}, N, h->simTheta, h->simU, h->simFlag, nullptr, warm ? h->simAct : nullptr, wm, st);
        if (rc != LMPC_OK) return rc;
        dispatch_nx(nx, [&](auto NX) {
            hipLaunchKernelGGL(plant_kernel<decltype(NX)::value>, dim3(grid), dim3(256), 0, st, x, uprev, h->simU, h->simFlag, h->simFG, nx,
                               nu, nuprev, X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr,
                               U_traj ? U_traj + (size_t)k * N * nu : nullptr, flag_min, k == 0 ? 1 : 0, (long long)N);
        });
        HIP_TRY(h, hipGetLastError());
    }
    return LMPC_OK;
}

int lmpc_set_parameter_layout(lmpc_handle *h, const lmpc_param_layout *l) {
    if (!h || !l) return LMPC_ERR_BADARG;
    if (l->n_state < 0 || l->n_reference < 0 || l->n_disturbance < 0 || l->n_control_prev < 0 ||
        l->n_affine_parameter < 0 || l->n_preview_horizon < 0 || l->n_control_prev > h->P.nout ||
        (l->n_preview_horizon > 0 && !l->traj2setpoint))
        return fail(h, LMPC_ERR_BADARG, "lmpc_set_parameter_layout: negative size, n_control_prev > nout, or "
                                        "n_preview_horizon > 0 without traj2setpoint");
    if (l->n_state + l->n_reference + l->n_disturbance + l->n_control_prev + l->n_affine_parameter != h->P.nth)
        return fail(h, LMPC_ERR_BADARG, "lmpc_set_parameter_layout: blocks do not add up to the handle's nth = " +
                                            std::to_string(h->P.nth));
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    h->ccT2S.reset();
    if (l->n_preview_horizon > 0 && l->n_reference > 0) {
        const size_t cnt = (size_t)l->n_reference * l->n_reference * l->n_preview_horizon;
        HIP_TRY(h, h->ccT2S.reserve(cnt));
        HIP_TRY(h, hipMemcpy(h->ccT2S, l->traj2setpoint, sizeof(double) * cnt, hipMemcpyHostToDevice));
    }
    h->ccNx = l->n_state; h->ccNr = l->n_reference; h->ccNd = l->n_disturbance; h->ccNup = l->n_control_prev;
    h->ccNp = l->n_affine_parameter; h->ccNph = l->n_reference > 0 ? l->n_preview_horizon : 0;
    h->ccWarmN = -1;
    return LMPC_OK;
}

int lmpc_compute_control_device(lmpc_handle *h, int64_t N, double *control, const double *state,
                                const double *reference, const double *disturbance,
                                const double *affine_parameter, int32_t *exitflag, int warm, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    if (h->ccNx < 0) return fail(h, LMPC_ERR_BADARG, "lmpc_compute_control: call lmpc_set_parameter_layout first");
    if (N < 0 || (N > 0 && (!control || (h->ccNx > 0 && !state))))
        return fail(h, LMPC_ERR_BADARG, "lmpc_compute_control: NULL control/state or negative N");
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    const size_t w = (size_t)h->P.words();
    if (N > h->ccCap) {
        h->ccWarmN = -1;
        HIP_TRY(h, reserve_group(h->ccCap, (int64_t)N, sized(h->ccTheta, (size_t)N * (h->P.nth ? h->P.nth : 1)),
                                 sized(h->ccAct, (size_t)N * w), sized(h->ccFlag, (size_t)N)));
    }
    // lane / screening path without reference condensation: the screening kernel assembles theta from the
    // five arrays itself (GatherArgs) and hands the records of the problems that need iterations to the
    // iterating kernel through ccTheta -- no theta buffer is written or read for the others
    if (api_will_screen(h, N) && h->ccNph == 0 && h->ccFused) {
        LoopMode mode;
        mode.gat = GatherArgs{state, reference, disturbance, control, affine_parameter, h->ccTheta,
                              h->ccNx, h->ccNr, h->ccNd, h->ccNup, h->ccNp, h->P.nout};
        const bool use_warm_g = warm && h->ccWarmN == N;
        int rcg = api_launch(h, mode, N, h->ccTheta, control, exitflag ? exitflag : h->ccFlag, nullptr, warm ? h->ccAct : nullptr,
                         use_warm_g ? h->ccAct : nullptr, st);
        if (rcg != LMPC_OK) return rcg;
        h->ccWarmN = warm ? N : -1;
        return LMPC_OK;
    }
    const long long total = (long long)N * h->P.nth;
    if (total > 0) {
        hipLaunchKernelGGL(update_parameter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           h->ccTheta, control, h->P.nout, state, h->ccNx, reference, h->ccNr, h->ccNph, h->ccT2S,
                           disturbance, h->ccNd, h->ccNup, affine_parameter, h->ccNp, (long long)N);
        HIP_TRY(h, hipGetLastError());
    }
    // DAQP_WARMSTART build (codegen/mpc_update_qp.c:44-47): the working sets the previous call ended
    // with are the next call's starting point; otherwise every call starts cold
    const bool use_warm = warm && h->ccWarmN == N && !h->bnb;
    int rc = api_launch(h, LoopMode{}, N, h->ccTheta, control, exitflag ? exitflag : h->ccFlag, nullptr,
                    (warm && !h->bnb) ? h->ccAct : nullptr, use_warm ? h->ccAct : nullptr, st);
    if (rc != LMPC_OK) return rc;
    h->ccWarmN = (warm && !h->bnb) ? N : -1;
    return LMPC_OK;
}

int lmpc_compute_control(lmpc_handle *h, int64_t N, double *control, const double *state,
                         const double *reference, const double *disturbance, const double *affine_parameter,
                         int32_t *exitflag, int warm) {
    if (!h) return LMPC_ERR_BADARG;
    if (h->ccNx < 0) return fail(h, LMPC_ERR_BADARG, "lmpc_compute_control: call lmpc_set_parameter_layout first");
    if (N < 0 || (N > 0 && (!control || (h->ccNx > 0 && !state))))
        return fail(h, LMPC_ERR_BADARG, "lmpc_compute_control: NULL control/state or negative N");
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const int nu = h->P.nout;
    const size_t wr = (size_t)h->ccNr * (h->ccNph > 0 ? h->ccNph : 1);
    // one staging block per handle, kept between calls (a closed loop calls this once per time step):
    // [control | state | reference | disturbance | parameter] doubles, then the flags
    const size_t per = (size_t)nu + h->ccNx + wr + h->ccNd + h->ccNp;
    if ((size_t)N * per * sizeof(double) <= (size_t)64 * 1024) {
        // a handful of problems -- the generated controller's call, one state per time step (mpc_update_qp.c:29-54): the
        // block lives in MAPPED host memory, the kernels read the arguments and write control and flags straight
        // through it, the host waits once for the handle's own stream (seven blocking copies before: ~100 us a call)
        const size_t need = ((size_t)N * per * sizeof(double) + 63 & ~(size_t)63) + sizeof(int32_t) * (size_t)N + 4096;
        if (need > h->ccMapHost.size()) {
            if (h->ccMapHost) (void)hipDeviceSynchronize();
            h->ccMapDev = nullptr;
            if (h->ccMapHost.reserve(need) != hipSuccess) return fail(h, LMPC_ERR_HIP, "lmpc_compute_control: mapped block");
            h->ccMapDev = h->ccMapHost.dev();
        }
        if (!h->oneStream) HIP_TRY(h, hipStreamCreateWithFlags(&h->oneStream, hipStreamNonBlocking));
        size_t off = 0;
        auto put = [&](const double *src, size_t w) -> double * {
            if (!src || w == 0) return nullptr;
            std::memcpy(h->ccMapHost + off, src, sizeof(double) * (size_t)N * w);
            double *d = reinterpret_cast<double *>(h->ccMapDev + off);
            off += sizeof(double) * (size_t)N * w;
            return d;
        };
        double *dc = put(control, (size_t)nu), *ds = put(state, (size_t)h->ccNx), *dr = put(reference, wr),
               *dd = put(disturbance, (size_t)h->ccNd), *dp = put(affine_parameter, (size_t)h->ccNp);
        const size_t oF = (off + 63) & ~(size_t)63;
        int32_t *hf = reinterpret_cast<int32_t *>(h->ccMapHost + oF);
        for (int64_t i = 0; i < N; i++) hf[i] = LMPC_EXIT_UNFINISHED;
        const int rc = lmpc_compute_control_device(h, N, dc, ds, dr, dd, dp, reinterpret_cast<int32_t *>(h->ccMapDev + oF), warm,
                                                   h->oneStream);
        const hipError_t es = hipStreamSynchronize(h->oneStream);
        if (rc != LMPC_OK) return rc;
        if (es != hipSuccess) return fail(h, LMPC_ERR_HIP, std::string("lmpc_compute_control: ") + hipGetErrorString(es));
        const int rcf = check_fast_err(h);
        if (rcf != LMPC_OK) return rcf;
        std::memcpy(control, h->ccMapHost, sizeof(double) * (size_t)N * nu);
        if (exitflag) std::memcpy(exitflag, hf, sizeof(int32_t) * (size_t)N);
        return LMPC_OK;
    }
    if (N > h->ccStageCap || per > h->ccStagePer) {
        // (a wider record regrows the group at the same N too: emptied here, so that capacity 0 never stands beside a
        // block; ccObsScratch is another entry point's buffer)
        h->ccStage.reset(); h->ccStageFlag.reset(); h->ccStageCap = 0; h->ccStagePer = 0;
        HIP_TRY(h, reserve_group(h->ccStageCap, (int64_t)N, sized(h->ccStage, (size_t)N * per), sized(h->ccStageFlag, (size_t)N)));
        h->ccStagePer = per;
    }
    Staging sg(h->ccStage);                            // carved from the handle's block: nothing is allocated per call
    auto up = [&](const double *src, size_t w) {
        return w ? static_cast<double *>(sg.in(src, sizeof(double) * (size_t)N * w)) : nullptr;
    };
    double *dc = static_cast<double *>(sg.out(control, sizeof(double) * (size_t)N * nu, true));
    double *ds = up(state, (size_t)h->ccNx), *dr = up(reference, wr), *dd = up(disturbance, (size_t)h->ccNd),
           *dp = up(affine_parameter, (size_t)h->ccNp);
    sg.out_from(exitflag, h->ccStageFlag, sizeof(int32_t) * (size_t)N);
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = lmpc_compute_control_device(h, N, dc, ds, dr, dd, dp, h->ccStageFlag, warm, nullptr);
    if (rc == LMPC_OK && !sg.download_all()) return sg.fail(h);
    return rc;
}

int lmpc_compute_control_observer_device(lmpc_handle *h, int64_t N, double *control, const double *observer_state,
                                         int n_measured_disturbance, const double *reference,
                                         const double *measured_disturbance, const double *affine_parameter,
                                         int32_t *exitflag, int warm, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    if (h->ccNx < 0) return fail(h, LMPC_ERR_BADARG, "lmpc_compute_control_observer: call lmpc_set_parameter_layout first");
    const int ndm = n_measured_disturbance, ndo = h->ccNd - ndm;
    if (N < 0 || ndm < 0 || ndo < 0 || (N > 0 && (!control || !observer_state)))
        return fail(h, LMPC_ERR_BADARG, "lmpc_compute_control_observer: NULL array, negative N, or more measured "
                                        "disturbances than the layout's n_disturbance");
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const size_t per = (size_t)h->ccNx + h->ccNd;
    HIP_TRY(h, reserve_group(h->ccObsCap, (int64_t)N, sized(h->ccObsScratch, (size_t)N * (per ? per : 1))));
    double *st_ = h->ccObsScratch, *di_ = h->ccObsScratch + (size_t)N * h->ccNx;
    const long long total = (long long)N * (long long)per;
    if (total > 0) {
        hipLaunchKernelGGL(split_observer_state_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, st_, di_, observer_state, measured_disturbance, h->ccNx, ndm, ndo,
                           (long long)N);
        HIP_TRY(h, hipGetLastError());
    }
    return lmpc_compute_control_device(h, N, control, st_, reference, h->ccNd > 0 ? di_ : nullptr, affine_parameter,
                                       exitflag, warm, stream);
}

int lmpc_set_observer(lmpc_handle *h, const lmpc_observer *o) {
    if (!h || !o) return LMPC_ERR_BADARG;
    if (o->n_state <= 0 || o->n_state > 32 || o->n_control < 0 || o->n_disturbance < 0 || o->n_measurement <= 0 ||
        !o->plant_dynamics || !o->measurement_function || !o->k_transpose)
        return fail(h, LMPC_ERR_BADARG, "lmpc_set_observer: sizes (1 <= n_state <= 32, n_measurement >= 1) or NULL array");
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const size_t nd_ = (size_t)o->n_state * (1 + o->n_state + o->n_control + o->n_disturbance);
    const size_t nm_ = (size_t)o->n_measurement * (1 + o->n_state + o->n_disturbance);
    const size_t nk_ = (size_t)o->n_measurement * o->n_state;
    h->obsC.reset();
    HIP_TRY(h, h->obsC.reserve(nd_ + nm_ + nk_));
    HIP_TRY(h, hipMemcpy(h->obsC, o->plant_dynamics, sizeof(double) * nd_, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->obsC + nd_, o->measurement_function, sizeof(double) * nm_, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->obsC + nd_ + nm_, o->k_transpose, sizeof(double) * nk_, hipMemcpyHostToDevice));
    h->obsNx = o->n_state; h->obsNu = o->n_control; h->obsNd = o->n_disturbance; h->obsNy = o->n_measurement;
    return LMPC_OK;
}

int lmpc_predict_state_device(lmpc_handle *h, int64_t N, double *state, const double *control,
                              const double *disturbance, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    if (!h->obsC) return fail(h, LMPC_ERR_BADARG, "lmpc_predict_state: call lmpc_set_observer first");
    if (N < 0 || (N > 0 && (!state || (h->obsNu > 0 && !control))))
        return fail(h, LMPC_ERR_BADARG, "lmpc_predict_state: NULL state/control or negative N");
    if (N == 0) return LMPC_OK;
    LMPC_ENTER_DEVICE(h);
    dispatch_nx(h->obsNx, [&](auto NX) {
        hipLaunchKernelGGL(predict_state_kernel<decltype(NX)::value>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, state, control, disturbance, h->obsC, h->obsNx, h->obsNu, h->obsNd, (long long)N);
    });
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}

int lmpc_correct_state_device(lmpc_handle *h, int64_t N, double *state, const double *measurement,
                              const double *disturbance, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    if (!h->obsC) return fail(h, LMPC_ERR_BADARG, "lmpc_correct_state: call lmpc_set_observer first");
    if (N < 0 || (N > 0 && (!state || !measurement)))
        return fail(h, LMPC_ERR_BADARG, "lmpc_correct_state: NULL state/measurement or negative N");
    if (N == 0) return LMPC_OK;
    LMPC_ENTER_DEVICE(h);
    const size_t nd_ = (size_t)h->obsNx * (1 + h->obsNx + h->obsNu + h->obsNd);
    const size_t nm_ = (size_t)h->obsNy * (1 + h->obsNx + h->obsNd);
    dispatch_nx(h->obsNx, [&](auto NX) {
        hipLaunchKernelGGL(correct_state_kernel<decltype(NX)::value>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, state, measurement, disturbance, h->obsC + nd_, h->obsC + nd_ + nm_, h->obsNx,
                           h->obsNy, h->obsNd, (long long)N);
    });
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}

namespace {
// host-pointer wrapper shared by predict / correct: state in/out, one input array, optional disturbance
int observer_host(lmpc_handle *h, int64_t N, double *state, const double *in, int win, const double *dist, bool predict) {
    if (!h) return LMPC_ERR_BADARG;
    if (!h->obsC) return fail(h, LMPC_ERR_BADARG, "lmpc observer: call lmpc_set_observer first");
    if (N < 0 || (N > 0 && (!state || (win > 0 && !in)))) return fail(h, LMPC_ERR_BADARG, "lmpc observer: NULL array or negative N");
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    const size_t n = (size_t)N, nx = (size_t)h->obsNx, nd = (size_t)h->obsNd;
    Staging sg;
    double *ds = static_cast<double *>(sg.out(state, sizeof(double) * n * nx, true));
    double *di = win > 0 ? static_cast<double *>(sg.in(in, sizeof(double) * n * win)) : nullptr;
    double *dd = nd > 0 ? static_cast<double *>(sg.in(dist, sizeof(double) * n * nd)) : nullptr;
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = predict ? lmpc_predict_state_device(h, N, ds, di, dd, nullptr) : lmpc_correct_state_device(h, N, ds, di, dd, nullptr);
    if (rc == LMPC_OK && !sg.download_all()) return sg.fail(h);
    return rc;
}
}  // namespace

int lmpc_predict_state(lmpc_handle *h, int64_t N, double *state, const double *control, const double *disturbance) {
    return observer_host(h, N, state, control, h ? h->obsNu : 0, disturbance, true);
}

int lmpc_correct_state(lmpc_handle *h, int64_t N, double *state, const double *measurement, const double *disturbance) {
    return observer_host(h, N, state, measurement, h ? h->obsNy : 0, disturbance, false);
}

int lmpc_simulate(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev, const double *F, const double *G,
                  double *x, const double *r, double *uprev, double *U_traj, double *X_traj, int32_t *flag_min,
                  int warm) {
    return simulate_host<double>(h, N, T, nx, nr, nuprev, F, G, x, r, uprev, U_traj, X_traj, flag_min, warm);
}

int lmpc_simulate_f32(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev, const double *F, const double *G,
                      float *x, const float *r, float *uprev, float *U_traj, float *X_traj, int32_t *flag_min,
                      int warm) {
    return simulate_host<float>(h, N, T, nx, nr, nuprev, F, G, x, r, uprev, U_traj, X_traj, flag_min, warm);
}

}  // extern "C"
