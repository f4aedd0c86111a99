// One instantiation set of the wavefront kernel: real type LMPC_WV_REAL (double | float) with or
// without branch and bound (LMPC_WV_BNB 0 | 1), n-chain or Gram-scan form (LMPC_WV_GRAM 0 | 1).  Compiled
// eight times (see Makefile) so that the library's ~200 kernel instantiations build in parallel.
#include "lmpc_wave_launch.hpp"

namespace lmpc {
#ifndef LMPC_WV_SIM
#define LMPC_WV_SIM 1
#endif
template int launch_wave_inst<LMPC_WV_REAL, (LMPC_WV_BNB != 0), (LMPC_WV_GRAM != 0), (LMPC_WV_SIM != 0)>(lmpc_handle *, const WaveArgs &,
                                                                const LMPC_WV_REAL *, int64_t, const LMPC_WV_REAL *, LMPC_WV_REAL *,
                                                                int32_t *, int32_t *, uint64_t *, const uint64_t *, hipStream_t);
#ifdef LMPC_WV_HELPERS
// (one translation unit carries the launcher's non-template helpers the API file needs)
int wave_first_pass_cap(lmpc_handle *h, const WaveArgs &a, int64_t nprob) { return wave_first_pass_cap_impl(h, a, nprob, sizeof(double)); }
void wave_stat_read(const lmpc_handle *h, unsigned long long out[4]) { wave_stat_sums(h, out); }
int wave_reserve(lmpc_handle *h, int64_t nprob, hipStream_t st) { return wave_reserve_impl(h, nprob, st); }

// The ticket counter and the two sets of overflow counters (launch_wave_cfg describes their layout and protocol)
int wave_scratch_counters(lmpc_handle *h, hipStream_t st) {
    if (h->dQueue && h->dOvfCount) return LMPC_OK;
    HIP_TRY(h, h->dOvfCount.reserve(2 * kCountSetWords + 64));
    HIP_TRY(h, h->dQueue.reserve(64 / sizeof(int32_t)));
    HIP_TRY(h, hipMemsetAsync(h->dOvfCount, 0, sizeof(int32_t) * (2 * kCountSetWords + 64), st));
    HIP_TRY(h, hipMemsetAsync(h->dQueue, 0, 64, st));
    h->waveCtrSet = 0; h->waveOvfSet = 0;
    return LMPC_OK;
}

// working-set statistics: device counters + their mapped host copy
int wave_scratch_stats(lmpc_handle *h, hipStream_t st) {
    if (h->hStat) return LMPC_OK;
    // (the device block first: the mapped copy, which the test above and every reader go by, exists only with it)
    HIP_TRY(h, h->dStat.reserve(64 * 16));
    HIP_TRY(h, hipMemsetAsync(h->dStat, 0, sizeof(unsigned long long) * 64 * 16, st));
    HIP_TRY(h, h->hStat.reserve(8));
    for (int q = 0; q < 8; q++) h->hStat[q] = 0ull;
    h->dStatHost = const_cast<unsigned long long *>(h->hStat.dev());
    return LMPC_OK;
}

// the list of the points that outgrow a first pass
int wave_scratch_list1(lmpc_handle *h, int64_t nprob) {
    HIP_TRY(h, reserve_group(h->ovfCap1, nprob, sized(h->dOvfList1, (size_t)nprob)));
    return LMPC_OK;
}

// the slow path's list and its per-thread scratch (sized for binary64: the binary32 calls of the handle use the same slices)
int wave_scratch_slow(lmpc_handle *h, int64_t nprob) {
    HIP_TRY(h, reserve_group(h->ovfCap, nprob, sized(h->dOvfList, (size_t)nprob)));
    const int bigCap = h->capFull < kBigCap ? h->capFull : kBigCap;
    HIP_TRY(h, h->dBigR.reserve(sizeof(double) * (size_t)kBigThreads * (size_t)big_scratch_reals(h->W.n, h->W.m, bigCap)));
    HIP_TRY(h, h->dBigI.reserve((size_t)kBigThreads * (size_t)big_scratch_ints(h->W.m, bigCap)));
    return LMPC_OK;
}
#endif
}  // namespace lmpc

#ifdef LMPC_WAVE_TRACE
// diagnostic build only: per-phase shader-clock sums of THIS translation unit's kernels (see lmpc_wave_kernel.hpp)
extern "C" int lmpc_debug_wave_trace(unsigned long long *out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(lmpc::g_wave_trace), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(lmpc::g_wave_trace), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
