// The work list: how one kernel hands the problems it did not finish to the next.  kShards segments of seg_cap problem
// indices; segment s holds count[s * kCountStride] entries from list[s * seg_cap], one counter per 128-byte line.  A
// producer appends to the segment its workgroup or wavefront index selects (push), a consumer gives every segment its
// own walkers (walk).  A list's counters are cleared by a kernel behind its last reader (stream order).  DESIGN.md 3.2.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_wave_layout.hpp"      // kShards, kCountStride

namespace lmpc {

constexpr int kCountSetWords = kShards * kCountStride;      // words of one set of counters
static_assert(kShards == 64, "one work-list segment per lane (wl_clear_counts)");

// one list as a launch takes it (list == nullptr: no list, the whole batch); count_next: the set the consumer clears
struct WorkList { const int32_t *list = nullptr, *count = nullptr; int32_t *count_next = nullptr; long long seg_cap = 0; };

// set k of several counter sets that lie one behind the other
template <class T> __host__ __device__ inline T *count_set(T *base, size_t k) { return base + k * kCountSetWords; }

// ---- push: the lanes flagged `queue` append their problem index to segment `shard`, one atomic per wavefront -- at once
// (wl_push), or wl_push_reserve at the end of a tile and wl_push_write at the end of the NEXT: the atomic is not waited for
struct WlPush { unsigned long long mask = 0ull; int base = 0; int pid = 0; };
__device__ __forceinline__ void wl_push_reserve(WlPush &q, bool queue, long long pid, int lane, int shard,
                                                int32_t *__restrict__ count) {
    q.mask = __ballot(queue);
    q.pid = (int)pid;
    q.base = 0;
    if (q.mask != 0ull && lane == 0) q.base = atomicAdd(&count[shard * kCountStride], __popcll(q.mask));
}
// (mine = this lane's bit of q.mask: wl_push still holds it as its flag, wl_push_write takes it from the mask)
__device__ __forceinline__ void wl_push_store(const WlPush &q, bool mine, int lane, int shard, long long seg_cap,
                                              int32_t *__restrict__ list) {
    if (q.mask != 0ull) {
        const int base = __shfl(q.base, 0);
        if (mine) list[(long long)shard * seg_cap + base + __popcll(q.mask & ((1ull << lane) - 1ull))] = q.pid;
    }
}
__device__ __forceinline__ void wl_push_write(WlPush &q, int lane, int shard, long long seg_cap, int32_t *__restrict__ list) {
    wl_push_store(q, (q.mask >> lane) & 1ull, lane, shard, seg_cap, list);
    q.mask = 0ull;
}
__device__ __forceinline__ void wl_push(bool queue, long long pid, int lane, int shard, long long seg_cap,
                                        int32_t *__restrict__ list, int32_t *__restrict__ count) {
    WlPush q;
    wl_push_reserve(q, queue, pid, lane, shard, count);
    wl_push_store(q, queue, lane, shard, seg_cap, list);
}

// ---- the first 64 threads of workgroup 0 clear a set of counters (count == nullptr: nothing to clear)
__device__ __forceinline__ void wl_clear_counts(int32_t *__restrict__ count, int tid) {
    if (count != nullptr && blockIdx.x == 0 && tid < kShards) count[tid * kCountStride] = 0;
}

// ---- walk: walker u of nu (a multiple of kShards) takes segment u % kShards: positions first, first + stride, ... < count
struct WlWalk {
    int shard;
    long long first, stride;
    __device__ __forceinline__ const int32_t *segment(const int32_t *list, long long seg_cap) const { return list + (long long)shard * seg_cap; }
    __device__ __forceinline__ long long count(const int32_t *cnt) const { return (long long)cnt[shard * kCountStride]; }
};
// ... the walkers are the workgroups
__device__ __forceinline__ WlWalk wl_walk_block(int width) {
    return WlWalk{(int)(blockIdx.x % kShards), (long long)(blockIdx.x / kShards) * width, (long long)(gridDim.x / kShards) * width};
}
// ... the walkers are the wavefronts: gw of nw, 64 positions each time
__device__ __forceinline__ WlWalk wl_walk_wave(long long gw, long long nw) {
    return WlWalk{(int)(gw % kShards), (gw / kShards) * 64, (nw / kShards) * 64};
}

}  // namespace lmpc
