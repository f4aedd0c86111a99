// Internals shared by the translation units of liblmpc_hip.so: the handle, error plumbing, the
// wave kernel's launch interface.  The wavefront kernel's instantiations are compiled in their own
// translation units (lmpc_wave_inst.hip, one per real type x branch-and-bound) so that the library
// builds in parallel.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/lmpc_hip.h"
#include "lmpc_buffer.hpp"
#include "lmpc_pack.hpp"
#include "lmpc_wave_layout.hpp"
#include "lmpc_worklist.hpp"

namespace lmpc {
constexpr int kLaneSizes[] = {2, 3, 4, 5, 6, 8, 10, 12};
constexpr int kLaneMaxN = 12;
constexpr int kLaneMaxM = 64;
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kWaveMaxN = 127, kWaveMaxCap = 64, kWaveMaxM = 1024;
constexpr int64_t kProbe = 16384;       // points a fresh wavefront-kernel handle solves in front of its first large batch (wave_probe)

struct EventTriple { hipEvent_t a, mid, b; };

// The two allocation policies of lmpc::Buffer (lmpc_buffer.hpp) and the count of their live blocks (lmpc_debug_live_blocks)
inline std::atomic<int64_t> g_live_blocks{0};
struct DeviceAlloc {
    static hipError_t allocate(void **p, void **dev, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) { *p = nullptr; return e; }
        *dev = *p;
        g_live_blocks++;
        return hipSuccess;
    }
    static void release(void *p) { (void)hipFree(p); g_live_blocks--; }
};
// pinned host memory; with hipHostMallocMapped also its device address, and then both or nothing
template <unsigned FLAGS>
struct HostAlloc {
    static hipError_t allocate(void **p, void **dev, size_t bytes) {
        hipError_t e = hipHostMalloc(p, bytes, FLAGS);
        if (e != hipSuccess) { *p = nullptr; return e; }
        if (FLAGS & hipHostMallocMapped) {
            e = hipHostGetDevicePointer(dev, *p, 0);
            if (e != hipSuccess) { (void)hipHostFree(*p); *p = nullptr; return e; }
        }
        g_live_blocks++;
        return hipSuccess;
    }
    static void release(void *p) { (void)hipHostFree(p); g_live_blocks--; }
};
template <class T> using DevBuf = Buffer<T, DeviceAlloc>;
template <class T> using MappedBuf = Buffer<T, HostAlloc<hipHostMallocMapped>>;
template <class T> using PinnedBuf = Buffer<T, HostAlloc<hipHostMallocDefault>>;
using DevBytes = DevBuf<unsigned char>;       // a block whose element type varies with the call: as<R>()
// option "list_snapshot": one work list copied aside -- one set of counters, then the kShards segments (lmpc_api.hip)
struct ListSnapshot {
    DevBuf<int32_t> buf;
    long long segCap = 0;       // seg_cap of the list it holds (0: none)
    hipError_t prepare(long long seg_cap);                      // room for such a list, before anything is enqueued
    hipError_t take(const int32_t *count, const int32_t *list, long long seg_cap, hipStream_t st);
    // the counts and (list != nullptr) the segments back on the host; the list's seg_cap, 0 without one, or an error of `who`
    long long read(lmpc_handle *h, const char *who, int32_t *counts, int32_t *list, long long list_words) const;
};
}  // namespace lmpc

// What lmpc_release_scratch gives back: every buffer that grows with the batch, with its capacity and phase fields.
// The function resets this struct as a whole, so a buffer declared here is released without being named anywhere else.
struct lmpc_scratch {
    template <class T> using DevBuf = lmpc::DevBuf<T>;
    // staging for the host-pointer entry point (sWarm: allocated by the first warm call)
    DevBuf<double> sTheta, sX;
    DevBuf<int32_t> sFlag, sIter;
    DevBuf<uint64_t> sAct, sWarm;
    int64_t sCap = 0;
    // work list of the problems the screening pass leaves for the iterating kernel
    DevBuf<int32_t> dList, dCount;
    DevBuf<int32_t> dList2, dList3;        // second work list of the scenario-asynchronous closed loop (lists alternate per round; lazy)
    int64_t listCap = 0;        // batch size the list buffer was sized for
    int countSet = 0;           // which of the two counter sets the next call uses
    lmpc::ListSnapshot snap;    // option "list_snapshot": the list of the last front pass
    // the wavefront path's first-pass overflow list, and the slow path for working sets beyond the 64 lanes
    // (lmpc_big_kernel.hpp): overflow list, per-thread scratch
    DevBuf<int32_t> dOvfList1;
    int64_t ovfCap1 = 0;
    DevBuf<int32_t> dOvfList, dBigI;
    lmpc::DevBytes dBigR;
    int64_t ovfCap = 0;
    // branch and bound: per-wavefront snapshots of a node's state, one slot per search depth (lmpc_wave_kernel.hpp)
    lmpc::DevBytes dBnbR, dBnbI;
    lmpc::DevBytes dRowBnb;     // ... of the row kernel's searches (lmpc_row_inst.hip)
    // closed loop on the wavefront path: per-scenario working set + factor kept between two steps ("sim_keep_factor")
    lmpc::DevBytes dKeepR;
    DevBuf<int32_t> dKeepI;
    int64_t keepCap = 0;
    // variational handle: scratch slabs, the two work lists of the chain with their counters (two sets), the snapshot of both
    DevBuf<double> dAviR;
    DevBuf<int32_t> dAviI;
    int aviSlabs = 0;           // wavefront slabs of scratch allocated
    DevBuf<int32_t> dAviList[2], dAviCnt;
    int64_t aviListCap = 0;
    lmpc::ListSnapshot aviSnap[2];
    // closed-loop simulation scratch (simTheta2, simK: allocated by their first user)
    DevBuf<double> simTheta, simTheta2, simU, simFG;
    DevBuf<int32_t> simK;               // per-scenario step counters
    DevBuf<int32_t> simFlag;
    DevBuf<uint64_t> simAct;
    int64_t simCap = 0;
    // generated-controller entry point (lmpc_compute_control*): scratch, warm-start state
    DevBuf<double> ccTheta;
    DevBuf<uint64_t> ccAct;
    DevBuf<int32_t> ccFlag;
    int64_t ccCap = 0, ccWarmN = -1;    // ccWarmN: batch size whose final working sets ccAct holds
    DevBuf<double> ccObsScratch;        // lmpc_compute_control_observer: state and disturbance split from the observer state
    int64_t ccObsCap = 0;
    DevBuf<double> ccStage;             // host-pointer entry point: device copies of the five argument arrays
    DevBuf<int32_t> ccStageFlag;
    int64_t ccStageCap = 0;
    size_t ccStagePer = 0;
    // scenario loop (lmpc_scenario.hip): the run's constants (true plant, measurement, cost weights, constraint rows) and
    // its per-run scratch (observer state the caller does not keep, previous control of the cost's du term)
    DevBuf<double> scnC, scnScr;
    // differentiable solve (lmpc_sens.hip): the derived pack [G | P = M Rout' | Dth | Xth | soft] built by the first call,
    // the work list of the points left for the wavefront kernel and its counter
    DevBuf<double> dSens;
    DevBuf<int32_t> dSensList, dSensCnt;
    int64_t sensListCap = 0;
    // scenario loop adjoint (lmpc_scenario_adjoint.hip): per scenario [alpha | beta | gamma | ubar | theta-bar] of the
    // backward sweep and the step's VJP status; adjCap: scenarios the status holds, adjDoubles: doubles the state holds
    // (the doubles per scenario vary with the descriptor; both only grow)
    DevBuf<double> adjState;
    DevBuf<int32_t> adjStatus;
    int64_t adjCap = 0;
    size_t adjDoubles = 0;
    // gradient with respect to the pack (lmpc_pack_grad.hip): the constants [M | Rout | du | dl] built by the first call;
    // one slab of records [lambda | y] and statuses, its partials (one per 64 points), one sum per slab.  pgCap: the N
    // they were sized for, pgSlabLog: log2 of the slab they were sized for (the work list is dSensList)
    DevBuf<double> pgK, pgRec, pgPart, pgSum;
    DevBuf<int32_t> pgSt;
    int64_t pgCap = 0;
    int pgSlabLog = 0;
};

struct lmpc_handle : lmpc_scratch {
    template <class T> using DevBuf = lmpc::DevBuf<T>;
    template <class T> using MappedBuf = lmpc::MappedBuf<T>;
    ~lmpc_handle();             // events, streams, the unreported error word (lmpc_api.hip); the buffers free themselves
    lmpc::HostPack P;
    lmpc_settings S;
    int device = 0;
    int laneN = 0;              // lane-kernel instantiation (row stride of M/Rout on the device)
    lmpc::PackLayout L{};
    DevBuf<double> dC;          // constant pack on the GPU
    size_t nC = 0;
    std::string err, kname;
    std::mutex errMu;           // `err` is written through fail() only: the host pipeline's upload thread and the caller's
                                // thread can both fail on one handle; everything else of a handle is
                                // single-caller state -- one thread at a time per handle, as for a DAQP workspace
    // the host-pointer entry point's three-stage pipeline: H2D copies, kernels, D2H copies on their own streams (lmpc_multi.hip)
    hipStream_t sUp = nullptr, sRun = nullptr, sDown = nullptr;
    std::vector<hipEvent_t> pipeEv;
    int hostChunk = 32768;      // tuning: smallest (= last) chunk of the pipeline's schedule ("host_chunk")
    int hostRegister = 0;       // tuning: pin the caller's arrays in place for the call ("host_register"; see lmpc_multi.hip)
    int hostThreads = 1;        // tuning: pageable arrays: upload and download sides on separate host threads ("host_threads")
    bool screen = true;         // two-pass (screen + iterate) for cold starts; lmpc_set_option
    // general path: one QP per wavefront
    bool useWave = false;
    bool bnb = false;           // rows flagged BINARY: branch and bound in the wavefront kernel
    int waveCap = 0;            // tuning: wavefronts per CU for the wave kernel's grid (0 = 16)
    bool waveQueue = true;      // tuning: dynamic problem queue of the wave kernel (0 = static split)
    int screenWave = 1;         // tuning: screening pass in front of the wavefront kernel where it applies ("screen_wave")
    bool screenPackOnly = false;   // the lane-style pack holds only what the screening pass reads (wave-only problem)
    DevBuf<int32_t> dQueue;
    int waveOvfSet = 0;         // ... and which pair of overflow counters this CALL uses
    int waveTwoPass = -1;       // option "wave_two_pass": -1 auto, 0 off, 1 whenever the capacity allows
    int waveCap1 = 24;          // option "wave_cap1": working-set capacity of the first pass when "wave_two_pass" is 1
    DevBuf<unsigned long long> dStat;                // working-set statistics of the wavefront kernel (device, cumulative)
    MappedBuf<volatile unsigned long long> hStat;    // ... their copy in mapped host memory, written by every launch
    unsigned long long *dStatHost = nullptr;         // ... and its device address
    bool waveProbed = false;    // a fresh handle's first large batch has been probed for its working-set sizes (wave_probe)
    int waveProbe = 1;          // option "wave_probe": 0 = never probe (first calls run in one pass until statistics exist)
    unsigned long long statA[4] = {0, 0, 0, 0}, statB[4] = {0, 0, 0, 0};   // window of the statistics: snapshots of the
                                // cumulative counters about 2^20 problems apart; decisions use (now - statA)
    int waveCtrSet = 0;         // which of the two (ticket, overflow) counter pairs the next wavefront-kernel launch uses
    // what launch_wave_cfg last enqueued (lmpc_wave_launch_info): a ring of the four most recent wavefront-kernel
    // launches, LMPC_WAVE_INFO_WORDS words each, and how many the handle has made in its life (host memory only)
    lmpc::LaunchRing<LMPC_WAVE_INFO_WORDS, 4> waveRec;
    // ... and launch_row_shape (lmpc_row_launch_info): the four most recent row-kernel launches, counted apart
    lmpc::LaunchRing<LMPC_ROW_INFO_WORDS, 4> rowRec;
    // ... and of the front passes (lmpc_front_pass_info): the four most recent screening / tiers launches, counted apart
    lmpc::LaunchRing<LMPC_FRONT_INFO_WORDS, 4> frontRec;
    // option "list_snapshot": every front pass's counter set and work list copied aside for lmpc_work_list_read (snap)
    int listSnapshot = 0;
    DevBuf<int32_t> dRegTable;     // hash table of lmpc_distinct_active_sets_device (lmpc_regions.hip): 16 control words + slots
    int regCap = 0;
    DevBuf<unsigned long long> dRegW1;      // one-word masks: key / count / first-index tables of regW1Cap slots each (clean
    int regW1Cap = 0;                       // between calls: the publishing kernel resets what it read)
    int regW1 = 1;                          // tuning: 0 = the ballot-loop kernels also for one-word masks ("region_lockfree")
    bool regOvStale = false;                // dRegTable[0] may hold the overflow word of a ballot-kernel call: the lock-free path clears it first
    int regBlocks = 0;          // tuning: workgroups per CU of the two-level distinct-mask reduction ("region_blocks", 0 = 1)
    MappedBuf<long long> hRegOut;   // lmpc_discover_regions_device: result block in mapped host memory ...
    long long *dRegOut = nullptr;   // ... and its device address
    // slow path for working sets beyond the 64 lanes (lmpc_big_kernel.hpp): the counters of its overflow lists
    int capFull = 0;            // n + 2 + #soft: the rows a working set of this problem can reach (one beyond the kernels' own n + 1 + #soft)
    DevBuf<int32_t> dOvfCount;
    int simKeep = 1;            // closed loop on the wavefront path: working set + factor kept between two steps ("sim_keep_factor")
    int simRunAhead = 1;        // scenario-asynchronous loop on the wavefront path: consecutive steps of a scenario inside the kernel
    int nBinary = 0;            // rows flagged BINARY = the search's largest depth
    int bigPath = 1;            // tuning: 0 = leave such points at exit flag -7 ("big_path")
    int wavePacked = -1;        // tuning: layout of the wave kernel's factor (-1 automatic, 0 square, 1 packed)
    int waveLevel = -1;         // tuning: LDS staging level of the wave kernel (-1 = automatic)
    int waveGram = 0;           // Gram-scan form of the wavefront kernel ("gram_scan"; lmpc_wave_kernel.hpp GRAM)
    int waveNwv = 0;            // tuning: wavefronts per wave-kernel workgroup (0 = automatic)
    int laneBlock = 0;          // tuning: workgroup size of the lane kernel (0 = automatic)
    int lanePer = 0;            // tuning: work-list workgroups per shard (0 = one resident round)
    int laneTier = 1;           // tuning: first-tier capacity in the boxed lane kernels (results identical either way)
    int laneStraight = 1;       // tuning: straight-line first tier in the boxed lane kernels ("lane_straight", lmpc_tiers.hpp)
    int fastPath = 1;           // tuning: one-launch kernel for small boxed problems ("fast", lmpc_fast_kernel.hpp)
    int fastTiles = 0;          // tuning: tiles of 64 problems per workgroup of that kernel (0 = 24)
    int fastNstr = 0;           // tuning: streaming wavefronts per workgroup of that kernel, 1..4 (0 = 3)
    int fastDyn = -1;           // tuning: tiles per workgroup of that kernel handed out through global tickets (-1 = default 4)
    DevBuf<int32_t> dFastCtr;      // ... their counters: two alternating sets of kFastCtrs, 128 bytes apart
    int fastCtrSet = 0;
    int fastDma = -1;           // tuning: LDS-DMA ring depth of its streaming wavefronts (-1 = default, 0 = registers, 2, 3)
    int32_t *dFastErr = nullptr;   // raised by that kernel if one of its bounded waits ran out (never expected):
    MappedBuf<volatile int32_t> hFastErr;   // ... a word of pinned host memory, dFastErr its device address
    DevBuf<int32_t> dFastTrace;    // (-DLMPC_FAST_TRACE builds: dFastErr is this device block, the error word in front of the trace)
    int fastStage = -1;            // tuning: staged write-out of that kernel ("fast_stage"): 0 never, 1 wherever it applies,
                                   // -1 = where it applies with several batches in flight ("in_flight" >= 2)
    int inFlight = 1;              // the caller's hint "in_flight"
    // what launch_fast_t / launch_fast_multi_t last enqueued (lmpc_fast_launch_info) and how many launches the handle has made
    lmpc::LaunchRing<LMPC_FAST_INFO_WORDS, 1> fastRec;
    int fastSpinLimit = 0;         // test hook ("fast_spin_limit"): k > 0 = the kernel's waits give up after k - 1 polls
    // affine variational inequality (non-symmetric H, is_avi): its own kernel, pack and scratch (lmpc_avi.hip)
    bool avi = false;
    lmpc::AviLayout A{};
    DevBuf<double> dCa;
    DevBuf<int32_t> dSa;
    int aviWaves = 0;           // tuning: wavefronts per CU of its grid ("avi_waves", 0 = 16)
    // ... small box-constrained problems: register-resident straight-line kernels in front of it (lmpc_avi_tiers_kernel.hpp)
    int aviTiersN = 0;          // n if the problem qualifies (2 .. 8), else 0
    int aviTiers = 1;           // tuning: 0 = the generic kernel alone ("avi_tiers"; results identical either way)
    int aviTiersFirst = -1;     // tuning: tiers of the pass over the whole batch, 0 .. 3 ("avi_tiers_first"; -1: 3 up to n = 6, else 2;
                                // 0: the lane kernel over the whole batch)
    int aviTiersOcc[2] = {0, 0};   // workgroups per CU the two instantiations keep resident (0 = not asked yet)
    int aviChainGroups = 0;     // tuning: cap on the workgroups of the chain's three launches ("avi_chain_groups", 0 = none)
    // what launch_avi last enqueued (lmpc_avi_launch_info): a ring of the eight most recent launches of the chain
    lmpc::LaunchRing<LMPC_AVI_INFO_WORDS, LMPC_AVI_INFO_KEPT> aviRec;
    // differentiable solve (lmpc_sens.hip): what sens_launch last enqueued (lmpc_sens_launch_info), the four most recent calls
    lmpc::LaunchRing<LMPC_SENS_INFO_WORDS, 4> sensRec;
    // ... and the backward sweeps of the scenario loop (lmpc_scenario_adjoint_launch_info), the four most recent calls
    lmpc::LaunchRing<LMPC_SCENARIO_ADJOINT_INFO_WORDS, 4> adjRec;
    int sensCap = 0;            // tuning: CAP of the lane kernel, 5 or 8 ("sens_cap", 0 = by the rows a set of the problem reaches)
    int sensForceList = 0;      // tuning: every point with a non-empty set goes to the wavefront kernel ("sens_force_list")
    int sensReserve = 0;        // "sens_reserve": lmpc_reserve also allocates what the derivative calls need
    // ... and the pack gradients (lmpc_pack_grad_launch_info), the four most recent calls
    lmpc::LaunchRing<LMPC_PACK_GRAD_INFO_WORDS, 4> packGradRec;
    int packGradSlab = 0;       // tuning: log2 of the points of a slab ("pack_grad_slab", 0 = by the scratch budget)
    int packGradReserve = 0;    // "pack_grad_reserve": lmpc_reserve also allocates what lmpc_solve_pack_vjp_device needs
    lmpc::WaveLayout W{};
    DevBuf<double> dCw;
    DevBuf<float> dCwf;         // binary32 copy of the wave kernel's pack, built on the first f32 solve
    DevBuf<int32_t> dSw;
    int numCU = 256;
    int simAsync = 1;           // tuning: scenario-asynchronous closed loop ("sim_async"; one round: lmpc::AsyncRound)
    int simSmall = 1;                   // ... the all-in-registers instantiation of sim_run_kernel where it applies
    int simBlind = 2;                   // ... rounds enqueued between two reads of the work-list counters
    int ccFused = 1;            // tuning: lmpc_compute_control assembles theta inside the screening kernel ("cc_fused")
    int simFused = 1;           // tuning: plant step inside the lane / screening kernels (lmpc_set_option "sim_fused")
    // generated-controller entry point (lmpc_compute_control*): layout of theta
    int ccNx = -1, ccNr = 0, ccNd = 0, ccNup = 0, ccNp = 0, ccNph = 0;
    DevBuf<double> ccT2S;
    // generated observer (lmpc_set_observer): [MPC_PLANT_DYNAMICS | MPC_MEASUREMENT_FUNCTION | K_TRANSPOSE_OBSERVER]
    DevBuf<double> obsC;
    int obsNx = 0, obsNu = 0, obsNd = 0, obsNy = 0;
    // lmpc_solve_one: ONE record in mapped host memory (theta in, x and flag out), its device address, its own stream
    MappedBuf<char> oneHost;
    char *oneDev = nullptr;
    hipStream_t oneStream = nullptr;
    // lmpc_compute_control with a handful of problems (the generated controller's one call per time step): its five
    // argument arrays and the flags in mapped host memory likewise
    MappedBuf<char> ccMapHost;
    char *ccMapDev = nullptr;
    // small problems with many rows on the wavefront path: straight-line tiers, one problem per lane, in front of it
    // (lmpc_qp_tiers_kernel.hpp)
    bool qpTiersOk = false;     // the problem qualifies (n = 2 .. 12, m <= 64 hard or SOFT rows without other flags, nth <= 16)
    DevBuf<double> dQpScan;     // ... its scan pack (rows of M with their bounds), built with the first launch
    int qpTiers = 1;            // "qp_tiers": 0 = screening pass + wavefront kernel as before, 2 = always the tiers pass, 1 (default) =
                                // the tiers pass, and for large batches whichever of the two the handle has MEASURED faster
    // ... that measurement: one large call each way, timed by events that are read (without waiting) by later calls;
    // taken again every 512 calls.  Variant 0 = with the pass, 1 = without.
    struct QpAb {
        hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};      // (kept by reset(): created once, destroyed with the handle)
        bool pending[2] = {false, false};
        int64_t n[2] = {0, 0};
        double nsPer[2] = {-1.0, -1.0};     // measured nanoseconds per problem (-1: not measured yet)
        double acc[2] = {-1.0, -1.0};       // ... best sample of the current round of measurements, and how many it holds
        int cnt[2] = {0, 0};
        long long calls = 0;
        void reset() { calls = 0; nsPer[0] = nsPer[1] = -1.0; pending[0] = pending[1] = false; cnt[0] = cnt[1] = 0; }   // measure again
    } qpAb;
    // four problems per wavefront (lmpc_row_kernel.hpp) in front of / instead of the wavefront kernel
    int rowKernel = -1;         // "row_kernel": -1 = where it applies (large cold batches), 0 = never, 1 = whenever an instantiation covers
    int rowBlocks = 0;          // tuning: workgroups per CU of its grid ("row_blocks", 0 = what LDS and registers allow)
    bool waveWarmed = false;    // lmpc_reserve has sent its one dummy problem through the wavefront kernel
    // profiling: the user's switch (lmpc_profile and nothing else writes it; a launch ANDs it with LoopMode::prof)
    bool prof = false;
    std::vector<lmpc::EventTriple> events;
    std::vector<hipEvent_t> eventPool;   // recycled by lmpc_profile_read
};

extern thread_local std::string g_setup_err;

namespace lmpc {

int fail(lmpc_handle *h, int code, const std::string &msg);
// the one-launch kernel's error word (lmpc_fast_inst.hip): LMPC_OK, or LMPC_ERR_HIP once per raised error
int check_fast_err(lmpc_handle *h);

#define HIP_TRY(h, call)                                                                     \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess)                                                               \
            return lmpc::fail(h, LMPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

#define LMPC_TRY(call) do { const int rct__ = (call); if (rct__ != LMPC_OK) return rct__; } while (0)

// Profiling bracket of one call: three pooled events on the launch stream -- begin, mid (between a front pass and the
// iterating kernel), end.  end() hands a call that succeeded to h->events (lmpc_profile_read); on every other way out,
// an early return included, the events are given back.  Nothing is created or recorded while profiling is off.
hipError_t pool_event(lmpc_handle *h, hipEvent_t *e);
struct ProfBracket {
    lmpc_handle *const h;
    const hipStream_t st;
    EventTriple ev{nullptr, nullptr, nullptr};
    bool on = false;
    ProfBracket(lmpc_handle *h_, hipStream_t st_) : h(h_), st(st_) {}
    ProfBracket(const ProfBracket &) = delete;
    ProfBracket &operator=(const ProfBracket &) = delete;
    ~ProfBracket() { drop(); }
    // with_mid false: a call of one launch from the start (no middle event is taken)
    int begin(bool enable, bool with_mid = true) {
        if (!enable) return LMPC_OK;
        on = true;
        HIP_TRY(h, pool_event(h, &ev.a));
        if (with_mid) HIP_TRY(h, pool_event(h, &ev.mid));
        HIP_TRY(h, pool_event(h, &ev.b));
        HIP_TRY(h, hipEventRecord(ev.a, st));
        return LMPC_OK;
    }
    int mid() {
        if (on && ev.mid) HIP_TRY(h, hipEventRecord(ev.mid, st));
        return LMPC_OK;
    }
    // the call turned out to be one launch: the middle event goes back unrecorded
    void skip_mid() {
        if (on && ev.mid) { h->eventPool.push_back(ev.mid); ev.mid = nullptr; }
    }
    int end(int rc) {
        if (on && rc == LMPC_OK) {
            HIP_TRY(h, hipEventRecord(ev.b, st));
            h->events.push_back(ev);
            on = false;
        }
        return rc;
    }
    void drop() {
        if (!on) return;
        for (hipEvent_t e : {ev.a, ev.mid, ev.b}) if (e) (void)hipEventDestroy(e);
        on = false;
    }
};

// One round of the scenario-asynchronous closed loop.  lmpc_simulate_device keeps it on its stack and points
// LoopMode::round at it: the inputs of the round's two launches, and what the streaming half leaves for the iterating
// half and for the next round.
struct AsyncRound {
    int phase = 1;                      // which half `launch` runs: 1 streaming (sim_run_kernel), 2 iterating
    int T = 0;                          // steps of the run
    int cap = 0;                        // steps a scenario may run ahead in this streaming pass
    bool resetPark = false;             // this pass consumes the parked list: clear its counters afterwards
    long long maxIn = 0;                // longest shard segment of listIn (sizes the grid)
    const int32_t *listIn = nullptr, *cntIn = nullptr;               // the round before's list (nullptr: every scenario)
    const double *x = nullptr, *r = nullptr, *up = nullptr;          // first pass only: form theta from these
    int32_t *cntNow = nullptr, *cntNext = nullptr, *listOut = nullptr;   // OUT (launch_sim_run): counter sets, the list it wrote
};

// What a loop around the batched solve tells a launch: an argument of launch() and everything below it, filled by
// lmpc_simulate_device (fused plant step, rounds, kept factors, no profiling) and lmpc_compute_control_device (the
// gather).  A default-constructed one is a plain call: every other entry point passes that.
struct LoopMode {
    SimFuse sim{};                      // lane / screening kernels: plant step fused in (FG == nullptr: off)
    GatherArgs gat{};                   // screening / one-launch kernel: theta from the controller's five arrays (state == nullptr: off)
    WaveSim waveSim{};                  // wavefront kernel: plant step fused in, run-ahead (FG == nullptr: off)
    bool keep = false;                  // wavefront kernel: working set + factor kept between two steps (dKeepR, dKeepI)
    bool raWarm = false;                // the run-ahead loop in progress is a warm one
    bool prof = true;                   // ANDed with the handle's switch (the rounds, the probe and lmpc_reserve: false)
    AsyncRound *round = nullptr;        // scenario-asynchronous closed loop (nullptr: off)
    bool plain() const { return sim.FG == nullptr && gat.state == nullptr && waveSim.FG == nullptr && !keep && round == nullptr; }
};
// the handle's layout as a lane / screening / sim_run / one-launch kernel of this call takes it: h->L itself without
// fusion or gather (whose two structs it holds empty), else `tmp` = a copy of it with the mode's two filled in
inline const PackLayout &pack_layout(const lmpc_handle *h, const LoopMode &mode, PackLayout &tmp) {
    if (mode.sim.FG == nullptr && mode.gat.state == nullptr) return h->L;
    tmp = h->L; tmp.sim = mode.sim; tmp.gat = mode.gat;
    return tmp;
}

// What one launch on the wavefront path (wavefront kernel or row kernel) is told by its caller, the wavefront side of its
// LoopMode included, down launch_wave -> launch_wave_t -> launch_wave_inst -> launch_wave_cfg and launch_row* -> launch_row_shape.
struct WaveArgs {
    int pass = 0;               // 0: the only pass; 1: first of two (smaller capacity); 2: second (walks the first one's overflow list)
    WorkList list{};            // work list of a front pass (list == nullptr: the whole batch)
    int cap = 0;                // working-set capacity of this launch (the kernel's ldc = cap | 1)
    int level = -1, nwv = 0;    // preferred LDS staging level (-1 = automatic) and wavefronts per workgroup (0 = automatic)
    WaveSim waveSim{};          // LoopMode::waveSim, keep, raWarm, prof
    bool keep = false, raWarm = false, prof = true;
    bool preload = false;       // setup: bring the kernel's code object onto the device, launch nothing (preload_code)
    bool in_loop() const { return waveSim.FG != nullptr || keep; }
};
// ... of a launch at the handle's own capacity and tuning ("wave_cap", "wave_level", "wave_nwv")
inline WaveArgs wave_args(const lmpc_handle *h, const LoopMode &mode, const WorkList &list = WorkList{}) {
    WaveArgs a;
    a.list = list; a.cap = h->W.cap; a.level = h->waveLevel; a.nwv = h->waveNwv;
    a.waveSim = mode.waveSim; a.keep = mode.keep; a.raWarm = mode.raWarm; a.prof = mode.prof;
    return a;
}

// LMPC_OK, or LMPC_ERR_NOGPU with the library's one text for it; `count`: the number of devices, for the callers that
// go on to check an ordinal (h == nullptr: the text goes where a failed setup's does)
int need_device(lmpc_handle *h, int *count = nullptr);
#define LMPC_NEED_DEVICE(h) do { const int rcd__ = lmpc::need_device(h); if (rcd__ != LMPC_OK) return rcd__; } while (0)

// The glue kernels' state count as a template argument: f(std::integral_constant<int, NXT>) with NXT = nx for
// 1 <= nx <= 8 (compile-time state count), NXT = 0 (run-time nx) for everything else
template <class F>
void dispatch_nx(int nx, F &&f) {
    switch (nx) {
#define LMPC_NX_CASE(NX) case NX: f(std::integral_constant<int, NX>{}); break;
        LMPC_NX_CASE(1) LMPC_NX_CASE(2) LMPC_NX_CASE(3) LMPC_NX_CASE(4)
        LMPC_NX_CASE(5) LMPC_NX_CASE(6) LMPC_NX_CASE(7) LMPC_NX_CASE(8)
#undef LMPC_NX_CASE
        default: f(std::integral_constant<int, 0>{}); break;
    }
}

// Device copies of the arrays of one host-pointer call, released when the call returns.  A NULL host array gives a
// NULL device array.  The first HIP error sticks (`err`, `what`): every later request does nothing and returns NULL,
// so a wrapper asks for all its arrays and tests once.  With an `arena` the arrays are carved from that block, which
// the caller keeps, instead of being allocated.
struct Staging {
    struct Back { void *host; const void *dev; size_t bytes; };
    std::vector<void *> owned;
    std::vector<Back> back;
    char *arena = nullptr;
    hipError_t err = hipSuccess;
    const char *what = "";
    Staging() = default;
    explicit Staging(void *block) : arena(static_cast<char *>(block)) {}
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging() { for (void *p : owned) (void)hipFree(p); }
    bool ok(hipError_t e, const char *call) {
        if (e != hipSuccess && err == hipSuccess) { err = e; what = call; }
        return err == hipSuccess;
    }
    void *alloc(size_t bytes) {
        void *p = arena;
        if (err != hipSuccess) return nullptr;
        if (arena) { arena += bytes; return p; }
        if (!ok(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc")) return nullptr;
        owned.push_back(p);
        return p;
    }
    void *zeros(size_t bytes) {
        void *p = alloc(bytes);
        if (p) ok(hipMemset(p, 0, bytes), "hipMemset");
        return p;
    }
    void *in(const void *host, size_t bytes) {
        void *p = host ? alloc(bytes) : nullptr;
        if (p) ok(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice), "hipMemcpy");
        return p;
    }
    // an array download_all() copies back: the helper's own (uploaded first with `upload`), or one at `dev`
    void *out(void *host, size_t bytes, bool upload = false) {
        void *p = !host ? nullptr : upload ? in(host, bytes) : alloc(bytes);
        if (p) back.push_back(Back{host, p, bytes});
        return p;
    }
    void out_from(void *host, const void *dev, size_t bytes) { if (host) back.push_back(Back{host, dev, bytes}); }
    bool download_all() {
        for (const Back &b : back)
            if (!ok(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost), "hipMemcpy")) break;
        return err == hipSuccess;
    }
    int fail(lmpc_handle *h) const { return lmpc::fail(h, LMPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(err)); }
};

// Every entry point works on the handle's GPU and hands the caller's current device back when it returns
// (a host application with several GPUs keeps its own notion of "current device").
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t enter(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == dev) return hipSuccess;
        const hipError_t e = hipSetDevice(dev);
        switched = (e == hipSuccess) && prev >= 0;
        return e;
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};
#define LMPC_ENTER_DEVICE(h) lmpc::DeviceScope lmpc_dev_scope__; HIP_TRY(h, lmpc_dev_scope__.enter((h)->device))

// affine-variational-inequality mode (lmpc_avi.hip): pack upload, settings, launch
int finalize_avi(lmpc_handle *h);
void avi_fill_settings(lmpc_handle *h);
int launch_avi(lmpc_handle *h, int64_t nprob, const double *theta, double *x, int32_t *flag, int32_t *iters,
               uint64_t *active, const uint64_t *warm, hipStream_t st);
int snapshot_capture_check(lmpc_handle *h, hipStream_t st);      // "list_snapshot": refuses a call inside a stream capture
// what launch_avi_tiers enqueued, for the handle's record (lmpc_avi_launch_info)
struct AviLaunchShape { int stage = 0, n = 0, k = 0, list = 0; size_t lds = 0; };
int launch_avi_tiers(lmpc_handle *h, bool first, int kfirst, unsigned grid, hipStream_t st, const double *theta, double *x,
                     int32_t *flag, int32_t *iters, uint64_t *active, const int32_t *list_in, const int32_t *count_in,
                     int32_t *list_out, int32_t *count_out, int32_t *count_clear, long long seg_cap, long long nprob, int *occ,
                     AviLaunchShape *shape = nullptr);

// what a front pass's launcher enqueued, for the handle's record (lmpc_front_pass_info)
struct FrontLaunch { int kind = 0, n = 0; long long grid = 0; size_t lds = 0; };

// one-launch solver for small box-constrained problems (lmpc_fast_inst.hip)
bool fast_covers(const lmpc_handle *h);
void fast_preload(lmpc_handle *h);
size_t qp_tiers_lds_bytes(int n, int m);
int launch_qp_tiers(lmpc_handle *h, int64_t nprob, const double *theta, double *x, int32_t *flag, int32_t *iters,
                    uint64_t *active, int32_t *list, int32_t *count, long long seg_cap, hipStream_t st, bool preload,
                    FrontLaunch *fl = nullptr);
void avi_preload(lmpc_handle *h);
int avi_reserve(lmpc_handle *h, int64_t nprob, hipStream_t st);
int launch_fast(lmpc_handle *h, const LoopMode &mode, int64_t nprob, const double *theta, double *x, int32_t *flag, int32_t *iters,
                uint64_t *active, hipStream_t st);
int launch_fast_multi(lmpc_handle *h, int nb, int64_t nprob, const double *const *theta, double *const *x, int32_t *const *flag,
                      hipStream_t st);

// capacity of the first of two passes the wavefront kernel would run a batch of nprob problems at as `a` says (0: one
// pass; lmpc_wave_launch.hpp, compiled into the binary64 translation unit)
int wave_first_pass_cap(lmpc_handle *h, const WaveArgs &a, int64_t nprob);
void wave_stat_read(const lmpc_handle *h, unsigned long long out[4]);
int wave_reserve(lmpc_handle *h, int64_t nprob, hipStream_t st);
// the wavefront path's lazily allocated scratch (defined once, next to wave_reserve; each does nothing where its
// buffer is in place and large enough): ticket and overflow counters, working-set statistics with their mapped host
// copy, the first pass's overflow list, the slow path's list with its per-thread scratch
int wave_scratch_counters(lmpc_handle *h, hipStream_t st);
int wave_scratch_stats(lmpc_handle *h, hipStream_t st);
int wave_scratch_list1(lmpc_handle *h, int64_t nprob);
int wave_scratch_slow(lmpc_handle *h, int64_t nprob);

// lmpc_api.hip's launch policy and scratch for the second API unit (lmpc_api_loop.hip); that unit's code preload
int api_launch(lmpc_handle *h, const LoopMode &mode, int64_t nprob, const double *theta, double *x, int32_t *flag, int32_t *iters,
               uint64_t *active, const uint64_t *warm, hipStream_t st);
int api_ensure_sim(lmpc_handle *h, int64_t N);
int api_ensure_f32(lmpc_handle *h);
bool api_will_screen(const lmpc_handle *h, int64_t nprob);
bool api_wave_screens(const lmpc_handle *h, int64_t nprob);
int api_wave_probe(lmpc_handle *h, const double *theta, int64_t nprob, hipStream_t st);
int api_launch_wave_f32(lmpc_handle *h, const float *dC, int64_t nprob, const float *theta, float *x, int32_t *flag, int32_t *iters,
                        uint64_t *active, const uint64_t *warm, hipStream_t st);
void loop_preload();
// differentiable solve (lmpc_sens.hip): derived pack and work list for a batch of N; the same for lmpc_reserve (nothing
// on a handle the derivative calls refuse)
struct SensDims;
struct SensView;
int sens_ensure(lmpc_handle *h, int64_t N);
int sens_reserve(lmpc_handle *h, int64_t N);
// ... why a handle has no derivative (nullptr: it has one) with the refusal's code, and the refusal itself
const char *sens_no_derivative(const lmpc_handle *h, int *code);
int sens_refuse(lmpc_handle *h, const char *who);
// ... CAP of the lane kernels and the grid of the wavefront kernels for N points (one copy for every derivative)
int sens_cap_of(const lmpc_handle *h);
unsigned sens_wave_grid(const lmpc_handle *h, int64_t N);
// ... the launches of lmpc_solve_vjp_device for a caller that has passed its refusals (the scenario adjoint, once per
// step); *list_pass: whether the wavefront kernel's pass over the work list was enqueued
int sens_vjp_enqueue(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *flag, const double *xbar, double *thbar,
                     int32_t *status, hipStream_t st, int *list_pass);
// ... for the _host twins: what they refuse of a raw pack (`bounds`: du and dl are there; *st: the settings in force),
// its derived pack [G | P | Dth | Xth | soft] (G == nullptr: accumulated from M), the points' loop
int sens_check_pack(const char *who, int n, int m, int ms, int nth, int nout, const double *M, const double *Dth, const double *Rout,
                    const double *Xth, const int32_t *sense, bool bounds, const lmpc_settings *s, int is_avi, int64_t N,
                    lmpc_settings *st);
void sens_build_pack(int n, const SensDims &d, const double *M, const double *G, const double *Dth, const double *Rout,
                     const double *Xth, const int32_t *sense, std::vector<double> &C);
void sens_host_points(const SensView &S, const SensDims &d, bool jac, int64_t N, const uint64_t *active, const int32_t *flag,
                      const double *xbar, double *out, int32_t *status);
// gradient with respect to the pack (lmpc_pack_grad.hip): its scratch for a batch of N, for lmpc_reserve
int pack_grad_reserve(lmpc_handle *h, int64_t N);
void scenario_preload();
void offset_free_preload();

// four problems per wavefront (lmpc_row_inst.hip): capacity the batch would run at on that kernel (0: it does not take
// the batch), and its launch as the only pass (a.pass 0) or the first of two (a.pass 1) of a wavefront-kernel call at
// a.cap rows
int row_pass_cap(lmpc_handle *h, const WaveArgs &a, int64_t nprob, size_t rs, bool warm, bool gram, bool bnb);
template <typename R>
int launch_row(lmpc_handle *h, const WaveArgs &a, const R *dC, int64_t nprob, const R *theta, R *x, int32_t *flag,
               int32_t *iters, uint64_t *active, hipStream_t st);
extern template int launch_row<double>(lmpc_handle *, const WaveArgs &, const double *, int64_t, const double *, double *, int32_t *,
                                       int32_t *, uint64_t *, hipStream_t);
extern template int launch_row<float>(lmpc_handle *, const WaveArgs &, const float *, int64_t, const float *, float *, int32_t *,
                                      int32_t *, uint64_t *, hipStream_t);
// ... with branch and bound
int row_bnb_pass_cap(lmpc_handle *h, const WaveArgs &a, int64_t nprob, size_t rs);
template <typename R>
int launch_row_bnb(lmpc_handle *h, const WaveArgs &a, const R *dC, int64_t nprob, const R *theta, R *x, int32_t *flag,
                   int32_t *iters, uint64_t *active, hipStream_t st);
extern template int launch_row_bnb<float>(lmpc_handle *, const WaveArgs &, const float *, int64_t, const float *, float *, int32_t *,
                                          int32_t *, uint64_t *, hipStream_t);
extern template int launch_row_bnb<double>(lmpc_handle *, const WaveArgs &, const double *, int64_t, const double *, double *, int32_t *,
                                           int32_t *, uint64_t *, hipStream_t);

// launch of the wavefront kernel for one batch (defined in lmpc_wave_launch.hpp, instantiated once per
// (R, BNB) in lmpc_wave_inst.hip)
template <typename R, bool BNB, bool GRAM, bool SIM = true>
int launch_wave_inst(lmpc_handle *h, const WaveArgs &a, const R *dC, int64_t nprob, const R *theta, R *x, int32_t *flag,
                     int32_t *iters, uint64_t *active, const uint64_t *warm, hipStream_t st);
#define LMPC_WAVE_EXTERN4(R, B, G, S)                                                                                \
    extern template int launch_wave_inst<R, B, G, S>(lmpc_handle *, const WaveArgs &, const R *, int64_t, const R *, R *, \
                                                     int32_t *, int32_t *, uint64_t *, const uint64_t *, hipStream_t);
#define LMPC_WAVE_EXTERN(R, B, G) LMPC_WAVE_EXTERN4(R, B, G, true)
LMPC_WAVE_EXTERN(double, false, false) LMPC_WAVE_EXTERN(double, true, false)
LMPC_WAVE_EXTERN(float, false, false) LMPC_WAVE_EXTERN(float, true, false)
LMPC_WAVE_EXTERN(double, false, true) LMPC_WAVE_EXTERN(double, true, true)
LMPC_WAVE_EXTERN(float, false, true) LMPC_WAVE_EXTERN(float, true, true)
// (binary64 without branch and bound also WITHOUT the closed-loop machinery: the plain batched solve, its own units)
LMPC_WAVE_EXTERN4(double, false, false, false) LMPC_WAVE_EXTERN4(double, false, true, false)
#undef LMPC_WAVE_EXTERN
#undef LMPC_WAVE_EXTERN4

}  // namespace lmpc
