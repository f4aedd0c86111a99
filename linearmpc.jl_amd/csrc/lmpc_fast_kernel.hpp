// ONE launch for small box-constrained problems (m == ms == n <= 6, cold start): streaming pass and the
// iterations of the problems that need them in the same kernel, overlapped in time.
//
// Why: in the two-launch form (screen_kernel, then lane_kernel on the work list) the second kernel is a latency
// chain -- launch, count -> list -> record loads, then ~1500 dependent instructions per wavefront -- of 16 us
// behind 16 us of streaming, although its work is a tenth of the first kernel's.  Here the same work runs
// UNDER the stream:
//
//   * a workgroup of four wavefronts covers R consecutive tiles of 64 problems.  The first `nstr` wavefronts
//     stream them (the record of a wavefront's next tile is in flight while the current one is screened exactly
//     as screen_kernel does it), finish the problems whose unconstrained optimum is feasible and push the
//     indices of the others into the workgroup's queue in LDS (reserve with one LDS atomic per tile, write);
//   * the remaining wavefronts -- and every streaming wavefront once its tiles are done -- claim 64 queued
//     problems at a time (compare-and-swap on the read index) and solve them one per lane: the straight-line
//     tiers of lmpc_tiers.hpp first, the generic loop of lane_kernel (lane_loop, out of line: fast_fallback) for the lanes
//     the tiers do not finish, so the kernel is complete by itself and no second launch follows.
//
// Synchronisation is workgroup-local and one-directional: producers never wait (the queue holds every problem
// of the workgroup), consumers wait only for producers -- for the queue to fill up to a claim, and for a
// reserved slot to be written (slots start at -1; a producer writes its slots right after reserving them).
// Every wait is bounded by a spin limit that raises an error flag instead of hanging.
//
// Outputs: a call with one output per problem and no iters / active array (the plain and the several-batches launch
// on a static split; by default only under the hint "in_flight" >= 2, see launch_fast_t) keeps x and the exit flags of a
// workgroup's tiles in LDS and stores them once, as whole lines, at the workgroup's end (fast_staged_kernel, see fast_body); every
// other call stores them where they are found -- the streaming wavefront its finished lanes, the solving lanes theirs.
//
// Results are those of the two-launch form bit for bit: the screening test, the tiers and lane_loop are the
// same code or the same fma chains.
//
// Replaces, per problem: mpc_update_qp (reference codegen/mpc_update_qp.c:1-10), daqp_ldp ([EXT] libdaqp,
// called at mpc_update_qp.c:48 / utils.jl:282) and mpc_get_solution (mpc_update_qp.c:14-22).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "lmpc_lane_kernel.hpp"
#include "lmpc_tiers.hpp"

namespace lmpc {

#ifndef LMPC_FAST_WAVES
#define LMPC_FAST_WAVES 4      // wavefronts per SIMD the kernel is register-budgeted for (128 VGPRs; see fast_fallback)
#endif
constexpr int kFastGridWaves = 3;         // workgroups per CU the default grid is sized for (launch_fast_t)
constexpr int kFastSpinLimit = 1 << 22;
constexpr int kFastTraceSlots = 9;         // (-DLMPC_FAST_TRACE) words of a wavefront's trace record: stamps 0 .. 6, where it ran, entry
constexpr int kFastCtrs = 16;              // ticket counters of the dynamic tail (a power of two)
constexpr int kFastMaxTiles = 96;          // tiles of 64 problems per workgroup at most (LDS queue: 256 bytes per tile)
#ifndef LMPC_FAST_AHEAD
#define LMPC_FAST_AHEAD 1
#endif
constexpr int kFastAhead = LMPC_FAST_AHEAD;      // tiles a streaming wavefront requests before it consumes the first
// the staged kernels' register path (fast_body): its own tile loop (0: the loop of the other kernels), which asks for the
// next tile's record before the screened tile is published (0: behind it)
#ifndef LMPC_FAST_TURN
#define LMPC_FAST_TURN 1
#endif
#ifndef LMPC_FAST_TURN_EARLY
#define LMPC_FAST_TURN_EARLY 1
#endif

// One LDS-DMA piece: every active lane moves 16 bytes from its own global address straight into LDS at
// lds_dst + 16 * lane (lds_dst wave-uniform, in M0) -- no vector register on the way, 1 KiB per wave-instruction.
// Inline assembly on purpose: the compiler would drain a DMA it knows about with vmcnt(0) in front of the next LDS
// read, and the point of the ring below is to keep the NEXT tile's pieces in flight across that read.
#ifndef LMPC_FAST_DMA_POLICY
#define LMPC_FAST_DMA_POLICY " nt"         // "" default cache policy, " nt" nontemporal
#endif
__device__ __forceinline__ void fast_dma16(const void *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" LMPC_FAST_DMA_POLICY
                 "\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
#ifndef LMPC_FAST_DMA_DEPTH
#define LMPC_FAST_DMA_DEPTH 2              // tiles per streaming wavefront in its LDS ring (0 = records through registers)
#endif
// bytes of one ring slot = one tile of 64 records
__host__ __device__ constexpr size_t fast_tile_bytes(int NT) { return (size_t)64 * NT * sizeof(double); }

// the values as they are HERE, to the compiler: what computes them stays in front, memory accesses stay where they are
__device__ __forceinline__ void fast_pin(double &s) { asm volatile("" : "+v"(s) :: "memory"); }
template <int N> __device__ __forceinline__ void fast_pin(double (&b)[N]) {
#pragma unroll
    for (int j = 0; j < N; j++) fast_pin(b[j]);
}

__device__ __forceinline__ int lds_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// bytes of dynamic LDS a workgroup of fast_kernel<.., N> needs for R tiles
// doubles of the screening constants kept in LDS: rows of Dth padded to NTHMAX columns, (du, dl) pairs, the first
// output's row of Xth, x0 of the first output (+ padding to an even count)
__host__ __device__ constexpr int fast_scr_doubles(int N, int NTHMAX) { return (N * NTHMAX + 2 * N + NTHMAX + 1 + 1) & ~1; }
// doubles of M, G, du0, dl0 at the front of LDS (m == n == N; padded to an even count)
__host__ __device__ constexpr int fast_const_doubles(int N) { return (N * N + N * (N + 1) / 2 + 2 * N + 1) & ~1; }
// THE CONSTANTS AS ONE IMAGE.  What a workgroup keeps at the front of LDS -- the two blocks above -- lies in the handle's
// constant pack a second time, contiguous and in LDS order, right behind the closed loop's F / G block (fill_layout
// appends it for the handles fast_covers() can accept): a staged workgroup's set-up is then ONE 16-byte load per thread
// and one 16-byte LDS store instead of five dependent round trips through the pack's sections (see fast_body).  The
// image's words are copies of the pack's own (fast_image_fill), so every LDS word holds the bits it held when the
// sections were read one by one.
__host__ __device__ constexpr int fast_image_doubles(int N, int NTHMAX) { return fast_const_doubles(N) + fast_scr_doubles(N, NTHMAX); }
__host__ __device__ constexpr int fast_image_pieces(int N, int NTHMAX) { return fast_image_doubles(N, NTHMAX) / 2; }
__host__ __device__ constexpr int fast_image_offset(int oFG) { return oFG + kPackFG; }   // (oFG and kPackFG: multiples of 8 doubles)
static_assert(kPackFG % 8 == 0, "the image starts on a 64-byte boundary");
// which packs carry the image: the sizes the kernel is instantiated for (fast_covers() narrows this by flags and settings)
inline bool fast_image_wanted(int N, int n, int m, int ms, int nth) {
    return N >= 2 && N <= 5 && n == N && m == N && ms == N && nth >= 1 && nth <= 16;
}
// the image from the sections of the pack `buf` it lies in (host; L.nthp is the kernel's NTHMAX); paddings are zero
inline void fast_image_fill(double *buf, const PackLayout &L, int N) {
    const int nconst = N * N + N * (N + 1) / 2 + 2 * N, NTHMAX = L.nthp;
    double *img = buf + fast_image_offset(L.oFG), *scr = img + fast_const_doubles(N);
    for (int i = 0; i < fast_image_doubles(N, NTHMAX); i++) img[i] = 0.0;
    for (int i = 0; i < nconst; i++) img[i] = buf[L.oM + i];                       // M, G, du0, dl0: consecutive in the pack
    for (int i = 0; i < N * NTHMAX; i++) scr[i] = buf[L.oDthP + i];
    for (int i = 0; i < 2 * N; i++) scr[N * NTHMAX + i] = buf[L.oBnd + i];
    for (int i = 0; i < NTHMAX; i++) scr[N * NTHMAX + 2 * N + i] = buf[L.oXthP + i];
    scr[N * NTHMAX + 2 * N + NTHMAX] = buf[L.ox0];
}
// Hand-over of a queued problem: the streaming wavefront that found it has its shifts b_j = Dth_j . theta and the
// output shift x0 + Xth theta in registers; the first kFastPay queue positions of a workgroup carry them in LDS next
// to the index, so the solving wavefront starts on an LDS read instead of re-reading the record from L2 and
// re-forming the products (1.2 us of a 6 us pass).  Positions beyond (a batch where most points iterate) take the
// record from memory as before.  The values are the ones the solving side would compute: same chains, same constants.
#ifndef LMPC_FAST_PAY
#define LMPC_FAST_PAY 256
#endif
constexpr int kFastPay = LMPC_FAST_PAY;
// (stage: the staged write-out below -- the hand-over loses its x-shift column, x and the flags of the workgroup's
// R tiles are kept behind the queue: 8 + 1 bytes per problem)
__host__ __device__ constexpr size_t fast_lds_bytes(int N, int R, int NTHMAX, bool stage = false) {
    return sizeof(double) * (size_t)(((N * N + N * (N + 1) / 2 + 2 * N + 1) & ~1) + fast_scr_doubles(N, NTHMAX) +
                                     (size_t)kFastPay * (N + (stage ? 0 : 1))) +
           sizeof(int32_t) * ((size_t)R * 64 + 4) + (stage ? (size_t)R * 64 * (sizeof(double) + 1) : 0);
}
// ... plus the streaming wavefronts' LDS-DMA rings behind it (dk slots of one tile per streaming wavefront)
__host__ __device__ constexpr size_t fast_lds_bytes_dma(int N, int R, int NTHMAX, int NT, int nstr, int dk, bool stage = false) {
    return fast_lds_bytes(N, R, NTHMAX, stage) + (size_t)dk * nstr * fast_tile_bytes(NT);
}
// LDS of one CU (gfx950) and the headline shapes' budget with the staged write-out: four workgroups per CU at the
// in-flight shape (28 tiles, four streaming wavefronts, registers), three at the stand-alone one (21 tiles, rings of two)
constexpr size_t kFastCuLds = 160 * 1024;
static_assert(4 * fast_lds_bytes(5, 28, 8, true) <= kFastCuLds, "in-flight shape: four staged workgroups per CU");
static_assert(3 * fast_lds_bytes_dma(5, 21, 8, 7, 3, 2, true) <= kFastCuLds, "stand-alone shape: three staged workgroups per CU");

// The generic loop of lane_kernel (lane_loop) for a lane the straight-line tiers did not finish -- about one problem
// in 10^6 of an iterating batch -- as a function of its own.  Inlined, its working set (LaneState<N, N>: ~60 registers
// for N = 5) set the register budget of the whole kernel and its b[j][lane] columns took 4 N 64 doubles of every
// workgroup's LDS; out of line the kernel is budgeted for the stream, the screen and the tiers, and the call's
// registers are saved around it on the (rare) lanes that take it.  b goes to lane_loop through this frame's private
// copy (stride 1); the constants are the workgroup's LDS copies, as in lane_kernel.  Same loop, same values: the
// results do not change by a bit.
template <int N> struct FastShifts { double b[N]; };
template <int N> struct FastFallback { double u[N]; unsigned long long act, low; int flag, iter; };
// (the pack fields lane_loop reads, by value: a reference to the kernel's PackLayout argument would make the kernel
// copy all of it to its stack at entry)
struct FastLoopArgs {
    unsigned long long imm_mask, eq_mask;
    double primal_tol, dual_tol, zero_tol, progress_tol, fval_bound;
    int n, m, words, oM, odu, odl, cycle_tol, iter_limit;
};
__device__ __forceinline__ FastLoopArgs fast_loop_args(const PackLayout &P) {
    return FastLoopArgs{P.imm_mask, P.eq_mask, P.primal_tol, P.dual_tol, P.zero_tol, P.progress_tol, P.fval_bound,
                        P.n, P.m, P.words, P.oM, P.odu, P.odl, P.cycle_tol, P.iter_limit};
}
template <int N>
__device__ __attribute__((noinline)) FastFallback<N> fast_fallback(const FastLoopArgs A, const double *__restrict__ C,
                                                                    const FastShifts<N> sh, const long long pid) {
    PackLayout P{};
    P.imm_mask = A.imm_mask; P.eq_mask = A.eq_mask;
    P.primal_tol = A.primal_tol; P.dual_tol = A.dual_tol; P.zero_tol = A.zero_tol; P.progress_tol = A.progress_tol;
    P.fval_bound = A.fval_bound;
    P.n = A.n; P.m = A.m; P.words = A.words; P.oM = A.oM; P.odu = A.odu; P.odl = A.odl;
    P.cycle_tol = A.cycle_tol; P.iter_limit = A.iter_limit;
    extern __shared__ __align__(16) double lds[];             // (fast_body's layout: M, G, du0, dl0 first)
    const double *sM = lds, *sG = sM + N * N, *sdu = sG + N * (N + 1) / 2, *sdl = sdu + N;
    double sB[N];
#pragma unroll
    for (int j = 0; j < N; j++) sB[j] = sh.b[j];
    LaneState<N, N> s;
    s.init();
    lane_loop<N, N, N, false>(P, C, sM, sG, sdu, sdl, sB, 1, 0, pid, nullptr, s);
    FastFallback<N> r;
#pragma unroll
    for (int c = 0; c < N; c++) r.u[c] = s.u[c];
    r.act = s.act; r.low = s.low; r.flag = s.flag; r.iter = s.iter;
    return r;
}

// GATHER: the generated controller's call (lmpc_compute_control*): theta is assembled from the five argument arrays
// of mpc_compute_control (codegen/mpc_update_parameter.c) instead of read from a buffer, X is the caller's `control`
// array -- read (previous control, first n_control_prev entries) and overwritten (u*).  A problem's control entries
// are read by the wavefront that streams it and, if it needs iterations, once more by the lane that solves it; they
// are written once, by whichever of the two finishes the problem -- after its own reads, so the in/out array needs
// no copy.
// (the kernel's body: shared by the one-batch launch and the several-batches launch below)
template <int NTHMAX, int NT, int N, bool GATHER = false, bool STAGE = false>
__device__ __forceinline__ void fast_body(
    const PackLayout &P, const double *__restrict__ C, const double *__restrict__ theta,
    double *__restrict__ X, int32_t *__restrict__ exitflag, int32_t *__restrict__ iters,
    uint64_t *__restrict__ active, long long nprob, int R, int nstr, int32_t *__restrict__ errflag, int spinLimit,
    int dk, int Rs, int Dcap, int32_t *__restrict__ tctr, int32_t *__restrict__ tctr_next) {
    constexpr int KMAX = LMPC_FAST_KMAX < N ? LMPC_FAST_KMAX : N;
    constexpr int nconst = N * N + N * (N + 1) / 2 + 2 * N;
    extern __shared__ __align__(16) double lds[];
    double *sconst = lds;                                      // M, G, du0, dl0 (as in the pack, as lane_kernel keeps them)
    double *sScr = sconst + ((nconst + 1) & ~1);               // screening constants (see fast_scr_doubles)
    // STAGED WRITE-OUT (STAGE: the body of fast_staged_kernel / fast_staged_kernel_multi, kernels of their own so that
    // fast_kernel and fast_kernel_multi are compiled exactly as without it -- as a runtime argument of those the flag cost
    // every caller scalar registers through the solving pass and a call issued alone 1 us; the host launches the staged
    // kernels for one output, no iters / active, no gather, a static split): x and the flag of every problem of the workgroup's tiles live in LDS (sX, sF: slot = problem - first
    // problem of the workgroup) until the workgroup's end, and are stored ONCE, as whole consecutive lines, by all 256
    // threads.  Unstaged, a line of X is written in part by the streaming wavefront (its finished lanes) and again in
    // part, a workgroup's life later, by the solving lanes: two partial writes of a line that has left the L2 in between.
    constexpr bool stage = STAGE;
    constexpr int payw = stage ? N : N + 1;                        // (staged: the x shift is handed over in sX)
    double *sPay = sScr + fast_scr_doubles(N, NTHMAX);         // (b_0 .. b_{N-1}, x shift) of the first kFastPay queue positions
    // (the flags at a compile-time offset and x right behind ctrl: no address of its own to keep in a scalar register)
    signed char *sF = reinterpret_cast<signed char *>(sPay + (size_t)kFastPay * payw);  // staged: exit flags of the R tiles' problems
    int32_t *ring = reinterpret_cast<int32_t *>(sF + (stage ? R * 64 : 0));
    int *ctrl = reinterpret_cast<int *>(ring + R * 64);        // [0] write index, [1] read index, [2] producers done
    double *sX = reinterpret_cast<double *>(ctrl + 4);         // staged: x (a queued problem's x shift until it is solved)
    char *dma0 = reinterpret_cast<char *>(sX + (stage ? R * 64 : 0));                  // the LDS-DMA rings, if any
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef LMPC_FAST_TRACE
    const long long trc_entry = (long long)wall_clock64();     // (before the first constant is asked for)
#endif
    // Set-up.  The staged kernels take the constants in ONE round trip: they lie in the pack once more as a contiguous
    // image in LDS order (fast_image_fill); every thread below `pieces` asks for its 16 bytes, the queue is initialised
    // while they travel, then they are stored -- the longer of the two, not their sum (1.8 -> 0.8 us of a workgroup's
    // 17 us at the in-flight shape, 13.0 -> 12.6 us per step; profiles/fast_setup.md).  The other kernels copy section
    // by section as before: with the image a call issued alone took 25.8 instead of 22.7 us on fast_kernel (measured, not
    // explained -- the sections the solving pass reads with scalar loads are then no longer touched first), and the
    // generated controller's kernel compiled to more scalar spills and scratch reloads in its tile loop.  Same words in the
    // same LDS places either way.
    constexpr bool image = STAGE;
    constexpr int pieces = fast_image_pieces(N, NTHMAX);
    static_assert(fast_image_doubles(N, NTHMAX) % 2 == 0, "the image is a whole number of 16-byte pieces");
    static_assert(fast_const_doubles(N) == ((nconst + 1) & ~1), "image and LDS layout agree");
    static_assert(pieces <= 256, "one piece per thread");
    typedef double img2d __attribute__((ext_vector_type(2)));
    img2d piece = {0.0, 0.0};
    if constexpr (image) {
        if (tid < pieces) piece = reinterpret_cast<const img2d *>(C + fast_image_offset(P.oFG))[tid];
    } else {
        for (int i = tid; i < nconst; i += 256) sconst[i] = C[P.oM + i];
        for (int i = tid; i < N * NTHMAX; i += 256) sScr[i] = C[P.oDthP + i];
        if (tid < 2 * N) sScr[N * NTHMAX + tid] = C[P.oBnd + tid];
        if (tid < NTHMAX) sScr[N * NTHMAX + 2 * N + tid] = C[P.oXthP + tid];
        if (tid == 0) sScr[N * NTHMAX + 2 * N + NTHMAX] = C[P.ox0];
    }
    for (int i = tid; i < R * 64; i += 256) ring[i] = -1;
    if (tid < 4) ctrl[tid] = 0;
    if (image && tid < pieces) reinterpret_cast<img2d *>(lds)[tid] = piece;
    __syncthreads();
    const double *sM = sconst, *sG = sM + N * N, *sdu = sG + N * (N + 1) / 2, *sdl = sdu + N;
    const double ntol = -P.primal_tol;
    const long long ntiles = (nprob + 63) / 64;
#ifdef LMPC_FAST_TRACE      // diagnostic build: 100 MHz timestamps per wavefront, kFastTraceSlots words each, behind errflag[16]
    long long *trc = reinterpret_cast<long long *>(errflag + 16) + ((long long)blockIdx.x * 4 + wv) * kFastTraceSlots;
    int npass = 0;
    if (lane == 0) trc[8] = trc_entry;                         // kernel entry: stamp 0 - this = the set-up
#define LMPC_TRC(i) do { if (lane == 0) trc[i] = (long long)wall_clock64(); } while (0)
#else
#define LMPC_TRC(i) do { } while (0)
#endif
    LMPC_TRC(0);
    // Static share + dynamic tail (round 3, tctr != nullptr).  Streams end 12 - 16 us after the launch depending on
    // the XCD a workgroup landed on (tools/fast_trace_cu.py: per-XCD means 11.7 ... 16.4 us in one call, different
    // XCDs slow from batch to batch), and the kernel ends one solving pass after the LAST of them.  A workgroup
    // therefore owns only Rs of its R tiles; the batch's remaining tiles [nstat, ntiles) are handed out one at a time
    // through kFastCtrs global counters (tile = nstat + ticket * kFastCtrs + counter; 128 bytes apart, ~190 tickets
    // each) to the streaming wavefronts that finish their share early.  Tickets are drawn while the previous tile is
    // processed; a workgroup takes at most Dcap of them (its LDS queue has room for Rs + Dcap tiles).  The counter
    // set of the NEXT launch on this handle is cleared here (two sets alternate: no memset in front of the kernel).
    const bool dyn = tctr != nullptr;
    const long long nstat = dyn ? ((long long)gridDim.x * Rs < ntiles ? (long long)gridDim.x * Rs : ntiles) : ntiles;
    if (dyn && blockIdx.x == 0 && tid < kFastCtrs) tctr_next[tid * 32] = 0;
    const long long t0 = (long long)blockIdx.x * (dyn ? Rs : R);
    const long long t1 = t0 + (dyn ? Rs : R) < nstat ? t0 + (dyn ? Rs : R) : nstat;
    const long long base0 = dyn ? 0 : t0 * 64;               // queue entries are problem indices relative to this

    auto load_record = [&](long long pid, double *dst) {
        const long long pc = pid < nprob ? pid : nprob - 1;
        if constexpr (GATHER) {
            const GatherArgs &Ga = P.gat;      // theta = [state; reference; disturbance; control[0:nup]; parameter]; NULL = zeros
            const int o1 = Ga.nx, o2 = o1 + Ga.nr, o3 = o2 + Ga.nd, o4 = o3 + Ga.nup;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                double v = 0.0;
                if (t < o1) v = Ga.state[pc * Ga.nx + t];
                else if (t < o2) { if (Ga.reference) v = Ga.reference[pc * Ga.nr + (t - o1)]; }
                else if (t < o3) { if (Ga.disturbance) v = Ga.disturbance[pc * Ga.nd + (t - o2)]; }
                else if (t < o4) { if (Ga.control) v = Ga.control[pc * Ga.ncontrol + (t - o3)]; }
                else { if (Ga.parameter) v = Ga.parameter[pc * Ga.np + (t - o4)]; }
                dst[t] = v;
            }
        } else {
            const double *src = theta + pc * NT;               // NT == nth: the host dispatches on the handle's nth
#pragma unroll
            for (int t = 0; t < NT; t++) dst[t] = src[t];
        }
    };
    auto write_x = [&](long long pid, const double (&th)[NT], const double (&u)[N], bool with_u) {
        const double *xk = C + P.oXthP;
        for (int k = 0; k < P.nout; k++, xk += NTHMAX) {
            double sh = C[P.ox0 + k];
#pragma unroll
            for (int t = 0; t < NT; t++) sh = __builtin_fma(xk[t], th[t], sh);
            double xs = 0.0;
            if (with_u) {
#pragma unroll
                for (int c = 0; c < N; c++) xs = __builtin_fma(C[P.oRout + k * N + c], u[c], xs);
            }
            X[pid * P.nout + k] = xs + sh;
        }
    };

    // Roles rotate with the workgroup index: a workgroup's wavefronts sit on the four SIMDs of its CU in order,
    // and with a fixed role all dedicated solving wavefronts of a CU -- the VALU-heavy ones -- would share ONE
    // SIMD while the other three only stream.
    const int role = (wv + (int)(blockIdx.x & 3)) & 3;
    // ------------------------------------------------------------------ producer: stream this wavefront's tiles
    if (role < nstr) {
        // A streaming wavefront has ONE tile in flight and one register set for it (kFastAhead = 1): it asks for a tile,
        // waits, screens it, publishes it and asks for the next -- the staged kernels' register path asks for the next
        // BEFORE it publishes, into the registers the screen has just read for the last time (see that loop).  Measured on
        // the headline batch with no point needing iterations (tools/stream_floor.py; one call, cold HBM, event-timed):
        // this form 20.3 us; the next tile requested before the current one is screened (two register sets used
        // alternately; removed) 21.2 us; two / four / seven tiles requested back to back before the first is
        // consumed (straight-line code, so that the compiler's waits are vmcnt(4 (T - 1 - d)) instead of the vmcnt(0)
        // it puts at the head of every loop with stores behind it: loads and stores share one in-order counter)
        // 22.6 / 22.6 / 26.3 us; each wavefront on a contiguous run of tiles (removed) the same.  More
        // requests in flight per wavefront make THIS access shape slower, not faster: a record is 56 bytes per lane,
        // the four load instructions of a tile touch the same 28 lines one after the other and rely on the 32 KB L1
        // to merge them -- nine streaming wavefronts with one tile each are 31.5 KB.  (Read in address order through a
        // wave-private LDS image instead -- no reuse of lines across instructions -- a call took 31.3 us: the round
        // trip through LDS costs more than it saves.  tools/stream_floor.hip has the shapes in isolation: one tile
        // per wavefront at full occupancy reads the same bytes in 15.7 us, event overhead of 6.3 us included.)
        double buf[kFastAhead][NT];
        // A tile in two halves: screen() is every use of the record -- the fma chains, the adds and the compares --,
        // publish() everything that makes the result visible (flags, queue, stores).  Back to back they are one tile's
        // work (process, below); the staged register path asks for its next record between the two.
        // (held: the record was asked for an iteration ago -- the staged register path -- and the compiler sees no load
        // to hide: the Dth rows are then read from LDS FIRST and the record's arrival pinned behind them, so that those
        // reads travel under the record's latency as they do where the request stands in front of them in the same block)
        auto screen = [&](auto held, double (&th)[NT], const bool valid, double (&bq)[N], double &shift) -> bool {
            constexpr bool HELD = decltype(held)::value;
            // screening test of screen_kernel: any row of dl + b <= 0 <= du + b violated by more than primal_tol?
            // (the constants come from LDS, uniform addresses, for every tile anew: as scalar loads the compiler
            // kept all ~110 scalar registers' worth of them live, more than there are, parked the kernel's pointers
            // in vector-register lanes instead and paid 60-100 v_readlane per tile -- a third of the pass's vector
            // instructions (436 -> 330 instructions per tile); the empty asm hides that the addresses repeat.
            // Bitwise | instead of ||: no branch per comparison.)
            typedef const double __attribute__((address_space(3))) *lds_cdp;
            unsigned scr_off = (unsigned)(size_t)(lds_cdp)sScr;
            asm volatile("" : "+v"(scr_off));                 // (opaque, in a vector register: ONE base address, immediate offsets)
            const lds_cdp scr = (lds_cdp)(size_t)scr_off;
            bool hard = false;
            // (16-byte reads: ds_read_b128 moves a broadcast pair in half the LDS cycles of the ds_read2_b64 the
            // compiler picks for 8-byte-aligned doubles; one LDS pipe serves the four SIMDs of a CU)
            typedef double v2d __attribute__((ext_vector_type(2)));
            typedef const v2d __attribute__((address_space(3))) *lds_c2p;
            const lds_c2p c2 = (lds_c2p)(size_t)scr_off;
            static_assert(NTHMAX % 2 == 0, "rows of pairs");
            // (all N rows up to NT = 8 -- at most 20 reads, 80 registers; beyond, where the record itself is 18 - 32
            // registers, the first row only)
            constexpr int RQ = (NT + 1) / 2, NA = !HELD ? 0 : (NT > 8 ? 1 : (20 / RQ < N ? 20 / RQ : N));
            v2d ahead[NA ? NA : 1][RQ];
            if constexpr (HELD) {
#pragma unroll
                for (int j = 0; j < NA; j++)
#pragma unroll
                    for (int q = 0; q < RQ; q++) ahead[j][q] = c2[j * (NTHMAX / 2) + q];
                fast_pin(th);
            }
#pragma unroll
            for (int j = 0; j < N; j++) {
                double row[NTHMAX];
#pragma unroll
                for (int q = 0; q < (NT + 1) / 2; q++) {
                    v2d v;
                    if (j < NA) v = ahead[j][q];
                    else v = c2[j * (NTHMAX / 2) + q];
                    row[2 * q] = v.x; row[2 * q + 1] = v.y;
                }
                double acc = 0.0;
#pragma unroll
                for (int t = 0; t < NT; t++) acc = __builtin_fma(row[t], th[t], acc);
                bq[j] = acc;
                const v2d bb = c2[N * (NTHMAX / 2) + j];                   // (du, dl) of row j
                const double vu = (bb.x + acc) - 0.0;
                const double vl = -((bb.y + acc) - 0.0);
                hard = hard | (vu < ntol) | (vl < ntol);
            }
            hard = hard & valid;
            // x0 + Xth theta of the first output: stored by a finished lane, handed over by a queued one
            double sh = scr[N * NTHMAX + 2 * N + NTHMAX];
            {
                double row[NTHMAX];
#pragma unroll
                for (int q = 0; q < (NT + 1) / 2; q++) {
                    const v2d v = c2[(N * NTHMAX + 2 * N) / 2 + q];
                    row[2 * q] = v.x; row[2 * q + 1] = v.y;
                }
#pragma unroll
                for (int t = 0; t < NT; t++) sh = __builtin_fma(row[t], th[t], sh);
            }
            shift = sh;
            return hard;
        };
        // (th: the record once more, for the unstaged stores of several outputs only -- the staged kernels never read it
        // here, which is what lets the register path below overwrite it with the next tile's while this runs)
        auto publish = [&](long long tile, const double (&bq)[N], const double sh, const bool hard, const bool valid,
                           const double (&th)[NT]) {
            const long long pid = tile * 64 + lane;
            const unsigned long long mask = __ballot(hard);
            // every problem gets a flag HERE -- BEFORE a queued problem is published in the ring, so that the release below
            // orders this store in front of the solving lane's final one (issued after the publish, the
            // provisional flag could land last and leave a solved problem at -8) --, queued ones the provisional
            // EXIT_UNFINISHED that the solving lane overwrites: should a bounded wait below ever run out, no caller reads a stale flag as success (the
            // reference asserts exitflag >= 1, utils.jl:46); an unmasked store of whole lines, as screen_kernel's.
            // Staged: both go to the problem's LDS slot instead -- a hard lane's slot holds its x SHIFT until the solving
            // lane replaces it with x -- and nothing is stored to memory here.  The release / acquire argument around
            // the provisional flag does not apply on that path: a slot is written by this lane, then (behind the ring's
            // release / acquire) by the solving lane, and read after the workgroup's closing barrier.
            if (stage) {
                if (valid) {
                    const int slot = (int)(tile - t0) * 64 + lane;
                    sX[slot] = hard ? sh : 0.0 + sh;
                    sF[slot] = (signed char)(hard ? EXIT_UNFINISHED : EXIT_OPTIMAL);
                }
            } else {
#ifdef LMPC_FAST_NT_STORES
            if (valid) __builtin_nontemporal_store(hard ? EXIT_UNFINISHED : EXIT_OPTIMAL, &exitflag[pid]);
#else
            if (valid) exitflag[pid] = hard ? EXIT_UNFINISHED : EXIT_OPTIMAL;
#endif
            }
            if (mask != 0ull) {
                int base = 0;
                if (lane == 0) base = __hip_atomic_fetch_add(&ctrl[0], __popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // (staged: the branch is wave-uniform, lane 0 is active and holds the value -- no trip through the LDS
                // crossbar and its wait to broadcast it)
                if constexpr (stage) base = __builtin_amdgcn_readfirstlane(base);
                else base = __shfl(base, 0);
                if (hard) {
                    const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
                    if (pos < kFastPay) {
                        double *pay = sPay + pos * payw;
#pragma unroll
                        for (int j = 0; j < N; j++) pay[j] = bq[j];
                        if (!stage) pay[N] = sh;
                    }
                    // (release: the payload is in LDS before the index that announces it.  Staged, everything the index
                    // announces -- payload, x shift, provisional flag -- is in LDS and nothing is in memory, and one
                    // wavefront's LDS operations complete in the order they were issued (the add on ctrl[2] below relies
                    // on the same): an LDS wait and a relaxed store order them.  A release store would wait on every
                    // counter, the next tile's records in flight included -- see the staged register path below.)
                    if constexpr (stage) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __hip_atomic_store(&ring[pos], (int32_t)(pid - base0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        __hip_atomic_store(&ring[pos], (int32_t)(pid - base0), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
            if (!stage && valid && !hard) {
                if (P.nout == 1) {
#ifdef LMPC_FAST_NT_STORES
                    __builtin_nontemporal_store(0.0 + sh, &X[pid]);
#else
                    X[pid] = 0.0 + sh;                         // x = x0 + Xth theta (screen_kernel's `0.0 + sh`)
#endif
                } else {
                    double u0[N];
#pragma unroll
                    for (int c = 0; c < N; c++) u0[c] = 0.0;
                    write_x(pid, th, u0, false);
                }
                if (iters) iters[pid] = 1;
                if (active) active[pid * P.words] = 0ull;
            }
        };
        auto process = [&](long long tile, double (&th)[NT], bool live) {
            const bool valid = live && tile * 64 + lane < nprob;
            double bq[N], sh;
            const bool hard = screen(std::false_type{}, th, valid, bq, sh);
            publish(tile, bq, sh, hard, valid, th);
        };
        if (!GATHER && dk >= 2) {
            // Records by LDS-DMA (round 3).  The wavefront owns a ring of dk tile slots in LDS; a tile (64 records,
            // 64 NT 8 bytes, contiguous in theta) is moved by ceil(bytes / 1 KiB) wave-instructions of 16 bytes per
            // lane -- fully coalesced, no vector register involved -- and the lane then reads ITS record from the slot
            // (NT 8-byte LDS reads at a stride of NT doubles).  The pieces of the next dk - 1 tiles are in flight while
            // this one is screened: twice (dk = 2) the bytes in flight of the register path at no register cost, which
            // is what the stream was short of (4.7 TB/s with one 3.5 KB tile per streaming wavefront in flight).
            // Vector-memory operations complete in order, so "all but the youngest (dk - 1) tiles' pieces" = this
            // tile's pieces and every store issued before them: a counted s_waitcnt vmcnt.
            constexpr unsigned TB = (unsigned)fast_tile_bytes(NT);
            constexpr int PIECES = (int)((TB + 1023) / 1024);
            constexpr unsigned LASTB = TB - (PIECES - 1) * 1024u;            // bytes of the last piece (16 per lane)
            typedef const double __attribute__((address_space(3))) *lds_cdp;
            char *dring = dma0 + (size_t)role * dk * TB;
            const unsigned dbase = (unsigned)(size_t)(lds_cdp) reinterpret_cast<double *>(dring);
            const char *tbytes = reinterpret_cast<const char *>(theta);
            // whole tiles only: the batch's last, partial tile (one per call) takes the register path below
            const long long tfull = nprob / 64;
            const long long te = t1 < tfull ? t1 : tfull;
            auto issue = [&](long long tile, int slot) {
                const char *src = tbytes + tile * (long long)TB + lane * 16;
#pragma unroll
                for (int p = 0; p < PIECES; p++) {
                    const unsigned dst = __builtin_amdgcn_readfirstlane(dbase + (unsigned)slot * TB + (unsigned)p * 1024u);
                    if (p + 1 < PIECES || LASTB == 1024u || lane * 16 < (int)LASTB) fast_dma16(src + p * 1024, dst);
                }
            };
            // ticket of the dynamic tail (see `dyn` above; the lambda is shared with the register path's loop below)
            int cc = (int)((blockIdx.x * (unsigned)nstr + (unsigned)role) & (kFastCtrs - 1));
            auto take = [&]() -> long long {
                int t = -1;
                if (lane == 0) {
                    if (__hip_atomic_fetch_add(&ctrl[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < Dcap)
                        t = atomicAdd(&tctr[cc * 32], 1);
                }
                t = __builtin_amdgcn_readfirstlane(t);
                const long long tile = nstat + (long long)t * kFastCtrs + cc;
                return (t >= 0 && tile < ntiles) ? tile : -1;
            };
            if (dk == 2) {
                // Two-slot pipeline over "this wavefront's static tiles, then tickets": while tile `cur` is screened the
                // pieces of `nxt` are in flight and -- in the dynamic tail -- the ticket for the tile after it is being
                // drawn (one returning atomic: a vector-memory operation like the pieces, counted with them below).
                // Whole tiles only (the ticket range ends at tfull): the batch's partial tile is handled behind the loop.
                long long sidx = t0 + role, tk = -1;
                bool drew = false;                                           // a ticket's atomic was issued in this iteration
                auto take_full = [&]() -> long long { const long long t = take(); return t < tfull ? t : -1; };
                if (dyn && sidx >= te) tk = take_full();
                auto peek = [&]() -> long long { return sidx < te ? sidx : (dyn ? tk : -1); };
                auto advance = [&]() {                                       // hand the peeked tile out; prefetch behind it
                    drew = false;
                    if (sidx < te) { sidx += nstr; if (dyn && sidx >= te) { tk = take_full(); drew = true; } }
                    else if (dyn && tk >= 0) { tk = take_full(); drew = true; }
                };
                long long cur = peek();
                int sc = 0;
                if (cur >= 0) { issue(cur, 0); advance(); }
                // (the prologue's atomic, if any, is older than everything the loop counts: harmless)
                while (cur >= 0) {
                    const long long nxt = peek();
                    const bool nd = nxt >= 0;
                    if (nd) { issue(nxt, sc ^ 1); advance(); } else drew = false;
                    // all but the youngest operations: the pieces of `nxt` (if requested) and this iteration's ticket
                    if (nd && drew) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PIECES + 1) : "memory");
                    else if (nd) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PIECES) : "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    const double *rec = reinterpret_cast<const double *>(dring + (size_t)sc * TB) + lane * NT;
#pragma unroll
                    for (int t = 0; t < NT; t++) buf[0][t] = rec[t];
                    process(cur, buf[0], true);
                    cur = nxt;
                    sc ^= 1;
                }
                // the batch's last, partial tile: its static owner, or (dynamic tail) the first workgroup's first streamer
                const long long part = dyn ? ((blockIdx.x == 0 && role == 0 && tfull < ntiles) ? tfull : -1)
                                           : ((sidx < t1 && sidx == tfull) ? tfull : -1);
                if (part >= 0) {
                    load_record(part * 64 + lane, buf[0]);
                    process(part, buf[0], true);
                }
            } else {
            const long long first = t0 + role;
            long long ahead = first;                                         // next tile to request
            int sa = 0;                                                      // ... and its slot
            for (int d = 0; d < dk - 1 && ahead < te; d++, ahead += nstr) { issue(ahead, sa); sa = sa + 1 == dk ? 0 : sa + 1; }
            int sc = 0;
            long long tile = first;
            for (; tile < te; tile += nstr) {
                if (ahead < te) { issue(ahead, sa); sa = sa + 1 == dk ? 0 : sa + 1; ahead += nstr; }
                // pieces still allowed in flight: those of the tiles requested after this one
                const long long younger = (ahead - tile) / nstr - 1;
                if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * PIECES) : "memory");
                else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PIECES) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const double *rec = reinterpret_cast<const double *>(dring + (size_t)sc * TB) + lane * NT;
#pragma unroll
                for (int t = 0; t < NT; t++) buf[0][t] = rec[t];
                sc = sc + 1 == dk ? 0 : sc + 1;
                process(tile, buf[0], true);
            }
            if (tile < t1) {                                                 // (tile == tfull: the partial one)
                load_record(tile * 64 + lane, buf[0]);
                process(tile, buf[0], true);
            }
            if (dyn) {                                                       // deeper rings: the tail one tile at a time
                long long tl = take();
                while (tl >= 0) {
                    load_record(tl * 64 + lane, buf[0]);
                    const long long nx = take();
                    process(tl, buf[0], true);
                    tl = nx;
                }
            }
            }
        } else if constexpr (STAGE && LMPC_FAST_TURN) {
            // Staged kernels, records through registers (the in-flight shape: four streaming wavefronts, no rings).  Still
            // ONE tile and one register set per wavefront, but the next tile is asked for as soon as screen() has read
            // the record for the last time -- its registers are dead from there on -- and BEFORE this tile is published:
            // the ballot, the reservation (an LDS atomic and its wait), the payload, the ring store and the loop's own
            // bookkeeping then run under the next record's latency instead of in front of it.  What keeps publish()
            // from waiting for that record: its ring store is relaxed behind an LDS wait (see there; a release would
            // wait on vmcnt as well), and nothing else in it touches a vector-memory counter -- the staged kernels store
            // to LDS only.  The record's address is a running 64-bit value per lane, clamped to the batch's last
            // record exactly as load_record clamps (a partial last tile reads that record on its idle lanes and never
            // beyond the batch); the kernel argument theta is not read again per tile.  A request is made only if the
            // wavefront has a further tile.  Three batches in flight: 12.84 -> 12.53 us per step, a call issued alone
            // (not this kernel) unchanged (profiles/fast_turnaround.md).  The early request is the gain: this loop with the
            // request behind publish() (-DLMPC_FAST_TURN_EARLY=0) measured 12.79, the loop below with the relaxed publish
            // and no broadcast through LDS (-DLMPC_FAST_TURN=0) 12.80.  Raised priority from the loop's head to the request
            // (-DLMPC_FAST_TURN_PRIO=1) stayed inside the spread over five alternated runs and is not compiled in.
            const long long first = t0 + role;
            if (first < t1) {
                const uintptr_t last = reinterpret_cast<uintptr_t>(theta + (nprob - 1) * NT);
                const uintptr_t step = (uintptr_t)nstr * (64 * NT * sizeof(double));
                uintptr_t at = reinterpret_cast<uintptr_t>(theta + (first * 64 + lane) * NT);
                typedef const double __attribute__((address_space(1))) *glb_cdp;     // (an integer cast back: say it is memory)
                auto request = [&]() {
                    const glb_cdp src = (glb_cdp)(at < last ? at : last);
#pragma unroll
                    for (int t = 0; t < NT; t++) buf[0][t] = src[t];
                };
                request();
                for (long long tile = first;; tile += nstr) {
                    const bool more = tile + nstr < t1;
#ifdef LMPC_FAST_TURN_PRIO
                    __builtin_amdgcn_s_setprio(LMPC_FAST_TURN_PRIO);
#endif
                    double bq[N], sh;
                    const bool valid = tile * 64 + lane < nprob;
                    const bool hard = screen(std::true_type{}, buf[0], valid, bq, sh);
                    // (every use of the record feeds bq or sh: behind this point its registers are free.  Opaque and a
                    // memory barrier, or the compiler asks for the next record FIRST, into registers of its own, and
                    // spills the screen's constants to make room -- 44 instead of 12 spilled registers, seen)
                    fast_pin(bq);
                    fast_pin(sh);
                    at += step;
                    if (LMPC_FAST_TURN_EARLY && more) request();
#ifdef LMPC_FAST_TURN_PRIO
                    __builtin_amdgcn_s_setprio(0);
#endif
                    publish(tile, bq, sh, hard, valid, buf[0]);
                    if (!more) break;
                    if (!LMPC_FAST_TURN_EARLY) request();
                }
            }
        } else
        for (long long base = t0 + role; base < t1; base += (long long)kFastAhead * nstr) {
#pragma unroll
            for (int d = 0; d < kFastAhead; d++) {
                const long long tl = base + (long long)d * nstr;
                load_record((tl < t1 ? tl : base) * 64 + lane, buf[d]);
            }
#pragma unroll
            for (int d = 0; d < kFastAhead; d++) {
                const long long tl = base + (long long)d * nstr;
                process(tl < t1 ? tl : base, buf[d], tl < t1);
            }
        }
        if (dyn && !(!GATHER && dk >= 2)) {
            // dynamic tail (register path): one tile per ticket, the next ticket in flight while this tile is screened
            int cc = (int)((blockIdx.x * (unsigned)nstr + (unsigned)role) & (kFastCtrs - 1));
            auto take = [&]() -> long long {
                int t = -1;
                if (lane == 0) {
                    if (__hip_atomic_fetch_add(&ctrl[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < Dcap)
                        t = atomicAdd(&tctr[cc * 32], 1);
                }
                t = __builtin_amdgcn_readfirstlane(t);
                const long long tile = nstat + (long long)t * kFastCtrs + cc;
                return (t >= 0 && tile < ntiles) ? tile : -1;
            };
            long long tile = take();
            while (tile >= 0) {
                load_record(tile * 64 + lane, buf[0]);
                const long long nxt = take();
                process(tile, buf[0], true);
                tile = nxt;
            }
        }
        // all of this wavefront's reservations are in the LDS queue ahead of this add (LDS keeps a wave's order)
        if (lane == 0) __hip_atomic_fetch_add(&ctrl[2], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        LMPC_TRC(1);
    }

    // ------------------------------------------------------------------ consumer: claim and solve queued problems
    int spins = 0;
    for (;;) {
        int start = 0, n = 0;
        if (lane == 0) {
            for (;;) {
                // read BEFORE the write index (acquire keeps the order): d == nstr => the write index is final
                const int d = __hip_atomic_load(&ctrl[2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                const int w = lds_load(&ctrl[0]);
                int r = lds_load(&ctrl[1]);
                const int avail = w - r;
                if (avail >= 64 || (d >= nstr && avail > 0)) {
                    const int take = avail < 64 ? avail : 64;
                    if (__hip_atomic_compare_exchange_strong(&ctrl[1], &r, r + take, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_WORKGROUP)) { start = r; n = take; break; }
                } else if (d >= nstr) {
                    n = -1;                                    // nothing left and nothing to come
                    break;
                } else {
                    __builtin_amdgcn_s_sleep(8);
                }
                if (++spins > spinLimit) { n = -2; break; }
            }
        }
        start = __builtin_amdgcn_readfirstlane(start);
        n = __builtin_amdgcn_readfirstlane(n);
        // (system scope: the word lives in host memory, the host looks at it without a copy -- lmpc_check)
        if (n == -2 && lane == 0 && errflag) __hip_atomic_store(errflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (n < 0) break;
#ifdef LMPC_FAST_TRACE
        if (npass < 2) LMPC_TRC(2 + npass);
        npass++;
#endif
#ifdef LMPC_FAST_PRIO
        __builtin_amdgcn_s_setprio(LMPC_FAST_PRIO);           // a solving pass is a latency chain: ahead of the streamers
#endif
        const bool mine = lane < n;
        int rel = -1;
        if (mine) {
            int sp = 0;
            while ((rel = __hip_atomic_load(&ring[start + lane], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < 0) {
                if (++sp > spinLimit) break;                   // (a reserved slot is written at once: never in practice)
            }
        }
        if (__any(mine && rel < 0)) {
            if (lane == 0 && errflag) __hip_atomic_store(errflag, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        const long long pid = mine ? base0 + rel : base0;
        double b[N], u[N];
        double sh0 = C[P.ox0];                                 // x0 + Xth theta of the first output (kept: 2 registers)
        const bool handed = start + lane < kFastPay;           // shifts handed over in LDS by the streaming wavefront
#pragma unroll
        for (int j = 0; j < N; j++) b[j] = 0.0;
        if (handed) {
            const double *pay = sPay + (start + (mine ? lane : 0)) * payw;
#pragma unroll
            for (int j = 0; j < N; j++) b[j] = pay[j];
            if (!stage) sh0 = pay[N];
        }
        // (staged: the x shift of EVERY queued problem waits in its sX slot and is read where x is formed, below)
        if (__any(mine && !handed)) {
            double th0[NT];
            load_record(pid, th0);
            // (scalar loads here: the LDS copy the streaming pass uses made a call 1.7 us SLOWER on this side --
            // a solving pass already lives on LDS reads, 26.8 vs 28.5 us same-box)
            const double *dj = C + P.oDthP;
            double sh1 = C[P.ox0];
#pragma unroll
            for (int j = 0; j < N; j++) {
                double acc = 0.0;
#pragma unroll
                for (int t = 0; t < NT; t++) acc = __builtin_fma(dj[j * NTHMAX + t], th0[t], acc);
                b[j] = handed ? b[j] : acc;
            }
            if constexpr (!stage) {                            // (staged: the shift is in the slot, nothing to re-form)
                const double *xk = C + P.oXthP;
#pragma unroll
                for (int t = 0; t < NT; t++) sh1 = __builtin_fma(xk[t], th0[t], sh1);
                sh0 = handed ? sh0 : sh1;
            }
        }
#ifdef LMPC_FAST_TRACE
        if (npass == 1) { if (lane == 0) trc[4] = (long long)(b[0] != 12345.678 ? wall_clock64() : 0); }
#endif
        int iter = 1, nact = 0, wrow[KMAX], flag = EXIT_ITERLIMIT;
        bool wlow[KMAX];
        unsigned long long act = 0ull, low = 0ull;
        const int res = fast_tiers<N, KMAX>(P, sM, sG, sdu, sdl, mine, b, u, iter, wrow, wlow, nact);
        bool solved = res == EXIT_OPTIMAL;
#ifdef LMPC_FAST_TRACE
        if (npass == 1) { if (lane == 0) trc[5] = (long long)(res != 77 ? wall_clock64() : 0); }
#endif
        if (solved) {
            flag = EXIT_OPTIMAL;
#pragma unroll
            for (int i = 0; i < KMAX; i++)
                if (i < nact) { act |= 1ull << wrow[i]; if (wlow[i]) low |= 1ull << wrow[i]; }
        }
#ifndef LMPC_FAST_NO_FALLBACK      // (diagnostic build without it: what the tiers and the stream need on their own)
        if (mine && !solved) {
            // the generic loop of lane_kernel on the lanes the tiers did not finish (from scratch), out of line
            FastShifts<N> bs;
#pragma unroll
            for (int j = 0; j < N; j++) bs.b[j] = b[j];
            const FastFallback<N> r = fast_fallback<N>(fast_loop_args(P), C, bs, pid);
#pragma unroll
            for (int c = 0; c < N; c++) u[c] = r.u[c];
            flag = r.flag; iter = r.iter; act = r.act; low = r.low;
        }
#endif
        if (mine && stage) {
            double xs = 0.0;
#pragma unroll
            for (int c = 0; c < N; c++) xs = __builtin_fma(C[P.oRout + c], u[c], xs);
            const unsigned slot = (unsigned)rel;               // (the static split's queue entries ARE slots)
            sX[slot] = xs + sX[slot];                          // the slot held the x shift the streaming lane left
            sF[slot] = (signed char)flag;                      // (exit flags are -8 ... 2)
        } else if (mine) {
            if (P.nout == 1) {
                double xs = 0.0;
#pragma unroll
                for (int c = 0; c < N; c++) xs = __builtin_fma(C[P.oRout + c], u[c], xs);
                X[pid] = xs + sh0;
            } else {
                double th[NT];                                 // several outputs: the record is read again (an L2 hit)
                load_record(pid, th);
                write_x(pid, th, u, true);
            }
            exitflag[pid] = flag;
            if (iters) iters[pid] = iter;
            if (active) active[pid * P.words] = (act & ~low) | ((act & low) << N);     // m == N <= 6: one word
        }
#ifdef LMPC_FAST_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
    }
    // Staged write-out: every wavefront of the workgroup gets here -- the two bounded-wait exits above leave the loop,
    // they do not return -- and the workgroup's contiguous range of X and of exitflag is stored from LDS, consecutive
    // lanes to consecutive elements (no more alignment asked than of the unstaged stores).  A problem a spent wait
    // left unsolved keeps its provisional EXIT_UNFINISHED (and its x shift as x), as on the unstaged path.
    if (stage) {
        __syncthreads();
        const long long g0 = t0 * 64;
        const int cnt = (int)((t1 * 64 < nprob ? t1 * 64 : nprob) - g0);
        // (nontemporal: written once, read by nobody on the device; 13.94 against 14.11 us per step, three batches in flight)
        for (int i = tid; i < cnt; i += 256) __builtin_nontemporal_store(sX[i], &X[g0 + i]);
        for (int i = tid; i < cnt; i += 256) __builtin_nontemporal_store((int32_t)sF[i], &exitflag[g0 + i]);
    }
    LMPC_TRC(6);
#ifdef LMPC_FAST_TRACE
    // (+ where the wavefront ran: HW_REG_HW_ID (4) and HW_REG_XCC_ID (20), for per-CU / per-XCD statistics)
    if (lane == 0) trc[7] = (long long)npass | ((long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 16) |
                            ((long long)((unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xffu) << 48);
#endif
#undef LMPC_TRC
}

template <int NTHMAX, int NT, int N, bool GATHER = false>
__global__ __launch_bounds__(256, LMPC_FAST_WAVES) void fast_kernel(
    const PackLayout P, const double *__restrict__ C, const double *__restrict__ theta,
    double *__restrict__ X, int32_t *__restrict__ exitflag, int32_t *__restrict__ iters,
    uint64_t *__restrict__ active, long long nprob, int R, int nstr, int32_t *__restrict__ errflag, int spinLimit,
    int dk, int Rs, int Dcap, int32_t *__restrict__ tctr, int32_t *__restrict__ tctr_next) {
    fast_body<NTHMAX, NT, N, GATHER>(P, C, theta, X, exitflag, iters, active, nprob, R, nstr, errflag, spinLimit, dk, Rs, Dcap, tctr,
                                     tctr_next);
}

// The staged write-out's kernel (see STAGE in fast_body): x and exitflag alone, one output, a static split of R tiles.
template <int NTHMAX, int NT, int N>
__global__ __launch_bounds__(256, LMPC_FAST_WAVES) void fast_staged_kernel(
    const PackLayout P, const double *__restrict__ C, const double *__restrict__ theta,
    double *__restrict__ X, int32_t *__restrict__ exitflag, long long nprob, int R, int nstr, int32_t *__restrict__ errflag,
    int spinLimit, int dk) {
    fast_body<NTHMAX, NT, N, false, true>(P, C, theta, X, exitflag, nullptr, nullptr, nprob, R, nstr, errflag, spinLimit, dk, R, 0,
                                          nullptr, nullptr);
}

// SEVERAL batches of the same size in ONE launch (lmpc_solve_batches_device): blockIdx.y picks the batch, its buffers
// come from a table in the kernel arguments.  A launch of the one-batch kernel lives 22 us for a 13 us stream: the
// solving tail, the spread of the streams' ends over the XCDs and the ramp are paid per launch.  Here the workgroups of
// batch b + 1 are dispatched as those of batch b retire, so the tail of one batch runs under the stream of the next
// -- what a caller gets from three streams, inside one launch on one stream.
constexpr int kFastMaxBatches = 8;
struct FastBatches {
    const double *theta[kFastMaxBatches];
    double *x[kFastMaxBatches];
    int32_t *flag[kFastMaxBatches];
};
template <int NTHMAX, int NT, int N>
__global__ __launch_bounds__(256, LMPC_FAST_WAVES) void fast_kernel_multi(
    const PackLayout P, const double *__restrict__ C, const FastBatches B, long long nprob, int R, int nstr,
    int32_t *__restrict__ errflag, int spinLimit, int dk) {
    const int b = blockIdx.y;
    fast_body<NTHMAX, NT, N, false>(P, C, B.theta[b], B.x[b], B.flag[b], nullptr, nullptr, nprob, R, nstr, errflag, spinLimit, dk, R, 0,
                                    nullptr, nullptr);
}
template <int NTHMAX, int NT, int N>
__global__ __launch_bounds__(256, LMPC_FAST_WAVES) void fast_staged_kernel_multi(
    const PackLayout P, const double *__restrict__ C, const FastBatches B, long long nprob, int R, int nstr,
    int32_t *__restrict__ errflag, int spinLimit, int dk) {
    const int b = blockIdx.y;
    fast_body<NTHMAX, NT, N, false, true>(P, C, B.theta[b], B.x[b], B.flag[b], nullptr, nullptr, nprob, R, nstr, errflag, spinLimit, dk,
                                          R, 0, nullptr, nullptr);
}

}  // namespace lmpc
