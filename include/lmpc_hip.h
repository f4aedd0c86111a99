/*
 * lmpc_hip.h -- C ABI of the MI355X (gfx950) batched QP backend for LinearMPC.jl's online path.
 *
 * Drop-in boundary: everything LinearMPC.jl does between "theta is formed" and "x*, exitflag
 * come back from DAQP" (reference /root/reference/src/utils.jl:268-283 `solve`, with the
 * one-time half at /root/reference/src/setup.jl:7-29 `setup!`), for N parameter points at once.
 * The reference-side binding a maintainer would add (Julia `ccall`) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, opaque handle, no exceptions; every entry point returns an int status.
 *  - "QP" arrays arrive exactly as Julia stores mpc.mpQP (COLUMN-major Float64, Cint senses),
 *    so the ccall passes the struct fields without copies or transposes.
 *  - batched arrays are "one problem per contiguous record": theta is nth x N column-major on
 *    the Julia side == N records of nth doubles; x is nout x N == N records of nout doubles.
 *  - exit flags per problem use DAQP's sign convention (reference asserts exitflag >= 1,
 *    utils.jl:46):  1 optimal, 2 soft-optimal, -1 infeasible, -2 cycle, -3 unbounded,
 *    -4 iteration limit, -5 non-convex, -6 over-determined initial working set.  One flag is this
 *    library's own: -7 = the working set outgrew what the kernels hold.  The wavefront kernel keeps 64 rows; a
 *    point that wants more is re-solved behind it by a one-problem-per-thread kernel with room for 256, so -7 is
 *    left only beyond 256 rows, for hybrid problems (branch and bound) with n + 1 + #SOFT > 64, and under
 *    lmpc_set_option("big_path", 0).  Like every flag < 1 it fails the reference's assertion.
 *  - sense bit flags are DAQP's (reference mpc2mpqp.jl:868-885): 1 ACTIVE, 2 LOWER,
 *    4 IMMUTABLE, 5 EQUALITY (=ACTIVE|IMMUTABLE), 8 SOFT, 16 BINARY.  A problem with BINARY rows
 *    (hybrid MPC, mpQP.has_binaries) is solved by branch and bound: every BINARY row ends up
 *    active at one of its two bounds; the flag is 1 with the best assignment found, -1 if none is
 *    feasible, -4 if the node limit (100000) was hit; `iters` is the sum over all nodes.
 *  - active-set masks: lmpc_active_words(h) 64-bit words per problem; bit j (0 <= j < m) set
 *    = constraint j active at its UPPER bound, bit m+j set = active at its LOWER bound.
 *  - a handle is bound to one GPU (the `device` given at setup); calls on one handle must not
 *    overlap in time, different handles are independent (the reference's DAQP workspace is
 *    one-per-MPC and not thread-safe either: types.jl:93-97,141).
 */
#ifndef LMPC_HIP_H
#define LMPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lmpc_handle lmpc_handle;

/* Solver settings == the DAQP settings LinearMPC.jl documents
 * (/root/reference/docs/src/manual/solver.md:49-56) plus the two DAQP-internal tolerances the
 * algorithm needs (zero_tol for singular pivots, fval_bound). rho_soft = 1/soft_weight
 * (setup.jl:26).  Replaces DAQP.settings(model, Dict(...)). */
typedef struct lmpc_settings {
    double primal_tol;   /* 1e-6  */
    double dual_tol;     /* 1e-12 */
    double zero_tol;     /* 1e-11 */
    double progress_tol; /* 1e-6  */
    double fval_bound;   /* 1e30  */
    double rho_soft;     /* 1e-6  */
    int32_t cycle_tol;   /* 10    */
    int32_t iter_limit;  /* 10000 */
    /* ABI version 2: DAQP's proximal-point settings.  (PARITY: UNPINNED -- libdaqp's own prox loop is not available to
     * restate and no reference test holds a vector for it; this is the textbook method the setting is named after,
     * checked against this build's own oracle twin and by KKT certificates of the original problem.)
     * eps_prox > 0 AT SETUP selects the proximal-point mode, the one
     * that accepts a merely positive SEMIdefinite (symmetric) H -- without it such an H is answered with -5, as by
     * DAQP.setup (/root/reference/src/setup.jl:18-19):  x_{k+1} = argmin 1/2 x'Hx + f(theta)'x + eps_prox/2 |x - x_k|^2
     * over the constraint set, x_0 = 0, until |x_{k+1} - x_k|_inf < eta_prox; every subproblem is solved by the
     * library's L D U kernel on the Hessian H + eps_prox I, warm from the previous one's working set; iteration counts
     * add up against iter_limit.  The limit is a KKT point of the ORIGINAL problem (not unique if H is singular).
     * Changing eps_prox on a live handle (lmpc_set_settings) is refused: the factorisation depends on it. */
    double eps_prox;     /* 0     */
    double eta_prox;     /* 1e-6  */
} lmpc_settings;
/* The layout every binding mirrors (integration/LmpcHipExt.jl::LmpcSettings, linearmpc.jl_amd/_cabi.py::Settings): ten
 * fields, 72 bytes, the two 32-bit counters side by side at offset 48.  Checked here at compile time and against the
 * Julia struct's text by tests/test_host.py::test_settings_layout_is_the_same_in_every_binding. */
typedef char lmpc_settings_is_72_bytes[(sizeof(lmpc_settings) == 72) ? 1 : -1];

/* status codes of the API itself (solver outcomes are the per-problem exit flags) */
#define LMPC_OK 1
#define LMPC_ERR_INFEASIBLE (-1)      /* setup: bl > bu somewhere (DAQP.setup flag -1)        */
#define LMPC_ERR_NONCONVEX (-5)       /* setup: H not positive definite (DAQP.setup flag -5)  */
#define LMPC_ERR_OVERDETERMINED (-6)  /* setup: equality rows linearly dependent (flag -6)    */
#define LMPC_ERR_BADARG (-100)
#define LMPC_ERR_NOGPU (-101)         /* no usable HIP device: there is NO CPU fallback       */
#define LMPC_ERR_HIP (-102)           /* a HIP runtime call failed, see lmpc_last_error       */
#define LMPC_ERR_UNSUPPORTED (-103)   /* problem shape outside what the kernels cover         */

/* Fills *s with the defaults listed above. */
void lmpc_default_settings(lmpc_settings *s);

/*
 * One-time setup from the mpQP, replacing DAQP.setup + DAQP.settings (setup.jl:11-13,26) and
 * doing what DAQP.update / qp2ldp precompute (utils.jl:272-281, codegen.jl:239-280):
 * Cholesky H = R'R, LDP rows M = [I_ms;A] R^-1 (normalised), Dth = W + M R^-T f_theta,
 * du/dl, the output maps, and the upload of that constant pack to GPU `device`.
 *
 *   n      decision variables (Nc*nu)            m     two-sided constraints (ms simple first)
 *   ms     leading simple bounds  bl<=U[i]<=bu   nth   length of theta = [x; r; d; uprev; p]
 *   nout   leading entries of U* returned per problem (nu for compute_control, n for
 *          compute_control_trajectory)
 *   H[n*n] f[n] f_theta[n*nth] A[(m-ms)*n] bu[m] bl[m] W[m*nth]   column-major, as in mpc.mpQP
 *   sense[m]  Cint flags        Kfb[nout*nx] or NULL  prestabilising feedback mpc.K
 *          (column-major): output k gets  - Kfb[k,:]*theta[0:nx]  (utils.jl:48-49)
 *   s      settings or NULL for defaults          device  HIP device ordinal
 *
 * Returns LMPC_OK (1) or a negative code; *out is NULL on failure.
 */
int lmpc_setup(lmpc_handle **out, int n, int m, int ms, int nth, int nout,
               const double *H, const double *f, const double *f_theta,
               const double *A, const double *bu, const double *bl, const double *W,
               const int32_t *sense, const double *Kfb, int nx,
               const lmpc_settings *s, int device);

/*
 * The same setup with the two keywords the reference passes to DAQP.setup next to the matrices
 * (/root/reference/src/setup.jl:11-13):
 *
 *   break_points[n_break_points]  mpQP.break_points (Cint; /root/reference/src/mpc2mpqp.jl:890-892): the ends of the
 *          constraint priority levels (`prio` of set_bounds! / add_constraint!, setup.jl:50-97).  Empty (NULL, 0) for
 *          every controller without priorities.  A non-empty list asks DAQP for its hierarchical mode, which the
 *          batched backend does not implement: LMPC_ERR_UNSUPPORTED (never silently ignored).
 *   is_avi  !mpQP.is_symmetric: H is NOT symmetric (several objectives, one per player: set_objective!(mpc, uids; ...),
 *          setup.jl:137-151, mpc2mpqp.jl:900-950) and the problem is the affine variational inequality
 *              find x in the constraint set with (H x + f + f_theta theta)'(y - x) >= 0 for every feasible y
 *          (H + H' must be positive definite: LMPC_ERR_NONCONVEX otherwise).  Solved by the library's AVI kernel
 *          (one problem per lane, recursive L D U factorisation; binary64; no BINARY rows); every entry point that
 *          takes a handle works on it except the binary32 ones and the Gram-scan option.  is_avi == 0 with a
 *          non-symmetric H is LMPC_ERR_BADARG.  (PARITY OF THE ITERATION: UNPINNED -- libdaqp's AVI mode is not
 *          restated; the solution of a strongly monotone AVI is unique, which is what the reference-held numbers
 *          -- the game-theoretic closed loop's end values, test/runtests.jl:1337-1358 -- and the KKT certificates
 *          pin; iteration counts and working-set sequences are this build's own.)
 * lmpc_setup itself decides is_avi from H exactly as the reference decides mpQP.is_symmetric
 * (isapprox(H, H', rtol = 1e-9), mpc2mpqp.jl:897) and has no priorities.
 * lmpc_is_avi: 1 / 0.  lmpc_get_avi: the AVI pack's second matrix MR[m*n] (row j = (H^-1 ML_j')', ML = what
 * lmpc_get_ldp returns as M) and the full Gram matrix G[m*m] = ML MR' (row-major; either may be NULL).
 */
int lmpc_setup_ex(lmpc_handle **out, int n, int m, int ms, int nth, int nout,
                  const double *H, const double *f, const double *f_theta,
                  const double *A, const double *bu, const double *bl, const double *W,
                  const int32_t *sense, const double *Kfb, int nx,
                  const lmpc_settings *s, const int32_t *break_points, int n_break_points,
                  int is_avi, int device);
int lmpc_is_avi(const lmpc_handle *h);
int lmpc_get_avi(const lmpc_handle *h, double *MR, double *G);
/* The extra arrays of a handle in proximal-point mode (lmpc_settings.eps_prox > 0 at setup; its subproblems' pack is
 * what lmpc_get_ldp / lmpc_get_avi return, for H + eps_prox I): Hinv[n*n] = (H + eps_prox I)^-1, x0f[n] and
 * Xthf[n*nth] = the full-length affine map of the unconstrained optimum, Kth[nout*nth] = the outputs' feedback term.
 * LMPC_ERR_BADARG on any other handle. */
int lmpc_get_prox(const lmpc_handle *h, double *Hinv, double *x0f, double *Xthf, double *Kth);

/*
 * Setup from an already-transformed least-distance problem -- the data the reference's code
 * generator writes into C arrays (codegen.jl:183-189: Dth, du, dl, Uth_offset, u_offset, plus
 * DAQP's M) -- all ROW-major:
 *   M[m*n] normalised rows, du[m], dl[m], Dth[m*nth], Rout[nout*n] (rows of R^-1),
 *   x0[nout] (= u_offset), Xth[nout*nth] (= Uth_offset incl. -K), sense[m].
 * Replaces the static workspace of generated mpc_workspace.c / mpc_compute_control
 * (codegen/mpc_update_qp.c:29-54).
 */
int lmpc_setup_ldp(lmpc_handle **out, int n, int m, int ms, int nth, int nout,
                   const double *M, const double *du, const double *dl, const double *Dth,
                   const double *Rout, const double *x0, const double *Xth,
                   const int32_t *sense, const lmpc_settings *s, int device);

/*
 * Host-only half of lmpc_setup: the QP -> LDP transform (reference codegen.jl:239-280 `qp2ldp`,
 * i.e. what LinearMPC.codegen writes into the generated C arrays) without touching a GPU.
 * Inputs as lmpc_setup, outputs row-major as lmpc_setup_ldp takes them; any output may be NULL.
 */
int lmpc_transform(int n, int m, int ms, int nth, int nout,
                   const double *H, const double *f, const double *f_theta,
                   const double *A, const double *bu, const double *bl, const double *W,
                   const int32_t *sense, const double *Kfb, int nx,
                   double *M, double *du, double *dl, double *Dth,
                   double *Rout, double *x0, double *Xth);

/* Host-only half of an is_avi setup (no GPU touched): the transform described at lmpc_setup_ex, outputs row-major --
 * ML[m*n], MR[m*n], G[m*m], du[m], dl[m], Dth[m*nth], Rout[nout*n] (leading rows of I), x0[nout], Xth[nout*nth];
 * any output may be NULL.  LMPC_ERR_NONCONVEX if H + H' is not positive definite. */
int lmpc_transform_avi(int n, int m, int ms, int nth, int nout,
                       const double *H, const double *f, const double *f_theta,
                       const double *A, const double *bu, const double *bl, const double *W,
                       const int32_t *sense, const double *Kfb, int nx,
                       double *ML, double *MR, double *G, double *du, double *dl, double *Dth,
                       double *Rout, double *x0, double *Xth);

/* Copies the constant pack held by the handle back to the caller (row-major, sizes as in
 * lmpc_setup_ldp); any pointer may be NULL.  Lets a test feed the SAME pack to the oracle. */
int lmpc_get_ldp(const lmpc_handle *h, double *M, double *du, double *dl, double *Dth,
                 double *Rout, double *x0, double *Xth, int32_t *sense);

/* dims[0..5] = n, m, ms, nth, nout, active words per problem */
int lmpc_get_dims(const lmpc_handle *h, int32_t dims[6]);
int lmpc_active_words(const lmpc_handle *h);

/* Replaces DAQP.settings on a live model. */
int lmpc_set_settings(lmpc_handle *h, const lmpc_settings *s);

/*
 * THE hot path.  Replaces, for N parameter points at once, the body of `solve`
 * (utils.jl:272-282: bu/bl/f update, DAQP.update, DAQP.solve) and the primal recovery
 * x = R^-1 u + offsets (codegen/mpc_update_qp.c:14-22).  Cold start per problem
 * (mpc_update_qp.c:44-47) unless `warm` is given.
 *
 *   theta     N records of nth doubles        x        N records of nout doubles (out)
 *   exitflag  N int32 (out)                   iters    N int32 (out) or NULL
 *   active    N records of lmpc_active_words words (out) or NULL
 *   warm      N records of the same layout: initial working sets (in) or NULL = cold
 *
 * lmpc_solve_batch: HOST pointers; synchronous.  Large batches move through a three-stage pipeline in chunks
 * (each half of what is left, the last one "host_chunk" problems): H2D copy of chunk k+1, kernels of chunk k,
 * D2H copy of chunk k-1 on three streams.  With arrays the caller pinned (lmpc_pin_host) every copy is
 * asynchronous and one thread drives the pipeline (1.17 ms per 10^6 pendulum problems, PCIe-bound: 56 MB in at
 * 52 GB/s); with pageable arrays, whose copy calls block, the upload and download sides run on two host threads
 * ("host_threads" 0: one chunk, one thread; 1.25 against 1.30 ms).  (The option "host_register", which pinned the
 * caller's arrays for the duration of each call, was removed in round 5 -- it ended in a GPU memory fault after a few
 * hundred calls -- and lmpc_set_option answers LMPC_ERR_UNSUPPORTED for it.)
 * lmpc_solve_batch_device: DEVICE pointers on the handle's GPU; enqueues the kernels on
 * `stream` (a hipStream_t passed as void*, NULL = default stream) and returns without
 * synchronising -- this is what bench.py times with inputs resident in HBM.
 * One exception, once per handle: the FIRST large batch (>= 65 536 points) of a fresh wavefront-kernel handle whose
 * working sets can exceed 40 rows first solves its own leading 16 384 points into scratch and WAITS for that launch
 * (the probe that decides the launch shape; lmpc_set_option "wave_probe" 0 switches it off).  Inside a stream capture
 * (hipStreamBeginCapture) the probe is skipped and left for the first call outside a capture.
 */
int lmpc_solve_batch(lmpc_handle *h, int64_t N, const double *theta, double *x,
                     int32_t *exitflag, int32_t *iters, uint64_t *active,
                     const uint64_t *warm);
/* lmpc_solve_batches_device: n_batches batches of N points each in ONE call -- theta / x / exitflag are HOST tables of
 * n_batches DEVICE pointers (the tables are read during the call, the batches' buffers need not be adjacent).  Cold
 * plain solves; results are those of n_batches calls of lmpc_solve_batch_device bit for bit.  On the handles the
 * one-launch kernel covers (small box-constrained problems: the headline configuration) up to eight batches go into
 * one kernel launch, in which the solving tail of a batch runs under the stream of the next: 10^6-point pendulum
 * batches cost ~16 us each in a call of three against 22 us one call at a time.  Elsewhere it enqueues the batches one
 * after the other.  Caller side: the same loop over parameter batches that calls solve (reference src/utils.jl:268-283). */
int lmpc_solve_batches_device(lmpc_handle *h, int32_t n_batches, int64_t N, const double *const *theta, double *const *x,
                              int32_t *const *exitflag, void *stream);
int lmpc_solve_batch_device(lmpc_handle *h, int64_t N, const double *theta, double *x,
                            int32_t *exitflag, int32_t *iters, uint64_t *active,
                            const uint64_t *warm, void *stream);

/*
 * The same hot path in binary32 -- the reference's single-precision build of this path
 * (codegen.jl:19,31-37,82: float_type = "float" makes `c_float` a float and compiles DAQP with
 * DAQP_SINGLE_PRECISION, so mpc_compute_control takes and returns floats).  theta and x are float
 * records; the constant pack is the handle's binary64 pack rounded to binary32 on the first call;
 * tolerances are the handle's settings rounded to binary32 -- give the handle settings that make
 * sense at that precision (lmpc_default_settings_f32: primal 1e-4, dual 1e-6, zero 1e-6,
 * progress 1e-4, rho_soft 1e-3; libdaqp's own single-precision defaults live in a header that is
 * not part of the reference tree).  Runs on the wavefront kernel (any handle whose problem it covers:
 * n <= 127, 1 <= m <= 1024), including branch and bound over BINARY rows (n <= 64)
 * (BASELINE config 5); LMPC_ERR_UNSUPPORTED otherwise.
 */
void lmpc_default_settings_f32(lmpc_settings *s);
int lmpc_solve_batch_f32(lmpc_handle *h, int64_t N, const float *theta, float *x,
                         int32_t *exitflag, int32_t *iters, uint64_t *active,
                         const uint64_t *warm);
int lmpc_solve_batch_f32_device(lmpc_handle *h, int64_t N, const float *theta, float *x,
                                int32_t *exitflag, int32_t *iters, uint64_t *active,
                                const uint64_t *warm, void *stream);

/* A caller that reuses its Theta / X / exitflag arrays from call to call (a Monte-Carlo loop, a closed
 * loop over many scenarios) can pin them ONCE: lmpc_solve_batch* then runs fully asynchronous copies on them.
 * Pinning works on whole pages: give every array pages of its own (a page-aligned allocation, e.g. mmap /
 * posix_memalign; Julia: Mmap.mmap(Matrix{Float64}, dims)) -- a range that shares a page with memory pinned
 * earlier is refused with LMPC_ERR_BADARG.  Unpin before the memory is freed. */
int lmpc_pin_host(void *p, size_t bytes);
int lmpc_unpin_host(void *p);

/*
 * Several GPUs behind ONE call -- the shape the reference's caller has (one process, one Theta:
 * /root/reference/src/utils.jl:268-283 `solve`; SURVEY.md section 8(b) `n_devices`, section 8(e)).
 *
 * lmpc_setup_multi: lmpc_setup on every listed device (devices == NULL or n_devices <= 0: all visible
 * devices, 0 .. count-1); the constant pack is replicated, each device gets its own handle.
 * lmpc_solve_batch_multi: HOST pointers as lmpc_solve_batch.  The batch is cut into contiguous shards
 * (lmpc_multi_partition: N/n_devices each, the remainder on the leading devices); every device moves its
 * shard through the same chunked H2D / kernels / D2H pipeline lmpc_solve_batch uses, all driven from the
 * calling thread, results written straight into the caller's x / exitflag / iters / active.
 * lmpc_solve_batch_multi_device: shards already RESIDENT on their GPUs (theta[d], x[d], exitflag[d] are
 * DEVICE pointers on device d, N_dev[d] problems).  Every device solves its shard on its own stream; if
 * x_root / exitflag_root (DEVICE pointers on the FIRST device, sum(N_dev) records) are given, the
 * per-shard solutions are gathered there over xGMI with RCCL (ncclCommInitAll in this process,
 * ncclSend / ncclRecv pairs: every device sends on its own link).  Returns after all devices finished.
 * The problems are independent: no collective runs inside the solve.
 */
typedef struct lmpc_multi lmpc_multi;
int lmpc_setup_multi(lmpc_multi **out, int n, int m, int ms, int nth, int nout,
                     const double *H, const double *f, const double *f_theta,
                     const double *A, const double *bu, const double *bl, const double *W,
                     const int32_t *sense, const double *Kfb, int nx,
                     const lmpc_settings *s, const int *devices, int n_devices);
int lmpc_multi_devices(const lmpc_multi *hm);
/* "transport": how lmpc_solve_batch_multi_device gathers the shards on the first device -- 0 (default) RCCL
 * ncclSend / ncclRecv pairs, every device on its own xGMI link; 1 = event-ordered peer copies issued by the first
 * device's stream (hipMemcpyPeerAsync: the copy engines; needs no RCCL).  With the environment variable
 * LMPC_MULTI_TRANSPORT=copy at setup time transport 1 is the default AND the device list may name a device more than
 * once: several shards, handles, streams and host threads on one GPU -- the way the n_devices > 1 code is exercised on
 * a machine with a single GPU (tests/test_gpu_parity.py::test_multi_device_control_flow_on_one_gpu). */
int lmpc_multi_set_option(lmpc_multi *hm, const char *name, int value);
lmpc_handle *lmpc_multi_handle(lmpc_multi *hm, int i);      /* device i's handle (options, inspection) */
void lmpc_multi_partition(int64_t N, int n_devices, int64_t *offsets /* n_devices + 1 */);
int lmpc_solve_batch_multi(lmpc_multi *hm, int64_t N, const double *theta, double *x,
                           int32_t *exitflag, int32_t *iters, uint64_t *active, const uint64_t *warm);
int lmpc_solve_batch_multi_device(lmpc_multi *hm, const int64_t *N_dev, const double *const *theta,
                                  double *const *x, int32_t *const *exitflag,
                                  double *x_root, int32_t *exitflag_root);
const char *lmpc_multi_last_error(const lmpc_multi *hm);
void lmpc_free_multi(lmpc_multi *hm);

/* N = 1 convenience with DAQP.solve's shape: returns the exit flag (or an LMPC_ERR_* <= -100),
 * x[nout] out.  What Simulation's per-step compute_control (simulation.jl:106) would call.
 * Ordering: the call runs on a stream of the handle's own, NOT ordered with the caller's streams, and
 * uses the handle's scratch (work lists, counters, warm-start state).  Everything enqueued earlier on this handle through
 * a *_device entry point must have completed before lmpc_solve_one (or a host-array lmpc_compute_control with a handful
 * of states, which takes the same route) is called; such a call also counts as one call for the "even number of calls
 * per captured graph" rule of the *_device entry points.  One thread at a time per handle, as for a DAQP workspace. */
int lmpc_solve_one(lmpc_handle *h, const double *theta, double *x);

/*
 * Batched closed-loop simulation: N independent scenarios advanced T steps on the GPU (by default each
 * scenario at its own pace -- the scenarios do not interact, so the arrays returned are those of the
 * step-by-step loop bit for bit; lmpc_set_option "sim_async").  That execution order reads a few
 * counters back between rounds: lmpc_simulate_device waits on `stream` a few times before it returns
 * (its outputs are still only complete once `stream` is), so it cannot be captured into a hipGraph;
 * with "sim_async" 0 it only enqueues.
 * Per step and scenario it does what one pass of the reference's Simulation loop does
 * (src/simulation.jl:93-113 without observer): theta = [x; r; uprev] (src/explicit.jl:54-63),
 * u = compute_control (the batched solve of this handle, which must have been set up with
 * nout = nu and, if used, the prestabilising feedback folded in), x <- F x + G u, uprev <- u.
 * warm != 0 starts each solve from the previous step's final working set (the reference's
 * DAQP_WARMSTART build, codegen/mpc_update_qp.c:44-47); the first step is cold.  On the wavefront-kernel
 * path (binary64, no binaries) the working set comes back WITH its factorisation, in its order -- libdaqp's
 * workspace under DAQP_WARMSTART is simply not cleared between two calls (mpc_update_qp.c:44-54) -- kept per
 * scenario in device memory (17 KB at the largest capacity); lmpc_set_option "sim_keep_factor" 0 re-appends the
 * rows of the previous step's mask instead, as the lane kernels and the binary32 loop do.  Either way the
 * inputs are those of the cold loop up to the tolerances (K6, test/runtests.jl:85-117).
 *
 *   nx + nr + nuprev must equal nth.  F[nx*nx], G[nx*nu] row-major HOST arrays (the plant).
 *   x      N records of nx: in = initial states, out = states after T steps
 *   r      N records of nr (constant reference per scenario) or NULL = 0
 *   uprev  N records of nuprev, in/out (NULL allowed when nuprev == 0)
 *   U_traj T*N*nu (step-major) or NULL;  X_traj (T+1)*N*nx or NULL
 *   flag_min N int32: smallest exit flag seen over the T steps (>= 1 means every solve succeeded) or NULL
 * lmpc_simulate takes HOST pointers; lmpc_simulate_device DEVICE pointers (except F, G) and a stream.
 */
int lmpc_simulate(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev,
                  const double *F, const double *G, double *x, const double *r, double *uprev,
                  double *U_traj, double *X_traj, int32_t *flag_min, int warm);
int lmpc_simulate_device(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev,
                         const double *F, const double *G, double *x, const double *r, double *uprev,
                         double *U_traj, double *X_traj, int32_t *flag_min, int warm, void *stream);

/*
 * The closed loop in binary32 -- the reference's generated controller built with float_type = "float"
 * (codegen.jl:19,31-37) inside a simulation: x, r, uprev and the trajectories are float records, the
 * plant (F, G: HOST binary64 arrays as everywhere) is rounded to binary32 like the constant pack, the
 * plant step is an fmaf chain in the same order.  Wavefront kernel (see lmpc_solve_batch_f32).
 */
int lmpc_simulate_f32(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev,
                      const double *F, const double *G, float *x, const float *r, float *uprev,
                      float *U_traj, float *X_traj, int32_t *flag_min, int warm);
int lmpc_simulate_f32_device(lmpc_handle *h, int64_t N, int T, int nx, int nr, int nuprev,
                             const double *F, const double *G, float *x, const float *r, float *uprev,
                             float *U_traj, float *X_traj, int32_t *flag_min, int warm, void *stream);

/*
 * Batched form_parameter on the device, previews included: theta_i = [x_i; r; d; uprev_i; p]
 * (reference explicit.jl:54-63) with r, d, p formatted as format_reference / format_disturbance /
 * format_affine_parameters do (utils.jl:78-261) and, inside a closed loop, as Simulation's
 * get_preview does (simulation.jl:100-103,128-134).
 *
 * A block is cut from a trajectory: `w` values per column, `T` columns stored column by column
 * (a Julia w x T matrix) -- one matrix per scenario, `stride` doubles apart, or one shared by all
 * scenarios (stride 0).  H == 0: the block is column k0 (a constant reference: T = 1, k0 = 0);
 * H > 0 (preview over H steps, H = mpc.Np): columns k0 .. k0+H-1, flattened column by column.
 * Columns past the end repeat the last one (how the reference pads a short trajectory); src == NULL
 * gives zeros (the reference's `nothing` default); w == 0 leaves the block out.
 * nx + width(r) + width(d) + nuprev + width(p) must equal the handle's nth.
 */
typedef struct lmpc_block {
    const double *src;   /* DEVICE pointer or NULL                                  */
    int64_t stride;      /* doubles between two scenarios' matrices, 0 = shared     */
    int32_t w;           /* values per column (ny, nd or the base parameter count)  */
    int32_t T;           /* columns available                                       */
    int32_t k0;          /* first column taken                                      */
    int32_t H;           /* 0 = one column, > 0 = preview over H columns            */
} lmpc_block;
int lmpc_form_parameter_device(lmpc_handle *h, int64_t N, double *theta, const double *x, int nx,
                               const lmpc_block *r, const lmpc_block *d, const double *uprev,
                               int nuprev, const lmpc_block *p, void *stream);

/*
 * Closed loop with a reference TRAJECTORY (reference simulation.jl:69-73,93-113: `rs` held at its
 * last column, and with settings.reference_preview the controller sees columns k+1 .. k+Np at
 * step k).  As lmpc_simulate_device, but the reference of step k (0-based) is cut from `r`:
 * r->H == 0: column k; r->H > 0: columns k+1 .. k+H (r->k0 is ignored).  DEVICE pointers.
 */
int lmpc_simulate_ref_device(lmpc_handle *h, int64_t N, int T, int nx, const lmpc_block *r, int nuprev,
                             const double *F, const double *G, double *x, double *uprev,
                             double *U_traj, double *X_traj, int32_t *flag_min, int warm, void *stream);

/*
 * The batched counterpart of the reference's GENERATED controller
 *   int mpc_compute_control(c_float* control, c_float* state, c_float* reference,
 *                           c_float* disturbance[, c_float* affine_parameter])
 * (reference src/codegen.jl:1-17, codegen/mpc_update_qp.h:3-7, body codegen/mpc_update_qp.c:29-54):
 * mpc_update_parameter (codegen/mpc_update_parameter.c:1-29) + mpc_update_qp + daqp_ldp/daqp_bnb +
 * mpc_get_solution for N problems at once.  The handle must have been set up with nout = N_CONTROL.
 *
 * lmpc_set_parameter_layout gives the handle the constants the generated header defines
 * (codegen.jl:154-165): N_STATE, N_REFERENCE, N_DISTURBANCE, N_CONTROL_PREV, N_AFFINE_PARAMETER --
 * they must add up to nth -- and, for settings.reference_condensation (codegen.jl:191-195),
 * N_PREVIEW_HORIZON with traj2setpoint[n_reference*n_preview_horizon*n_reference] exactly as the
 * generator writes it (mpc.traj2setpoint[:], HOST array, copied).
 *
 *   control   N records of nout doubles: in = previous control (first n_control_prev entries are
 *             read), out = u* -- the in/out convention of the generated function
 *   state     N records of n_state            reference  N records of n_reference doubles, or of
 *             n_reference*n_preview_horizon (an n_reference x n_preview_horizon trajectory, column by
 *             column) when condensing; disturbance / affine_parameter: N records of their widths.
 *             NULL for reference / disturbance / affine_parameter = zeros (runtests.jl:943 passes NULL
 *             for absent blocks).
 *   exitflag  N int32 (out) or NULL           warm != 0 = the DAQP_WARMSTART build
 *             (mpc_update_qp.c:44-47): each problem starts from the working set its previous call
 *             with the same N ended with; 0 = cold start every call.
 * lmpc_compute_control: HOST pointers, synchronous.  lmpc_compute_control_device: DEVICE pointers,
 * enqueued on `stream`, no synchronisation.
 */
typedef struct lmpc_param_layout {
    int32_t n_state, n_reference, n_disturbance, n_control_prev, n_affine_parameter;
    int32_t n_preview_horizon;       /* 0 unless settings.reference_condensation */
    const double *traj2setpoint;     /* HOST, or NULL when n_preview_horizon == 0 */
} lmpc_param_layout;
int lmpc_set_parameter_layout(lmpc_handle *h, const lmpc_param_layout *layout);
int lmpc_compute_control(lmpc_handle *h, int64_t N, double *control, const double *state,
                         const double *reference, const double *disturbance,
                         const double *affine_parameter, int32_t *exitflag, int warm);
int lmpc_compute_control_device(lmpc_handle *h, int64_t N, double *control, const double *state,
                                const double *reference, const double *disturbance,
                                const double *affine_parameter, int32_t *exitflag, int warm, void *stream);

/*
 * The reference's GENERATED state observer for N scenarios at once: mpc_predict_state(state, control,
 * disturbance) and mpc_correct_state(state, measurement, disturbance) (codegen/mpc_observer.c:1-28,
 * mpc_observer.h; Julia: predict! / correct! of the KalmanFilter, src/observer.jl:104-123), the other
 * two functions the generated controller exports next to mpc_compute_control.
 *
 * lmpc_set_observer takes the arrays exactly as the generator writes them (src/observer.jl:124-140):
 *   plant_dynamics        MPC_PLANT_DYNAMICS       n_state rows [f_offset_i, F_i(n_state), G_i(n_control), Gd_i(n_disturbance)]
 *   measurement_function  MPC_MEASUREMENT_FUNCTION n_measurement rows [h_offset_j, C_j(n_state), Dd_j(n_disturbance)]
 *   k_transpose           K_TRANSPOSE_OBSERVER     n_measurement rows of n_state (the Kalman gain, transposed)
 * (HOST arrays, copied).  state: N records of n_state, updated in place; control / measurement /
 * disturbance: N records of their widths; disturbance may be NULL (zeros), as in the reference's calls
 * (runtests.jl:942-946).  *_device variants take DEVICE pointers and a stream and do not synchronise.
 */
typedef struct lmpc_observer {
    int32_t n_state, n_control, n_disturbance, n_measurement;
    const double *plant_dynamics, *measurement_function, *k_transpose;
} lmpc_observer;
int lmpc_set_observer(lmpc_handle *h, const lmpc_observer *obs);
int lmpc_predict_state(lmpc_handle *h, int64_t N, double *state, const double *control, const double *disturbance);
int lmpc_correct_state(lmpc_handle *h, int64_t N, double *state, const double *measurement,
                       const double *disturbance);
int lmpc_predict_state_device(lmpc_handle *h, int64_t N, double *state, const double *control,
                              const double *disturbance, void *stream);
int lmpc_correct_state_device(lmpc_handle *h, int64_t N, double *state, const double *measurement,
                              const double *disturbance, void *stream);

/*
 * The generated offset-free observer's controller call for N scenarios (reference src/observer.jl:156-196):
 *   int mpc_compute_control_observer(control, observer_state, reference, measured_disturbance[, affine_parameter])
 * = mpc_get_estimated_state (state = observer_state[0:n_state]) + mpc_get_estimated_disturbance (disturbance =
 * [measured_disturbance or zeros; observer_state[n_state : n_state + n_offset_free]]) + mpc_compute_control.
 * n_offset_free = the layout's n_disturbance - n_measured_disturbance; observer_state: N records of
 * n_state + n_offset_free doubles.  DEVICE pointers, enqueued on `stream`.
 */
int lmpc_compute_control_observer_device(lmpc_handle *h, int64_t N, double *control, const double *observer_state,
                                         int n_measured_disturbance, const double *reference,
                                         const double *measured_disturbance, const double *affine_parameter,
                                         int32_t *exitflag, int warm, void *stream);

/* Which kernel variant the handle dispatches to (for benchmark reports), e.g. "lane<5>". */
const char *lmpc_kernel_name(const lmpc_handle *h);

/* Working-set statistics of the wavefront kernel, as the handle last saw them (cumulative over its launches, a launch or
 * two behind; read from mapped host memory, no synchronisation): out[0] problems the kernel finished, out[1..3] of them
 * those whose working set never held more than 24 / 32 / 48 rows, out[4] the working-set capacity of the first pass the
 * next call would use (0 = one pass).  This is what decides whether a batch first runs at a smaller capacity
 * (lmpc_set_option "wave_two_pass"); reported for benchmark logs and tests.  Returns LMPC_OK (all zeros before the
 * first wavefront-kernel launch). */
int lmpc_wave_stats(lmpc_handle *h, unsigned long long out[5]);

/* Which wavefront-kernel instantiations the handle last launched, and in which launch shape: the handle keeps a record
 * of its four most recent wavefront-kernel launches (one call makes up to three: a first pass at a smaller capacity,
 * the second pass at the full one, and -- once per fresh handle -- the probe in front).  Written on the host when a
 * launch is enqueued; nothing is read from the device and nothing is waited for.  Copies min(launches so far, 4, max)
 * entries into out, OLDEST first, LMPC_WAVE_INFO_WORDS words each, and returns how many (< 0: error).  Words of an entry:
 *    [0] running number of the launch in the handle's life (1, 2, ...): read it before and after a call to tell that
 *        call's launches from earlier ones
 *    [1] sizeof(real): 8 / 4      [2] constraint slots MR    [3] staging level LDSC the kernel was built for
 *    [4] BNB   [5] PACKED   [6] variable slots NU   [7] GRAM   [8] SIM  -- the template arguments of wave_kernel
 *    [9] wavefronts per workgroup (nwv)   [10] staging level of the launch configuration   [11] workgroups (grid)
 *   [12] problems per ticket (qchunk)     [13] pass: 0 the only one, 1 / 2 first / second of two
 *   [14] working-set capacity of this launch   [15] 1 = the slow path (big_kernel) was enqueued behind it
 *   [16] 1 = problems handed out through the ticket counter, 0 = static split
 *   [17] 1 = the launch walks a work list (behind a screening / tiers / row pass, or as a second pass)
 *   [18] dynamic LDS bytes per workgroup  [19] problems of the batch (saturated at 2^31 - 1)
 * A request the launcher could not honour ("wave_level" 3 where the packed Gram matrix does not fit the LDS, say) shows
 * here as the configuration that ran instead.  For tests and benchmark reports. */
#define LMPC_WAVE_INFO_WORDS 20
int lmpc_wave_launch_info(const lmpc_handle *h, int32_t *out, int max);

/* The same for the four-problems-per-wavefront kernel (row_kernel): the handle's four most recent row-kernel launches,
 * OLDEST first, LMPC_ROW_INFO_WORDS words each; returns how many (< 0: error).  A call makes at most one (the only pass
 * of a batch, or the first of two -- the second is a wavefront-kernel launch and shows in lmpc_wave_launch_info).
 * Host memory only.  A batch the row kernel does not take ("row_kernel" 1 is a request: warm starts, the Gram form, a
 * closed loop, an ACTIVE row, an iteration limit below 2, no covering shape, ...) leaves no entry.  Words of an entry:
 *    [0] running number of the launch in the handle's life (1, 2, ...), counted apart from the wavefront kernel's
 *    [1] sizeof(real): 8 / 4   [2] position slots S   [3] variable slots NS   [4] constraint slots MS
 *    [5] leading dimension CAPP   [6] BNB  -- the template arguments of row_kernel
 *    [7] wavefronts per workgroup (nwv; each carries four problems)   [8] workgroups per CU chosen
 *    [9] workgroups (grid)     [10] spacing ps of a problem's factor in LDS (reals)
 *   [11] dynamic LDS bytes per workgroup   [12] aux: 1 = the per-problem constants staged in LDS (ten-slot shapes)
 *   [13] pass: 0 the only one, 1 the first of two   [14] working-set capacity of this launch
 *   [15] problems per ticket (qchunk)   [16] 1 = problems handed out through the ticket counter, 0 = static split
 *   [17] 1 = the launch walks a work list (behind a screening / tiers pass)
 *   [18] problems of the batch (saturated at 2^31 - 1)
 *   [19] bytes of search snapshots the handle holds after this launch (BNB; saturated at 2^31 - 1; 0 otherwise)
 * For tests and benchmark reports. */
#define LMPC_ROW_INFO_WORDS 20
int lmpc_row_launch_info(const lmpc_handle *h, int32_t *out, int max);

/* The one-launch kernel (fast_kernel / fast_kernel_multi): the handle's most recent launch of it, LMPC_FAST_INFO_WORDS
 * words; returns 1, 0 if the handle never launched it (< 0: error).  Host memory only, written when the launch is
 * enqueued.  Words:
 *    [0] running number of the launch in the handle's life (1, 2, ...)
 *    [1] form: 0 plain, 1 gather (the generated controller's call), 2 several batches in one launch
 *    [2] 1 = staged write-out: x and the exit flags of a workgroup's tiles are kept in LDS and stored once, as whole
 *        lines, at the workgroup's end (one output, no iters / active array, no gather, a static split, and LDS that
 *        keeps the shape's workgroups per CU; by default only under "in_flight" >= 2, see "fast_stage"); 0 = stored where found
 *    [3] tiles of 64 problems a workgroup's queue holds   [4] streaming wavefronts per workgroup
 *    [5] LDS-DMA ring depth (0 = records through registers)   [6] workgroups per batch (grid x)   [7] batches (grid y)
 *    [8] dynamic LDS bytes per workgroup   [9] tiles per workgroup handed out through tickets ("fast_dyn"; 0 = static)
 * For tests and benchmark reports. */
#define LMPC_FAST_INFO_WORDS 10
int lmpc_fast_launch_info(const lmpc_handle *h, int32_t *out);

/* The same for the pass that runs IN FRONT of an iterating kernel and fills its work list (the screening pass or the
 * tiers pass, qp_tiers_kernel): the handle's four most recent front-pass launches, OLDEST first, LMPC_FRONT_INFO_WORDS
 * words each; returns how many (< 0: error).  Host memory only, written when the launch is enqueued.  A call without a
 * front pass (the one-launch kernel, a wavefront-kernel call without screening, "screen" 0) leaves no entry.  Words:
 *    [0] running number of the launch in the handle's life (1, 2, ...), counted apart from the other records
 *    [1] kind: LMPC_FRONT_SCREEN (1) the screening pass, LMPC_FRONT_TIERS (2) the tiers pass
 *    [2] template argument N of qp_tiers_kernel (0 for the screening pass)
 *    [3] workgroups (grid)   [4] dynamic LDS bytes per workgroup   [5] problems of the batch (saturated at 2^31 - 1)
 *    [6] seg_cap: entries a segment of the work list holds (saturated likewise)
 *    [7] the kernel that walks the list: LMPC_WALK_LANE (1), LMPC_WALK_WAVE (2), LMPC_WALK_ROW (3)
 * For tests and benchmark reports. */
#define LMPC_FRONT_INFO_WORDS 8
#define LMPC_FRONT_SCREEN 1
#define LMPC_FRONT_TIERS 2
#define LMPC_WALK_LANE 1
#define LMPC_WALK_WAVE 2
#define LMPC_WALK_ROW 3
int lmpc_front_pass_info(const lmpc_handle *h, int32_t *out, int max);

/* What a front pass left on the work list, for tests: with lmpc_set_option(h, "list_snapshot", 1) every call that runs
 * a front pass enqueues, between that pass and the kernel behind it, a device-to-device copy of the call's counter set
 * and of its LMPC_LIST_SHARDS x seg_cap list into a buffer the handle owns (allocated when the option is set, grown by
 * the call that needs more, freed with the handle and by lmpc_release_scratch).  lmpc_work_list_read waits for the
 * handle's device, then copies the counters of the most recent snapshot into counts[LMPC_LIST_SHARDS] and the list,
 * segment after segment at seg_cap (word [6] of that call's lmpc_front_pass_info entry) words each, into
 * list[list_words] (list may be NULL: counters only; list_words smaller than LMPC_LIST_SHARDS x seg_cap: LMPC_ERR_BADARG).
 * Returns seg_cap, 0 if no snapshot has been taken (since the option was set or the scratch released), < 0 on error.
 * With the option off (the default) no call changes; with it on, a call made inside a stream capture is refused
 * (LMPC_ERR_UNSUPPORTED): the snapshot may have to allocate. */
#define LMPC_LIST_SHARDS 64
long long lmpc_work_list_read(lmpc_handle *h, int32_t *counts, int32_t *list, long long list_words);

/* The same for the chain of a variational handle (is_avi; lmpc_avi.hip): the handle's eight most recent launches of
 * avi_tiers_kernel, avi_lane_kernel and avi_kernel, OLDEST first, LMPC_AVI_INFO_WORDS words each; returns how many
 * (< 0: error).  A call makes three (the chain) or one (the slab kernel alone: warm start, iter_limit <= n + 1,
 * "avi_tiers" 0, a problem the register kernels do not cover).  Host memory only, written when a launch is enqueued.
 *    [0] running number of the launch in the handle's life (1, 2, ...), counted apart from the other records
 *    [1] stage: LMPC_AVI_TIERS (1) avi_tiers_kernel<N, K, false>, LMPC_AVI_LANE (2) avi_lane_kernel<N, LIST>,
 *        LMPC_AVI_SLAB (3) avi_kernel<LDSC, PROX>
 *    [2] N   [3] K (0: lane and slab kernel)   [4] LIST: 1 = the launch walks a work list   [5] LDSC   [6] PROX
 *    [7] workgroups (grid)   [8] dynamic LDS bytes per workgroup
 *    [9] what the grid was sized with: workgroups per CU the instantiation keeps resident (register kernels, from
 *        hipOccupancyMaxActiveBlocksPerMultiprocessor on the kernel that is launched), wavefronts per CU (slab kernel)
 *   [10] problems of the batch (saturated at 2^31 - 1)   [11] seg_cap of the chain's lists (0: no list)
 * For tests and benchmark reports. */
#define LMPC_AVI_INFO_WORDS 12
#define LMPC_AVI_INFO_KEPT 8
#define LMPC_AVI_TIERS 1
#define LMPC_AVI_LANE 2
#define LMPC_AVI_SLAB 3
int lmpc_avi_launch_info(const lmpc_handle *h, int32_t *out, int max);

/* What the chain's first two launches left on their work lists, for tests: with lmpc_set_option(h, "list_snapshot", 1)
 * a call that runs the chain enqueues a device-to-device copy of each list's counter set and of its LMPC_LIST_SHARDS x
 * seg_cap entries right after the launch that filled it -- before the slab kernel, which clears the first set, and
 * before the next call's first launch, which clears the second.  which = 0: the list of the launch over the whole
 * batch, 1: the lane kernel's.  Arguments and return value as lmpc_work_list_read; 0 also after a call that made no
 * list (the slab kernel alone).  A call made inside a stream capture is refused with the option on. */
long long lmpc_avi_list_read(lmpc_handle *h, int which, int32_t *counts, int32_t *list, long long list_words);

/* Device and pinned-host blocks that the library's handles and explicit controllers hold at this moment, in the whole
 * process (the copies of a host-pointer call's arrays, which live for that call only, are not counted).  The same
 * before a handle is set up and after it is freed.  For tests. */
int64_t lmpc_debug_live_blocks(void);

/* Device time per lmpc_solve_batch* call, measured with HIP events recorded on the launch
 * stream (switch on with lmpc_profile(h, 1); timing-only events, hipEventDisableSystemFence: a default event's
 * system-scope cache writeback added ~1.7 us to a 24 us call that rocprofv3's kernel trace does not see).  lmpc_profile_read waits for the recorded calls,
 * averages over the calls made since the last read and returns how many there were (<0: error):
 *   avg_ms[0] whole call (screening pass + iterating pass), avg_ms[1] screening kernel,
 *   avg_ms[2] iterating kernel. */
int lmpc_profile(lmpc_handle *h, int enable);
int lmpc_profile_read(lmpc_handle *h, double avg_ms[3]);

/* Tuning switches (none of them changes a result): "in_flight" k = a HINT: the caller keeps k independent batches in
 * flight on this GPU (one handle and one stream each; default 1).  From k = 2 on the kernels take the workgroup shapes
 * that suit a shared chip ("fast_nstr" 4, "fast_tiles" 28, "lane_block" 64) instead of the stand-alone ones.
 * "fast_dma" = how the one-launch kernel's streaming wavefronts take their records: 2 (default with up to three
 * streaming wavefronts per workgroup) = by LDS-DMA (global_load_lds_dwordx4, nontemporal) into a ring of two tiles per
 * wavefront, 0 = through registers.  "gram_scan" (default 0) is NOT one of them: it selects the wavefront kernel's
 * Gram-scan form, whose results differ from the default form in the last bits (see lmpc_wave_kernel.hpp; checker: the
 * oracle's mode 1).  "fast" (default 1) = small box-constrained problems
 * (m == ms == n <= 5, up to 16 parameters -- 8 for n = 5 --, cold start) are solved by ONE kernel that streams the batch and
 * runs the iterations underneath (0 = the two-kernel form below); "fast_nstr" 1..4 = streaming wavefronts per
 * workgroup of that kernel (default 3; 4 suits several batches in flight), "fast_tiles" = tiles of 64 problems per workgroup
 * (default: one resident round of workgroups; 28 suits three 10^6-point batches in flight); "fast_stage" (default -1 =
 * where it applies -- see lmpc_fast_launch_info -- with "in_flight" >= 2; 1 = wherever it applies; 0 = never) = that kernel
 * keeps x and the exit flags of a workgroup's tiles in LDS and stores them once, as whole lines; "lane_straight" (default 1) =
 * straight-line first tier in the boxed iterating kernels.  "screen" (default 1) = run cold-start batches through the streaming
 * screening pass before the iterating kernel; 0 = iterating kernel only.  "screen_wave" (default 1) = the same pass in
 * front of the wavefront kernel (binary64 problems without binary rows and without initially active rows, 1..32
 * parameters): it finishes every problem whose unconstrained optimum is feasible -- what the wavefront kernel's first
 * iteration would do -- and the wavefront kernel walks a work list of the others.  "big_path" (default 1) = points
 * whose working set outgrows the wavefront kernel's 64 rows are re-solved by the one-problem-per-thread kernel
 * (0 = they keep exit flag -7).  Results are
 * bit-identical either way.  Closed loop (lmpc_simulate*): "sim_async" (default 1) = scenarios
 * advance independently of each other (rounds of a streaming kernel and the iterating kernel; on the wavefront-kernel
 * path whenever "sim_run_ahead" applies, 2 = there in any case), 0 = all scenarios step by step together;
 * "sim_run_ahead" (default 1; wavefront-kernel path) = a scenario whose step ends with a non-empty working set stays
 * inside the wavefront kernel for its next step, warm on the factorisation as it stands (cold: from nothing) -- same
 * results as the step-synchronous loop with "sim_keep_factor" 1; "sim_blind" (default 2) = rounds enqueued between two
 * reads of the work-list counters; "sim_small" (default 1) = the all-in-registers instantiation
 * of the streaming kernel for single-input problems with nx <= 4, m <= 8; "sim_fused" (default 1) = plant step inside the solve's
 * kernels (lane kernels; round 3: the wavefront-kernel path's lock-step loop too).  All of them change the execution
 * order only, never a result.  "sim_keep_factor" (default 1; wavefront-kernel path, warm closed loop) = continue each
 * step from the kept factorisation instead of re-appending the previous mask's rows: same optimum up to the
 * tolerances, last bits of u may differ (checker: oracle_simulate warm = 2 against warm = 1).
 * Wavefront kernel, working-set capacity: "wave_two_pass" (default -1 = decided by the handle's statistics, see
 * lmpc_wave_stats; 0 = never; 1 = always, at "wave_cap1" rows, default 24) = run a batch first at a smaller capacity
 * (more wavefronts resident) and hand the points that outgrow it to a second launch at the full capacity;
 * "wave_cap" c (8 .. 64, 0 = the problem's own) = the full capacity itself, points beyond it go to the slow path.
 * Neither changes a result.
 * "row_kernel" (default -1): cold plain batches with n <= 64 variables, m <= 160 rows (from 8 192 problems on; 16 < n <= 32,
 * m <= 96: whatever the batch size) and branch-and-bound searches (m <= 64, up to 47 binary rows; whatever the batch
 * size: ONE search takes 1.0 ms there against 1.5 ms) run on the four-problems-per-wavefront kernel
 * (lmpc_row_kernel.hpp: one problem per 16-lane DPP row) where the handle's statistics let its working-set capacity --
 * 16 / 31 / 32 rows, searches 16 / 48 -- hold nearly all points; what outgrows it is listed for the wavefront kernel
 * (the two-pass protocol above).  -1 = where it measured faster (binary64 every shape, binary32 the two-slot shape and
 * the searches), 1 = wherever an instantiation covers the problem, whatever the batch size, 0 = never.  "row_blocks" =
 * its workgroups per CU (tuning).  Results identical either way (tools/fuzz_row.py, tools/fuzz_row_bnb.py).
 * "qp_tiers": problems with n = 2 .. 12 variables and up to 64 hard or SOFT rows (no other flags) can send cold plain
 * binary64 batches through a tiers pass (one problem per lane, append-only paths finished in registers) in front of the
 * wavefront / lane kernel.  2 = always, 0 = never (the screening pass as before), 1 (default) = yes -- and for batches of
 * 65 536 problems and more on the wavefront path whichever of the two the handle has measured faster (the best of three
 * calls each way, timed by events that later calls read without waiting; measured again every 512 calls).  Results identical either way.
 * Variational handles (is_avi) with n <= 8 simple bounds run a chain of register-resident kernels in front of the
 * generic one: "avi_tiers" (default 1; 0 = the generic kernel alone), "avi_tiers_first" (-1 = default: 3 up to n = 6,
 * else 2; 1 .. 3 = straight-line tiers of the pass over the whole batch; 0 = the complete lane kernel over the whole
 * batch), "avi_waves" (generic kernel: wavefronts per CU, default 16), "avi_chain_groups" (default 0 = no cap; g > 0
 * caps the workgroups of all three launches: rounded up to a multiple of 16 for the register kernels, down to a
 * multiple of 64 -- 64 at least -- for the generic kernel behind a list; small values make every wavefront walk
 * several tiles).  Results identical either way.
 * hipGraph capture of calls on one handle: the work-list and ticket counters alternate between two sets, each call
 * clearing the set of the next one -- capture an EVEN number of calls per handle. */
int lmpc_set_option(lmpc_handle *h, const char *name, int value);

/* Distinct optimal active sets of a solved batch, reduced on the device: the caller side of a sampling-based
 * explicit-MPC region discovery / complexity certificate (/root/reference/src/explicit.jl:23-48 hands the mpQP to
 * ParametricDAQP for an exact enumeration; what the batched backend contributes is the sample: solve, then one entry per
 * critical region the sample hit).  `active` and `exitflag` are lmpc_solve_batch_device's outputs (device pointers;
 * exitflag == NULL: every problem counts, else those with exitflag >= 1).  Outputs, device pointers, dense in
 * [0, *n_sets): set_masks[k * words ..] the mask, set_count[k] how many problems ended on it, set_first[k] the
 * smallest problem index that did.  `capacity` = room in the three arrays; more distinct sets than that raise the
 * overflow word (lmpc_distinct_active_sets_overflowed: 0 / nonzero, synchronises the stream) and *n_sets then counts
 * the claims, not the stored sets.  Order of the sets is unspecified (sort on the host).  Asynchronous on `stream`.
 * Precondition: a ONE-word mask (2 m <= 64 bits) is never all ones -- that value is the empty key of the lock-free
 * reduction (N >= 65536, option "region_lockfree"); the solver cannot produce it, a row is never active at both bounds.
 * The overflow word belongs to the LAST call on the handle: 0 if its sets fitted, 1 if there were more than `capacity`
 * (then *n_sets >= capacity, the first min(*n_sets, capacity) entries hold complete sets, but counts and first indices
 * are not final), 2 if a table slot was never published.  A call that is not repeated leaves its word standing until
 * the next call on the handle, which starts from 0 whatever this one reported and whichever kernel either one took. */
int lmpc_distinct_active_sets_device(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag,
                                     int32_t capacity, uint64_t *set_masks, int64_t *set_count, int64_t *set_first,
                                     int32_t *n_sets, void *stream);
int lmpc_distinct_active_sets_overflowed(lmpc_handle *h, void *stream);

/* One step of a sampling-based region discovery in ONE enqueue: lmpc_solve_batch_device on the resident sample with the
 * active-set masks kept on the device, lmpc_distinct_active_sets_device on them, and a last kernel that writes the
 * distinct sets into a block of mapped host memory owned by the handle -- no copy call, no synchronisation inside.
 * theta / x / exitflag / active and the four set arrays are DEVICE pointers as in the two calls it chains.
 * *result_host (valid until the next call of this function on the handle or lmpc_free) is read after ONE
 * synchronisation of `stream`: 64-bit words
 *     [0] sets found (more than `capacity`: the call overflowed, repeat with more room; -1: not finished yet)
 *     [1] overflow word   [2] problems counted (exit flag >= 1)   [3] unused
 *     then per set k < min([0], capacity): `words` words of mask, its count, the smallest problem index that hit it.
 * The sets come in no particular order (sort on the host).  Caller side of /root/reference/src/explicit.jl:23-48. */
int lmpc_discover_regions_device(lmpc_handle *h, int64_t N, const double *theta, double *x, int32_t *exitflag,
                                 uint64_t *active, int32_t capacity, uint64_t *set_masks, int64_t *set_count,
                                 int64_t *set_first, int32_t *n_sets, const long long **result_host, void *stream);

/* Per-problem exit flags are DAQP's (1 optimal, 2 soft optimal, -1 infeasible, -2 cycle, -4 iteration limit, -6
 * over-determined initial working set) plus two of this library's own:
 *   -7  the working set outgrew what the kernels hold (wavefront kernel: 64 rows, slow path: 256 rows);
 *   -8  LMPC_EXIT_UNFINISHED: the problem was queued inside the one-launch kernel and never solved because one of that
 *       kernel's bounded waits ran out (not expected to happen; the provisional flag every queued problem carries until
 *       its solving lane overwrites it -- so a failure can never be read as success, /root/reference/src/utils.jl:46
 *       `@assert exitflag>=1`).
 * The *_device entry points are asynchronous, so such a failure is reported by the handle afterwards: the next call on
 * the handle, lmpc_profile_read, lmpc_release_scratch and lmpc_check return LMPC_ERR_HIP once (text in
 * lmpc_last_error); the host-pointer entry points (lmpc_solve_batch, ...) report it from the call itself.
 * lmpc_check waits for the handle's GPU first, i.e. it answers for everything enqueued so far.
 * ("fast_spin_limit" k > 0 of lmpc_set_option is the test hook: the waits give up after k - 1 polls.) */
#define LMPC_EXIT_UNFINISHED (-8)
int lmpc_check(lmpc_handle *h);

/* lmpc_reserve: allocate NOW what the *_device entry points would allocate lazily inside their first call on a batch of
 * N problems (work lists, overflow lists, counters, the slow path's scratch), so that the first call enqueues kernels
 * and nothing else.  Optional; on a wavefront-kernel handle it also sends ONE dummy problem through the kernel on
 * `stream` and waits for it (the queue's first dispatch of that kernel costs ~4 ms), otherwise asynchronous (a few
 * memsets).  (The kernels' code objects are loaded by lmpc_setup*, not by the first solve.)  What a first call on a fresh
 * wavefront-kernel handle still does by itself, once: it solves the leading 16 384 points of its own batch in front
 * into scratch outputs, waits for that launch and reads the working-set sizes it saw, so that the batch runs in the
 * launch shape a warmed-up handle would choose (lmpc_set_option "wave_probe" 0: never; such a handle's first calls run
 * in one pass until its statistics exist).  The statistics behind that choice cover the most recent one to two
 * million problems, not the handle's whole life. */
int lmpc_reserve(lmpc_handle *h, int64_t N, void *stream);

/* Staging and scratch buffers of a handle grow with the largest batch it has seen and are kept between calls.
 * lmpc_release_scratch waits for the handle's GPU and gives them back (the constant pack stays; the next call
 * allocates what it needs again, and a DAQP_WARMSTART state kept by lmpc_compute_control* is dropped). */
int lmpc_release_scratch(lmpc_handle *h);

void lmpc_free(lmpc_handle *h);

/* Last error text of this handle (or of the failed setup call when h == NULL). */
const char *lmpc_last_error(const lmpc_handle *h);

/* Library/ABI version, bumped on any signature change. */
int lmpc_abi_version(void);

/*
 * Explicit MPC: a piecewise-affine controller built from a solved training sample and evaluated on the GPU -- the
 * counterpart of the reference's ExplicitMPC + build_tree! + compute_control(empc, x) (src/explicit.jl:23-76,
 * src/utils.jl:53-60), with the regions taken from the sample instead of an exact enumeration.
 *
 * Build (host only, no GPU touched): the distinct optimal active sets of the sample's points with exit flag >= 1 are
 * the regions, most frequent first.  For each, in the handle's LDP form (the pack lmpc_get_ldp returns), the working
 * set A gives the multipliers lambda_A(theta) = -(M_A M_A' + rho_soft S_A)^-1 (d_A0 + Dth_A theta) (S_A: 1 on SOFT
 * rows), u = -M_A' lambda, outputs x = Rout u + x0 + Xth theta.  Stored per region: the output law, the law of the
 * active SOFT rows' multipliers (their slack rho * sum lambda^2 against primal_tol decides exit flag 2 vs 1), and the
 * halfspaces a . theta <= b: both finite bounds of every inactive non-IMMUTABLE row, the dual sign of every active
 * non-IMMUTABLE row (upper >= 0, lower <= 0), optionally the box lb <= theta <= ub.  Rows with a zero theta part that
 * always hold are dropped; nothing else is (no LP redundancy removal).  A singular reduced system (pivot < zero_tol)
 * drops the region.  A point-location tree is grown on the labelled sample (splits: halfspace rows of the most frequent
 * regions at a node, scored by the larger child candidate set); the tree is approximate, the leaf check is exact.
 * The sample certifies nothing: regions it did not hit, or dropped for capacity, are not in the table, and their
 * points go to the implicit solve.  Refused with LMPC_ERR_UNSUPPORTED: BINARY rows, is_avi handles, proximal-point
 * handles, nth > LMPC_EXPLICIT_MAX_NTH.  Binary64 only.
 *
 * Evaluation: one point per lane -- tree walk, the leaf's candidates in frequency order, the law with explicit fmas.
 * A point is UNLOCATED (region -1) when no candidate holds it, or when its soft slack lies within soft_band *
 * primal_tol of primal_tol.  lmpc_explicit_eval_device then solves the unlocated points with the handle's own
 * implicit path (lmpc_solve_batch_device) on the same stream and writes their x / exitflag at their indices: it
 * SYNCHRONISES `stream` once to read how many there are (one 4-byte copy), then enqueues a gather, the solve and a
 * scatter, and returns without waiting for those.  Infeasible points always end there.  The same answers as
 * lmpc_solve_batch_device wherever the located region is the solver's final active set (up to rounding), within the
 * solver's own primal_tol band elsewhere; fallback points are the implicit results bit for bit.
 */
#define LMPC_EXPLICIT_MAX_NTH 32
#define LMPC_EXPLICIT_INFO 12
typedef struct lmpc_explicit lmpc_explicit;
typedef struct lmpc_explicit_opts {
    int32_t max_regions;     /* 4096: regions kept, most frequent first */
    int32_t leaf_size;       /* 8: a node with this many candidate regions or fewer is a leaf */
    int32_t max_depth;       /* 24: 0 = one leaf, a frequency-ordered scan of every region */
    int32_t split_regions;   /* 4: a node tries the halfspace rows of its this many most frequent regions as splits */
    int32_t split_rows;      /* 96: ... at most this many rows */
    int32_t score_points;    /* 65536: training points a node scores its candidate splits on (evenly strided subset) */
    int64_t max_bytes;       /* 256 MiB: cap on the region table (region records, halfspace rows, laws, soft rows; the
                              * tree's nodes and leaf lists come on top); regions beyond it are dropped like those beyond
                              * max_regions */
    double soft_band;        /* 0.1: relative band around primal_tol in which the soft slack leaves a point unlocated */
    const double *box_lb;    /* NULL, or nth lower bounds of theta: adds lb <= theta <= ub to every region */
    const double *box_ub;
} lmpc_explicit_opts;
void lmpc_explicit_default_opts(lmpc_explicit_opts *o);

/* Host-only build from an LDP pack (row-major, as lmpc_setup_ldp takes it) and its settings (NULL = defaults), no
 * GPU.  theta: N records of nth doubles (not read when nth == 0); active: N records of (2m + 63) / 64 words (the
 * solver's masks); exitflag: N int32.  is_avi != 0 states that the pack is a variational problem's (refused).
 * *out is NULL on failure; lmpc_last_error(NULL) has the text.  Such a controller can be inspected and evaluated
 * on the host (lmpc_explicit_locate_host), not on a GPU. */
int lmpc_explicit_build_ldp(lmpc_explicit **out, int n, int m, int ms, int nth, int nout,
                            const double *M, const double *du, const double *dl, const double *Dth,
                            const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                            const lmpc_settings *s, int is_avi, int64_t N, const double *theta,
                            const uint64_t *active, const int32_t *exitflag, const lmpc_explicit_opts *opts);
/* The same build from the handle's own pack and settings (HOST arrays), then one upload of the table to the
 * handle's GPU.  The controller keeps using `h` for its fallback: free it before the handle. */
int lmpc_explicit_build(lmpc_explicit **out, lmpc_handle *h, int64_t N, const double *theta, const uint64_t *active,
                        const int32_t *exitflag, const lmpc_explicit_opts *opts);
/* out[LMPC_EXPLICIT_INFO]: regions kept, dropped for capacity (max_regions / max_bytes), dropped as singular,
 * halfspace rows in total, tree nodes, tree depth, leaves, largest leaf, table bytes, training points in kept
 * regions, distinct optimal active sets in the sample, SOFT multiplier rows in total. */
int lmpc_explicit_info(const lmpc_explicit *e, int64_t *out);
/* Region r: output law F[nout*nth] (row-major) and g[nout]; halfspaces A[rows*nth], b[rows]; its mask[words] and
 * training count.  *nrows = the region's halfspace rows (call with A == NULL first to size A, b); any output may be
 * NULL. */
int lmpc_explicit_region(const lmpc_explicit *e, int32_t r, double *F, double *g, double *A, double *b,
                         int32_t *nrows, uint64_t *mask, int64_t *count);
/* The serialised table (layout: csrc/lmpc_explicit_kernel.hpp); *bytes = its size, out == NULL: size only. */
int lmpc_explicit_blob(const lmpc_explicit *e, void *out, int64_t *bytes);
/* Per training point: its region (-1: failed, or in a dropped region) and the tree leaf (node index) the build
 * sent it to (-1 if unlabelled).  Either may be NULL. */
int lmpc_explicit_training(const lmpc_explicit *e, int32_t *label, int32_t *leaf);
/* The kernel's evaluation on the host, same arithmetic: region[N] (-1 unlocated), and where located x[N*nout] and
 * exitflag[N] (unlocated points: exitflag 0, x left as it is); rows_checked[N] = tree nodes + halfspace rows
 * evaluated.  Any output but region may be NULL.  No fallback. */
int lmpc_explicit_locate_host(const lmpc_explicit *e, int64_t N, const double *theta, double *x, int32_t *exitflag,
                              int32_t *region, int32_t *rows_checked);
/* DEVICE pointers on the handle's GPU (see above for the one synchronisation); region may be NULL.  The fallback's
 * gather / solve / scatter are still enqueued when the call returns and use the controller's own scratch, and the
 * implicit solve uses the handle's: one controller serves one stream at a time, and a call on another stream (or the
 * handle's other entry points) must wait until that stream has finished the previous call. */
int lmpc_explicit_eval_device(lmpc_explicit *e, int64_t N, const double *theta, double *x, int32_t *exitflag,
                              int32_t *region, void *stream);
/* HOST pointers; synchronous. */
int lmpc_explicit_eval(lmpc_explicit *e, int64_t N, const double *theta, double *x, int32_t *exitflag, int32_t *region);
const char *lmpc_explicit_last_error(const lmpc_explicit *e);
void lmpc_explicit_free(lmpc_explicit *e);

/*
 * The scenario loop: the closed loop of the reference's Simulation (src/simulation.jl:37-116) for N independent
 * scenarios, WITH what lmpc_simulate* leaves out -- a disturbance trajectory d acting on the plant (Gd) and on the
 * measurement (Dd), an affine-parameter trajectory p, plant and measurement offsets, optional additive measurement
 * noise, the generated state observer in the loop, the outputs y / ym / xhat / d next to x / u, and the running cost and
 * worst constraint violation of every scenario (evaluate_cost / constraint_violation, src/utils.jl:397-425).
 * Lock-step, shaped like lmpc_simulate_ref_device: per time step a PRE kernel, the handle's batched solve, a POST
 * kernel, all enqueued on `stream`; no host synchronisation inside (the once-per-handle probe that
 * lmpc_solve_batch_device documents is the one exception, as everywhere).  Binary64.  Every handle the plain solve
 * accepts works (is_avi, hybrid / branch and bound, proximal-point), because the solve is the handle's own.  The
 * scenario-asynchronous machinery ("sim_async", run-ahead, "sim_keep_factor") does not apply to this loop.  The
 * offset-free observer runs in a loop of its own, lmpc_simulate_scenario_offset_free_device below, which takes the same
 * descriptor.
 *
 * Step k (0-based), per scenario:
 *   PRE   d_k = column k of d;  ym_j = h_offset_j + sum_i C_ji x_i + sum_q Dd_jq d_q (+ noise_j of column k), summed in
 *         exactly that order with separate multiply and add;  y_j = sum_i C_ji x_i + sum_q Dd_jq d_q (from 0, same
 *         order) with an observer -- simulation.jl:95 -- and y = ym without one;
 *         xhat <- mpc_correct_state(xhat, ym, d_k) with the handle's lmpc_set_observer arrays, the arithmetic of
 *         lmpc_correct_state_device bit for bit; without an observer xhat = x;
 *         theta = [xhat; r-block; d-block; uprev; p-block]:  r column k, or columns k+1 .. k+H with r.H > 0;  d and p
 *         column k, or columns k .. k+H-1 (simulation.jl:101-104); columns past the end repeat the last one.
 *   solve u = the handle's solve of theta (nout == nu); warm != 0: from the previous step's final working set (the first
 *         step cold), as lmpc_simulate_ref_device does.
 *   POST  running cost and violation on (x_k, u_k), see lmpc_sim_cost;  xhat <- mpc_predict_state(xhat, u, d_k), the
 *         arithmetic of lmpc_predict_state_device bit for bit;  x <- f_offset + F x + G u + Gd d_k by the SAME row sums
 *         on `plant`, so that one plant step equals lmpc_predict_state_device called with the plant's array;
 *         uprev <- u; trajectories; flag_min.
 * Consequence of the unfused plant step: with no d, no offsets and no observer this loop is NOT bit-identical to
 * lmpc_simulate_ref_device, whose plant step is a chain of fused multiply-adds.
 *
 * The blocks' k0 is ignored (the loop sets it).  d.w is nd (or 0: d_k = 0 and no d block in theta), noise.w is ny (or
 * 0: none; noise.H must be 0), p.w the base parameter count, r.w the reference's width.  A block with src == NULL and
 * w > 0 gives zeros.  Output trajectories are step-major like U_traj: Y_traj / Ym_traj T x N x ny, Xhat_traj T x N x nx
 * (the corrected estimate the controller saw), D_traj T x N x nd.
 */
typedef struct lmpc_sim_cost {
    int32_t ny;                          /* rows of C = length of the reference column the cost reads            */
    int32_t nc;                          /* constraint rows                                                      */
    const double *C, *Q, *R, *Rr, *S;    /* HOST, dense row-major: C ny x nx, Q ny x ny, R and Rr nu x nu, S nx x nu;
                                          * NULL = zero (the term is left out)                                   */
    const double *Ax, *Au, *lb, *ub;     /* HOST, dense row-major: Ax nc x nx, Au nc x nu (NULL = zero), lb, ub nc */
} lmpc_sim_cost;
/* Cost (evaluate_cost, utils.jl:397-411):  0.5 * sum_k [ e_k'Q e_k + u_k'R u_k + du_k'Rr du_k + x_k'S u_k ],
 * e_k = C x_k - r_k (r_k = column k of r, held at its last column; zeros without r), du_k = u_k - u_{k-1} with
 * u_{-1} = 0 whatever uprev holds (diff([zeros(nu) us])), x_k the state BEFORE step k's move.  Order of summation, the
 * same in the loop and in lmpc_evaluate_cost_device: a form a'M b is sum_j a_j * (sum_l M_jl b_l), inner and outer sums
 * from 0 in index order; (C x)_j from 0 in index order, then minus r_j; a step's four terms are added to 0 in the order
 * written; the steps' values are added to 0 in the order k = 0, 1, ...; the product with 0.5 comes last.  Separate
 * multiply and add throughout.
 * Violation (constraint_violation, utils.jl:417-425): rows lb <= Ax x_k + Au u_k <= ub; v_j = sum Ax_ji x_i, then
 * + sum Au_jl u_l (from 0, index order); per step max over j of max(lb_j - v_j, v_j - ub_j, 0); the loop keeps the
 * maximum over the steps.  Both bit for bit what the stand-alone functions below give on the stored X_traj / U_traj. */
typedef struct lmpc_scenario_sim {
    int32_t nx, nu, nd, ny;              /* plant dimensions; nd = model.nd (ONE column of d); nx <= 32, nd, ny <= 32 */
    const double *plant;                 /* HOST, nx rows [f_offset_i, F_i(nx), G_i(nu), Gd_i(nd)]: the TRUE plant, in
                                          * the MPC_PLANT_DYNAMICS layout of lmpc_observer                        */
    const double *measurement;           /* HOST, ny rows [h_offset_j, C_j(nx), Dd_j(nd)], or NULL with ny == 0  */
    lmpc_block r, d, p, noise;           /* DEVICE trajectories (per scenario or shared), H > 0 = preview        */
    int32_t nuprev, use_observer, warm;  /* use_observer != 0: the handle's lmpc_set_observer arrays run in the loop */
    double *Y_traj, *Ym_traj, *Xhat_traj, *D_traj;   /* DEVICE, optional outputs, or NULL                        */
    const lmpc_sim_cost *cost;           /* HOST, optional                                                       */
    double *cost_out, *violation_out;    /* DEVICE, N doubles each, or NULL                                      */
} lmpc_scenario_sim;
/* Host-only check of a descriptor against a handle's dimensions (no GPU touched): `observer` = the dimensions
 * lmpc_set_observer was given (arrays not read) or NULL = none set.  LMPC_OK, or LMPC_ERR_BADARG with a text in
 * lmpc_last_error(NULL) that names the offending field first: nx > 32, nu != nout, a negative width or preview length
 * ("d.w", "r.H", ...), d.w / noise.w that disagree with nd / ny, use_observer without an observer, an observer set with
 * other nx / nu / nd / ny than the descriptor, block widths that do not add up to nth ("nth"), outputs asked for
 * without their inputs.  lmpc_simulate_scenario* runs the same check first, with the handle's own dimensions. */
int lmpc_scenario_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s);
/*   x      N records of nx: in = initial TRUE states, out = states after T steps
 *   xhat   N records of nx, in/out: the observer's state; NULL = it starts at x (set_state!, simulation.jl:92) and is
 *          kept in the handle's scratch; must be NULL without use_observer
 *   uprev  N records of nuprev, in/out (NULL allowed when nuprev == 0)
 *   U_traj T x N x nu, X_traj (T+1) x N x nx, flag_min N: as lmpc_simulate_device, any may be NULL
 * lmpc_simulate_scenario_device: DEVICE pointers except where marked HOST; asynchronous on `stream` (the HOST arrays
 * are read before the call returns).  lmpc_simulate_scenario: the same call with every DEVICE array (the blocks'
 * sources and the descriptor's outputs included) given as a HOST array; synchronous; uprev NULL = zeros. */
int lmpc_simulate_scenario_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                  double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, void *stream);
int lmpc_simulate_scenario(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                           double *uprev, double *U_traj, double *X_traj, int32_t *flag_min);
/*
 * The scenario loop with the reference's OFFSET-FREE observer (set_offset_free_observer!, src/setup.jl:392-487,
 * src/observer.jl:13-122, 203-225): a Kalman filter on the state augmented with n_offset_free constant disturbance
 * channels, whose estimate is fed into the controller's d block -- the closed loop of lmpc_correct_state_device ->
 * lmpc_compute_control_observer_device -> lmpc_predict_state_device, plus the true plant, in one call and with a
 * disturbance preview.  Dimensions: nx = plant and controller state; s->nd = ndm, the MEASURED disturbances (the
 * plant's Gd / Dd and the trajectory d have ndm rows); ndo = n_offset_free; na = nx + ndo = the observer's state; the
 * controller's model.nd = ndm + ndo.  The handle's lmpc_set_observer arrays are those of the AUGMENTED filter:
 * n_state = na, n_control = nu, n_disturbance = ndm, n_measurement = ny.
 *
 * Step k (0-based), per scenario; everything not said here is the loop above, sum for sum:
 *   PRE   ym, y from the TRUE state (nx wide) and d_k (ndm wide) through `measurement`, as above;
 *         xaug <- mpc_correct_state(xaug, ym, d_k) on the augmented arrays: lmpc_correct_state_device on this handle,
 *         bit for bit;  xhat = xaug[0:nx], dhat = xaug[nx:na], both read AFTER the correction (observer.jl:119-122);
 *         theta = [xhat; r-block; d-block; uprev; p-block];  the d-block is max(d.H, 1) columns of width ndm + ndo,
 *         column c = [d column k + c, held at the last; dhat]: the measured rows first, dhat repeated in every column
 *         (get_control_disturbance, observer.jl:203-222; format_disturbance, utils.jl:155-205).  d.w == 0 (no
 *         trajectory, or ndm == 0): the measured rows are zeros (absent with ndm == 0), dhat is repeated all the same.
 *   solve as above.
 *   POST  cost and violation on the TRUE (x_k, u_k);  xaug <- mpc_predict_state(xaug, u, d_k) on the augmented arrays
 *         (lmpc_predict_state_device bit for bit);  x <- the row sums of `plant` (nx rows of 1 + nx + nu + ndm);  uprev
 *         <- u, trajectories, flag_min last.
 *   xaug  N records of na, in/out; NULL = it starts at [x; 0] (set_state!, observer.jl:74-90) in the handle's scratch.
 * Outputs: Xhat_traj T x N x nx = the first nx entries of the corrected estimate, D_traj T x N x ndm, and Dhat_traj
 * T x N x ndo (DEVICE, or NULL) = the disturbance estimate the controller saw.  na <= 8: kernels with both counts at
 * compile time; larger, up to na = 32: run-time loops.
 * Refused (LMPC_ERR_BADARG, the field's name first, before the GPU is touched): of NULL, n_offset_free <= 0,
 * nx + n_offset_free > 32, use_observer == 0, no observer set or one set with other dimensions than (nx + ndo, nu, nd,
 * ny), d.w neither 0 nor nd, widths with nx + width(r) + (nd + n_offset_free) * max(d.H, 1) + nuprev + width(p) != nth,
 * xaug given to a handle without an observer, and all that lmpc_scenario_check refuses.
 * lmpc_scenario_offset_free_check asks that without a handle.  lmpc_simulate_scenario_offset_free: the HOST twin
 * (Dhat_traj HOST as well).  The explicit controller's loop (lmpc_explicit_simulate_scenario*) is NOT extended: given a
 * descriptor of this kind it refuses through its own dimension check ("nth").
 */
typedef struct lmpc_offset_free {
    int32_t n_offset_free;               /* ndo: estimated disturbance channels                                   */
    double *Dhat_traj;                   /* T x N x ndo, optional output, or NULL                                 */
} lmpc_offset_free;
int lmpc_scenario_offset_free_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s,
                                    const lmpc_offset_free *of);
int lmpc_simulate_scenario_offset_free_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                              const lmpc_offset_free *of, double *x, double *xaug, double *uprev,
                                              double *U_traj, double *X_traj, int32_t *flag_min, void *stream);
int lmpc_simulate_scenario_offset_free(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                       const lmpc_offset_free *of, double *x, double *xaug, double *uprev, double *U_traj,
                                       double *X_traj, int32_t *flag_min);
/*
 * The scenario loop UNDER UNCERTAINTY: what the reference's users put into the plant hook of its Simulation
 * (`Simulation(dynamics, mpc)`, `scenario.dynamics`, src/simulation.jl:40,110,118-126) wherever its manual, examples and
 * tests use it -- additive process noise on the state (docs/src/manual/robust.md:17,78, example/robust.jl:5,25,
 * example/observer.jl:11) and a plant that is not the controller's model (test/runtests.jl:992,1081) -- for N scenarios
 * in one call, with the draws made on the device.  A side struct next to the unchanged lmpc_scenario_sim.
 *
 * Step k (0-based), per scenario i; everything not said here is lmpc_simulate_scenario_device, sum for sum:
 *   PRE   ym as there; then ym_j <- ym_j + v_j as the LAST addition (the place s->noise has, with which `measurement`
 *         is exclusive).
 *   POST  cost, violation and the observer's predict as there: the observer predicts with the handle's model and sees
 *         no w.  x <- the row sums of THIS SCENARIO's plant array; then for each row a, onto the finished row sum and in
 *         index order, x_a <- x_a + Gw_a0 * e_0 + Gw_a1 * e_1 + ... with separate multiply and add (Gw == NULL:
 *         x_a <- x_a + e_a).
 *   W_traj T x N x nx (DEVICE, optional): row a holds 0 + Gw_a0 * e_0 + ... in the same order (Gw == NULL: e_a).
 * A source (process e_k with process.w components, measurement v_k with ny) is one of
 *   supplied  lo == NULL: column k of the block `src` (w rows, H must be 0, per scenario or shared, held at its last
 *             column; k counts from THIS call's first step); src.src == NULL gives zeros;
 *   drawn     lo, hi (HOST, w each): uniform in [lo_q, hi_q] from Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11;
 *             multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with
 *             key (seed & 0xffffffff, seed >> 32) and counter (g & 0xffffffff, g >> 32, step_offset + k,
 *             (stream << 16) | j), g = scenario_offset + i, stream 0 = process and 1 = measurement, j the PAIR index:
 *             components 2j and 2j + 1 come from the output words (0, 1) and (2, 3).  From a word pair (a, b):
 *             u = (double)(((uint64_t)a << 21) | (b >> 11)) * 2^-53, exact and in [0, 1);  e_q = min(hi_q, lo_q + u *
 *             span_q), span_q = hi_q - lo_q formed once on the host in binary64, one multiply and one add.
 * A draw depends on (seed, global scenario, global step, stream, component) and on nothing of the launch: a run split
 * over calls by scenario (scenario_offset) or by time (step_offset, with x / xhat / uprev carried over and the
 * trajectories shifted by the caller) reproduces the unsplit one bit for bit.
 * GAUSSIAN draws (dist == LMPC_NOISE_GAUSSIAN; example/observer.jl:11-12, test/runtests.jl:958,1082): lo holds the means
 * and hi the standard deviations (HOST, w each).  The same block, key and counter as above; one block gives the
 * standard normal PAIR (z_2j, z_2j+1) by Box-Muller, through stated operations alone -- never the device library's
 * log, sin, cos -- so that a host restates a draw bit for bit (a closed loop turns a last-bit difference into another
 * active set).  With (a, b, c, d) the block's words and unit(a, b) the u above:
 *   u1  = 1 - unit(a, b)                                   exact, a multiple of 2^-53 in (0, 1]
 *   u2  = unit(c, d)
 *   t   = TWO_PI * u2                                      one multiply
 *   rho = sqrt(-2 * log_(u1))                              one multiply; sqrt: THE correctly rounded binary64 root
 *   (sn, cs, m) of t as in sin_ / cos_ below (lmpc_plant_program), with their quadrant selection
 *   z_2j = rho * cos_(t),  z_2j+1 = rho * sin_(t)           an odd count uses half of the last pair
 *   e_q = mean_q + std_q * z_q                             separate multiply and add, NO clamp
 * log_(t), for t a multiple of 2^-53 in [2^-53, 1] (all that occurs), on the bits B of t (hi = B >> 32, 32 bits):
 *   hi = hi + 0x00095F62;  k = (hi >> 20) - 0x3FF;  hi = (hi & 0x000FFFFF) + 0x3FE6A09E
 *   m  = the binary64 with high word hi and the low word of B        (t = 2^k * m, m in [sqrt(2)/2, sqrt(2)); exact)
 *   f  = m - 1 (exact);  s = f / (2 + f);  z = s * s
 *   p  = L7; p = fma(p, z, L6); p = fma(p, z, L5); p = fma(p, z, L4); p = fma(p, z, L3); p = fma(p, z, L2);
 *   p  = fma(p, z, L1);  R = p * z;  hf = (0.5 * f) * f;  dk = (double)k
 *   lo = s * (hf + R) + dk * LN2_LO                        (multiply, add, multiply, add: nothing fused)
 *   log_ = dk * LN2_HI - ((hf - lo) - f)                   (dk * LN2_HI is exact)
 * with (hexadecimal binary64)
 *   TWO_PI 0x401921FB54442D18   LN2_HI 0x3FE62E42FEE00000   LN2_LO 0x3DEA39EF35793C76
 *   L1 0x3FE5555555555593  L2 0x3FD999999997FA04  L3 0x3FD2492494229359  L4 0x3FCC71C51D8E78AF  L5 0x3FC7466496CB03DE
 *   L6 0x3FC39A09D078C69F  L7 0x3FC2F112DF3E5244
 * (the classic kernel on [sqrt(2)/2, sqrt(2)), its polynomial by Horner in z).  log_(1) is exactly +0.  Accuracy: below
 * 2 ulp against a correctly rounded logarithm on the stated domain.  |z| <= sqrt(106 ln 2) = 8.5717..., reached only by
 * u1 = 2^-53.  std_q == 0 gives the mean.  Correlated process noise goes through Gw (a Cholesky factor of the
 * covariance); measurement components are independent.
 * lmpc_noise_draw_host / lmpc_noise_draw_device return the e a DRAWN source (either dist) gives the loop, for N
 * scenarios from scenario_offset and T steps from step_offset, stream 0 = process or 1 = measurement: out[i * w * T +
 * k * w + q] -- laid out to be handed back as the per-scenario supplied block {src = out, stride = w * T, w, T}.  The
 * host one needs no GPU and no handle; the device one is one kernel, one (scenario, step) per lane, asynchronous on
 * hip_stream, out DEVICE.  Both refuse (LMPC_ERR_BADARG, text in lmpc_last_error(NULL) / (h)): noise NULL, what the
 * loop refuses of a source, a source without lo / hi, stream not 0 or 1, negative N, T or step_offset, step_offset + T
 * beyond 2^31 - 1, out NULL.
 * Plant ensemble: n_plants > 0 arrays in the layout of s->plant, one after the other (HOST), staged once per call;
 * scenario i steps array plant_index[i] (DEVICE, N entries), or (scenario_offset + i) mod n_plants with plant_index
 * NULL.  An entry is taken as UNSIGNED, modulo n_plants: no entry addresses outside the staged table.  n_plants == 0:
 * s->plant for every scenario.  The ensemble shares ONE measurement (s->measurement).
 * Every source absent and n_plants == 0 runs and is lmpc_simulate_scenario_device bit for bit.
 * Refused (LMPC_ERR_BADARG, the field's name first, before the GPU is touched): all that lmpc_scenario_check refuses; un
 * NULL; a negative w; dist neither 0 nor 1; with dist == 1: lo (the means) or hi (the standard deviations) NULL, a
 * non-finite mean, a standard deviation that is negative or not finite; lo without hi or the reverse; lo_q > hi_q or a
 * non-finite bound; src.H != 0; process.w not in
 * {0, nx} with Gw NULL; measurement.w not in {0, ny}; measurement.w > 0 with s->noise.w > 0; n_plants < 0; n_plants > 0
 * with plants NULL; plant_index with n_plants == 0; W_traj with process.w == 0; step_offset < 0, or step_offset + T
 * beyond 2^31 - 1 (the call alone knows T).  lmpc_scenario_uncertain_check asks that without a handle.
 * lmpc_simulate_scenario_uncertain: the HOST twin (the sources' blocks, plant_index and W_traj HOST as well).
 * NOT extended: the offset-free loop and the explicit controller's loop, for drawn noise of either distribution; and
 * the plant program gets no new opcode from this (opcode 17 stays unknown, there is no SQRT or LOG operation).
 */
#define LMPC_NOISE_UNIFORM 0
#define LMPC_NOISE_GAUSSIAN 1
typedef struct lmpc_noise {              /* one noise source                                                      */
    int32_t w;                           /* components; 0 = absent                                                */
    int32_t dist;                        /* LMPC_NOISE_UNIFORM (0, what a zeroed struct says) or LMPC_NOISE_GAUSSIAN;
                                          * in the four bytes that were padding: no size or offset moved           */
    lmpc_block src;                      /* DEVICE, supplied draws: w rows, column k at step k, H must be 0; read
                                          * when lo == NULL (src.src == NULL then gives zeros)                    */
    const double *lo, *hi;               /* HOST, w each: drawn on the device, uniform in [lo_q, hi_q]; both or none.
                                          * dist == LMPC_NOISE_GAUSSIAN: lo = the means, hi = the standard deviations */
} lmpc_noise;
typedef struct lmpc_uncertainty {
    lmpc_noise process;                  /* e_k, nw = process.w components                                        */
    const double *Gw;                    /* HOST nx x nw row-major: w_k = Gw e_k; NULL = identity, then nw == nx   */
    lmpc_noise measurement;              /* v_k, ny components, added to ym; exclusive with s->noise              */
    uint64_t seed;
    int64_t scenario_offset;             /* global index of scenario 0 of this call (sharded runs)                */
    int32_t step_offset;                 /* global index of step 0 of this call (continued runs)                  */
    int32_t n_plants;                    /* 0 = the descriptor's `plant` for every scenario                       */
    const double *plants;                /* HOST, n_plants arrays in the layout of s->plant, one after the other  */
    const int32_t *plant_index;          /* DEVICE, N entries, or NULL = (scenario_offset + i) mod n_plants       */
    double *W_traj;                      /* DEVICE T x N x nx, optional: the w_k that acted                       */
} lmpc_uncertainty;
int lmpc_scenario_uncertain_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s,
                                  const lmpc_uncertainty *un);
int lmpc_simulate_scenario_uncertain_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                            const lmpc_uncertainty *un, double *x, double *xhat, double *uprev,
                                            double *U_traj, double *X_traj, int32_t *flag_min, void *stream);
int lmpc_simulate_scenario_uncertain(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                     const lmpc_uncertainty *un, double *x, double *xhat, double *uprev, double *U_traj,
                                     double *X_traj, int32_t *flag_min);
int lmpc_noise_draw_host(const lmpc_noise *noise, uint64_t seed, int stream, int64_t scenario_offset, int64_t N,
                         int32_t step_offset, int T, double *out);
int lmpc_noise_draw_device(lmpc_handle *h, const lmpc_noise *noise, uint64_t seed, int stream, int64_t scenario_offset,
                           int64_t N, int32_t step_offset, int T, double *out, void *hip_stream);
/* Scoring of a stored run, one thread per scenario: X = the states x_0 .. x_{T-1}, step-major (the first T slices of an
 * X_traj), U = T x N x nu as U_traj.  r: the reference trajectory as in the loop (column k at step k; NULL = zeros).
 * cost_out: N doubles.  violation_out: N doubles (maximum over the steps) and / or violation_steps: T x N, the
 * per-step values the reference's constraint_violation(c, xs, us) returns.  DEVICE arrays, asynchronous on `stream`.
 * lmpc_evaluate_cost_device reads the weights of `cost`, lmpc_constraint_violation_device the rows of `rows`. */
int lmpc_evaluate_cost_device(lmpc_handle *h, int64_t N, int T, int nx, int nu, const lmpc_sim_cost *cost, const double *X,
                              const double *U, const lmpc_block *r, double *cost_out, void *stream);
int lmpc_constraint_violation_device(lmpc_handle *h, int64_t N, int T, int nx, int nu, const lmpc_sim_cost *rows,
                                     const double *X, const double *U, double *violation_out, double *violation_steps,
                                     void *stream);

/*
 * Scenario loop with an explicit controller: the loop above with compute_control(empc, x) (reference src/utils.jl:53-60)
 * in place of the solve -- Simulation(empc, scenario) of src/simulation.jl:37.  A step whose theta lies in a kept region
 * takes that region's law and flag 1 / 2 (lmpc_explicit_eval_device's rule); every other step is solved COLD by the
 * controller's handle, so that step's numbers are those of lmpc_simulate_scenario_device with warm == 0.  PRE and POST
 * arithmetic are those of the loop above, bit for bit; the observer is the one lmpc_set_observer put on that handle.
 *   mode 1  run-ahead: one kernel runs every scenario forward through the steps it can locate (no launch and no theta
 *           record in memory per located step); the scenarios it could not locate wait in a dense batch, which the
 *           handle solves; the kernel resumes them through the list; at most T + 1 launches of that kernel (T
 *           solves), one stream synchronisation (the count of waiting scenarios) per launch.
 *   mode 0  lock-step, from the older entry points' kernels alone: per step the PRE kernel, lmpc_explicit_eval_device
 *           on the formed theta, the POST kernel; one synchronisation per step.  Same numbers.
 * region_traj  T x N (step-major) or NULL: the region of every scenario-step, -1 = solved by the handle.
 * stats        HOST, 4 values or NULL: launches of the run-ahead kernel (all located: 1; every step solved by the
 *              handle: T + 1; mode 0: the steps), scenario-steps solved by the handle, scenario-steps located, largest
 *              batch handed to the handle.
 * Refused (LMPC_ERR_BADARG, text in lmpc_explicit_last_error, the field's name first, before the GPU is touched): all
 * that lmpc_scenario_check refuses, warm != 0, nth > LMPC_EXPLICIT_MAX_NTH, a controller built without a handle, a
 * mode other than 0 / 1.  lmpc_explicit_scenario_check asks the descriptor's part of that without a controller (text
 * in lmpc_last_error(NULL)).  Scratch lives in the controller and is freed with it: one controller serves one
 * stream at a time.  Other arguments as lmpc_simulate_scenario_device / lmpc_simulate_scenario (HOST twin).
 */
int lmpc_explicit_scenario_check(int nth, int nout, const lmpc_observer *observer, const lmpc_scenario_sim *s, int mode);
int lmpc_explicit_simulate_scenario_device(lmpc_explicit *e, int64_t N, int T, const lmpc_scenario_sim *s, double *x,
                                           double *xhat, double *uprev, double *U_traj, double *X_traj, int32_t *flag_min,
                                           int32_t *region_traj, int mode, int64_t *stats, void *stream);
int lmpc_explicit_simulate_scenario(lmpc_explicit *e, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                    double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, int32_t *region_traj,
                                    int mode, int64_t *stats);

/*
 * A NONLINEAR TRUE PLANT in the scenario loop: the reference's Simulation steps mpc.model.true_dynamics
 * (src/simulation.jl:40,110,126), which for Model(f, h, xo, uo, Ts) is x + Ts * f(x, u, d) (src/model.jl:87,114-118).
 * Here the plant is a straight-line PROGRAM -- data, not code -- that one kernel interprets, one scenario per lane.
 *
 * Inputs of the program: x (nx <= 32), u (nu <= 64), d (nd <= 32: column k of the descriptor's d block) and q (nq <= 32
 * plant parameters: N x nq on the device, one row per scenario, or nq values shared by all).  The program has a table
 * of n_consts binary64 constants, n_ins instructions over a file of n_slots binary64 slots, and out_slot[nx]: slot
 * out_slot[a] holds x+_a after the last instruction.  An instruction is five int32: op, dst, a, b, c.
 *   op  name     dst <-                              operands
 *    1  LOADX    x[a]                                a < nx
 *    2  LOADU    u[a]                                a < nu
 *    3  LOADD    d[a]                                a < nd
 *    4  LOADQ    q[a]                                a < nq
 *    5  CONST    consts[a]                           a < n_consts
 *    6  ADD      s[a] + s[b]                         a, b slots written earlier (likewise below)
 *    7  SUB      s[a] - s[b]
 *    8  MUL      s[a] * s[b]
 *    9  DIV      s[a] / s[b]
 *   10  NEG      -s[a]                               (the sign bit flipped)
 *   11  ABS      |s[a]|                              (the sign bit cleared)
 *   12  FMA      fma(s[a], s[b], s[c])               one rounding
 *   13  MIN      s[a] < s[b] ? s[a] : s[b]           (so MIN(NaN, t) = t, MIN(t, NaN) = NaN, MIN(-0, +0) = +0)
 *   14  MAX      s[a] > s[b] ? s[a] : s[b]
 *   15  SIN      sin_(s[a])
 *   16  COS      cos_(s[a])
 * Unused operand fields must be 0.  Every operation is ONE IEEE-754 binary64 operation, round to nearest even, nothing
 * fused that is not written as fma; SQRT, EXP, TANH, comparisons and selects are not operations of this version.
 * sin_ / cos_ are NOT the device library's: they are this sequence, which a host restates bit for bit.
 *   kd = rint(t * TWO_OVER_PI)                                      (one multiply; rint: to nearest, ties to even)
 *   r  = fma(-kd, P1, t);  r = fma(-kd, P2, r);  r = fma(-kd, P3, r)      (Cody-Waite, three constants)
 *   z  = r * r
 *   ps = S6; ps = fma(ps, z, S5); ps = fma(ps, z, S4); ps = fma(ps, z, S3); ps = fma(ps, z, S2); ps = fma(ps, z, S1)
 *   sn = fma(r * z, ps, r)
 *   pc = C6; pc = fma(pc, z, C5); pc = fma(pc, z, C4); pc = fma(pc, z, C3); pc = fma(pc, z, C2); pc = fma(pc, z, C1)
 *   hz = 0.5 * z;  w = 1 - hz;  cs = w + fma(z * z, pc, (1 - w) - hz)
 *   m  = kd - 4 * rint(0.25 * kd)                  (exact; m in {-2, -1, 0, 1, 2}: k & 3 with 3 as -1 and 2 as +-2)
 *   sin_: m == 0: sn;  m == 1: cs;  m == -1: -cs;  otherwise -sn
 *   cos_: m == 0: cs;  m == 1: -sn; m == -1: sn;   otherwise -cs
 * with (hexadecimal binary64)
 *   TWO_OVER_PI 0x3FE45F306DC9C883
 *   P1 0x3FF921FB54400000 (33 bits of pi/2)   P2 0x3DD0B4611A600000 (the next 33)   P3 0x3BA3198A2E037073 (pi/2 - P1 - P2)
 *   S1 0xBFC5555555555549  S2 0x3F8111111110F8A6  S3 0xBF2A01A019C161D5  S4 0x3EC71DE357B1FE7D  S5 0xBE5AE5E68A2B9CEB
 *   S6 0x3DE5D93A5ACFD57C
 *   C1 0x3FA555555555554C  C2 0xBF56C16C16C15177  C3 0x3EFA01A019CB1590  C4 0xBE927E4F809C52AD  C5 0x3E21EE9EBDB4B1C4
 *   C6 0xBDA8FAE9BE8838D4
 * (the polynomials of the classic kernels on [-pi/4, pi/4]).  Both polynomials are always evaluated.  Accuracy (below
 * 2 ulp against a correctly rounded result) is claimed for |t| <= 2^20 ONLY.  Beyond that the same operations run
 * unchanged: the result is defined and restated but carries no accuracy (r leaves [-pi/4, pi/4]; for |kd| >= 2^54, m
 * is 0).  t = +-inf or NaN gives NaN (r is NaN).  t = -0 gives sin_ = +0.
 * Caps: n_ins <= LMPC_PLANT_MAX_INS, n_slots <= LMPC_PLANT_MAX_SLOTS, n_consts <= LMPC_PLANT_MAX_CONSTS.
 *
 * lmpc_plant_program_check (HOST only; every entry point below runs it first): LMPC_OK, or LMPC_ERR_BADARG with the
 * field's name first in lmpc_last_error(NULL): prog NULL; nx not in 1 .. 32, nu not in 0 .. 64, nd or nq not in 0 .. 32;
 * a count beyond its cap or negative, n_slots < 1; a NULL array with a non-zero count; an unknown op; dst not a slot; an
 * input or constant index out of range; a slot operand out of range or read before an instruction wrote it; a non-zero
 * unused field; an out_slot entry out of range or never written.  A program that passes reads and writes nothing
 * outside its n_slots slots, its constants and the nx / nu / nd / nq inputs it declares.
 * lmpc_plant_program_eval_host: xnext[i, :] = program(x[i, :], u[i, :], d[i, :], q) for i < N on the CPU, HOST arrays
 * (N x nx, N x nu, N x nd, N x nq or nq with q_shared != 0; an array whose width is 0 may be NULL).  Needs no GPU.
 * lmpc_plant_program_eval_device: the same on the handle's GPU with DEVICE arrays, one kernel, asynchronous on `stream`;
 * the program itself (HOST) is staged by the call.  The two execute the same source and agree bit for bit (a NaN
 * result's sign and payload excepted).
 * lmpc_simulate_scenario_nonlinear_device: lmpc_simulate_scenario_uncertain_device with the plant's row sums replaced by
 * the program.  PRE is that loop's (the measurement stays the linear s->measurement, the reference's default
 * get_measurement, simulation.jl:45-50).  POST: cost, violation and the observer's predict (with the handle's LINEAR
 * model) as there; x+ = the program on (x, u_k, d_k, q_i); then the process noise onto the finished x+ as there.
 * un may be NULL (no noise); s->plant is ignored and may be NULL; un->n_plants > 0 is refused (q takes its place: DEVICE,
 * N x nq, or nq values with q_shared != 0; NULL with nq == 0); prog->nx / nu / nd must equal s->nx / nu / nd.
 * Everything lmpc_scenario_uncertain_check refuses is refused here too.  lmpc_simulate_scenario_nonlinear: the HOST
 * twin (q HOST as well).  NOT extended: the offset-free loop, the explicit controller's loop, a nonlinear measurement.
 */
#define LMPC_PLANT_MAX_INS 1024
#define LMPC_PLANT_MAX_SLOTS 64
#define LMPC_PLANT_MAX_CONSTS 256
#define LMPC_PLANT_LOADX 1
#define LMPC_PLANT_LOADU 2
#define LMPC_PLANT_LOADD 3
#define LMPC_PLANT_LOADQ 4
#define LMPC_PLANT_CONST 5
#define LMPC_PLANT_ADD 6
#define LMPC_PLANT_SUB 7
#define LMPC_PLANT_MUL 8
#define LMPC_PLANT_DIV 9
#define LMPC_PLANT_NEG 10
#define LMPC_PLANT_ABS 11
#define LMPC_PLANT_FMA 12
#define LMPC_PLANT_MIN 13
#define LMPC_PLANT_MAX 14
#define LMPC_PLANT_SIN 15
#define LMPC_PLANT_COS 16
typedef struct lmpc_plant_program {
    int32_t nx, nu, nd, nq;              /* widths of the inputs                                                  */
    int32_t n_slots, n_consts, n_ins;
    const double *consts;                /* HOST, n_consts                                                        */
    const int32_t *ins;                  /* HOST, n_ins x 5: op, dst, a, b, c                                     */
    const int32_t *out_slot;             /* HOST, nx: the slots that hold x+ after the last instruction           */
} lmpc_plant_program;
int lmpc_plant_program_check(const lmpc_plant_program *prog);
int lmpc_plant_program_eval_host(const lmpc_plant_program *prog, int64_t N, const double *x, const double *u, const double *d,
                                 const double *q, int q_shared, double *xnext);
int lmpc_plant_program_eval_device(lmpc_handle *h, const lmpc_plant_program *prog, int64_t N, const double *x, const double *u,
                                   const double *d, const double *q, int q_shared, double *xnext, void *stream);
int lmpc_simulate_scenario_nonlinear_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                            const lmpc_uncertainty *un, const lmpc_plant_program *prog, const double *q,
                                            int q_shared, double *x, double *xhat, double *uprev, double *U_traj,
                                            double *X_traj, int32_t *flag_min, void *stream);
int lmpc_simulate_scenario_nonlinear(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un,
                                     const lmpc_plant_program *prog, const double *q, int q_shared, double *x, double *xhat,
                                     double *uprev, double *U_traj, double *X_traj, int32_t *flag_min);

/*
 * Differentiable solve: the derivative of the solution map x*(theta) per point, from the optimal active set the solve
 * returned (`active`, (2m + 63) / 64 words: bit j the upper side of row j, bit m + j the lower side) and its exit flag.
 * Neither theta nor x is needed.
 *
 * On a point with exit flag >= 1 and active rows A (the rows with either side bit set; a row with both bits counts
 * once; both sides share the row of M and of Dth, so the side does not matter) the map is affine:
 *     K_A = M_A M_A' + rho_soft S_A                            (S_A: 1 on the diagonal of SOFT rows)
 *     J   = dx/dtheta = Xth + Rout M_A' K_A^-1 Dth_A           (nout x nth)
 *     thbar = J' xbar = Xth' xbar + Dth_A' K_A^-1 (M_A Rout') xbar
 * Where the active set is degenerate the map has a kink; the result is then the derivative of the affine piece the
 * solver reported (the convention of OptNet and of differentiable MPC), not a subgradient chosen otherwise.
 *
 * Per-point status (status[N], may be NULL); every output row 0 .. N - 1 is always written:
 *      1  done: the result
 *      0  the point's exit flag is < 1: zeros
 *     -1  a pivot of K_A is below the handle's zero_tol (dependent active rows): zeros
 *     -7  |A| is beyond the 64 rows the kernels hold: zeros
 * (a failed point has status 0 whatever its mask; -7 is decided before the factorisation).
 *
 * Arithmetic contract (binary64; every multiply-add an explicit fma, nothing else fused; restated in numpy in
 * tests/sens_reference.py; the lane kernel, the wavefront kernel and the *_host functions give the same bits):
 *   - derived pack, kept on the device next to the constant pack from the first call on: P = M Rout' (m x nout),
 *     P[a][q] = the chain acc = fma(M[a][k], Rout[q][k], acc) from 0 over k = 0 .. n - 1; G the pack's packed triangle.
 *   - rows of A in ascending row index a_0 < a_1 < ...; K[i][j] = G[a_i][a_j], plus ONE addition of rho_soft on the
 *     diagonal entries of SOFT rows.
 *   - K = L D L' without pivoting in that order, column by column: for j, c_p = L[j][p] * D[p] (p < j); for i >= j
 *     v = K[i][j], then v = fma(-L[i][p], c_p, v) for p = 0 .. j - 1; D[j] = v (i = j; v < zero_tol: status -1),
 *     rD[j] = 1 / D[j], L[i][j] = v * rD[j] (i > j).
 *   - w_i = the chain acc = fma(P[a_i][q], xbar[q], acc) from 0 over q = 0 .. nout - 1.
 *   - forward: z_i = w_i, then z_i = fma(-L[i][p], z_p, z_i) for p = 0 .. i - 1; diagonal: z_i = z_i * rD[i];
 *     backward: y_i = z_i, then y_i = fma(-L[p][i], y_p, y_i) for p = |A| - 1 DOWN TO i + 1 (the order in which the
 *     y_p become available to a column-by-column substitution).
 *   - thbar[t] = one chain from 0: acc = fma(Xth[q][t], xbar[q], acc) over q ascending, then
 *     acc = fma(Dth[a_i][t], y_i, acc) over i ascending.
 *   - the Jacobian is the same computation on one factor with xbar = e_r for row r, the products with the exact zeros
 *     and the one of e_r left out (w_i = P[a_i][r], the output chain starts at Xth[r][t]): row r of J equals the VJP of
 *     e_r wherever values are compared (the sign of a zero may differ).
 * The K form loses digits with cond(K_A) (SOFT-heavy sets); that loss is accepted and measured.
 *
 * Device calls: DEVICE pointers on the handle's GPU; they only enqueue on `stream` (one 4-byte memset, the lane kernel,
 * and where a set can exceed its capacity the wavefront kernel over the work list, whose length is read on the device)
 * and never wait.  The first call builds the derived pack (one blocking upload) and allocates the work list for its N;
 * later calls of that size allocate nothing (lmpc_set_option "sens_reserve" 1 makes lmpc_reserve do both).  One
 * stream at a time per handle, as for the solve.  xbar: N x nout; thbar: N x nth; J: N x nout x nth, row-major.
 * Refused: BINARY rows, is_avi and proximal-point handles (LMPC_ERR_UNSUPPORTED); nth == 0 (LMPC_ERR_BADARG).
 * Binary64 only.  Options: "sens_cap" 0 / 5 / 8 (capacity of the lane kernel's register factor; 0 = 5 where a set of
 * the problem reaches at most 5 rows, else 8), "sens_force_list" 1 (every non-empty set goes to the wavefront kernel;
 * results identical).
 */
int lmpc_solve_vjp_device(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, const double *xbar,
                          double *thbar, int32_t *status, void *stream);
int lmpc_solve_jacobian_device(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, double *J,
                               int32_t *status, void *stream);
/* HOST pointers; synchronous (as lmpc_solve_batch is to lmpc_solve_batch_device). */
int lmpc_solve_vjp(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, const double *xbar, double *thbar,
                   int32_t *status);
int lmpc_solve_jacobian(lmpc_handle *h, int64_t N, const uint64_t *active, const int32_t *exitflag, double *J, int32_t *status);
/* The kernels' arithmetic on the CPU, no GPU and no handle: the raw LDP pack (row-major, as lmpc_explicit_build_ldp
 * takes it; du, dl, x0 are not read and may be NULL) and its settings (NULL = defaults; rho_soft and zero_tol are
 * used, eps_prox > 0 is refused).  Same results bit for bit; lmpc_last_error(NULL) has the text of a refusal. */
int lmpc_solve_vjp_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                        const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                        const lmpc_settings *s, int is_avi, int64_t N, const uint64_t *active, const int32_t *exitflag,
                        const double *xbar, double *thbar, int32_t *status);
int lmpc_solve_jacobian_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                             const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                             const lmpc_settings *s, int is_avi, int64_t N, const uint64_t *active, const int32_t *exitflag,
                             double *J, int32_t *status);
/* The handle's most recent derivative calls (at most four are kept), oldest first, LMPC_SENS_INFO_WORDS words each:
 * number of the call in the handle's life (from 1), 1 for the Jacobian / 0 for the VJP, CAP of the sens_lane_kernel
 * instantiation, the capacity it ran with (0: forced list pass), its grid, workgroup size, LDS bytes, what it staged in
 * LDS (bit 0: the derived pack, bit 1: its results, stored as whole lines), 1 if sens_wave_kernel was enqueued behind it,
 * that kernel's grid and LDS bytes, N.  Returns the number of records written (out holds max records). */
#define LMPC_SENS_INFO_WORDS 12
int lmpc_sens_launch_info(const lmpc_handle *h, int32_t *out, int max);

/*
 * Gradient with respect to the pack: what a cotangent xbar of the batch's solutions gives for the pack itself, SUMMED
 * over the N points -- one small gradient per handle.  With lmpc_transform_vjp behind it this is the derivative with
 * respect to the controller's data (H, f, f_theta, A, bu, bl, W, K).
 *
 * A point with exit flag >= 1 has active rows a_0 < a_1 < ... (as above) and sides u_i = 1 if the upper bit of row a_i
 * is set, else 0 (a row with both bits counts as upper).  Its solution is one affine piece of the pack:
 *     d_i = (u_i ? du : dl)[a_i] + Dth[a_i] . theta      lambda = K_A^-1 d      v = M_A' lambda
 *     x = x0 + Xth theta + Rout v
 * With y = K_A^-1 (M_A Rout') xbar (the y of the VJP above), w = M_A' y, vbar = Rout' xbar and g = vbar - w the point
 * contributes
 *     Mbar[a_i][c]   lambda_i g_c - y_i v_c            Routbar[q][c]  xbar_q v_c
 *     dubar[a_i]     y_i where u_i = 1                 x0bar[q]       xbar_q
 *     dlbar[a_i]     y_i where u_i = 0                 Xthbar[q][t]   xbar_q theta_t
 *     Dthbar[a_i][t] y_i theta_t
 * Status per point and thbar (N x nth; both may be NULL) are those of lmpc_solve_vjp_device on the same inputs, bit
 * for bit.  A point whose status is not 1 contributes +0.0 to every sum.
 *
 * Arithmetic contract (binary64; every multiply-add an explicit fma, nothing else fused; restated in numpy in
 * tests/pack_grad_reference.py; the lane path, the wavefront path, the host-pointer call and the *_host function give
 * the same values):
 *   - the derived pack, the factor, w_i (here the right-hand side of y), both substitutions and thbar are those of the
 *     contract above.
 *   - d_i is one chain: it starts at the side's bound, then acc = fma(Dth[a_i][t], theta[t], acc) for t ascending.
 *     lambda comes from d by the same forward, diagonal and backward order as y.
 *   - v_c, w_c, vbar_c are chains from 0: fma(M[a_i][c], lambda_i, acc) over i ascending, the same with y_i, and
 *     fma(Rout[q][c], xbar[q], acc) over q ascending; g_c = vbar_c - w_c.
 *   - the Mbar contribution is fma(lambda_i, g_c, -(y_i * v_c)); every other contribution is one product or a copy.
 *   - every output entry is the root of the balanced binary tree over the point indices 0 .. 2^ceil(log2 N) - 1: a leaf
 *     is the point's contribution, +0.0 for an absent index, a row outside the point's set or a status other than 1; a
 *     node is left + right.  Results are compared as values (the sign of a zero is free).  No atomic touches a double.
 *
 * Device call: DEVICE pointers; it only enqueues on `stream` and never waits.  The batch is processed in slabs of 2^s
 * points: per slab the lane kernel (and the wavefront kernel over the work list) leaves [lambda | y] per point, the
 * reduce kernel one partial per 64 points, and launches of the tree kernel the slab's sum; a last tree sums the slab
 * sums into the caller's arrays.  Scratch: one slab of records and partials plus one sum per slab, allocated by the
 * first call of a size (or by lmpc_reserve after lmpc_set_option "pack_grad_reserve" 1), released by
 * lmpc_release_scratch.  lmpc_set_option "pack_grad_slab" s (8 .. 20; 0 = the largest s whose records and partials stay
 * within 64 MiB).  Outputs row-major as lmpc_get_ldp lays the pack out (Mbar m x n, dubar m, dlbar m, Dthbar m x nth,
 * Routbar nout x n, x0bar nout, Xthbar nout x nth); any of them may be NULL, and with all of them NULL only stage 1 runs
 * (thbar and status at the VJP's cost).  theta: N x nth, xbar: N x nout.  As for the VJP, the first call on a handle also
 * uploads the constants it needs with one blocking copy (lmpc_reserve with "pack_grad_reserve" 1 does it ahead of time).
 * Refusals and options "sens_cap" / "sens_force_list" as for lmpc_solve_vjp_device.  Binary64 only.
 */
int lmpc_solve_pack_vjp_device(lmpc_handle *h, int64_t N, const double *theta, const uint64_t *active, const int32_t *exitflag,
                               const double *xbar, double *Mbar, double *dubar, double *dlbar, double *Dthbar, double *Routbar,
                               double *x0bar, double *Xthbar, double *thbar, int32_t *status, void *stream);
/* HOST pointers; synchronous. */
int lmpc_solve_pack_vjp(lmpc_handle *h, int64_t N, const double *theta, const uint64_t *active, const int32_t *exitflag,
                        const double *xbar, double *Mbar, double *dubar, double *dlbar, double *Dthbar, double *Routbar,
                        double *x0bar, double *Xthbar, double *thbar, int32_t *status);
/* The same arithmetic on the CPU, no GPU and no handle, from the raw LDP pack and settings as lmpc_solve_vjp_host takes
 * them (here du, dl are read wherever m > 0; x0 is not read and may be NULL). */
int lmpc_solve_pack_vjp_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                             const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                             const lmpc_settings *s, int is_avi, int64_t N, const double *theta, const uint64_t *active,
                             const int32_t *exitflag, const double *xbar, double *Mbar, double *dubar, double *dlbar,
                             double *Dthbar, double *Routbar, double *x0bar, double *Xthbar, double *thbar, int32_t *status);
/* The handle's most recent pack-gradient calls (at most four are kept), oldest first, LMPC_PACK_GRAD_INFO_WORDS words
 * each: number of the call (from 1), CAP of the pack_grad_lane_kernel instantiation, the capacity it ran with, its grid
 * on the first slab, its LDS bytes, what was staged in LDS (bit 0: the derived pack by the lane kernel, bit 1: M and
 * Rout by the reduce kernel), 1 if pack_grad_wave_kernel was enqueued, its grid, the reduce kernel's grid on the first
 * slab, its LDS bytes, log2 of the slab, the number of slabs, the tree kernel's launches in the call, the scratch in
 * KiB, the doubles of one partial, N, the column chunks of M the reduce kernel's grid was split into on the first slab
 * (its grid.y less one).  Without any output array the reduce and tree fields are 0. */
#define LMPC_PACK_GRAD_INFO_WORDS 17
int lmpc_pack_grad_launch_info(const lmpc_handle *h, int32_t *out, int max);
/* Host only: the adjoint of lmpc_transform.  Inputs as lmpc_transform (column-major H, f_theta, A, W, Kfb), then the
 * gradients with respect to its seven outputs (row-major as it writes them; a NULL one counts as zero), then the
 * gradients with respect to its inputs in the inputs' own layout (Hbar symmetric, as the transform reads (H + H') / 2;
 * any may be NULL).  Plain binary64, no bit contract.  Fails as lmpc_transform fails. */
int lmpc_transform_vjp(int n, int m, int ms, int nth, int nout, const double *H, const double *f, const double *f_theta,
                       const double *A, const double *bu, const double *bl, const double *W, const int32_t *sense,
                       const double *Kfb, int nx, const double *Mbar, const double *dubar, const double *dlbar,
                       const double *Dthbar, const double *Routbar, const double *x0bar, const double *Xthbar, double *Hbar,
                       double *fbar, double *fthbar, double *Abar, double *bubar, double *blbar, double *Wbar, double *Kfbbar);

/*
 * Scenario loop adjoint: the gradient of a run of lmpc_simulate_scenario_device with respect to its initial values and
 * its r / d / p trajectories.  Once a step's active set is known the step is affine in its inputs, so the adjoint of a
 * run is a backward sweep over the steps: one VJP of the differentiable solve per step (above) and one transposed glue
 * step.  A run is recorded by the TAPED forward call and differentiated by lmpc_scenario_vjp*, which reads only the tape
 * and the constants -- not theta, x or u.
 *
 * lmpc_simulate_scenario_taped_device: lmpc_simulate_scenario_device (the same PRE / POST kernels, the same loop, every
 * output the same bits) whose step k writes its solve's final working set and exit flags into slice k of the tape
 * (DEVICE arrays of the caller, step-major: active T x N x lmpc_active_words(h), flag T x N); with s->warm step k starts
 * from slice k - 1.  lmpc_simulate_scenario_taped: HOST arrays throughout, synchronous.
 *
 * The fields of lmpc_scenario_grad -- DEVICE arrays for lmpc_scenario_vjp_device, HOST arrays for the other two:
 *   Xbar       in   (T+1) x N x nx   cotangent of X_traj, NULL = zeros        Ubar  in  T x N x nu  cotangent of U_traj
 *   x0bar      out  N x nx           xhat0bar  out  N x nx: non-NULL exactly when the forward run was given an xhat
 *   uprev0bar  out  N x nuprev
 *   rbar, dbar, pbar  out, each optional: max(r.T, 1) x N x r.w (d, p alike; a block with T < 1 counts as one column, as
 *              in the forward), STEP-major -- column c of the trajectory is slice c -- and always per scenario, also for
 *              a shared source block (stride 0: the caller sums over scenarios)
 *   status_min out  N int32, optional: the smallest per-step VJP status; 1 = every step was differentiated (T = 0: 1)
 * The call zeroes rbar / dbar / pbar first and writes every other output.  The blocks' src and k0, the noise block, the
 * output trajectories and the cost of the descriptor are not read.
 *
 * State carried from step k + 1 to step k, per scenario: alpha = d/dx_{k+1} (nx), beta = d/d(predicted xhat_{k+1}) (nx,
 * observer only), gamma = d/duprev_{k+1} (nuprev).  At k = T: alpha = Xbar[T], beta = gamma = 0.  With the TRUE plant's
 * rows [f, F, G, Gd] and [h, C, Dd] and the handle's observer rows [f^, F^, G^, Gd^], [h^, C^, Dd^], Kt, step k is
 * (binary64; every sum ONE chain of explicit fmas in index order, every "+" below one addition, nothing else fused):
 *   1. ubar_l = Ubar[k][l]; fma(G[a][l], alpha_a, .) over a; observer: fma(G^[a][l], beta_a, .) over a; l < nuprev:
 *      + gamma_l.
 *   2. thbar = lmpc_solve_vjp's arithmetic on tape slice k with xbar = ubar.  A step whose status is not 1 (exit flag
 *      < 1, dependent rows, more than 64 rows) gives thbar = 0: its control is treated as a constant, and status_min
 *      says so.
 *   3. xi_c = thbar[c] (c < nx); observer: fma(F^[a][c], beta_a, .) over a, then eta_j = fma(Kt[j][c], xi_c, .) over c
 *      from 0.
 *   4. alpha'_c = Xbar[k][c]; fma(F[a][c], alpha_a, .) over a; without observer + xi_c; with observer
 *      fma(C[j][c], eta_j, .) over j, and beta'_c = xi_c; fma(-C^[j][c], eta_j, .) over j.
 *   5. delta_q = from 0: fma(Gd[a][q], alpha_a, .) over a; observer: fma(Gd^[a][q], beta_a, .) over a,
 *      fma(Dd[j][q], eta_j, .) over j, fma(-Dd^[j][q], eta_j, .) over j.  dbar[column the POST kernel read d_k from] +=
 *      delta_q (alpha, beta: the carried ones, not the primed).
 *   6. the entries of thbar behind the state, in theta's order r-block, d-block, uprev, p-block: each r / d / p entry is
 *      added once into the gradient column the forward read it from (the preview's k + 1 offset of r and the hold of the
 *      last column are the forward's own rule, one function serves both); gamma' = the uprev entries.
 * After step 0: x0bar = alpha, + beta where an observer ran from xhat == NULL (it started at x); xhat0bar = beta
 * otherwise; uprev0bar = gamma.  Restated in numpy in tests/scenario_adjoint_reference.py; scenario_adjoint_kernel and
 * lmpc_scenario_vjp_host run one body and give the same bits.
 *
 * lmpc_scenario_vjp_device enqueues on `stream` and never waits: T + 1 launches of scenario_adjoint_kernel (launch k
 * finishes step k + 1 and forms ubar of step k) with the launches of lmpc_solve_vjp_device between them.  Its scratch
 * (alpha, beta, gamma, ubar, thbar, the step's status) is one group of the handle, allocated by the first call of a
 * size and released by lmpc_release_scratch.  lmpc_scenario_vjp: HOST arrays, synchronous.  lmpc_scenario_vjp_host: the
 * same arithmetic on the CPU, no GPU and no handle, from the raw LDP pack and settings as lmpc_solve_vjp_host takes them
 * plus the observer's arrays (NULL without use_observer).
 * Refused: what lmpc_solve_vjp refuses -- BINARY rows, is_avi and proximal-point handles (LMPC_ERR_UNSUPPORTED), nth == 0
 * (LMPC_ERR_BADARG) -- and a descriptor lmpc_scenario_check refuses.  Binary64 only; the offset-free, uncertain, nonlinear
 * and explicit loops have no adjoint.  Not covered: gradients with respect to the noise block and the plant's matrices,
 * cotangents of Y_traj / Xhat_traj.
 */
typedef struct lmpc_scenario_tape {
    uint64_t *active;                    /* T x N x lmpc_active_words(h) */
    int32_t *flag;                       /* T x N                        */
} lmpc_scenario_tape;
typedef struct lmpc_scenario_grad {
    const double *Xbar, *Ubar;
    double *x0bar, *xhat0bar, *uprev0bar, *rbar, *dbar, *pbar;
    int32_t *status_min;
} lmpc_scenario_grad;
int lmpc_simulate_scenario_taped_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                        double *uprev, double *U_traj, double *X_traj, int32_t *flag_min,
                                        const lmpc_scenario_tape *tape, void *stream);
int lmpc_simulate_scenario_taped(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, double *x, double *xhat,
                                 double *uprev, double *U_traj, double *X_traj, int32_t *flag_min, const lmpc_scenario_tape *tape);
int lmpc_scenario_vjp_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape,
                             const lmpc_scenario_grad *g, void *stream);
int lmpc_scenario_vjp(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape,
                      const lmpc_scenario_grad *g);
int lmpc_scenario_vjp_host(int n, int m, int ms, int nth, int nout, const double *M, const double *du, const double *dl,
                           const double *Dth, const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                           const lmpc_settings *settings, int is_avi, const lmpc_observer *observer, int64_t N, int T,
                           const lmpc_scenario_sim *s, const lmpc_scenario_tape *tape, const lmpc_scenario_grad *g);
/* The handle's most recent backward sweeps (at most four are kept), oldest first, LMPC_SCENARIO_ADJOINT_INFO_WORDS words
 * each: number of the call in the handle's life (from 1), NX of the scenario_adjoint_kernel instantiation (0: run-time
 * nx), its grid, LDS bytes, T, N, 1 if the VJP's pass over its work list was enqueued, entries of a theta-bar record
 * staged at a time.  Returns the number of records written (out holds max records). */
#define LMPC_SCENARIO_ADJOINT_INFO_WORDS 8
int lmpc_scenario_adjoint_launch_info(const lmpc_handle *h, int32_t *out, int max);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_HIP_H */
