// Explicit MPC controller object (include/lmpc_hip.h, "Explicit MPC"): the host tables written by the builder
// (lmpc_explicit.cpp) and the device copy and fallback scratch kept by lmpc_explicit.hip.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lmpc_hip.h"
#include "lmpc_internal.hpp"

struct lmpc_explicit {
    int n = 0, m = 0, ms = 0, nth = 0, nout = 0, words = 0;
    double primal_tol = 1e-6, rho_soft = 1e-6, band = 1e-3;
    std::vector<uint64_t> blob;                 // the serialised table (lmpc_explicit_kernel.hpp), 8-byte words
    std::vector<uint64_t> masks;                // kept regions' masks, `words` each
    std::vector<int64_t> counts;                // ... and their training counts
    std::vector<int32_t> label, leaf;           // per training point: region, tree leaf
    int64_t info[LMPC_EXPLICIT_INFO] = {};
    std::string err;
    // device side: the handle whose GPU holds the table and whose implicit path takes the unlocated points
    lmpc_handle *h = nullptr;
    int device = -1;
    lmpc::DevBuf<uint64_t> dBlob;
    lmpc::DevBuf<int32_t> dCount;               // the count word of the unlocated points ...
    lmpc::PinnedBuf<int32_t> hCount;            // ... and where the host reads it
    lmpc::DevBuf<int32_t> dList, dFlag;         // the fallback scratch: one group of `cap` points
    lmpc::DevBuf<double> dTheta, dX;
    int64_t cap = 0;
    // scenario loop (lmpc_explicit_sim.hip): per-scenario step counters, the second work list, the lock-step form's
    // theta / u / flag, and [xhat | ulast] when the caller keeps none
    lmpc::DevBuf<int32_t> simStep, simList2, simFlag;
    lmpc::DevBuf<double> simTheta, simU, simScr;
    int64_t simCap = 0, simLockCap = 0;
};

// the text into the controller's error slot, the code handed back
inline int efail(lmpc_explicit *e, int code, const std::string &msg) {
    e->err = msg;
    return code;
}

#define EXP_TRY(e, call)                                                                              \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess) return efail(e, LMPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

namespace lmpc {
int explicit_build_pack(lmpc_explicit *e, int n, int m, int ms, int nth, int nout, const double *M, const double *du,
                        const double *dl, const double *Dth, const double *Rout, const double *x0, const double *Xth,
                        const int32_t *sense, const lmpc_settings &s, int is_avi, int64_t N, const double *theta,
                        const uint64_t *active, const int32_t *exitflag, const lmpc_explicit_opts &o);
// the fallback scratch (dList, dTheta, dX, dFlag, the count words) sized for N points (lmpc_explicit.hip)
int explicit_reserve(lmpc_explicit *e, int64_t N);
}  // namespace lmpc
