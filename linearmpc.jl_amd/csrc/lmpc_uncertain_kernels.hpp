// Glue kernels of the uncertain scenario loop (lmpc_simulate_scenario_uncertain_device): the scenario loop of
// lmpc_scenario_kernels.hpp with what the reference's users put into `scenario.dynamics` (reference
// src/simulation.jl:40,110,118-126; docs/src/manual/robust.md:17,78; example/observer.jl:11) -- additive process noise
// w_k = Gw e_k on the state, additive measurement noise v_k, and a table of plant variants one of which steps each
// scenario.  e_k and v_k are either read from a supplied block or drawn here, uniform in a box, from a counter-based
// generator: a draw depends on (seed, global scenario, global step, stream, component) and on nothing of the launch.
//
// The sums are the ones of the scenario loop, called, not restated: the PRE kernel is scn_pre_step with the measurement
// source added to ym, the POST kernel scn_score_step, scn_observer_predict, dynamics_rows and step_tail around the
// process noise (unc_process_noise).  With every source absent and no plant table both kernels execute the arithmetic
// of scenario_pre_kernel / scenario_post_kernel operation for operation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "lmpc_noise_math.hpp"
#include "lmpc_scenario_kernels.hpp"

namespace lmpc {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written out: ten
// rounds of two 32 x 32 -> 64 bit multiplies, the key bumped between rounds.  Counter c[0..3] in, output in place.
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// a word pair -> [0, 1): the 53 bits (a << 21) | (b >> 11) times 2^-53, exact
__host__ __device__ __forceinline__ double philox_unit(uint32_t a, uint32_t b) {
    return (double)(((uint64_t)a << 21) | (uint64_t)(b >> 11)) * 0x1.0p-53;
}

// one noise source: a supplied block (drawn == 0: column k of src, absent = zeros), the box [lo, hi] in ScnConst::c
// (drawn == 1) or a Gaussian (drawn == 2: the record carries the descriptor's dist as drawn = 1 + dist, so its size and
// the kernels' argument layout are the ones they had)
struct UncSource {
    ThetaBlock src;
    int w, drawn;
    int lo, span, hi;                 // offsets in doubles into ScnConst::c; span = hi - lo formed on the host;
                                      // Gaussian: lo = the means, span = hi = the standard deviations
};
constexpr int UNC_UNIFORM = 1, UNC_GAUSSIAN = 2;

// what one step's launches know of the uncertainty
struct UncStep {
    UncSource process, meas;
    int gw;                           // offset of Gw (nx x nw row-major) in ScnConst::c, -1 = identity
    uint32_t key0, key1;              // seed & 0xffffffff, seed >> 32
    uint32_t step;                    // step_offset + k
    unsigned long long goff;          // scenario_offset
    int n_plants;                     // 0 = ScnConst::plant for everyone; else the table starts at ScnConst::plant
    const int32_t *plant_index;       // N entries or nullptr = (scenario_offset + i) mod n_plants
    double *w_out;                    // this step's slice of W_traj or nullptr
};

// The draws of one (scenario, step, stream), component after component: counter (g lo, g hi, step, stream << 16 | j)
// gives components 2j (words 0, 1) and 2j + 1 (words 2, 3); a block is computed when its first component is asked
// for, so an odd count uses half of the last one.  No array: the four words live in registers.
struct UncDraws {
    uint32_t g0, g1, step, stream, k0, k1;
    uint32_t r0, r1, r2, r3;
    int j;
    __device__ __forceinline__ UncDraws(const UncStep &U, long long i, uint32_t stream_)
        : step(U.step), stream(stream_), k0(U.key0), k1(U.key1), r0(0), r1(0), r2(0), r3(0), j(-1) {
        const unsigned long long g = U.goff + (unsigned long long)i;
        g0 = (uint32_t)g; g1 = (uint32_t)(g >> 32);
    }
    __device__ __forceinline__ double unit(int q) {
        if ((q >> 1) != j) {
            j = q >> 1;
            uint32_t c[4] = {g0, g1, step, (stream << 16) | (uint32_t)j};
            philox4x32_10(c, k0, k1);
            r0 = c[0]; r1 = c[1]; r2 = c[2]; r3 = c[3];
        }
        return (q & 1) ? philox_unit(r2, r3) : philox_unit(r0, r1);
    }
};

// UncDraws of the kernels instantiated with GAUSS: the standard normal pair of a block (lmpc_noise_math.hpp) is formed
// when its first component is asked for and kept next to the words, which the uniform path goes on using.
struct UncDrawsGauss : UncDraws {
    double z0, z1;
    int jz;
    __device__ __forceinline__ UncDrawsGauss(const UncStep &U, long long i, uint32_t stream_) : UncDraws(U, i, stream_), z0(0.0), z1(0.0), jz(-1) {}
    __device__ __forceinline__ double normal(int q) {
        if ((q >> 1) != jz) {
            const double ua = unit(q & ~1), ub = unit(q | 1);
            jz = q >> 1;
            nm_gauss_pair(ua, ub, z0, z1);
        }
        return (q & 1) ? z1 : z0;
    }
};

// component q of a source at step k for scenario i: e = min(hi, lo + u * span), one multiply and one add; with Draws =
// UncDrawsGauss a Gaussian source gives e = mean + std * z, one multiply and one add, no clamp
template <class Draws>
__device__ __forceinline__ double unc_value(const UncSource &S, const double *__restrict__ c, Draws &D, long long i, int k, int q) {
    if (!S.drawn) return block_at(S.src, i, k, q);
    if constexpr (std::is_same<Draws, UncDrawsGauss>::value)
        if (S.drawn == UNC_GAUSSIAN) return nm_gauss_value(c[S.lo + q], c[S.span + q], D.normal(q));
    const double e = __dadd_rn(c[S.lo + q], __dmul_rn(D.unit(q), c[S.span + q]));
    const double hi = c[S.hi + q];
    return e < hi ? e : hi;
}

// PRE kernel of step k: scenario_pre_kernel with v_j added to ym_j as the last addition (the place the descriptor's
// noise block has; the two are exclusive).  Same two phases, same 256 * nx doubles of dynamic LDS.  GAUSS: the
// instantiation that can draw a Gaussian source (chosen on the host when either source is one), so that the logarithm,
// the square root and sin_ / cos_ cost the other runs no register.
template <int NXT, bool GAUSS = false>
__global__ __launch_bounds__(256) void uncertain_pre_kernel(ScnPre A, ScnConst K, UncStep U) {
    extern __shared__ double unc_lds[];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    typename std::conditional<GAUSS, UncDrawsGauss, UncDraws>::type dv(U, i, 1u);
    scn_pre_step<NXT>(A, K, unc_lds, [&](int j, double ym) {
        return U.meas.w > 0 ? __dadd_rn(ym, unc_value(U.meas, K.c, dv, i, A.k, j)) : ym;
    });
}

// Process noise onto the finished row sums xn of scenario i: x_a <- x_a + Gw_a0 e_0 + Gw_a1 e_1 + ... term by term
// (x_a <- x_a + e_a without Gw).  W_traj: row a = 0 + Gw_a0 e_0 + ... in the same order, or e_a.  The terms are visited
// component by component (one draw per component) with the rows' running sums side by side, which is the same order of
// additions for every row.
template <int NXT, class Draws>
__device__ __forceinline__ void unc_process_noise(const UncStep &U, const double *__restrict__ c, long long i, int k, int nx, double *xn) {
    const int nw = U.process.w;
    if (nw <= 0) return;
    Draws de(U, i, 0u);
    if (U.gw < 0) {
        for_nx<NXT>(nx, [&](int a) {
            const double e = unc_value(U.process, c, de, i, k, a);
            xn[a] = __dadd_rn(xn[a], e);
            if (U.w_out) U.w_out[i * nx + a] = e;
        });
    } else {
        const double *gw = c + U.gw;
        double wv[NXT > 0 ? NXT : 32];
        for_nx<NXT>(nx, [&](int a) { wv[a] = 0.0; });
        for (int q = 0; q < nw; q++) {
            const double e = unc_value(U.process, c, de, i, k, q);
            for_nx<NXT>(nx, [&](int a) {
                const double t = __dmul_rn(gw[a * nw + q], e);
                xn[a] = __dadd_rn(xn[a], t);
                wv[a] = __dadd_rn(wv[a], t);
            });
        }
        if (U.w_out) for_nx<NXT>(nx, [&](int a) { U.w_out[i * nx + a] = wv[a]; });
    }
}

// POST kernel of step k: scenario_post_kernel with the scenario's own plant rows (table + idx * nx * (1 + nx + nu + nd);
// a plant_index entry is taken as unsigned, modulo n_plants, so no entry addresses outside the table), and then
// unc_process_noise onto the finished row sums.
template <int NXT, bool COST, bool GAUSS = false>
__global__ __launch_bounds__(256) void uncertain_post_kernel(ScnPost A, ScnConst K, UncStep U) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    constexpr int NXA = NXT > 0 ? NXT : 32;
    const int nx = NXT > 0 ? NXT : A.nx;
    const int nu = A.nu;
    const double *u = A.u + i * nu;
    auto dk = [&](int q) { return block_at(A.d, i, A.k, q); };
    double xo[NXA], xn[NXA];
    for_nx<NXT>(nx, [&](int c) { xo[c] = A.x[i * nx + c]; });
    if constexpr (COST) scn_score_step<true>(K, xo, nx, u, nu, A.cost, A.viol, A.ulast, A.r, i, A.k, A.first, A.last);
    if (A.xhat) scn_observer_predict<NXT>(A.obs_dyn, A.xhat + i * nx, nx, nu, A.nd, u, dk);
    long long prow = 0;
    if (U.n_plants > 0) {
        const unsigned long long g = U.plant_index ? (unsigned long long)(uint32_t)U.plant_index[i] : U.goff + (unsigned long long)i;
        prow = (long long)(g % (unsigned long long)U.n_plants) * ((long long)nx * (1 + nx + nu + A.nd));
    }
    dynamics_rows<NXT>(K.c + K.plant + prow, xo, xn, nx, nu, A.nd, u, dk);
    unc_process_noise<NXT, typename std::conditional<GAUSS, UncDrawsGauss, UncDraws>::type>(U, K.c, i, A.k, nx, xn);
    for_nx<NXT>(nx, [&](int a) { A.x[i * nx + a] = xn[a]; });
    if (A.xtraj_next) for_nx<NXT>(nx, [&](int a) { A.xtraj_next[i * nx + a] = xn[a]; });
    step_tail(i, u, nu, A.uprev + i * A.nup, (double *)nullptr, A.nup, A.utraj, A.flag, A.flag_min, A.first);
}

}  // namespace lmpc
