// Host check of the register form of the derivative kernels (csrc/lmpc_sens_kernel.hpp, csrc/lmpc_pack_grad_kernel.hpp;
// tests/test_sens_cap_host.py builds it with the address and undefined-behaviour sanitizers and runs it): the
// capacities the lane kernels are built at (5 and 8) against the host twins' 64, on every row set of a small pack that
// fits the capacity -- equal statuses and bitwise equal results.  Links neither HIP nor the library.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../linearmpc.jl_amd/csrc/lmpc_pack_grad_kernel.hpp"

using namespace lmpc;

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); g_failed++; } \
    } while (0)

constexpr int N = 6, M = 9, NTH = 3, NOUT = 2, WORDS = 1;
constexpr int SOFT_ROW = 4, DUP_OF = 2, DUP_ROW = 8;      // row 8 of M repeats row 2
constexpr double RHO = 0.5, ZERO_TOL = 1e-9;
constexpr double SENTINEL = -777.25;

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static double rnd() {       // uniform in [-1, 1)
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_seed >> 11) / 4503599627370496.0 - 1.0;
}

struct Pack {
    std::vector<double> Mm, Rout, du, dl, theta, xbar, C;
    SensDims d;
    SensView S;
};

static void make_pack(Pack &P) {
    P.Mm.resize(M * N); P.Rout.resize(NOUT * N); P.du.resize(M); P.dl.resize(M); P.theta.resize(NTH); P.xbar.resize(NOUT);
    for (double &v : P.Mm) v = rnd();
    for (int c = 0; c < N; c++) P.Mm[DUP_ROW * N + c] = P.Mm[DUP_OF * N + c];
    for (double &v : P.Rout) v = rnd();
    for (int j = 0; j < M; j++) { P.du[j] = 1.0 + rnd(); P.dl[j] = -1.0 + rnd(); }
    for (double &v : P.theta) v = rnd();
    for (double &v : P.xbar) v = rnd();
    P.d.m = M; P.d.nth = NTH; P.d.nout = NOUT; P.d.words = WORDS;
    P.C.assign(sens_pack_doubles(P.d), 0.0);
    double *g = P.C.data(), *p = g + sens_tri(M), *dt = p + M * NOUT, *xt = dt + M * NTH, *so = xt + NOUT * NTH;
    for (int a = 0; a < M; a++)
        for (int b = 0; b <= a; b++) {
            double acc = 0.0;
            for (int k = 0; k < N; k++) acc = std::fma(P.Mm[a * N + k], P.Mm[b * N + k], acc);
            g[sens_tri(a) + b] = acc;
        }
    for (int a = 0; a < M; a++)
        for (int q = 0; q < NOUT; q++) {
            double acc = 0.0;
            for (int k = 0; k < N; k++) acc = std::fma(P.Mm[a * N + k], P.Rout[q * N + k], acc);
            p[a * NOUT + q] = acc;
        }
    for (int i = 0; i < M * NTH; i++) dt[i] = rnd();
    for (int i = 0; i < NOUT * NTH; i++) xt[i] = rnd();
    so[SOFT_ROW] = 1.0;
    P.S = sens_view(P.C.data(), P.d, RHO, ZERO_TOL);
}

// the mask of a row set: even rows at their upper side, odd rows at their lower side
static uint64_t mask_of(unsigned set) {
    uint64_t u = 0;
    for (int j = 0; j < M; j++)
        if (set >> j & 1) u |= 1ull << (j % 2 == 0 ? j : M + j);
    return u;
}

struct Result {
    int k = 0, st_vjp = 0, st_jac = 0, st_pg = 0;
    double vjp[NTH], jac[NOUT * NTH], lam[kSensMaxSet], y[kSensMaxSet], thbar[NTH];
};

template <int CAP>
static Result run(const Pack &P, uint64_t mask) {
    Result R;
    for (double &v : R.vjp) v = SENTINEL;
    for (double &v : R.jac) v = SENTINEL;
    for (double &v : R.thbar) v = SENTINEL;
    for (int i = 0; i < kSensMaxSet; i++) R.lam[i] = R.y[i] = SENTINEL;
    int a[CAP] = {};
    double lam[CAP], y[CAP];
    for (int i = 0; i < CAP; i++) lam[i] = y[i] = SENTINEL;
    R.k = sens_active_rows<CAP>(&mask, WORDS, M, a);
    if (R.k > CAP) return R;
    R.st_vjp = sens_point<CAP, false>(P.S, a, R.k, P.xbar.data(), R.vjp);
    R.st_jac = sens_point<CAP, true>(P.S, a, R.k, nullptr, R.jac);
    R.st_pg = pack_grad_point<CAP>(P.S, P.du.data(), P.dl.data(), &mask, a, R.k, P.theta.data(), P.xbar.data(), lam, y, R.thbar);
    if (R.st_pg == SENS_DONE)
        for (int i = 0; i < R.k; i++) { R.lam[i] = lam[i]; R.y[i] = y[i]; }
    return R;
}

static bool same(const Result &a, const Result &b) {
    return a.k == b.k && a.st_vjp == b.st_vjp && a.st_jac == b.st_jac && a.st_pg == b.st_pg &&
           std::memcmp(a.vjp, b.vjp, sizeof(a.vjp)) == 0 && std::memcmp(a.jac, b.jac, sizeof(a.jac)) == 0 &&
           std::memcmp(a.lam, b.lam, sizeof(a.lam)) == 0 && std::memcmp(a.y, b.y, sizeof(a.y)) == 0 &&
           std::memcmp(a.thbar, b.thbar, sizeof(a.thbar)) == 0;
}

int main() {
    Pack P;
    make_pack(P);
    int done[M + 1] = {}, singular[M + 1] = {}, compared5 = 0, compared8 = 0;
    for (unsigned set = 0; set < (1u << M); set++) {
        const uint64_t mask = mask_of(set);
        const Result r64 = run<kSensMaxSet>(P, mask);
        CHECK(r64.k == __builtin_popcount(set));
        // the three entry points factor the same matrix
        CHECK(r64.st_vjp == r64.st_jac && r64.st_vjp == r64.st_pg);
        CHECK(r64.st_vjp == SENS_DONE || r64.st_vjp == SENS_SINGULAR);
        (r64.st_vjp == SENS_DONE ? done : singular)[r64.k]++;
        // a result is written with SENS_DONE only
        if (r64.st_vjp != SENS_DONE) CHECK(r64.vjp[0] == SENTINEL && r64.jac[0] == SENTINEL && r64.lam[0] == SENTINEL);
        if ((set >> DUP_OF & 1) && (set >> DUP_ROW & 1)) CHECK(r64.st_vjp == SENS_SINGULAR);
        if (r64.k <= 8) { CHECK(same(run<8>(P, mask), r64)); compared8++; }
        if (r64.k <= 5) { CHECK(same(run<5>(P, mask), r64)); compared5++; }
    }
    // the duplicated row, at every capacity
    const uint64_t dup = mask_of(1u << DUP_OF | 1u << DUP_ROW);
    CHECK(run<5>(P, dup).st_vjp == SENS_SINGULAR && run<8>(P, dup).st_vjp == SENS_SINGULAR && run<kSensMaxSet>(P, dup).st_vjp == SENS_SINGULAR);
    CHECK(run<5>(P, dup).st_pg == SENS_SINGULAR && run<8>(P, dup).st_pg == SENS_SINGULAR && run<kSensMaxSet>(P, dup).st_pg == SENS_SINGULAR);
    // the SOFT row alone: rho on the diagonal, in the contract's operations
    {
        const Result r = run<5>(P, mask_of(1u << SOFT_ROW));
        CHECK(r.st_vjp == SENS_DONE && r.k == 1);
        const double piv = P.S.G[sens_tri(SOFT_ROW) + SOFT_ROW] + RHO;
        double w = 0.0;
        for (int q = 0; q < NOUT; q++) w = std::fma(P.S.P[SOFT_ROW * NOUT + q], P.xbar[q], w);
        const double yv = w * (1.0 / piv);
        CHECK(std::memcmp(&r.y[0], &yv, sizeof(double)) == 0);
        for (int t = 0; t < NTH; t++) {
            double acc = 0.0;
            for (int q = 0; q < NOUT; q++) acc = std::fma(P.S.Xth[q * NTH + t], P.xbar[q], acc);
            acc = std::fma(P.S.Dth[SOFT_ROW * NTH + t], yv, acc);
            CHECK(std::memcmp(&r.vjp[t], &acc, sizeof(double)) == 0);
            CHECK(std::memcmp(&r.thbar[t], &acc, sizeof(double)) == 0);
        }
    }
    std::printf("compared at CAP 5: %d sets, at CAP 8: %d sets\ndone by size:", compared5, compared8);
    for (int k = 0; k <= M; k++) std::printf(" %d", done[k]);
    std::printf("\nsingular by size:");
    for (int k = 0; k <= M; k++) std::printf(" %d", singular[k]);
    std::printf("\n");
    if (g_failed) { std::printf("sens_cap_check: %d checks failed\n", g_failed); return 1; }
    std::printf("sens_cap_check ok\n");
    return 0;
}
