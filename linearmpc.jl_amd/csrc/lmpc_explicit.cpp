// Explicit MPC, host half (include/lmpc_hip.h, "Explicit MPC"): from a solved training sample to a serialised
// piecewise-affine controller -- regions, their laws and halfspaces in the handle's LDP form, a point-location tree --
// plus the host-side inspection and evaluation entry points.  Nothing here touches a GPU; lmpc_explicit.hip uploads
// the table and evaluates it there.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <unordered_map>

#include "lmpc_explicit.hpp"
#include "lmpc_explicit_kernel.hpp"
#include "lmpc_pack.hpp"

extern thread_local std::string g_setup_err;

namespace lmpc {
namespace {

constexpr double kNoBound = 1e30;     // |bound| >= this (or not finite): that side of the row does not exist

struct Region {
    std::vector<double> rows;         // halfspaces, (nth + 1) doubles each
    std::vector<double> law;          // nout records of (nth + 1)
    std::vector<double> soft;         // one record per active SOFT row
    int32_t softRows = 0;             // the leading halfspaces that are bounds of inactive SOFT rows
};

struct PackIn {
    int n, m, ms, nth, nout;
    const double *M, *du, *dl, *Dth, *Rout, *x0, *Xth;
    const int32_t *sense;
};

// K = L L' in place (lower triangle); false if a pivot (before the square root, the D of L D L') is below tol
bool cholesky(std::vector<double> &K, int k, double tol) {
    for (int j = 0; j < k; j++) {
        double d = K[(size_t)j * k + j];
        for (int p = 0; p < j; p++) d -= K[(size_t)j * k + p] * K[(size_t)j * k + p];
        if (!(d > tol)) return false;
        const double l = std::sqrt(d);
        K[(size_t)j * k + j] = l;
        for (int i = j + 1; i < k; i++) {
            double s = K[(size_t)i * k + j];
            for (int p = 0; p < j; p++) s -= K[(size_t)i * k + p] * K[(size_t)j * k + p];
            K[(size_t)i * k + j] = s / l;
        }
    }
    return true;
}

// K Y = Y in place by Gaussian elimination with partial pivoting (K row-major ns x ns, Y ns x cols); false if K is
// numerically singular
bool lu_solve(std::vector<double> &K, int ns, std::vector<double> &Y, int cols) {
    double scale = 0.0;
    for (double v : K) scale = std::max(scale, std::fabs(v));
    for (int c = 0; c < ns; c++) {
        int piv = c;
        for (int i = c + 1; i < ns; i++)
            if (std::fabs(K[(size_t)i * ns + c]) > std::fabs(K[(size_t)piv * ns + c])) piv = i;
        if (!(std::fabs(K[(size_t)piv * ns + c]) > 1e-14 * scale)) return false;
        if (piv != c) {
            for (int j = 0; j < ns; j++) std::swap(K[(size_t)c * ns + j], K[(size_t)piv * ns + j]);
            for (int j = 0; j < cols; j++) std::swap(Y[(size_t)c * cols + j], Y[(size_t)piv * cols + j]);
        }
        const double d = K[(size_t)c * ns + c];
        for (int i = c + 1; i < ns; i++) {
            const double f = K[(size_t)i * ns + c] / d;
            if (f == 0.0) continue;
            for (int j = c; j < ns; j++) K[(size_t)i * ns + j] -= f * K[(size_t)c * ns + j];
            for (int j = 0; j < cols; j++) Y[(size_t)i * cols + j] -= f * Y[(size_t)c * cols + j];
        }
    }
    for (int c = ns - 1; c >= 0; c--)
        for (int j = 0; j < cols; j++) {
            double acc = Y[(size_t)c * cols + j];
            for (int i = c + 1; i < ns; i++) acc -= K[(size_t)c * ns + i] * Y[(size_t)i * cols + j];
            Y[(size_t)c * cols + j] = acc / K[(size_t)c * ns + c];
        }
    return true;
}

// a . theta <= b, kept unless its theta part is zero and it always holds
void add_row(std::vector<double> &rows, const double *a, double b, int nth) {
    bool zero = true;
    for (int t = 0; t < nth; t++) zero = zero && a[t] == 0.0;
    if (zero && b >= 0.0) return;
    rows.insert(rows.end(), a, a + nth);
    rows.push_back(b);
}

inline bool bit(const uint64_t *mask, int b) { return (mask[b >> 6] >> (b & 63)) & 1u; }

// Law and halfspaces of the region whose optimal active set is `mask`; false if the reduced system is singular.
bool region_law(const PackIn &P, const uint64_t *mask, const lmpc_explicit_opts &o, double zero_tol, double rho,
                Region &R) {
    const int n = P.n, m = P.m, nth = P.nth, nout = P.nout, w = nth + 1;
    std::vector<int> A;
    std::vector<char> lower, inA(m, 0);
    for (int j = 0; j < m; j++) {
        const bool up = bit(mask, j), lo = bit(mask, m + j);
        if (!up && !lo) continue;
        A.push_back(j);
        lower.push_back(lo && !up);
        inA[j] = 1;
    }
    const int k = (int)A.size();
    // Hard rows H and SOFT rows S of the working set.  lambda_A = -(M_A M_A' + rho S_A)^-1 d_A(theta) is formed
    // without that matrix, whose condition grows like 1 / rho once there are more active rows than variables: u
    // minimises 1/2 |u|^2 + |M_S u - d_S|^2 / (2 rho) subject to M_H u = d_H, i.e.
    //     [I + M_S' M_S / rho   M_H'] [u       ]   [M_S' d_S / rho]
    //     [M_H                  0   ] [lambda_H] = [d_H           ],    lambda_S = (M_S u - d_S) / rho,
    // every right-hand side affine in theta: columns (Dth_row, d0_row).
    std::vector<int> hard;
    for (int r = 0; r < k; r++)
        if (!(P.sense[A[r]] & SENSE_SOFT)) hard.push_back(r);
    const int kh = (int)hard.size(), ns = n + kh;
    auto rhs = [&](int r, int t) { return t < nth ? P.Dth[(size_t)A[r] * nth + t] : (lower[r] ? P.dl[A[r]] : P.du[A[r]]); };
    {   // the hard rows must be independent (the solver's own test: pivots of M_H M_H' above zero_tol)
        std::vector<double> G((size_t)kh * kh);
        for (int a2 = 0; a2 < kh; a2++)
            for (int b2 = 0; b2 <= a2; b2++) {
                double acc = 0.0;
                for (int i = 0; i < n; i++) acc = std::fma(P.M[(size_t)A[hard[a2]] * n + i], P.M[(size_t)A[hard[b2]] * n + i], acc);
                G[(size_t)a2 * kh + b2] = G[(size_t)b2 * kh + a2] = acc;
            }
        if (kh > 0 && !cholesky(G, kh, zero_tol)) return false;
    }
    std::vector<double> K((size_t)ns * ns, 0.0), Y((size_t)ns * w, 0.0);
    for (int i = 0; i < n; i++) K[(size_t)i * ns + i] = 1.0;
    for (int r = 0; r < k; r++) {
        const double *mr = P.M + (size_t)A[r] * n;
        if (!(P.sense[A[r]] & SENSE_SOFT)) continue;
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < n; j++) K[(size_t)i * ns + j] += mr[i] * mr[j] / rho;
            for (int t = 0; t < w; t++) Y[(size_t)i * w + t] += mr[i] * rhs(r, t) / rho;
        }
    }
    for (int h = 0; h < kh; h++) {
        const double *mr = P.M + (size_t)A[hard[h]] * n;
        for (int i = 0; i < n; i++) K[(size_t)(n + h) * ns + i] = K[(size_t)i * ns + n + h] = mr[i];
        for (int t = 0; t < w; t++) Y[(size_t)(n + h) * w + t] = rhs(hard[h], t);
    }
    if (!lu_solve(K, ns, Y, w)) return false;
    std::vector<double> U(Y.begin(), Y.begin() + (size_t)n * w);
    // multipliers of the working set, row r: lambda_r = lam[r] . (theta, 1)
    std::vector<double> lam((size_t)k * w);
    for (int h = 0; h < kh; h++)
        for (int t = 0; t < w; t++) lam[(size_t)hard[h] * w + t] = Y[(size_t)(n + h) * w + t];
    for (int r = 0; r < k; r++) {
        if (!(P.sense[A[r]] & SENSE_SOFT)) continue;
        const double *mr = P.M + (size_t)A[r] * n;
        for (int t = 0; t < w; t++) {
            double acc = 0.0;
            for (int i = 0; i < n; i++) acc += mr[i] * U[(size_t)i * w + t];
            lam[(size_t)r * w + t] = (acc - rhs(r, t)) / rho;
        }
    }
    R.law.assign((size_t)nout * w, 0.0);
    for (int q = 0; q < nout; q++)
        for (int t = 0; t < w; t++) {
            double acc = t < nth ? P.Xth[(size_t)q * nth + t] : P.x0[q];
            for (int i = 0; i < n; i++) acc += P.Rout[(size_t)q * n + i] * U[(size_t)i * w + t];
            R.law[(size_t)q * w + t] = acc;
        }
    std::vector<double> a(w), p(w), softIn;
    // primal feasibility of every inactive row that can be violated: dl_j + Dth_j theta <= M_j u <= du_j + Dth_j theta
    for (int j = 0; j < m; j++) {
        if (inA[j] || (P.sense[j] & SENSE_IMMUTABLE)) continue;
        const double *mj = P.M + (size_t)j * n;
        for (int t = 0; t < w; t++) {
            double acc = 0.0;
            for (int i = 0; i < n; i++) acc += mj[i] * U[(size_t)i * w + t];
            p[t] = acc;
        }
        const double *dth = P.Dth + (size_t)j * nth;
        std::vector<double> &dst = (P.sense[j] & SENSE_SOFT) ? softIn : R.rows;
        if (std::fabs(P.du[j]) < kNoBound) {
            for (int t = 0; t < nth; t++) a[t] = p[t] - dth[t];
            add_row(dst, a.data(), P.du[j] - p[nth], nth);
        }
        if (std::fabs(P.dl[j]) < kNoBound) {
            for (int t = 0; t < nth; t++) a[t] = dth[t] - p[t];
            add_row(dst, a.data(), p[nth] - P.dl[j], nth);
        }
    }
    R.softRows = (int32_t)(softIn.size() / w);
    R.rows.insert(R.rows.begin(), softIn.begin(), softIn.end());
    // dual feasibility of the active rows (the solver's convention: upper lambda >= 0, lower lambda <= 0)
    for (int r = 0; r < k; r++) {
        const double *l = &lam[(size_t)r * w];
        if (!(P.sense[A[r]] & SENSE_IMMUTABLE)) {
            const double sg = lower[r] ? 1.0 : -1.0;          // upper: -lambda <= 0;  lower: lambda <= 0
            for (int t = 0; t < nth; t++) a[t] = sg * l[t];
            add_row(R.rows, a.data(), -sg * l[nth], nth);
        }
        if (P.sense[A[r]] & SENSE_SOFT) R.soft.insert(R.soft.end(), l, l + w);
    }
    if (o.box_lb && o.box_ub)
        for (int t = 0; t < nth; t++) {
            std::fill(a.begin(), a.end(), 0.0);
            a[t] = 1.0;
            add_row(R.rows, a.data(), o.box_ub[t], nth);
            a[t] = -1.0;
            add_row(R.rows, a.data(), -o.box_lb[t], nth);
        }
    return true;
}

struct MaskHash {
    const uint64_t *a;
    int w;
    size_t operator()(int64_t p) const {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (int k = 0; k < w; k++) {
            h ^= a[(size_t)p * w + k];
            h *= 0x100000001B3ull;
            h ^= h >> 29;
        }
        return (size_t)h;
    }
};
struct MaskEq {
    const uint64_t *a;
    int w;
    bool operator()(int64_t p, int64_t q) const {
        return w == 0 || std::memcmp(a + (size_t)p * w, a + (size_t)q * w, sizeof(uint64_t) * w) == 0;
    }
};

// Point-location tree grown on the labelled sample (include/lmpc_hip.h: the tree is approximate, the leaf check exact).
struct TreeBuilder {
    int nth;
    const double *theta;
    const std::vector<int32_t> &label;
    const std::vector<double> &rows;
    const std::vector<int32_t> &row0, &nrows;
    const lmpc_explicit_opts &o;
    std::vector<int32_t> &leaf;
    std::vector<int32_t> nodes, leafidx, seenL, seenR;
    int32_t stamp = 0;
    int depth = 0, leaves = 0, largest = 0;

    bool right_of(int row, int64_t p) const {
        return explicit_row_violated<kExplicitMaxNth>(&rows[(size_t)row * (nth + 1)], theta + (size_t)p * nth, nth);
    }

    int make_leaf(int id, const std::vector<int32_t> &C, const std::vector<int32_t> &pts) {
        nodes[4 * id] = -1;
        nodes[4 * id + 1] = (int32_t)leafidx.size();
        nodes[4 * id + 2] = (int32_t)C.size();
        leafidx.insert(leafidx.end(), C.begin(), C.end());
        for (int32_t p : pts) leaf[p] = id;
        leaves++;
        largest = std::max(largest, (int)C.size());
        return id;
    }

    int build(std::vector<int32_t> &pts, int d) {
        const int id = (int)(nodes.size() / 4);
        nodes.insert(nodes.end(), {-1, 0, 0, 0});
        depth = std::max(depth, d);
        std::vector<int32_t> C;
        ++stamp;
        for (int32_t p : pts)
            if (seenL[label[p]] != stamp) { seenL[label[p]] = stamp; C.push_back(label[p]); }
        std::sort(C.begin(), C.end());                 // region index = frequency rank
        if ((int)C.size() <= o.leaf_size || d >= o.max_depth) return make_leaf(id, C, pts);
        // candidates: every halfspace row of the node's split_regions most frequent regions, ranked on a small
        // strided subset of the points; the split_rows best are scored again on up to score_points points
        auto subset = [&](size_t want, std::vector<int32_t> &sub) -> const std::vector<int32_t> & {
            const size_t np = pts.size();
            if (np <= want) return pts;
            sub.resize(want);
            for (size_t i = 0; i < want; i++) sub[i] = pts[i * np / want];
            return sub;
        };
        struct Score { int row; size_t score; int64_t bal; };
        auto score_rows = [&](const std::vector<int32_t> &rowsIn, const std::vector<int32_t> &S) {
            std::vector<Score> out;
            for (int row : rowsIn) {
                ++stamp;
                size_t cl = 0, cr = 0;
                int64_t nl = 0, nr = 0;
                for (int32_t p : S) {
                    const int32_t r = label[p];
                    if (right_of(row, p)) {
                        nr++;
                        if (seenR[r] != stamp) { seenR[r] = stamp; cr++; }
                    } else {
                        nl++;
                        if (seenL[r] != stamp) { seenL[r] = stamp; cl++; }
                    }
                }
                if (nl == 0 || nr == 0) continue;
                const size_t score = std::max(cl, cr);
                if (score >= C.size()) continue;
                out.push_back({row, score, nl > nr ? nl - nr : nr - nl});
            }
            std::stable_sort(out.begin(), out.end(), [](const Score &x, const Score &y) {
                return x.score != y.score ? x.score < y.score : x.bal < y.bal;
            });
            return out;
        };
        std::vector<int32_t> cand;
        for (int c = 0; c < (int)C.size() && c < o.split_regions; c++)
            for (int i = 0; i < nrows[C[c]]; i++) cand.push_back(row0[C[c]] + i);
        std::vector<int32_t> sub1, sub2;
        std::vector<Score> first = score_rows(cand, subset(4096, sub1));
        cand.clear();
        for (size_t i = 0; i < first.size() && (int)i < o.split_rows; i++) cand.push_back(first[i].row);
        std::vector<Score> ranked = score_rows(cand, subset((size_t)o.score_points, sub2));
        const int best = ranked.empty() ? -1 : ranked[0].row;
        if (best < 0) return make_leaf(id, C, pts);
        std::vector<int32_t> L, R;
        for (int32_t p : pts) (right_of(best, p) ? R : L).push_back(p);
        if (L.empty() || R.empty()) return make_leaf(id, C, pts);
        std::vector<int32_t>().swap(pts);
        const int l = build(L, d + 1);
        const int r = build(R, d + 1);
        nodes[4 * id] = best;
        nodes[4 * id + 1] = l;
        nodes[4 * id + 2] = r;
        return id;
    }
};

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

int explicit_build_pack(lmpc_explicit *e, int n, int m, int ms, int nth, int nout, const double *M, const double *du,
                        const double *dl, const double *Dth, const double *Rout, const double *x0, const double *Xth,
                        const int32_t *sense, const lmpc_settings &s, int is_avi, int64_t N, const double *theta,
                        const uint64_t *active, const int32_t *exitflag, const lmpc_explicit_opts &o) {
    auto fail = [&](int code, const std::string &msg) { e->err = "lmpc_explicit_build: " + msg; return code; };
    if (n <= 0 || m < 0 || ms < 0 || ms > m || nth < 0 || nout <= 0 || nout > n || N < 0 || N > 0x7fffffffLL)
        return fail(LMPC_ERR_BADARG, "inconsistent dimensions (or more than 2^31 - 1 training points)");
    if ((m > 0 && (!M || !du || !dl || !sense || (nth > 0 && !Dth))) || !Rout || !x0 || (nth > 0 && !Xth))
        return fail(LMPC_ERR_BADARG, "NULL pack array");
    if (N > 0 && (!active || !exitflag || (nth > 0 && !theta))) return fail(LMPC_ERR_BADARG, "NULL training array");
    if (is_avi)
        return fail(LMPC_ERR_UNSUPPORTED, "variational (is_avi) problems have no explicit controller in this library");
    if (s.eps_prox > 0.0)
        return fail(LMPC_ERR_UNSUPPORTED, "proximal-point handles (eps_prox > 0) have no explicit controller in this library");
    if (nth > kExplicitMaxNth)
        return fail(LMPC_ERR_UNSUPPORTED, "nth = " + std::to_string(nth) + " is above LMPC_EXPLICIT_MAX_NTH (32)");
    for (int j = 0; j < m; j++)
        if (sense[j] & SENSE_BINARY)
            return fail(LMPC_ERR_UNSUPPORTED, "BINARY rows (hybrid MPC): no explicit controller, as in the reference (explicit.jl:25-28)");
    if (o.max_regions < 0 || o.leaf_size < 1 || o.max_depth < 0 || o.split_regions < 1 || o.split_rows < 1 ||
        o.score_points < 1 || o.max_bytes <= 0 || !(o.soft_band >= 0.0) || (!o.box_lb) != (!o.box_ub))
        return fail(LMPC_ERR_BADARG, "options out of range (lmpc_explicit_default_opts fills valid ones)");
    e->n = n; e->m = m; e->ms = ms; e->nth = nth; e->nout = nout;
    e->words = (2 * m + 63) / 64;
    e->primal_tol = s.primal_tol; e->rho_soft = s.rho_soft; e->band = o.soft_band;
    const int w = e->words, rw = nth + 1;
    const PackIn P{n, m, ms, nth, nout, M, du, dl, Dth, Rout, x0, Xth, sense};

    // distinct optimal active sets, most frequent first (ties: first occurrence)
    std::unordered_map<int64_t, int32_t, MaskHash, MaskEq> seen(1024, MaskHash{active, w}, MaskEq{active, w});
    std::vector<int64_t> first, cnt;
    std::vector<int32_t> lab((size_t)N, -1);
    for (int64_t p = 0; p < N; p++) {
        if (exitflag[p] < 1) continue;
        auto it = seen.find(p);
        int32_t id;
        if (it == seen.end()) {
            id = (int32_t)first.size();
            seen.emplace(p, id);
            first.push_back(p);
            cnt.push_back(0);
        } else {
            id = it->second;
        }
        cnt[id]++;
        lab[p] = id;
    }
    const int D = (int)first.size();
    std::vector<int32_t> order(D);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return cnt[a] != cnt[b] ? cnt[a] > cnt[b] : first[a] < first[b];
    });

    std::vector<Region> regs;
    std::vector<int32_t> newid(D, -1);
    int64_t dropCap = 0, dropSing = 0, bytes = 0;
    e->masks.clear(); e->counts.clear();
    for (int32_t idx : order) {
        if ((int)regs.size() >= o.max_regions) { dropCap++; continue; }
        Region R;
        if (!region_law(P, active + (size_t)first[idx] * w, o, s.zero_tol, s.rho_soft, R)) { dropSing++; continue; }
        const int64_t rb = 32 + (int64_t)sizeof(double) * (int64_t)(R.rows.size() + R.law.size() + R.soft.size());
        if (bytes + rb > o.max_bytes) { dropCap++; continue; }
        bytes += rb;
        newid[idx] = (int32_t)regs.size();
        regs.push_back(std::move(R));
        e->masks.insert(e->masks.end(), active + (size_t)first[idx] * w, active + (size_t)first[idx] * w + w);
        e->counts.push_back(cnt[idx]);
    }
    const int nreg = (int)regs.size();
    std::vector<int32_t> pts;
    for (int64_t p = 0; p < N; p++) {
        if (lab[p] >= 0) lab[p] = newid[lab[p]];
        if (lab[p] >= 0) pts.push_back((int32_t)p);
    }
    const int64_t labelled = (int64_t)pts.size();

    std::vector<double> rows, laws, soft;
    std::vector<int32_t> row0(nreg), nrows(nreg), soft0(nreg), nsoft(nreg), softRows(nreg);
    for (int r = 0; r < nreg; r++) {
        row0[r] = (int32_t)(rows.size() / rw);
        nrows[r] = (int32_t)(regs[r].rows.size() / rw);
        soft0[r] = (int32_t)(soft.size() / rw);
        nsoft[r] = (int32_t)(regs[r].soft.size() / rw);
        softRows[r] = regs[r].softRows;
        rows.insert(rows.end(), regs[r].rows.begin(), regs[r].rows.end());
        laws.insert(laws.end(), regs[r].law.begin(), regs[r].law.end());
        soft.insert(soft.end(), regs[r].soft.begin(), regs[r].soft.end());
    }

    e->leaf.assign((size_t)N, -1);
    TreeBuilder T{nth, theta, lab, rows, row0, nrows, o, e->leaf, {}, {}, std::vector<int32_t>(nreg, 0),
                  std::vector<int32_t>(nreg, 0)};
    T.build(pts, 0);
    e->label = std::move(lab);

    // serialise
    const size_t offNodes = sizeof(int64_t) * kHeadWords;
    const size_t offLeaf = offNodes + align8(sizeof(int32_t) * T.nodes.size());
    const size_t offRegions = offLeaf + align8(sizeof(int32_t) * T.leafidx.size());
    const size_t offRows = offRegions + sizeof(int32_t) * 8 * (size_t)nreg;
    const size_t offLaws = offRows + sizeof(double) * rows.size();
    const size_t offSoft = offLaws + sizeof(double) * laws.size();
    const size_t total = offSoft + sizeof(double) * soft.size();
    e->blob.assign(total / 8, 0);
    char *b = reinterpret_cast<char *>(e->blob.data());
    int64_t *head = reinterpret_cast<int64_t *>(b);
    head[kHeadNth] = nth; head[kHeadNout] = nout; head[kHeadRegions] = nreg;
    head[kHeadNodes] = (int64_t)(T.nodes.size() / 4); head[kHeadLeafIdx] = (int64_t)T.leafidx.size();
    head[kHeadRows] = (int64_t)(rows.size() / rw);
    head[kHeadOffNodes] = (int64_t)offNodes; head[kHeadOffLeafIdx] = (int64_t)offLeaf;
    head[kHeadOffRegions] = (int64_t)offRegions; head[kHeadOffRows] = (int64_t)offRows;
    head[kHeadOffLaws] = (int64_t)offLaws; head[kHeadOffSoft] = (int64_t)offSoft;
    head[kHeadBytes] = (int64_t)total; head[kHeadSoftRows] = (int64_t)(soft.size() / rw);
    std::memcpy(b + offNodes, T.nodes.data(), sizeof(int32_t) * T.nodes.size());
    if (!T.leafidx.empty()) std::memcpy(b + offLeaf, T.leafidx.data(), sizeof(int32_t) * T.leafidx.size());
    int32_t *rec = reinterpret_cast<int32_t *>(b + offRegions);
    for (int r = 0; r < nreg; r++) {
        rec[8 * r] = row0[r]; rec[8 * r + 1] = nrows[r]; rec[8 * r + 2] = r * nout;
        rec[8 * r + 3] = soft0[r]; rec[8 * r + 4] = nsoft[r]; rec[8 * r + 5] = softRows[r];
    }
    if (!rows.empty()) std::memcpy(b + offRows, rows.data(), sizeof(double) * rows.size());
    if (!laws.empty()) std::memcpy(b + offLaws, laws.data(), sizeof(double) * laws.size());
    if (!soft.empty()) std::memcpy(b + offSoft, soft.data(), sizeof(double) * soft.size());

    int64_t *in = e->info;
    in[0] = nreg; in[1] = dropCap; in[2] = dropSing; in[3] = head[kHeadRows]; in[4] = head[kHeadNodes];
    in[5] = T.depth; in[6] = T.leaves; in[7] = T.largest; in[8] = (int64_t)total; in[9] = labelled; in[10] = D;
    in[11] = head[kHeadSoftRows];
    return LMPC_OK;
}

}  // namespace lmpc

extern "C" {

void lmpc_explicit_default_opts(lmpc_explicit_opts *o) {
    if (!o) return;
    o->max_regions = 4096;
    o->leaf_size = 8;
    o->max_depth = 24;
    o->split_regions = 4;
    o->split_rows = 96;
    o->score_points = 65536;
    o->max_bytes = (int64_t)256 << 20;
    o->soft_band = 0.1;
    o->box_lb = nullptr;
    o->box_ub = nullptr;
}

int lmpc_explicit_build_ldp(lmpc_explicit **out, int n, int m, int ms, int nth, int nout,
                            const double *M, const double *du, const double *dl, const double *Dth,
                            const double *Rout, const double *x0, const double *Xth, const int32_t *sense,
                            const lmpc_settings *s, int is_avi, int64_t N, const double *theta,
                            const uint64_t *active, const int32_t *exitflag, const lmpc_explicit_opts *opts) {
    if (!out) return LMPC_ERR_BADARG;
    *out = nullptr;
    lmpc_settings st;
    if (s) st = *s; else lmpc_default_settings(&st);
    lmpc_explicit_opts o;
    if (opts) o = *opts; else lmpc_explicit_default_opts(&o);
    lmpc_explicit *e = new lmpc_explicit();
    const int rc = lmpc::explicit_build_pack(e, n, m, ms, nth, nout, M, du, dl, Dth, Rout, x0, Xth, sense, st, is_avi,
                                             N, theta, active, exitflag, o);
    if (rc != LMPC_OK) {
        g_setup_err = e->err;
        delete e;
        return rc;
    }
    *out = e;
    return LMPC_OK;
}

int lmpc_explicit_info(const lmpc_explicit *e, int64_t *out) {
    if (!e || !out) return LMPC_ERR_BADARG;
    std::memcpy(out, e->info, sizeof(e->info));
    return LMPC_OK;
}

int lmpc_explicit_region(const lmpc_explicit *e, int32_t r, double *F, double *g, double *A, double *b,
                         int32_t *nrows, uint64_t *mask, int64_t *count) {
    if (!e || r < 0 || r >= (int32_t)e->info[0]) return LMPC_ERR_BADARG;
    const int64_t *head = reinterpret_cast<const int64_t *>(e->blob.data());
    const lmpc::ExplicitView v = lmpc::explicit_view(e->blob.data(), head, e->primal_tol, e->band, e->rho_soft);
    const int nth = e->nth, w = nth + 1;
    const int32_t *rec = v.regions + 8 * r;
    if (nrows) *nrows = rec[1];
    for (int q = 0; q < e->nout; q++) {
        const double *law = v.laws + ((size_t)rec[2] + q) * w;
        if (F) std::memcpy(F + (size_t)q * nth, law, sizeof(double) * nth);
        if (g) g[q] = law[nth];
    }
    for (int i = 0; i < rec[1]; i++) {
        const double *row = v.rows + ((size_t)rec[0] + i) * w;
        if (A) std::memcpy(A + (size_t)i * nth, row, sizeof(double) * nth);
        if (b) b[i] = row[nth];
    }
    if (mask) std::memcpy(mask, e->masks.data() + (size_t)r * e->words, sizeof(uint64_t) * e->words);
    if (count) *count = e->counts[r];
    return LMPC_OK;
}

int lmpc_explicit_blob(const lmpc_explicit *e, void *out, int64_t *bytes) {
    if (!e || !bytes) return LMPC_ERR_BADARG;
    *bytes = (int64_t)(e->blob.size() * sizeof(uint64_t));
    if (out) std::memcpy(out, e->blob.data(), (size_t)*bytes);
    return LMPC_OK;
}

int lmpc_explicit_training(const lmpc_explicit *e, int32_t *label, int32_t *leaf) {
    if (!e) return LMPC_ERR_BADARG;
    if (label && !e->label.empty()) std::memcpy(label, e->label.data(), sizeof(int32_t) * e->label.size());
    if (leaf && !e->leaf.empty()) std::memcpy(leaf, e->leaf.data(), sizeof(int32_t) * e->leaf.size());
    return LMPC_OK;
}

int lmpc_explicit_locate_host(const lmpc_explicit *e, int64_t N, const double *theta, double *x, int32_t *exitflag,
                              int32_t *region, int32_t *rows_checked) {
    if (!e || N < 0 || (N > 0 && (!region || (e->nth > 0 && !theta)))) return LMPC_ERR_BADARG;
    const int64_t *head = reinterpret_cast<const int64_t *>(e->blob.data());
    const lmpc::ExplicitView v = lmpc::explicit_view(e->blob.data(), head, e->primal_tol, e->band, e->rho_soft);
    const int nth = e->nth, nout = e->nout;
    double th[lmpc::kExplicitMaxNth] = {};
    for (int64_t p = 0; p < N; p++) {
        for (int t = 0; t < nth; t++) th[t] = theta[(size_t)p * nth + t];
        int flag = 0, checked = 0;
        const int r = lmpc::explicit_locate<lmpc::kExplicitMaxNth>(v, th, &flag, &checked);
        region[p] = r;
        if (rows_checked) rows_checked[p] = checked;
        if (exitflag) exitflag[p] = flag;
        if (r >= 0 && x) {
            const double *law = v.laws + (size_t)v.regions[8 * r + 2] * (nth + 1);
            for (int q = 0; q < nout; q++)
                x[(size_t)p * nout + q] = lmpc::explicit_affine<lmpc::kExplicitMaxNth>(law + (size_t)q * (nth + 1), th, nth);
        }
    }
    return LMPC_OK;
}

const char *lmpc_explicit_last_error(const lmpc_explicit *e) { return e ? e->err.c_str() : g_setup_err.c_str(); }

}  // extern "C"
