// The decisions and the host arithmetic of the swept solve (cfmm_solve_sweep, and solve_tiny_kinks, its one-point form): the
// active-set loop over the kinks of the constant-sum pools (cfmm/problem.py: Problem._solve_kinks) -- tie the two prices of a pool
// found on its kink, re-solve the now smooth reduced dual, recover the fill fractions, release ties whose fill leaves (0, 1) -- the
// bounds of the group variables, the schedule of the legs, and the certificates of a point with its fills folded in.  Host only:
// nothing of HIP, nothing of cfmm_ctx -- cfmm_hip.hip (cfmm_solve_sweep and its phases) gathers the inputs, tests/test_host.py
// exercises the rules.  Every sum keeps one fixed order of operations.
#pragma once

#include <algorithm>
#include <cmath>
#include <map>
#include <set>
#include <vector>
#include "../../include/cfmm.h"
#include "tiny_limits.hpp"

namespace sweep {

using cfmm::TINY_N;

// weighted union-find over the tokens of a tiny network: log nu_j = s[group(j)] + off[j]   (problem.py: _Ties)
struct Ties {
    int parent[TINY_N]; double off[TINY_N]; int n;
    void init(int n_) { n = n_; for (int j = 0; j < n; ++j) { parent[j] = j; off[j] = 0.0; } }
    int find(int j)
    {
        int path[TINY_N], np = 0;
        while (parent[j] != j) { path[np++] = j; j = parent[j]; }
        const int root = j;
        for (int q = np - 1; q >= 0; --q) {            // from the top of the path down: the parent's offset is already relative to the root
            const int node = path[q], p = parent[node];
            if (p != root) off[node] += off[p];
            parent[node] = root;
        }
        return root;
    }
    bool tie(int a, int b, double delta)               // log nu_a - log nu_b = delta; false if it contradicts the ties so far
    {
        const int ra = find(a), rb = find(b);
        if (ra == rb) return std::fabs((off[a] - off[b]) - delta) < 1e-12;
        off[ra] = delta + off[b] - off[a];
        parent[ra] = rb;
        return true;
    }
    int groups(int *grp)                               // group ids in the order of the (sorted) roots, as np.unique numbers them
    {
        int root[TINY_N]; bool is_root[TINY_N] = {};
        for (int j = 0; j < n; ++j) { root[j] = find(j); is_root[root[j]] = true; }
        int id[TINY_N], ng = 0;
        for (int j = 0; j < n; ++j) if (is_root[j]) id[j] = ng++;
        for (int j = 0; j < n; ++j) grp[j] = id[root[j]];
        return ng;
    }
};

struct Tie { int sgn; bool loose; };
struct SumCols { int64_t m; const int32_t *ia, *ib; const double *fee, *Ra, *Rb; };

// least squares  min |A th - b|  over th in [0, 1]^K for a handful of tied pools (A: R x K, row-major): the unconstrained solution
// where it lies inside the box; otherwise the best of the 3^K assignments {free, at 0, at 1} whose free part stays inside (exact for
// a convex problem: the optimum is one of them, and none of the others can beat it); beyond 7 unknowns the clipped solution
inline bool small_lsq(const std::vector<double> &A, const std::vector<double> &b, int R, int K, const std::vector<int> &freev, const std::vector<double> &fixed,
                      std::vector<double> &th)
{
    // free variables by the normal equations (a whiff of ridge: a rank-deficient system gets the small-norm solution, as lstsq does)
    const int F = (int)freev.size();
    th = fixed;
    if (F == 0) return true;
    std::vector<double> N((size_t)F * F, 0.0), g(F, 0.0), rb(b);
    for (int r = 0; r < R; ++r) for (int k = 0; k < K; ++k) rb[r] -= A[(size_t)r * K + k] * fixed[k];
    double tr = 0.0;
    for (int i = 0; i < F; ++i) {
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int r = 0; r < R; ++r) v += A[(size_t)r * K + freev[i]] * A[(size_t)r * K + freev[j]];
            N[(size_t)i * F + j] = N[(size_t)j * F + i] = v;
        }
        for (int r = 0; r < R; ++r) g[i] += A[(size_t)r * K + freev[i]] * rb[r];
        tr += N[(size_t)i * F + i];
    }
    const double ridge = 1e-14 * (tr > 0.0 ? tr / F : 1.0);
    for (int i = 0; i < F; ++i) N[(size_t)i * F + i] += ridge;
    for (int i = 0; i < F; ++i) {                       // Cholesky, in place
        for (int j = 0; j <= i; ++j) {
            double v = N[(size_t)i * F + j];
            for (int q = 0; q < j; ++q) v -= N[(size_t)i * F + q] * N[(size_t)j * F + q];
            if (i == j) { if (!(v > 0.0)) return false; N[(size_t)i * F + i] = std::sqrt(v); }
            else N[(size_t)i * F + j] = v / N[(size_t)j * F + j];
        }
    }
    for (int i = 0; i < F; ++i) { double v = g[i]; for (int q = 0; q < i; ++q) v -= N[(size_t)i * F + q] * g[q]; g[i] = v / N[(size_t)i * F + i]; }
    for (int i = F - 1; i >= 0; --i) { double v = g[i]; for (int q = i + 1; q < F; ++q) v -= N[(size_t)q * F + i] * g[q]; g[i] = v / N[(size_t)i * F + i]; }
    for (int i = 0; i < F; ++i) th[freev[i]] = g[i];
    return true;
}
inline void box_lsq(const std::vector<double> &A, const std::vector<double> &b, int R, int K, std::vector<double> &th)
{
    std::vector<int> all(K);
    for (int k = 0; k < K; ++k) all[k] = k;
    std::vector<double> zero(K, 0.0);
    if (!small_lsq(A, b, R, K, all, zero, th)) { th.assign(K, 0.5); return; }
    bool inside = true;
    for (double v : th) inside = inside && v >= 0.0 && v <= 1.0;
    if (inside) return;
    if (K > 7) { for (double &v : th) v = std::min(1.0, std::max(0.0, v)); return; }
    auto resid = [&](const std::vector<double> &t) { double s2 = 0.0; for (int r = 0; r < R; ++r) { double v = -b[r]; for (int k = 0; k < K; ++k) v += A[(size_t)r * K + k] * t[k]; s2 += v * v; } return s2; };
    std::vector<double> best(th);
    for (double &v : best) v = std::min(1.0, std::max(0.0, v));
    double best_r = resid(best);
    int total = 1; for (int k = 0; k < K; ++k) total *= 3;
    std::vector<int> fr; std::vector<double> fx(K), cand;
    for (int code = 1; code < total; ++code) {           // (code 0 = all free: done above)
        fr.clear();
        int c = code;
        for (int k = 0; k < K; ++k, c /= 3) { const int m3 = c % 3; fx[k] = m3 == 2 ? 1.0 : 0.0; if (m3 == 0) fr.push_back(k); }
        if (!small_lsq(A, b, R, K, fr, fx, cand)) continue;
        bool ok = true;
        for (int k : fr) ok = ok && cand[k] >= 0.0 && cand[k] <= 1.0;
        if (!ok) continue;
        const double rr = resid(cand);
        if (rr < best_r) { best_r = rr; best = cand; }
    }
    th = best;
}

// fill fractions of the tied constant-sum pools (problem.py: Problem._recover_fills): theta in [0, 1]^K with
// (psi + h + sum_k theta_k d_k)_j = 0 on every token that must balance, >= 0 on GE tokens at their bound
inline bool recover_fills(int n, const double *nu, const double *psi, const double *c, const double *h, const int32_t *ctype, const SumCols &sc,
                          const std::map<int, Tie> &tied, double tol, std::vector<double> &th)
{
    const int K = (int)tied.size();
    std::vector<double> D((size_t)n * K, 0.0);
    int k = 0;
    for (auto &kv : tied) {
        const int i = kv.first, a = sc.ia[i], b = sc.ib[i];
        const double g = sc.fee[i];
        if (kv.second.sgn > 0) { D[(size_t)a * K + k] = -sc.Rb[i] / g; D[(size_t)b * K + k] = sc.Rb[i]; }      // tender a, drain b
        else { D[(size_t)b * K + k] = -sc.Ra[i] / g; D[(size_t)a * K + k] = sc.Ra[i]; }
        ++k;
    }
    std::vector<double> A, rhs;
    std::vector<char> must(n), atb(n);
    int R = 0;
    for (int j = 0; j < n; ++j) {
        const int ct = ctype ? ctype[j] : CFMM_GE;
        const double hj = h ? h[j] : 0.0;
        atb[j] = ct == CFMM_GE && nu[j] <= c[j] * (1.0 + 1e-9);
        must[j] = ct == CFMM_EQ || (ct == CFMM_GE && !atb[j]);
        bool touched = false;
        for (int q = 0; q < K; ++q) touched = touched || D[(size_t)j * K + q] != 0.0;
        if (must[j] && touched) {
            for (int q = 0; q < K; ++q) A.push_back(D[(size_t)j * K + q] * nu[j]);
            rhs.push_back(-(psi[j] + hj) * nu[j]);
            ++R;
        }
    }
    if (R == 0) th.assign(K, 0.5);
    else if (K == 1) {
        double aa = 0.0, ab = 0.0;
        for (int r = 0; r < R; ++r) { aa += A[r] * A[r]; ab += A[r] * rhs[r]; }
        th.assign(1, std::min(1.0, std::max(0.0, ab / std::max(aa, 1e-300))));
    } else box_lsq(A, rhs, R, K, th);
    double scale = 0.0, res_eq = 0.0, res_ge = 0.0;
    for (int j = 0; j < n; ++j) {
        const double hj = h ? h[j] : 0.0;
        scale += std::fabs(nu[j] * (std::fabs(psi[j]) + std::fabs(hj)));
        double tot = psi[j] + hj;
        for (int q = 0; q < K; ++q) tot += D[(size_t)j * K + q] * th[q];
        if (must[j]) res_eq += std::fabs(nu[j] * tot);
        if (atb[j]) res_ge += std::max(-(nu[j] * tot), 0.0);
    }
    scale = std::max(1.0, scale);
    return res_eq / scale <= 10.0 * tol && res_ge / scale <= 10.0 * tol;
}

// constant-sum pools whose price ratio sits on one of their two kinks (problem.py: Problem._kink_candidates)
inline void kink_candidates(const double *nu, const SumCols &sc, double kink_tol, const std::set<std::pair<int, int>> &banned, const std::map<int, Tie> &tied,
                            bool loose, std::map<int, Tie> &out)
{
    out.clear();
    for (int64_t i = 0; i < sc.m; ++i) {
        const double r = std::log(nu[sc.ia[i]]) - std::log(nu[sc.ib[i]]), lg = std::log(sc.fee[i]);
        const int sgn = r < 0.0 ? 1 : -1;               // a->b kink at r = lg < 0, b->a kink at r = -lg > 0
        const double dist = std::fabs(r - sgn * lg);
        const bool near = dist < kink_tol && (dist < 0.5 * std::fabs(lg) || lg == 0.0 || loose);
        if (near && !tied.count((int)i) && !banned.count({(int)i, sgn})) out[(int)i] = Tie{sgn, loose};
    }
}

// The one bounds rule: bounds of the ng group variables from (c, ctype) and the ties (grp, off), lo / hi: [ng].
// A price the utility does not bound (c = 0; an equality) is still kept within e^+-100 of the utility's own scale: a WORTHLESS token's
// log-price otherwise runs off until nu underflows to zero and the pool arithmetic turns it into NaNs -- "dual value is not finite"
// instead of a stalled solve the caller can classify (tools/fuzz_table.py: a liquidation whose target no pool lists).
// Returns -1, or the index of the first CFMM_FREE token with c <= 0 (unbounded: the caller fails).
inline int group_bounds(int n, const double *c, const int *ctype, const int *grp, const double *off, int ng, double *lo, double *hi)
{
    for (int r = 0; r < ng; ++r) { lo[r] = -INFINITY; hi[r] = INFINITY; }
    double cmax = 0.0;
    for (int j = 0; j < n; ++j) if (ctype[j] < CFMM_ULOG) cmax = std::max(cmax, c[j]);
    const double mid = cmax > 0.0 ? std::log(cmax) : 0.0, span = 100.0;
    for (int j = 0; j < n; ++j) {
        const int r = grp[j];
        double l = mid - span, u = mid + span;
        if (ctype[j] >= CFMM_ULOG) { l = -INFINITY; u = INFINITY; }       // (the utility table's entries: no bound; their conjugates hold the price)
        if (ctype[j] == CFMM_GE) { l = c[j] > 0.0 ? std::log(c[j]) : mid - span; u = INFINITY; }
        else if (ctype[j] == CFMM_FREE) {
            if (!(c[j] > 0.0)) return j;
            l = u = std::log(c[j]);
        }
        l -= off[j]; u -= off[j];
        if (l > lo[r]) lo[r] = l;
        if (u < hi[r]) hi[r] = u;
    }
    return -1;
}

// what a leg (one one-workgroup solve) leaves of its state record: what the loop reads and the statistics report
struct LegResult { int status, evals, iters; double f, primal, gap, infeas, pg; };

struct PointState {
    std::map<int, Tie> tied;
    std::set<std::pair<int, int>> banned;
    std::vector<double> theta;              // of `tied`, in its order, once the fills are recovered
    int budget = 0, evals = 0, iters = 0, rounds = 0;
    double kink_tol = 1e-3;
    bool done = false, fills_ok = false;
    LegResult st = {};
};

// ---- the schedule of the legs ------------------------------------------------------------------------------------------------------
// legs: short where kinks may have to be found (problem.py: _solve_kinks); a network without constant-sum pools is ONE leg
inline int first_budget(int msum, int64_t pools, int max_evals) { return msum ? std::min(max_evals, pools <= 1000 ? 40 : 100) : max_evals; }
// a point that has spent four times the caller's budget over its legs gets no further one
inline bool exhausted(const PointState &S, int max_evals) { return S.evals >= 4 * max_evals; }

// ---- the head of a round: this round's ties, bounds and tolerance of one point (problem.py: _solve_kinks, the head of its loop) -------
// Rebuilds the ties from S.tied: a record that contradicts the ties before it is dropped and banned.  Writes the tied-pool flags
// [sc.m], the groups and offsets [n] and the group bounds (the first ng entries; the rest of [n] is left unbounded).
struct RoundHead {
    int ng;
    bool tied;
    double tol_factor;      // of the caller's tolerance: a reduced dual is solved two decades tighter (the fills are recovered from its residual)
    int pg_rule;
};
inline RoundHead round_head(PointState &S, const SumCols &sc, int n, const double *c, const int *ctype, int *flags, int *grp, double *off, double *glo, double *ghi)
{
    Ties ties; ties.init(n);
    for (int64_t i = 0; i < sc.m; ++i) flags[i] = 0;
    for (auto it = S.tied.begin(); it != S.tied.end();) {
        const int i = it->first;
        if (ties.tie(sc.ia[i], sc.ib[i], it->second.sgn * std::log(sc.fee[i]))) { flags[i] = 1; ++it; }
        else { S.banned.insert({i, it->second.sgn}); it = S.tied.erase(it); }
    }
    RoundHead r;
    r.ng = n;
    if (!S.tied.empty()) { r.ng = ties.groups(grp); for (int j = 0; j < n; ++j) off[j] = ties.off[j]; }
    else for (int j = 0; j < n; ++j) { grp[j] = j; off[j] = 0.0; }
    (void)group_bounds(n, c, ctype, grp, off, r.ng, glo, ghi);          // (a CFMM_FREE token without c > 0 never gets here: refused with the arguments)
    for (int q = r.ng; q < n; ++q) { glo[q] = -INFINITY; ghi[q] = INFINITY; }
    r.tied = !S.tied.empty();
    r.tol_factor = r.tied ? 0.01 : 1.0;
    r.pg_rule = r.tied ? 1 : 0;
    return r;
}

// ---- the tail of a round: the host's half of the active-set loop for one point (problem.py: _solve_kinks, the tail of its loop) ------
// leg: what the point's leg left; nu, psi: its accepted prices and their net trade.  Ends the point (S.done) or leaves it the ties,
// bans, budget and kink tolerance of its next leg.
inline void round_tail(PointState &S, const LegResult &leg, int n, const double *nu, const double *psi, const double *c, const double *h, const int32_t *ctype,
                       const SumCols &sc, double tol, int max_evals)
{
    S.st = leg; S.evals += leg.evals; S.iters += leg.iters; S.rounds += 1;
    const int status = leg.status ? leg.status : 3;
    if (!std::isfinite(leg.f)) { S.done = true; S.st.status = CFMM_E_NUMERIC; return; }
    if (status == 1) {
        if (S.tied.empty()) { S.done = true; return; }
        const bool ok = recover_fills(n, nu, psi, c, h, ctype, sc, S.tied, tol, S.theta);
        std::vector<int> bad;
        { int k = 0; for (auto &kv : S.tied) { if (!(S.theta[k] > 1e-9 && S.theta[k] < 1.0 - 1e-9)) bad.push_back(kv.first); ++k; } }
        if (ok && bad.empty()) { S.done = true; S.fills_ok = true; return; }
        if (!bad.empty()) {                        // fully on / fully off after all: back to bang-bang
            int k = 0;
            std::map<int, double> th_of;
            for (auto &kv : S.tied) th_of[kv.first] = S.theta[k++];
            for (int i : bad) {
                const Tie rec = S.tied[i];
                S.tied.erase(i);
                S.banned.insert({i, rec.sgn});
                // a guessed kink that carries no trade: the optimum sits on the pool's OTHER kink (fee bands narrower than a leg resolves)
                if (rec.loose && th_of[i] <= 1e-9 && !S.banned.count({i, -rec.sgn})) S.tied[i] = Tie{-rec.sgn, false};
            }
            S.theta.clear();
            return;
        }
    }
    std::map<int, Tie> fresh;
    kink_candidates(nu, sc, S.kink_tol, S.banned, S.tied, false, fresh);
    double wide = S.kink_tol;
    while (fresh.empty() && status != 1 && wide < 0.05) { wide *= 10.0; kink_candidates(nu, sc, wide, S.banned, S.tied, true, fresh); }
    if (!fresh.empty()) {
        for (auto &kv : fresh) S.tied[kv.first] = kv.second;
        for (auto it = S.banned.begin(); it != S.banned.end();) { if (fresh.count(it->first)) ++it; else it = S.banned.erase(it); }      // bans expire when the active set changes
    } else if (status == 3 && S.budget < max_evals) S.budget = std::min(max_evals, 2 * S.budget);     // no kink in sight: longer legs
    else if (S.kink_tol < 0.05) S.kink_tol *= 10.0;
    else S.done = true;
    S.theta.clear();
}

// ---- a certified point with its fills folded in (cfmm_solve on a small network with constant-sum pools) ------------------------------
// psi_total = psi + sum theta d, the tied pools' tenders = theta x their full fill (cfmm.h: cfmm_solve_sweep).  theta: NaN where the
// pool is not tied; delta, lambda: the constant-sum bucket's block of the tenders, [2][m] each.
inline void fold_fills(const SumCols &sc, const double *theta, const int32_t *tsgn, double *psi, double *delta, double *lambda)
{
    for (int64_t i = 0; i < sc.m; ++i) {
        if (!std::isfinite(theta[i])) continue;
        const double ya = (tsgn[i] > 0 ? -sc.Rb[i] / sc.fee[i] : sc.Ra[i]) * theta[i];
        const double yb = (tsgn[i] > 0 ? sc.Rb[i] : -sc.Ra[i] / sc.fee[i]) * theta[i];
        psi[sc.ia[i]] += ya; psi[sc.ib[i]] += yb;
        delta[i] = std::max(-ya, 0.0); delta[sc.m + i] = std::max(-yb, 0.0);
        lambda[i] = std::max(ya, 0.0); lambda[sc.m + i] = std::max(yb, 0.0);
    }
}

// the certificates of the whole point (as cfmm/problem.py: _solve_sweep computes them).  Infeasibility is relative to the larger of
// trade and offset, but never to less than 1e-12 of the largest reserve
struct PointCertificates { double value, dual, gap, infeas; };
inline PointCertificates point_certificates(int n, const double *nu, const double *psi, const double *c, const double *h, const int32_t *ctype, double max_reserve)
{
    double value = 0.0, cs = 0.0, dual = 0.0, viol = 0.0, scale = 0.0;
    for (int j = 0; j < n; ++j) {
        const double r = psi[j] + h[j];
        value += c[j] * psi[j]; cs += (nu[j] - c[j]) * r; dual += (nu[j] - c[j]) * h[j] + nu[j] * psi[j];
        viol = std::max(viol, ctype[j] == CFMM_GE ? std::max(-r, 0.0) : (ctype[j] == CFMM_EQ ? std::fabs(r) : 0.0));
        scale = std::max(scale, std::max(std::fabs(psi[j]), std::fabs(h[j])));
    }
    PointCertificates k;
    k.value = value; k.dual = dual;
    k.gap = std::fabs(cs) / std::max(1.0, std::fabs(dual));
    k.infeas = viol / std::max(std::max(scale, 1e-12 * max_reserve), 1e-300);
    return k;
}

}  // namespace sweep
