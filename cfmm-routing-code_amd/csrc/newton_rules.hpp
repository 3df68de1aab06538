// The decisions and the host arithmetic of the second-order (barrier path) solve: what a token contributes to the smoothed dual and
// to the certificates, when an old factor may serve a step (chord steps), how the barrier weight and the diagonal shift move, and
// the trial point of a line-search pass.  Host only: nothing of HIP, nothing of cfmm_ctx -- cfmm_hip.hip (solve_newton and its
// phases) gathers the inputs, tests/test_host.py exercises the rules.  Every sum keeps one fixed order of operations: token order.
#pragma once

#include <algorithm>
#include <cmath>
#include "../../include/cfmm.h"

namespace newton {

// the utility table's entries on the host (the second-order loop keeps the utility on the host): the numbers of
// lbfgs::utility_term (lbfgs_rules.hpp), + nu^2 ubar''(nu) for the Hessian's diagonal in log-prices
struct HostUtilityTerm { double pstar, ubar, uval, viol, d2; };
inline HostUtilityTerm host_utility_term(int ctype, double c, double h, double nu, double psi)
{
    HostUtilityTerm t;
    if (ctype == CFMM_ULOG) {
        t.pstar = c / nu - h; t.ubar = c * std::log(c / nu) - c + nu * h;
        t.viol = std::max(-(psi + h), 0.0); t.uval = c * std::log(std::max(psi + h, 1e-300)); t.d2 = c;
    } else {
        t.pstar = h * (c - nu); t.ubar = 0.5 * h * (c - nu) * (c - nu);
        t.viol = 0.0; t.uval = c * psi - 0.5 * psi * psi / h; t.d2 = h * nu * nu;
    }
    return t;
}

// What the rules read of the tokens: the utility (c, h, ctype), and what the prologue's pass (token_pass) derives from it.
struct Tokens {
    int n = 0;
    const double *c = nullptr, *h = nullptr;
    const int *ctype = nullptr;
    const char *listed = nullptr;   // 0: the dual is flat in the token's price (token_pass)
    const int *mask = nullptr;      // pinned for the whole solve: CFMM_FREE, or flat
    const double *lob = nullptr;    // lower bound of the log-price: log c for a GE token with c > 0 (handled by projection)
    long long nbar = 0;             // barrier terms: of the pools (of every rank) + one per barrier token
    // (infeasibility is relative to the larger of trade and offset -- but never to less than 1e-12 of the largest reserve: at a
    //  no-arbitrage optimum the smoothed point's trades are rounding noise, and noise over noise is not an infeasibility;
    //  tools/fuzz_small.py)
    double infeas_floor = 0.0;      // 1e-12 * the largest reserve
    bool table(int j) const { return ctype[j] >= CFMM_ULOG; }
    // a GE token with c = 0 that some pool lists: nu_j > 0 is kept by a barrier term -mu log nu_j
    bool barrier_token(int j) const { return ctype[j] == CFMM_GE && !(c[j] > 0.0) && listed[j]; }
    bool has_table_entry() const { for (int j = 0; j < n; ++j) if (table(j)) return true; return false; }
};

// The prologue's pass over the tokens, from the utility, the pools' token lists and the start prices (nu: projected in place).
// listed[j] = 0 -- "flat": the dual does not depend on nu_j at all -- no pool lists the token AND its offset is zero (one of the
// reference's linear-box kinds): pinned, and without its barrier term.  (Unlisted with h_j > 0, GE: nu_j h_j - mu log nu_j has its
// minimum at mu / h_j and follows the barrier to zero, the free-disposal optimum: left alone.)
// Returns -1, or the index of a CFMM_FREE token with c = 0 (unbounded: the caller fails); *barrier_tokens: the local count.
inline int token_pass(int n, const double *c, const double *h, const int *ctype, const char *pool_lists, double *nu, char *listed,
                      int *mask, double *lob, double *s, long long *barrier_tokens)
{
    Tokens tk; tk.n = n; tk.c = c; tk.h = h; tk.ctype = ctype; tk.listed = listed;
    for (int j = 0; j < n; ++j) listed[j] = !(ctype[j] < CFMM_ULOG && !pool_lists[j] && h[j] == 0.0);
    *barrier_tokens = 0;
    for (int j = 0; j < n; ++j) {
        mask[j] = ctype[j] == CFMM_FREE || !listed[j];              // (a token the dual is flat in: its price stays where it starts)
        lob[j] = (ctype[j] == CFMM_GE && c[j] > 0.0) ? std::log(c[j]) : -INFINITY;
        if (tk.barrier_token(j)) *barrier_tokens += 1;
        double sj = std::log(nu[j]);
        if (ctype[j] == CFMM_FREE) {
            if (!(c[j] > 0.0)) return j;
            sj = std::log(c[j]);
        } else sj = std::max(sj, lob[j]);
        s[j] = sj; nu[j] = std::exp(sj);
    }
    return -1;
}

// the dual value at the start prices: the exact pools' value plus the utility's terms IN TOKEN ORDER (it sets the first weight)
inline double start_dual(const Tokens &tk, const double *nu, double arb)
{
    double dual = arb;
    for (int j = 0; j < tk.n; ++j) dual += tk.table(j) ? host_utility_term(tk.ctype[j], tk.c[j], tk.h[j], nu[j], 0.0).ubar : (nu[j] - tk.c[j]) * tk.h[j];
    return dual;
}

// smoothed dual value and its gradient in log-prices at the prices p from one smoothed evaluation (psi, value); grad, hdiag: may be null
inline double assemble(const Tokens &tk, const double *p, const double *psi, double value, double mu, double *grad, double *hdiag)
{
    double g = value;
    for (int j = 0; j < tk.n; ++j) {
        double Gj, hj = 0.0;
        if (tk.table(j)) {                            // the utility table: conjugate, gradient nu (psi - P*), nu^2 ubar'' on the diagonal
            const HostUtilityTerm ut = host_utility_term(tk.ctype[j], tk.c[j], tk.h[j], p[j], psi[j]);
            g += ut.ubar;
            Gj = p[j] * (psi[j] - ut.pstar);
            hj = ut.d2;
        } else {
            g += (p[j] - tk.c[j]) * tk.h[j];
            Gj = p[j] * (psi[j] + tk.h[j]);
        }
        // (the diagonal's own term: d^2/ds^2 of nu_j (psi_j + h_j) at fixed psi is nu_j (psi_j + h_j) itself -- taken BEFORE the barrier's
        //  -mu, which is linear in the log-price and has no curvature: with it folded in the entry vanished exactly where a barrier
        //  token sits at its optimum nu_j = mu / (psi_j + h_j), and a token no pool lists -- nothing else on its row -- made the
        //  system singular: tools/fuzz_small.py, a swap whose offered token is unlisted)
        const double Gj_lin = Gj;
        if (tk.barrier_token(j)) {                    // nu_j > 0: the barrier is -mu log nu_j, linear in the log-price
            g -= mu * std::log(p[j]);
            Gj -= mu;
        }
        if (grad) grad[j] = tk.mask[j] ? 0.0 : Gj;
        if (hdiag) hdiag[j] = std::max(Gj_lin, 0.0) + hj;
    }
    return g;
}

// The certificate sums of a point (nu, psi): psi the smoothed tenders (the loop) or the exact ones (the exact certificate).
struct Certificate {
    double lin = 0.0;        // the utility's part of the dual value
    double primal = 0.0;     // the utility of psi
    double cs = 0.0;         // complementarity (a table entry: its Fenchel-Young gap term, lbfgs_rules.hpp)
    double viol = 0.0, scale = 0.0;
    double infeas(const Tokens &tk) const { return viol / std::max(std::max(scale, tk.infeas_floor), 1e-300); }
};
inline Certificate certificate(const Tokens &tk, const double *nu, const double *psi)
{
    Certificate k;
    for (int j = 0; j < tk.n; ++j) {
        if (tk.table(j)) {
            const HostUtilityTerm ut = host_utility_term(tk.ctype[j], tk.c[j], tk.h[j], nu[j], psi[j]);
            k.lin += ut.ubar; k.primal += ut.uval;
            k.cs += ut.ubar + nu[j] * psi[j] - ut.uval;
            k.viol = std::max(k.viol, ut.viol);
            k.scale = std::max(k.scale, std::max(std::fabs(psi[j]), std::fabs(ut.pstar)));
            continue;
        }
        const double r = psi[j] + tk.h[j];
        k.lin += (nu[j] - tk.c[j]) * tk.h[j];
        k.primal += tk.c[j] * psi[j];
        k.cs += (nu[j] - tk.c[j]) * r;
        k.viol = std::max(k.viol, tk.ctype[j] == CFMM_GE ? std::max(-r, 0.0) : (tk.ctype[j] == CFMM_EQ ? std::fabs(r) : 0.0));
        k.scale = std::max(k.scale, std::max(std::fabs(psi[j]), std::fabs(tk.h[j])));
    }
    return k;
}

// The certificate of an EXACT evaluation (psi, arb) at nu.  Prices inside the utility's box at which psi + h is feasible and
// complementary ARE the optimum.  Linear-box utilities only: a table entry refuses it.
struct ExactCertificate { bool holds; double dual, gap, infeas, primal; };
inline ExactCertificate exact_certificate(const Tokens &tk, const double *nu, const double *psi, double arb, double tol_gap, double tol_infeas)
{
    ExactCertificate x = {false, 0.0, 0.0, 0.0, 0.0};
    if (tk.has_table_entry()) return x;
    const Certificate k = certificate(tk, nu, psi);
    x.dual = k.lin + arb;
    x.gap = std::fabs(k.cs) / std::max(1.0, std::fabs(x.dual));
    x.infeas = k.infeas(tk);
    x.primal = k.primal;
    x.holds = std::isfinite(x.dual) && x.gap <= tol_gap && x.infeas <= tol_infeas;
    return x;
}

// ---- chord steps ------------------------------------------------------------------------------------------------------------------
// Chord steps (round 4).  A step's direction needs H^-1 G; with the inverse factor W = L^-1 riding the factorisation
// (chol.hpp) the factor of an EARLIER step applies to a new gradient in two matrix-vector products (~20 us against ~400 for a
// fresh factorisation + solve), and such a step needs no Hessian assembly either.  Between two steps of the path the
// ONLY at an unchanged barrier weight: measured on config 5, a factor from the previous weight (10x larger) gives
// directions whose full step the Armijo test refuses (t = 1/8 .. 1/16) and the solve takes 20-24 steps instead of 9,
// 10.2-12.4 ms instead of 6.3 -- near their peg the stableswap pools' curvature terms kappa = 1 / (mu / D^2 - nu L'') follow
// the weight.  At the SAME weight (the centring steps at the final weight, which is where the step count of the path is
// decided) the Hessian barely moves: up to `chord_max` such steps in a row reuse the last factor; a chord direction that is not
// a descent direction, or whose full step the Armijo test refuses, sends the step back to a fresh factorisation.
// Pool-sharded: every rank holds the same all-reduced Hessian, factors it identically (fixed summation orders: chol.hpp) and
// takes these decisions on the same numbers -- the ranks stay in step.  CFMM_CHORD=0 switches it off (A/B).
// ... and only behind a step that was taken in full: where the Armijo test has just cut a fresh Newton step (the shipped
// instances' partially filled constant-sum pool: t = 1/4) the iteration is outside the region in which an old Hessian
// serves -- chord steps there were cut to 1/8 .. 1/128 and the solve took 34 steps instead of 10.
// (not in the low-order regime either -- moves below ~1e-10 in log-price, where a partially filled constant-sum pool's
//  fill reacts to price changes under the fp64 resolution of the prices: the Hessian changes by orders of magnitude from
//  step to step there, and steps on a stale one only feed the stall counter)
// The rule serves two questions.  "This step": the facts of the last accepted step.  "The step after this trial, were it accepted"
// (it decides whether the trial's evaluation carries a Hessian): the trial's move and regime, full = the first pass, and the run
// counted with this step if it is a chord step itself.
struct ChordFacts {
    bool fac_valid;          // a factor is held (the last factorisation was positive definite)
    double fac_mu, mu;       // its barrier weight, and the weight now
    bool full_step;          // the step behind which the chord step would come was (would be) taken in full
    bool slo;                // the low-order regime, at the point the chord step would start from
    double move;             // the largest log-price move of that step
    bool chord_bad;          // the factor has been refused since it was made
    int chord_run, chord_max;
    double reg;              // the diagonal shift
    bool inverse_factor;     // the inverse factor is kept (CFMM_BACKSUB) and allocated
};
inline bool chord_allowed(const ChordFacts &f)
{
    return f.fac_valid && f.fac_mu == f.mu && f.full_step && !f.slo && f.move > 1e-10 && !f.chord_bad && f.chord_run < f.chord_max && f.reg == 0.0 && f.inverse_factor;
}
// the old factor must still give a descent direction on the free tokens (dc = -G'd, finite)
// ... and the iteration must be contracting fast under it: a chord step shrinks the decrement by the square of its
// contraction factor, so "at least a hundredfold since the last step" = a factor <= 0.1 per step.  The shipped
// instances' final centring (a partially filled constant-sum pool, steps below the resolution of the log-prices)
// contracts only 3x per chord step where ONE fresh Newton step finishes: 30 steps instead of 24 without this test.
inline bool chord_direction_serves(bool finite, double dc, double dec_prev) { return finite && dc > 0.0 && dc <= 1e-2 * dec_prev; }

// ---- the barrier schedule -----------------------------------------------------------------------------------------------------------
struct Schedule {
    double mu = 0.0, sigma = 0.1, reg = 0.0;
    int stalled = 0, forced_shrinks = 0;
    bool shrink_now = false;
    double best_infeas = 1.7976931348623157e308;
};

inline double first_weight(double mu0_scale, double dual, long long nbar, double warm_mu, double warm_mult)
{
    double mu = mu0_scale * std::max(std::fabs(dual), 1e-300) / (double)std::max<long long>(nbar, 1);
    if (warm_mu > 0.0) mu = std::min(mu, warm_mult * warm_mu);
    return mu;
}
// (the exact evaluation is skipped while the barrier's bound on its share of the gap, sub = mu nbar, is still far from the tolerance,
//  and while psi_mu is still far from feasible: no certificate can hold at this point, and the bound serves the barrier schedule
//  just as well -- three evaluations of ~0.14 ms less per config-5 solve)
inline bool exact_due(int steps, double sub, double dual, double infeas, double tol_gap, double tol_infeas)
{
    return steps == 0 || (sub <= 10.0 * tol_gap * std::max(1.0, std::fabs(dual)) && infeas <= 10.0 * tol_infeas);
}
// sub = sum_i arb_i(nu) - nu'(L - D) >= 0 is the part of the gap the barrier weight controls (<= mu nbar);
// the rest, the complementarity term cs, vanishes with the centring.  The weight stops shrinking as soon as
// sub alone fits the tolerance: pushing it further only stiffens the smoothed dual (flows then react to price
// changes below fp64 resolution and the feasibility of psi_mu stops improving).
inline bool weight_is_final(double sub, double dual, double tol_gap) { return sub <= 0.5 * tol_gap * std::max(1.0, std::fabs(dual)); }
// the barrier weight stays behind this step: final, or the step's decrement says the point is not centred yet
inline bool weight_stays(bool final_mu, double dec, double mu, long long nbar) { return final_mu || !(dec < 10.0 * mu * (double)nbar); }
// ... and otherwise shrinks behind an accepted step taken in full, or one whose decrement is three decades under the weight's share
inline bool weight_shrinks(bool final_mu, double dec, double mu, long long nbar, bool full_step)
{
    return !weight_stays(final_mu, dec, mu, nbar) && (full_step || dec < 1e-3 * mu * (double)nbar);
}
// Centring at the final weight: give up (before moving, so that nu, psi and the certificates stay those of one point) once the
// Newton decrement is at rounding level and the feasibility of psi_mu has stopped improving all the same.  True: stalled.
inline bool final_weight_stalls(Schedule &sc, double infeas, double dec, double gmu, double gap, double tol_gap, double tol_infeas)
{
    if (infeas < 0.5 * sc.best_infeas) { sc.best_infeas = infeas; sc.stalled = 0; }
    else if (dec <= 1e-13 * std::max(1.0, std::fabs(gmu))) {
        // centred, feasible, and the gap a hair over the tolerance (1.01e-7 against 1e-7: tools/fuzz_table.py seeds 733, 757): what
        // is left of it is the complementarity term, which scales with the weight like the barrier's own share -- the weight
        // was final by that share alone.  One more decade of it (at most three) instead of four idle steps and "stalled".
        if (infeas <= tol_infeas && std::fabs(gap) > tol_gap && sc.forced_shrinks < 3) { sc.shrink_now = true; ++sc.forced_shrinks; }
        else ++sc.stalled;
    }
    return sc.stalled >= 4;
}
// not positive definite: shift the diagonal (md: the largest diagonal entry / gradient magnitude) and assemble again.  False: the
// shift has left the range of the numbers
inline bool raise_shift(Schedule &sc, double md)
{
    sc.reg = sc.reg == 0.0 ? 1e-12 * std::max(md, 1e-300) : sc.reg * 100.0;
    return sc.reg < 1e300;
}
// a singular Hessian (tokens no pool connects) tends to stay singular: keep most of the shift
inline void relax_shift(Schedule &sc) { sc.reg = sc.reg > 0.0 ? 0.1 * sc.reg : 0.0; }

// ---- the step ---------------------------------------------------------------------------------------------------------------------
// Newton direction: (H + diag) d = -G on the unpinned tokens.  Pinned: the masked tokens, and (projected Newton) every GE token
// sitting on its bound nu = c with the gradient pushing it further down.  G: zeroed where pinned; hdiag: + the shift.
inline void pin_and_right_hand_side(const Tokens &tk, const double *s, const double *slo, double reg, double *G, double *hdiag, int *pin, double *rhs)
{
    for (int j = 0; j < tk.n; ++j) {
        pin[j] = tk.mask[j] || (s[j] + slo[j] <= tk.lob[j] + 1e-13 * std::max(1.0, std::fabs(tk.lob[j])) && G[j] > 0.0);
        if (pin[j]) G[j] = 0.0;
        rhs[j] = -G[j]; hdiag[j] += reg;
    }
}

// step length: cap on the log-price move
inline double first_step_length(double max_step, double dmax) { return std::min(1.0, max_step / std::max(dmax, 1e-300)); }

// The trial point of a line-search pass at step length t: fraction to the boundary nu > c by projection on the lower bound.
// steps below the fp64 resolution of the log-prices go into their low-order part (smooth.hpp: apply_slo): the `small` regime
struct Trial { bool small; double gd; };      // gd = G'(projected move): the Armijo slope of the projected step
inline Trial trial_point(const Tokens &tk, const double *s, const double *nu, const double *slo, const double *d, const double *G, double t,
                         double dmax, bool final_mu, double *s2, double *nu2, double *slo2)
{
    double lo_max = 0.0;
    for (int j = 0; j < tk.n; ++j) lo_max = std::max(lo_max, std::fabs(slo[j] + t * d[j]));
    Trial tr;
    tr.small = final_mu && t * dmax < 1e-11 && lo_max < 1e-10;
    tr.gd = 0.0;
    for (int j = 0; j < tk.n; ++j) {
        if (tr.small) { s2[j] = s[j]; nu2[j] = nu[j]; slo2[j] = tk.mask[j] ? 0.0 : std::max(slo[j] + t * d[j], tk.lob[j] - s[j]); }
        else { s2[j] = std::max(s[j] + slo[j] + t * d[j], tk.lob[j]); nu2[j] = tk.mask[j] ? nu[j] : std::exp(s2[j]); slo2[j] = 0.0; }
        tr.gd += G[j] * ((s2[j] + slo2[j]) - (s[j] + slo[j]));
    }
    return tr;
}
// Armijo back-tracking on the smoothed dual
// (the value carries a few units of rounding of its own -- fp64 atomics over tens of thousands of pools: at the final weight the
//  required decrease armijo * gd falls BELOW one ulp of g_mu, and whether the full Newton step passed was decided by summation
//  noise: the same state took t = 1 and converged in one run and backed off to t = 1/16 and stalled in the next; round 5)
inline bool trial_accepted(double g2, double gmu, double armijo, double gd, double dec)
{
    return g2 <= gmu + armijo * gd + 2e-15 * std::fabs(gmu) || dec <= 1e-13 * std::fabs(gmu);
}
constexpr int LINE_SEARCH_PASSES = 40;

// a price that has collapsed by e^-60 since the start: a token that must be traded away but that no pool takes (the program is
// infeasible); no point in going on
inline bool price_collapsed(const Tokens &tk, const double *s, const double *s_start)
{
    bool collapsed = false;
    for (int j = 0; j < tk.n; ++j) collapsed = collapsed || (!tk.mask[j] && s[j] < s_start[j] - 60.0);
    return collapsed;
}

}  // namespace newton
