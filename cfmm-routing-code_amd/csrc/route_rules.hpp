// The decisions and the host arithmetic of the calls that handle a finished solve's route: the read-backs (cfmm_get_trades2 / N / G),
// the swept solve's tenders, cfmm_apply_trades and cfmm_audit_trades.  The order of the resident buckets -- part of the ABI: "the first
// pool in bucket order" of cfmm_apply_info and cfmm_audit, the swept solve's `trades` layout -- and the slot each bucket's record
// has; the layouts of host-held tenders; the folds of the per-bucket records into a report; the audited psi from its limbs, and its
// value and infeasibility under the utility; which point the tenders belong to.  Host only: nothing of HIP, nothing of cfmm_ctx --
// cfmm_hip.hip gathers the inputs, tests/test_host.py exercises the rules.  Every sum keeps one fixed order of operations.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include "../../include/cfmm.h"
#include "fixedpoint.hpp"

namespace cfmm {

// what a WRITE = false pass of cfmm_apply_trades leaves per bucket (apply.hpp; zeroed, `first` all ones, before the pass)
struct ApplyRec {
    unsigned long long moved;         // pools with a non-zero tender
    unsigned long long refused;       // pools with a leg that would not stay positive and finite
    unsigned long long first;         // smallest upload-order position among them
    unsigned long long maxbits;       // bit pattern of the largest new reserve (positive doubles order like their bits)
};

// doubles as unsigned integers of the same order (NaN counts as -inf: a quantity that cannot be computed is the worst one)
CFMM_FX_HD unsigned long long audit_ord(double x)
{
    if (x != x) x = -__builtin_huge_val();
    unsigned long long b;
    __builtin_memcpy(&b, &x, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double audit_unord(unsigned long long u)
{
    const unsigned long long b = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    double x;
    __builtin_memcpy(&x, &b, sizeof x);
    return x;
}

// one per bucket slot of cfmm_audit_trades (audit.hpp; and one partial per workgroup): counts, the smallest slack with the lowest upload
// position that holds it, the smallest tender and leg ratio (audit_ord images), and the workgroups that have left their partial
// (zeroed before the pass)
struct AuditRec {
    unsigned long long trading, violating, oor, slack, pos, tender, leg, done;
};

}  // namespace cfmm

namespace route {

// ---- bucket slots: one per record of the store's r2 | rn | rg[0] | rg[1] ------------------------------------------------------------
constexpr int KS = CFMM_MAX_POOL_SIZE + 1;                  // a family's records are indexed by k itself (the sizes no bucket has stay empty)
constexpr int SLOTS = CFMM_POOL_KINDS2 + KS + CFMM_POOLK_KINDS * KS;
constexpr int slot2(int kind) { return kind; }
constexpr int slotN(int k) { return CFMM_POOL_KINDS2 + k; }
constexpr int slotG(int kind, int k) { return CFMM_POOL_KINDS2 + KS * (1 + kind) + k; }

// a slot as cfmm_apply_info and cfmm_audit name it: family 0 two-asset (kind, k = 2), 1 geo-mean (kind 0, k), 2 the K-asset table (kind, k);
// no slot (q < 0): -1 each
struct SlotName { int family, kind, k; };
inline SlotName slot_name(int q)
{
    if (q < 0) return {-1, -1, -1};
    if (q >= slotG(0, 0)) return {2, (q - slotG(0, 0)) / KS, (q - slotG(0, 0)) % KS};
    if (q >= slotN(0)) return {1, 0, q - slotN(0)};
    return {0, q, 2};
}

// THE bucket order: two-asset kinds 0.., then geo-mean sizes 3..8, then the table's kinds, each by size 2..8 -- ascending slots.
// f(slot, family, kind, k) for every bucket a store can hold
template <class F> void each_slot(F &&f)
{
    for (int kind = 0; kind < CFMM_POOL_KINDS2; ++kind) f(slot2(kind), 0, kind, 2);
    for (int k = 3; k <= CFMM_MAX_POOL_SIZE; ++k) f(slotN(k), 1, 0, k);
    for (int kind = 0; kind < CFMM_POOLK_KINDS; ++kind)
        for (int k = 2; k <= CFMM_MAX_POOL_SIZE; ++k) f(slotG(kind, k), 2, kind, k);
}

struct Counts { int64_t m[SLOTS]; };                        // pools per slot (0: an empty bucket, or a slot no bucket has)

// ---- layouts of tenders ----------------------------------------------------------------------------------------------------------------
// the per-point layout of the tenders cfmm_solve_sweep hands out (and the kink loop's tenders keep): for every bucket in the order
// two-asset kinds 0.., then K = 3..8: delta [k][m] | lambda [k][m]
struct TradeLayout {
    size_t off2[CFMM_POOL_KINDS2], offn[KS], stride;                            // a bucket's first double; doubles per point
    size_t two_asset() const { return offn[3]; }                                // doubles of the two-asset kinds, which come first
};
inline TradeLayout trade_layout(const Counts &c)
{
    TradeLayout t = {};
    size_t off = 0;
    for (int k = 0; k < CFMM_POOL_KINDS2; ++k) { t.off2[k] = off; off += 4 * (size_t)c.m[slot2(k)]; }
    for (int k = 3; k <= CFMM_MAX_POOL_SIZE; ++k) { t.offn[k] = off; off += 2 * (size_t)k * c.m[slotN(k)]; }
    t.stride = off;
    return t;
}

// the device copy of the tenders an audit finds on the host: the kink loop's two-asset block (TradeLayout, while `kink`), then the
// caller's own for the constant-sum buckets it names -- the two-asset one (delta [2][m] | lambda [2][m]), then each k-asset one
// (delta [k][m] | lambda [k][m]).  An empty bucket's arrays are ignored.  half: the slot of the first bucket that names one array
// without the other (-1: none; nothing behind it is laid out)
struct AuditStage {
    size_t len, off_own2, off_ownk[KS];
    bool own2, ownk[KS];
    int half;
};
inline AuditStage audit_stage(const Counts &c, bool kink, const cfmm_audit_tenders *own)
{
    AuditStage s = {};
    s.half = -1;
    s.len = kink ? trade_layout(c).two_asset() : 0;
    if (!own) return s;
    const int64_t m2 = c.m[slot2(CFMM_POOL_SUM2)];
    s.own2 = m2 > 0 && (own->sum2_delta || own->sum2_lambda);
    if (s.own2 && !(own->sum2_delta && own->sum2_lambda)) { s.half = slot2(CFMM_POOL_SUM2); return s; }
    if (s.own2) { s.off_own2 = s.len; s.len += 4 * (size_t)m2; }
    for (int k = 2; k <= CFMM_MAX_POOL_SIZE; ++k) {
        const int64_t m = c.m[slotG(CFMM_POOLK_SUM, k)];
        if (m == 0 || !(own->sumk_delta[k] || own->sumk_lambda[k])) continue;
        if (!(own->sumk_delta[k] && own->sumk_lambda[k])) { s.half = slotG(CFMM_POOLK_SUM, k); return s; }
        s.ownk[k] = true; s.off_ownk[k] = s.len; s.len += 2 * (size_t)k * m;
    }
    return s;
}

// the audit's device scratch, in bytes: one record per slot | the [3][n] limbs | (256-aligned) `parts` partial records per slot; the
// pinned copy ends where the partials begin
struct AuditSpan { size_t recs, limbs, parts, total; };
inline AuditSpan audit_span(int n, int parts_per_slot)
{
    AuditSpan s;
    s.recs = 0; s.limbs = SLOTS * sizeof(cfmm::AuditRec);
    s.parts = (s.limbs + 3 * (size_t)n * sizeof(unsigned long long) + 255) & ~(size_t)255;
    s.total = s.parts + (size_t)SLOTS * parts_per_slot * sizeof(cfmm::AuditRec);
    return s;
}
inline int fixed_exponent(double sc)                         // F of sc = 2^F (the fixed-point scale of det_scales)
{
    int F = 0;
    (void)std::frexp(sc, &F);
    return F - 1;
}

// ---- the records folded into a report ---------------------------------------------------------------------------------------------------
// the apply's checking pass: totals, the first refused slot in bucket order with the position its record holds (-1s: none), and the
// largest reserve per slot and overall, exact (the pass visited every pool), as a fresh upload would record it.  Only slots that hold
// pools are read, on purpose: no launch wrote an empty slot's record, so whatever it holds is not this pass's
struct ApplyFold {
    int64_t moved, refused;
    int first; int64_t first_pos;
    double mx[SLOTS], mx_all;
};
inline ApplyFold fold_apply(const cfmm::ApplyRec *res, const Counts &c)
{
    ApplyFold f = {};
    f.first = -1; f.first_pos = -1;
    each_slot([&](int q, int, int, int) {
        if (c.m[q] == 0) return;
        f.moved += (int64_t)res[q].moved; f.refused += (int64_t)res[q].refused;
        if (f.first < 0 && res[q].refused) { f.first = q; f.first_pos = (int64_t)res[q].first; }
        double d; std::memcpy(&d, &res[q].maxbits, sizeof d);
        f.mx[q] = d; f.mx_all = std::max(f.mx_all, d);
    });
    return f;
}

// the audit's pass: counts, the worst slot (strictly smaller slack; ties: the first in bucket order) with the position its record
// holds, the minima.  An empty network: -1s and +inf
struct AuditFold {
    int64_t pools, trading, violating, oor;
    int worst; int64_t worst_pos;
    double min_slack, min_tender, min_leg;
};
inline AuditFold fold_audit(const cfmm::AuditRec *res, const Counts &c)
{
    AuditFold f = {};
    f.worst = -1; f.worst_pos = -1;
    f.min_slack = f.min_tender = f.min_leg = std::numeric_limits<double>::infinity();
    unsigned long long best = ~0ull, tender = ~0ull, leg = ~0ull;
    each_slot([&](int q, int, int, int) {
        const int64_t m = c.m[q];
        if (m == 0) return;
        f.pools += m; f.trading += (int64_t)res[q].trading; f.violating += (int64_t)res[q].violating; f.oor += (int64_t)res[q].oor;
        if (f.worst < 0 || res[q].slack < best) { best = res[q].slack; f.worst = q; }
        tender = std::min(tender, res[q].tender); leg = std::min(leg, res[q].leg);
    });
    if (f.worst >= 0) {
        f.worst_pos = (int64_t)res[f.worst].pos;
        f.min_slack = cfmm::audit_unord(best); f.min_tender = cfmm::audit_unord(tender); f.min_leg = cfmm::audit_unord(leg);
    }
    return f;
}

// ---- the audited psi -----------------------------------------------------------------------------------------------------------------
// psi[j] of the [3][n] limb sums at the fixed-point exponent F: one correctly rounded conversion, one exact scaling
inline void psi_from_limbs(const unsigned long long *hl, int n, int F, double *psi)
{
    for (int j = 0; j < n; ++j) {
        const cfmm::Fixed128 t = cfmm::fixed_combine(hl[j], hl[n + j], hl[2 * (size_t)n + j]);
        const __int128 v = (__int128)(((unsigned __int128)(unsigned long long)t.hi << 64) | (unsigned __int128)t.lo);
        psi[j] = std::ldexp((double)v, -F);
    }
}

// its value and infeasibility under the utility: linear-plus-box tokens as sweep::point_certificates (cfmm_stats); the utility table's
// entries by their own u, outside infeas (their |h| does not enter the scale either)
struct PsiWorth { double value, infeas; };
inline PsiWorth psi_worth(const double *hp, int n, const double *hc, const double *hh, const int *hctype, double max_reserve)
{
    double value = 0.0, viol = 0.0, scale = 0.0;
    for (int j = 0; j < n; ++j) {
        const double c = hc[j], h = hh[j], r = hp[j] + h;
        const int ct = hctype[j];
        if (ct == CFMM_ULOG) value += c * std::log(r);
        else if (ct == CFMM_UQUAD) value += c * hp[j] - hp[j] * hp[j] / (2.0 * h);
        else {
            value += c * hp[j];
            viol = std::max(viol, ct == CFMM_GE ? std::max(-r, 0.0) : (ct == CFMM_EQ ? std::fabs(r) : 0.0));
            scale = std::max(scale, std::fabs(h));
        }
        scale = std::max(scale, std::fabs(hp[j]));
    }
    return {value, viol / std::max(std::max(scale, 1e-12 * max_reserve), 1e-300)};
}

// ---- which point the tenders are of ---------------------------------------------------------------------------------------------------
// mu: the barrier weight of the last solve (0: first-order or set prices, exact tenders; > 0: the smoothed primal point); use_slo: that
// solve ended with low-order log-prices, which the pools were evaluated with -- the tenders handed out, applied and audited must be
// those of the same point, or they would not sum to psi.  The low-order part is read only while mu > 0
struct PointView { double mu; bool use_slo; };
inline PointView point_view(double mu_last, bool slo_active)
{
    const double mu = mu_last > 0.0 ? mu_last : 0.0;
    return {mu, mu > 0.0 && slo_active};
}

}  // namespace route
