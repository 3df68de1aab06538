// The host arithmetic of re-quoting a held route (include/cfmm.h: cfmm_hold_route, cfmm_requote_route; docs/requote.md): where each
// bucket's held tenders and scales sit in the context's arena, the record a pass leaves per bucket slot and how records merge, the
// classification of a pool's scale, the scratch's layout, and the fold of the records into the report.  Host only but for the three
// functions the kernels share (requote_identity / requote_merge / requote_class): nothing of HIP, nothing of cfmm_ctx -- cfmm_hip.hip
// gathers the inputs, tests/test_requote_host.py exercises the rules through a stand-alone program.
#pragma once

#include "route_rules.hpp"

namespace cfmm {

// one per bucket slot of cfmm_requote_route (requote.hpp; and one partial per workgroup): counts; the smallest scale among the pools
// that trade and whose root was found (its audit_ord image, all ones: none) with the lowest upload position that holds it; the
// workgroups that have left their partial (zeroed before the pass)
struct RequoteRec {
    unsigned long long trading, shrt, lng, capped, failed, oor, scale, pos, done;
};

CFMM_FX_HD RequoteRec requote_identity() { return RequoteRec{0ull, 0ull, 0ull, 0ull, 0ull, 0ull, ~0ull, ~0ull, 0ull}; }
CFMM_FX_HD void requote_merge(RequoteRec &a, const RequoteRec &b)
{
    a.trading += b.trading; a.shrt += b.shrt; a.lng += b.lng; a.capped += b.capped; a.failed += b.failed; a.oor += b.oor;
    if (b.scale < a.scale || (b.scale == a.scale && b.pos < a.pos)) { a.scale = b.scale; a.pos = b.pos; }
}

// a trading pool's scale against 1: -1 short (s < 1 - tol), +1 long (s > 1 + tol), 0 within; each bound rounded once
CFMM_FX_HD int requote_class(double s, double tol)
{
    const double lo = 1.0 - tol, hi = 1.0 + tol;
    return s < lo ? -1 : (s > hi ? 1 : 0);
}

}  // namespace cfmm

namespace requote {

constexpr double TOL_SCALE = 1e-9;                          // the default tol_scale: the audit's tol_pool
inline double tol_scale(double t) { return t > 0.0 ? t : TOL_SCALE; }

// the held route's arena, in doubles: every resident bucket in bucket order, delta [k][m] | lambda [k][m] (the audit's `ovr`
// layout), then every bucket's scales [m]; upload order throughout
struct HoldLayout {
    size_t ten[route::SLOTS], scl[route::SLOTS];            // a bucket's first tender / first scale
    size_t tenders, total;                                  // doubles of the tenders; of the arena
    int64_t pools;
};
inline HoldLayout hold_layout(const route::Counts &c)
{
    HoldLayout l = {};
    size_t off = 0;
    route::each_slot([&](int q, int, int, int k) { l.ten[q] = off; off += 2 * (size_t)k * (size_t)c.m[q]; l.pools += c.m[q]; });
    l.tenders = off;
    route::each_slot([&](int q, int, int, int) { l.scl[q] = off; off += (size_t)c.m[q]; });
    l.total = off;
    return l;
}
inline bool same_counts(const route::Counts &a, const route::Counts &b)
{
    for (int q = 0; q < route::SLOTS; ++q) if (a.m[q] != b.m[q]) return false;
    return true;
}

// the pass's device scratch, in bytes: one record per slot | the [3][n] limbs | (256-aligned) `parts` partial records per slot; the
// pinned copy ends where the partials begin (as route::audit_span)
struct Span { size_t recs, limbs, parts, total; };
inline Span span(int n, int parts_per_slot)
{
    Span s;
    s.recs = 0; s.limbs = route::SLOTS * sizeof(cfmm::RequoteRec);
    s.parts = (s.limbs + 3 * (size_t)n * sizeof(unsigned long long) + 255) & ~(size_t)255;
    s.total = s.parts + (size_t)route::SLOTS * parts_per_slot * sizeof(cfmm::RequoteRec);
    return s;
}

// the records folded: counts, and the slot that holds the smallest scale (strictly smaller; ties: the first in bucket order) with the
// position its record holds.  No pool trades with a root: -1s and +inf.  Only slots that hold pools are read
struct Fold {
    int64_t pools, trading, shrt, lng, capped, failed, oor;
    int min_slot; int64_t min_pos;
    double min_scale;
};
inline Fold fold(const cfmm::RequoteRec *res, const route::Counts &c)
{
    Fold f = {};
    f.min_slot = -1; f.min_pos = -1;
    f.min_scale = std::numeric_limits<double>::infinity();
    unsigned long long best = ~0ull;
    route::each_slot([&](int q, int, int, int) {
        const int64_t m = c.m[q];
        if (m == 0) return;
        f.pools += m; f.trading += (int64_t)res[q].trading; f.shrt += (int64_t)res[q].shrt; f.lng += (int64_t)res[q].lng;
        f.capped += (int64_t)res[q].capped; f.failed += (int64_t)res[q].failed; f.oor += (int64_t)res[q].oor;
        if (res[q].scale < best) { best = res[q].scale; f.min_slot = q; }
    });
    if (f.min_slot >= 0) { f.min_pos = (int64_t)res[f.min_slot].pos; f.min_scale = cfmm::audit_unord(best); }
    return f;
}

// a report no pass has filled in, and the fold written into one (value / infeas: the caller's, from psi_worth)
inline void blank(cfmm_requote *out)
{
    std::memset(out, 0, sizeof *out);
    out->min_family = out->min_kind = out->min_k = -1; out->min_pos = -1;
    out->min_scale = std::numeric_limits<double>::infinity();
    out->value = out->infeas = std::numeric_limits<double>::quiet_NaN();
}
inline void report(const Fold &f, int fixed_exponent, cfmm_requote *out)
{
    const route::SlotName s = route::slot_name(f.min_slot);
    out->pools = f.pools; out->pools_trading = f.trading; out->pools_short = f.shrt; out->pools_long = f.lng;
    out->pools_capped = f.capped; out->pools_failed = f.failed; out->legs_out_of_range = f.oor;
    out->min_family = s.family; out->min_kind = s.kind; out->min_k = s.k; out->fixed_exponent = fixed_exponent;
    out->min_pos = f.min_pos; out->min_scale = f.min_scale;
}

}  // namespace requote
