// The decisions and the host arithmetic of cfmm_pool_prices (include/cfmm.h; docs/pool_prices.md): where everything lies in the call's
// scratch and how many workgroups a relation pass takes, the zero-mean gauge of the potentials the device returns, the renumbering of
// its component labels, the anchoring offsets and the prices, and the fold into cfmm_prices_info.  Host only: nothing of HIP, nothing of
// cfmm_ctx -- cfmm_hip.hip gathers the inputs, prices.hpp holds the kernels, tests/test_prices_host.py exercises the rules through a
// stand-alone program.  Everything here is O(n); every sum keeps one fixed order of operations (token order, slot order, workgroup order).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "route_rules.hpp"

namespace cfmm {

// what the iteration's single workgroup leaves (prices.hpp: prices_cg_kernel)
struct PricesCg {
    double residual;                  // max |r| / max |rhs| at return (0 when rhs == 0)
    double rhs_max;                   // max |rhs|
    int iterations, status;           // status 1: the cap was reached
    int rounds, pad;                  // of the label propagation (prices_components_kernel)
};

}  // namespace cfmm

namespace prices {

constexpr int REL_THREADS = 256;      // the relation passes: pool i of a 256-pool chunk on thread i % 256 (apply.hpp: AP_THREADS)
constexpr int REL_GRID = 512;         // workgroups per pass at the most: 2 per CU of an MI355X (audit.hpp: AU_GRID), chunk-strided
constexpr int MAX_TOKENS = 6144;      // the iteration keeps its direction vector in one workgroup's LDS: 8 n bytes <= 48 KB
constexpr int ROW_ALIGN = 4;          // a row of the count matrix is read as 16-byte words
constexpr double STOP = 1e-12;        // the iteration stops at max |r| <= STOP max |rhs|

inline int64_t chunks(int64_t m) { return (m + REL_THREADS - 1) / REL_THREADS; }
inline int rel_grid(int64_t m) { const int64_t c = chunks(m); return (int)(c < REL_GRID ? c : REL_GRID); }
inline int row_stride(int n) { return (n + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN; }       // entries per matrix row (the tail stays zero)
inline int iteration_cap(int n) { return 4 * n + 100; }
// relations a bucket of m pools of k assets contributes
inline int64_t relations_of(int k, int64_t m) { return (int64_t)(k - 1) * m; }
inline int64_t relations(const route::Counts &c)
{
    int64_t r = 0;
    route::each_slot([&](int q, int, int, int k) { r += relations_of(k, c.m[q]); });
    return r;
}

// The call's scratch, in bytes.  What comes back in ONE copy lies first: phi [n] | degree [n] (32-bit) | label [n] (32-bit) | PricesCg |
// the misfit pass's workgroup partials {max, sum of squares}, every bucket's in slot order (part_off: in partials, one entry past the
// last slot; an empty bucket takes none).  Behind it (256-aligned each) what stays on the device: rhs [n] | r [n] | q [n] | the count
// matrix [n][row_stride(n)] of 32-bit words.  `back` bytes are copied, `clear_from` .. `total` are zeroed in front of every call (the
// partials, rhs, r, q and the matrix)
struct Layout {
    size_t part_off[route::SLOTS + 1];
    size_t phi, deg, label, cg, parts, back, rhs, r, q, mat, clear_from, total;
    int ld;
};
inline Layout layout(int n, const route::Counts &c)
{
    Layout l = {};
    for (int q = 0; q < route::SLOTS; ++q) l.part_off[q + 1] = l.part_off[q] + (size_t)rel_grid(c.m[q]);
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t nn = (size_t)n;
    l.ld = row_stride(n);
    l.phi = 0;
    l.deg = up(l.phi + nn * sizeof(double));
    l.label = up(l.deg + nn * sizeof(uint32_t));
    l.cg = up(l.label + nn * sizeof(int32_t));
    l.parts = up(l.cg + sizeof(cfmm::PricesCg));
    l.back = l.parts + l.part_off[route::SLOTS] * 2 * sizeof(double);
    l.clear_from = l.parts;
    l.rhs = up(l.back);
    l.r = up(l.rhs + nn * sizeof(double));
    l.q = up(l.r + nn * sizeof(double));
    l.mat = up(l.q + nn * sizeof(double));
    l.total = up(l.mat + nn * (size_t)l.ld * sizeof(uint32_t));
    return l;
}

// an anchor entry the call takes: 0 (unknown) or a positive finite price.  The first entry that is neither (-1: none; NULL: none)
inline int anchor_offender(const double *anchor, int n)
{
    if (!anchor) return -1;
    for (int j = 0; j < n; ++j)
        if (!(anchor[j] >= 0.0 && anchor[j] <= 1.79769313486231570815e308)) return j;
    return -1;
}

// The device's labels (every token carries the smallest token id of its component) renumbered 0.., by each component's first token.
// Returns the number of components, or -1 if the labels are not of that form (label[j] <= j and label[label[j]] == label[j])
inline int renumber(const int32_t *label, int n, int32_t *comp)
{
    int nc = 0;
    for (int j = 0; j < n; ++j) {
        const int32_t l = label[j];
        if (l < 0 || l > j || label[l] != l) return -1;
        comp[j] = l == j ? nc++ : comp[l];
    }
    return nc;
}

// the zero-mean gauge: every component's mean, summed in token order, is taken off its tokens.  sum / cnt: scratch of nc entries each
inline void gauge(double *phi, const int32_t *comp, int n, int nc, double *sum, int32_t *cnt)
{
    for (int q = 0; q < nc; ++q) { sum[q] = 0.0; cnt[q] = 0; }
    for (int j = 0; j < n; ++j) { sum[comp[j]] += phi[j]; ++cnt[comp[j]]; }
    for (int j = 0; j < n; ++j) phi[j] -= sum[comp[j]] / (double)cnt[comp[j]];
}

// The prices: on a component with anchored tokens exp(phi + off), off the mean of log anchor - phi over them in token order, and the
// anchored tokens bit for bit as given; on a component without one exp(phi).  Returns the number of anchored components
inline int anchor_prices(const double *phi, const int32_t *comp, int n, int nc, const double *anchor, double *prices, double *sum, int32_t *cnt)
{
    for (int q = 0; q < nc; ++q) { sum[q] = 0.0; cnt[q] = 0; }
    if (anchor)
        for (int j = 0; j < n; ++j)
            if (anchor[j] > 0.0) { sum[comp[j]] += std::log(anchor[j]) - phi[j]; ++cnt[comp[j]]; }
    int anchored = 0;
    for (int q = 0; q < nc; ++q) anchored += cnt[q] > 0;
    for (int j = 0; j < n; ++j) {
        const int q = comp[j];
        if (anchor && anchor[j] > 0.0) prices[j] = anchor[j];
        else prices[j] = cnt[q] > 0 ? std::exp(phi[j] + sum[q] / (double)cnt[q]) : std::exp(phi[j]);
    }
    return anchored;
}

// the misfit pass's partials {max, sum of squares}, folded bucket by bucket in slot order, workgroup by workgroup
struct Misfit { double max, ss; };
inline Misfit fold_misfit(const double *parts, const Layout &l, const route::Counts &c)
{
    Misfit f = {0.0, 0.0};
    route::each_slot([&](int q, int, int, int) {
        const int g = rel_grid(c.m[q]);
        for (int w = 0; w < g; ++w) {
            const double *p = parts + 2 * (l.part_off[q] + (size_t)w);
            f.max = p[0] > f.max ? p[0] : f.max;
            f.ss += p[1];
        }
    });
    return f;
}

// the report
inline void fold_info(const route::Counts &c, const uint32_t *deg, int n, int nc, int anchored, const cfmm::PricesCg &cg, const Misfit &mf, cfmm_prices_info *info)
{
    std::memset(info, 0, sizeof *info);
    info->relations = relations(c);
    info->components = nc;
    info->components_anchored = anchored;
    for (int j = 0; j < n; ++j) info->tokens_unlisted += deg[j] == 0u;
    info->iterations = cg.iterations;
    info->status = cg.status;
    info->residual = cg.residual;
    info->misfit_max = mf.max;
    info->misfit_ss = mf.ss;
}

}  // namespace prices
