// The decisions and the host arithmetic of the pool selection (include/cfmm.h: cfmm_select_pools, cfmm_get_selected2 / N / G): how many
// 64-bit words a bucket's mask has and where every bucket's words and workgroup partials lie in the context's selection arena, how many
// workgroups the compaction's count and write launches take, and the fold of the per-slot records into cfmm_select_info.  Host only:
// nothing of HIP, nothing of cfmm_ctx -- cfmm_hip.hip gathers the inputs, subset.hpp holds the kernels, tests/test_subset_host.py
// exercises the rules through a stand-alone program.  Every sum keeps one fixed order of operations.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include "route_rules.hpp"

namespace cfmm {

// what a selection pass leaves per workgroup, and (folded in workgroup order) per bucket slot
struct SelRec {
    unsigned long long selected;      // pools with a finite v > min_value_in
    unsigned long long non_finite;    // pools whose v is NaN or infinite (never selected, in neither sum)
    double value_total;               // sum of the finite v
    double value_selected;            // ... of the selected pools' v
};

}  // namespace cfmm

namespace subset {

static_assert(route::SLOTS == CFMM_BUCKET_SLOTS, "include/cfmm.h and route_rules.hpp disagree on the bucket slots");

constexpr int WORD_BITS = 64;         // one wave's ballot: pool o of a bucket is bit o % 64 of word o / 64, upload order
constexpr int SEL_THREADS = 256;      // the selection pass: pool i on thread i in stored order (apply.hpp: AP_THREADS)
constexpr int SCAN_THREADS = 256;     // the compaction: one mask word per thread, so 16 384 pools per workgroup

inline int64_t mask_words(int64_t m) { return (m + WORD_BITS - 1) / WORD_BITS; }
inline int64_t select_groups(int64_t m) { return (m + SEL_THREADS - 1) / SEL_THREADS; }           // workgroups (and partials) of the pass
inline int64_t scan_groups(int64_t m) { return (mask_words(m) + SCAN_THREADS - 1) / SCAN_THREADS; }   // workgroups of the count and write launches

// The selection arena of a context, in bytes: one SelRec per slot | every bucket's workgroup partials, in slot order | (256-aligned) every
// bucket's mask words, in slot order | (256-aligned) the compaction's group counts and offsets: scan_groups of the largest bucket, + 1
// for the total.  part_off / word_off are in elements, with one entry past the last slot; an empty bucket takes no room
struct Layout {
    size_t part_off[route::SLOTS + 1], word_off[route::SLOTS + 1];
    size_t recs, parts, words, scan, scan_len, total;
};
inline Layout layout(const route::Counts &c)
{
    Layout l = {};
    int64_t mx = 0;
    for (int q = 0; q < route::SLOTS; ++q) {
        l.part_off[q + 1] = l.part_off[q] + (size_t)select_groups(c.m[q]);
        l.word_off[q + 1] = l.word_off[q] + (size_t)mask_words(c.m[q]);
        mx = c.m[q] > mx ? c.m[q] : mx;
    }
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    l.recs = 0;
    l.parts = route::SLOTS * sizeof(cfmm::SelRec);
    l.words = up(l.parts + l.part_off[route::SLOTS] * sizeof(cfmm::SelRec));
    l.scan = up(l.words + l.word_off[route::SLOTS] * sizeof(unsigned long long));
    l.scan_len = (size_t)scan_groups(mx) + 1;
    l.total = l.scan + l.scan_len * sizeof(unsigned);
    return l;
}

// the per-slot records folded into the report, in slot order (only slots that hold pools are read)
inline void fold_select(const cfmm::SelRec *res, const route::Counts &c, cfmm_select_info *info)
{
    std::memset(info, 0, sizeof *info);
    route::each_slot([&](int q, int, int, int) {
        const int64_t m = c.m[q];
        if (m == 0) return;
        info->slot_pools[q] = m; info->slot_selected[q] = (int64_t)res[q].selected;
        info->pools += m; info->selected += (int64_t)res[q].selected; info->non_finite += (int64_t)res[q].non_finite;
        info->value_in_total += res[q].value_total; info->value_in_selected += res[q].value_selected;
    });
}

// how many of a bucket's `total` selected positions a caller's array of `cap` entries receives
inline int64_t listed(int64_t total, int64_t cap) { return cap < 0 ? 0 : (total < cap ? total : cap); }

// ---- the sub-network's lists (cfmm_subnetwork) -----------------------------------------------------------------------------------------
// a bucket's list: `count` positions of a bucket of m pools, strictly ascending and in [0, m).  The first entry that breaks the rule
// (-1: none; a negative count, or entries without an array: entry 0)
inline int64_t list_offender(const int32_t *pos, int64_t count, int64_t m)
{
    if (count < 0 || (count > 0 && !pos)) return 0;
    for (int64_t i = 0; i < count; ++i)
        if (pos[i] < 0 || pos[i] >= m || (i > 0 && pos[i] <= pos[i - 1])) return i;
    return -1;
}
// every slot's verdict: the first slot in bucket order whose list breaks the rule, and the entry (-1s: all lists stand)
struct ListVerdict { int slot; int64_t entry; };
inline ListVerdict check_lists(const cfmm_pool_lists *l, const route::Counts &c)
{
    ListVerdict v = {-1, -1};
    route::each_slot([&](int q, int, int, int) {
        if (v.slot >= 0) return;
        const int64_t e = list_offender(l->pos[q], l->count[q], c.m[q]);
        if (e >= 0) { v.slot = q; v.entry = e; }
    });
    return v;
}

// ---- a sub-bucket's arena: the columns in the order, and at the 256-byte aligned offsets, an upload of that many pools gives them -------
// (cfmm_hip.hip: upload_arena; the token-block ordering shifts a bucket's column pointers from one arena to the next by these offsets)
struct Arena { size_t off[8], total; int cols; };
inline Arena arena_of(const size_t *bytes, int cols)
{
    Arena a = {};
    a.cols = cols;
    for (int q = 0; q < cols; ++q) { a.off[q] = a.total; a.total += (bytes[q] + 255) & ~(size_t)255; }
    return a;
}
// two-asset: Ra | Rb | fee | [param] | ia | ib
inline Arena arena2(int64_t m, bool param)
{
    const size_t d = (size_t)m * sizeof(double), i = (size_t)m * sizeof(int32_t);
    const size_t with[6] = {d, d, d, d, i, i}, without[5] = {d, d, d, i, i};
    return param ? arena_of(with, 6) : arena_of(without, 5);
}
// geo-mean of k assets: idx | R | w | fee | lfee | lrw
inline Arena arenaN(int k, int64_t m)
{
    const size_t d = (size_t)m * sizeof(double);
    const size_t b[6] = {(size_t)k * m * sizeof(int32_t), k * d, k * d, d, d, k * d};
    return arena_of(b, 6);
}
// the K-asset table: idx | R | fee | [param] | ifee | sR | ws
inline Arena arenaG(int k, int64_t m, bool param)
{
    const size_t d = (size_t)m * sizeof(double);
    const size_t with[7] = {(size_t)k * m * sizeof(int32_t), k * d, d, d, d, d, d}, without[6] = {(size_t)k * m * sizeof(int32_t), k * d, d, d, d, d};
    return param ? arena_of(with, 7) : arena_of(without, 6);
}

}  // namespace subset
