// The host decisions of the in-place updates of resident pools' trading terms (include/cfmm.h: cfmm_update_terms2 / N / G; the
// kernels are in update.hpp): which fee and which weight a bucket holds -- the predicates the uploads apply, shared with them so
// that an update refuses exactly what an upload refuses --, the bucket's smallest fee after a scatter, and when a two-asset bucket's
// compact mirror has to be built again.  Host only: nothing of HIP, nothing of cfmm_ctx -- cfmm_hip.hip gathers the inputs,
// tests/test_terms_host.py exercises the rules.
#pragma once

#include <cstdint>
#include <cstring>

namespace terms {

// The predicates are function OBJECTS: a template that takes one (the uploads' column scans) calls it inline.
// a fee gamma: in (0, 1] (NaN fails every comparison, +inf the second)
struct FeeOk { bool operator()(double x) const { return x > 0.0 && x <= 1.0; } };
// a weight of a weighted geometric mean (the two-asset kind's wa, a geo-mean leg's w): in (0, 1); normalising is the caller's duty
struct WeightOk { bool operator()(double x) const { return x > 0.0 && x < 1.0; } };
inline constexpr FeeOk fee_ok{};
inline constexpr WeightOk weight_ok{};

// first entry of v[0 .. count) that fails `ok`, or -1; *mn (if given) takes the smallest entry seen up to there
template <class P> inline int64_t first_bad(const double *v, int64_t count, P ok, double *mn = nullptr)
{
    for (int64_t i = 0; i < count; ++i) {
        if (!ok(v[i])) return i;
        if (mn && v[i] < *mn) *mn = v[i];
    }
    return -1;
}

// Positive doubles order like their bit patterns; the device reduces a fee column to its SMALLEST entry with the one unsigned
// atomicMax it has a use for elsewhere, over the complements (update.hpp: upd_min_kernel; the word starts as zero).
inline double fee_from_reduced(unsigned long long complement)
{
    const unsigned long long bits = ~complement;
    double x;
    std::memcpy(&x, &bits, sizeof x);
    return x;
}

// The bucket's smallest fee after a scatter, exactly what a fresh upload of the new column would record.  `raised`: the scatter
// overwrote a fee equal to the recorded minimum with a larger one (it reads what it overwrites) -- only then can the minimum have gone
// UP, and the column is reduced again (`reduced`: its smallest entry, the new fees included); otherwise the old minimum still stands
// somewhere in the column, or was replaced by something no larger, and the smaller of it and the smallest new fee is the answer.
inline double min_fee_after(double mn_old, bool raised, double mn_new, double reduced)
{
    if (raised) return reduced < mn_new ? reduced : mn_new;
    return mn_new < mn_old ? mn_new : mn_old;
}

// The compact mirror of a two-asset bucket (kernels.hpp: Bucket2::cfee, a byte index into the table of the bucket's DISTINCT fees; more
// than 256 of them: no mirror) after an update: rebuilt from the new column by the builder the upload uses, so that stale table entries
// of fees no pool holds any more can neither crowd out a mirror a fresh upload would have nor keep one it would not.  Reset (freed, "not
// tried yet") when fees were written into a bucket whose mirror had been tried -- built or found not to apply; a bucket never tried has
// nothing to reset, and an update of weights alone leaves the mirror (ids and fees) as it is.
inline bool mirror_reset(bool tried, bool fees_given, int64_t count) { return tried && fees_given && count > 0; }

}  // namespace terms
