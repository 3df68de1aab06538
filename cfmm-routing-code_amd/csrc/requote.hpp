// Re-quoting a held route on the pools as they are now (include/cfmm.h: cfmm_hold_route, cfmm_requote_route; docs/requote.md).
//
// A held route is a copy of the tenders cfmm_get_trades* handed out when it was taken: per bucket delta [k][m] | lambda [k][m] in
// upload order (the layout of the audit's `ovr`).  On chain a route executes with its INPUTS fixed, and each pool pays what its curve
// gives at the reserves it has by then.  One templated pass per bucket family puts every trading pool back on its curve at the CURRENT
// resident reserves R, fee gamma and weights / parameter:
//     x_j(s) = (R_j + gamma Delta_j) - s Lambda_j,      Lambda'_j = fl(s Lambda_j)
// with s >= 0 the root of the pool's slack, the audit's expression per class (audit.hpp: audit_close), evaluated in the audit's order
// with contraction off -- so the slack the search sees at s is bitwise the slack an audit of (Delta, Lambda') would report:
//     AU_LOG      sum_j w_j log(x_j / R_j)                                       AU_SUM   closed form s = fl(fl(gamma sum Delta) / sum Lambda)
//     AU_STABLE   ((sum x - alpha / prod x) - (sum R - alpha / prod R)) / (sum R + alpha / prod R)
//     AU_POW      (sum x^e - sum R^e) / sum R^e
// The slack is concave and strictly decreasing in s and >= 0 at s = 0: the root is unique.
//   cap         s never exceeds s_cap = min over legs with Lambda_j > 0 of (R_j + gamma Delta_j) / Lambda_j, each quotient stepped down
//               (at most 6 ulps) until fl(s_cap Lambda_j) <= R_j + gamma Delta_j: no leg goes negative (constant sum, where a fully
//               drained leg is feasible), or < : every leg stays positive (every other class, as the audit asks).  A pool whose
//               slack is still >= 0 at s_cap pays s_cap and is counted as capped (the constant-sum kinds: a leg too small to pay)
//   special     no tender at all: s = 1, not trading;  sum Lambda = 0: s = 1;  sum Delta = 0 with a positive Lambda: s = 0
//   failed      a tender or R_j + gamma Delta_j negative or not finite, or a slack at s = 0 that is not >= 0: s = NaN, left out of psi
// THE STOPPING RULE.  The search keeps a bracket lo < hi with slack(lo) >= 0 evaluated and slack(hi) < 0 (or not a number) evaluated,
// from lo = 0, hi = s_cap.  Every trial point lies strictly inside the bracket and replaces the end of its sign.  The first
// RQ_NEWTON trials are Newton steps from the last trial (the derivative is formed next to the slack), taken only while they fall
// strictly inside the bracket and the bracket is wider than 2^-47 hi; otherwise -- and from then on -- the midpoint.  (Near the root
// the slack is its own rounding: a Newton step that moves less than 2^-44 s would creep along one end, an ulp at a time, while the
// other end stays where it started -- a lane that did so ran 85 trials and held its whole wave.  Such a step is aimed ACROSS the
// root instead, 4 steps + push s beyond it, push = 2^-50 and four times more at every such step, so that the far end follows.)
// The search ends when lo and hi are adjacent doubles (no point strictly inside), or after RQ_ITERS trials, and returns lo: an s whose
// OWN slack evaluation is >= 0, the last double in the bracket for which it is.  The pool accepts what the call says it pays.
// The search is per thread: the tenders are read, not recomputed, so nothing needs the read-backs' wave-wide stopping test.
//
// psi, exactly, as the audit forms it: every non-zero Lambda'_j adds +Lambda'_j, every non-zero Delta_j adds -Delta_j, floored on its
// own to the 96-bit fixed point (audit_add) in the workgroup's LDS tile, flushed with integer atomics.  Given the scales it is a
// function of (held tenders, s) alone: bitwise the same on every run and for any launch geometry.
//
// Geometry: the audit's.  256 threads, one pool per thread, chunks strided over a bounded grid, one partial record per workgroup,
// folded by the workgroup that arrives last.  Stored position i reads its tenders and writes its scale at b.perm ? b.perm[i] : i.
#pragma once
#include "audit.hpp"
#include "requote_rules.hpp"

namespace cfmm {

constexpr int RQ_THREADS = AU_THREADS;
constexpr int RQ_GRID_MAX = AU_GRID_MAX;          // partial records per bucket slot
constexpr int RQ_GRID = 2048;                     // workgroups per pass by default: the fastest of the sweep (docs/requote.md: measured)
constexpr int RQ_NEWTON = 24;                     // trials that may be Newton steps
constexpr int RQ_ITERS = 128;                     // trials in all
enum { RQ_CAPPED = 1u, RQ_FAILED = 2u };

struct RequoteArgs {
    int n;                            // tokens: the tile is [3][n]
    double sc;                        // 2^F (det_scales)
    double tol;                       // tol_scale
    unsigned long long *limbs;        // global [3][n], zeroed before the first pass
    RequoteRec *rec, *part;           // this bucket's record; its RQ_GRID_MAX partials
};

__device__ __forceinline__ bool rq_amount_ok(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }

// one pool's scale (header comment); flags: RQ_CAPPED / RQ_FAILED; trading: some tender is non-zero.
// The slack is evaluated at ONE place in the audit's order (sums from 0, products from 1, in leg order), its derivative in s next to
// it: the loop's first trials are the trading function at the reserves themselves (the power sum's sum R^e: trial -3), the slack at
// s = 0 (-2) and at s_cap (-1); one call site keeps the library routines (log, pow) inlined and the kernels free of a private segment
template <int CLS, int K>
__device__ __forceinline__ double requote_pool(const double (&R)[K], const double (&D)[K], const double (&L)[K], double g, const double (&we)[K],
                                               double param, unsigned &flags, bool &trading)
{
#pragma clang fp contract(off)
    double up[K];
    double SD = 0.0, SL = 0.0, SR = 0.0, PR = 1.0, fR = 0.0, cap = __builtin_huge_val();
    bool ok = true;
    trading = false;
    flags = 0u;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double in = g * D[j];
        up[j] = R[j] + in;
        SD = SD + D[j]; SL = SL + L[j]; SR = SR + R[j];
        if (CLS == AU_STABLE) PR = PR * R[j];
        trading |= D[j] != 0.0 || L[j] != 0.0;
        ok &= rq_amount_ok(D[j]) && rq_amount_ok(L[j]) && rq_amount_ok(up[j]);
        if (L[j] > 0.0) {
            double c = up[j] / L[j];
            for (int q = 0; q < 6; ++q) if (c > 0.0 && (CLS == AU_SUM ? c * L[j] > up[j] : c * L[j] >= up[j])) c = __longlong_as_double(__double_as_longlong(c) - 1);
            cap = c < cap ? c : cap;
        }
    }
    if (!trading) return 1.0;
    const double nan = __builtin_nan("");
    if (!ok || (SL > 0.0 && !rq_amount_ok(cap))) { flags = RQ_FAILED; return nan; }
    if (!(SL > 0.0)) return 1.0;
    if (!(SD > 0.0)) return 0.0;
    if (CLS == AU_SUM) {
        const double in = g * SD;
        double s = in / SL;
        if (!rq_amount_ok(s)) { flags = RQ_FAILED; return nan; }
        if (s > cap) { s = cap; flags = RQ_CAPPED; }
        return s;
    }
    const double cR = CLS == AU_STABLE ? param / PR : 0.0;
    double lo = 0.0, hi = cap, s = 0.0, push = 0x1p-50;
    for (int it = CLS == AU_POW ? -3 : -2; it < RQ_ITERS; ++it) {
        if (it >= 0 && !(s > lo && s < hi)) break;        // no double strictly inside: lo and hi are adjacent
        const bool base = it == -3;
        const double at = it == -1 ? cap : (it < 0 ? 0.0 : s);
        double Sx = 0.0, Px = 1.0, fx = 0.0, slog = 0.0, d = 0.0, dl = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double pay = at * L[j];
            const double x = (base ? R[j] : up[j]) - pay;
            Sx = Sx + x;
            if (CLS == AU_LOG) { const double q = x / R[j]; const double t = we[j] * log(q); slog = slog + t; d = d + we[j] * L[j] / x; }
            if (CLS == AU_STABLE) { Px = Px * x; dl = dl + L[j]; d = d + L[j] / x; }
        }
        if (CLS == AU_POW) {
            // (the legs one after the other through ONE expansion of pow, each leg's values selected into scalars: two expansions
            //  inside the search loop cost more scalar registers than the wave has)
#pragma nounroll
            for (int j = 0; j < K; ++j) {
                double Lj = L[0], bj = base ? R[0] : up[0], ej = we[0];
#pragma unroll
                for (int q = 1; q < K; ++q) if (j == q) { Lj = L[q]; bj = base ? R[q] : up[q]; ej = we[q]; }
                const double pay = at * Lj;
                const double x = bj - pay;
                const double p = pow(x, ej);
                fx = fx + p; d = d + ej * p / x * Lj;
            }
        }
        if (base) { fR = fx; continue; }
        double F, dF;
        if (CLS == AU_LOG) { F = slog; dF = -d; }
        else if (CLS == AU_STABLE) {
            const double cx = param / Px;
            const double phx = Sx - cx, phR = SR - cR;
            F = (phx - phR) / (SR + cR);
            dF = -(dl + cx * d) / (SR + cR);
        } else { F = (fx - fR) / fR; dF = -d / fR; }
        const bool above = F >= 0.0;                      // (a slack that is not a number lies beyond the root)
        if (it == -2) { if (!above) { flags = RQ_FAILED; return nan; } continue; }
        if (it == -1) { if (above) { flags = RQ_CAPPED; return cap; } s = cap > 1.0 ? 1.0 : 0.5 * cap; continue; }
        if (above) lo = s; else hi = s;
        double next = lo + 0.5 * (hi - lo);
        if (it < RQ_NEWTON && hi - lo > 0x1p-47 * hi) {
            double t = s - F / dF;
            const double step = fabs(s - t);
            if (step <= 0x1p-44 * s) {                    // at the slack's rounding: aim across the root, further every time
                t = above ? (t + 4.0 * step) + push * s : (t - 4.0 * step) - push * s;
                push = 4.0 * push;
            }
            if (t > lo && t < hi) next = t;
        }
        s = next;
    }
    return lo;
}

// the pool is complete: its scale to upload position o, its psi into the tile, its verdict into the thread's record
template <int CLS, int K>
__device__ __forceinline__ void requote_sink(unsigned long long *tile, const RequoteArgs &a, const double (&R)[K], const double (&D)[K], const double (&L)[K],
                                             double g, const double (&we)[K], double param, const int (&tok)[K], long long o, double *__restrict__ scale,
                                             RequoteRec &acc)
{
#pragma clang fp contract(off)
    unsigned flags, oor = 0u;
    bool trading;
    const double s = requote_pool<CLS, K>(R, D, L, g, we, param, flags, trading);
    scale[o] = s;
    const bool live = trading && !(flags & RQ_FAILED);
    if (live) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double Lp = s * L[j];
            if (Lp != 0.0) audit_add(tile, a.n, a.sc, tok[j], Lp, oor);
            if (D[j] != 0.0) audit_add(tile, a.n, a.sc, tok[j], -D[j], oor);
        }
    }
    const int cls = live ? requote_class(s, a.tol) : 0;
    const RequoteRec mine{trading ? 1ull : 0ull, cls < 0 ? 1ull : 0ull, cls > 0 ? 1ull : 0ull, (flags & RQ_CAPPED) ? 1ull : 0ull, (flags & RQ_FAILED) ? 1ull : 0ull,
                          (unsigned long long)oor, live ? audit_ord(s) : ~0ull, live ? (unsigned long long)o : ~0ull, 0ull};
    requote_merge(acc, mine);
}

// every thread of the workgroup arrives; the result is thread 0's
__device__ __forceinline__ RequoteRec requote_reduce(RequoteRec a)
{
    __shared__ RequoteRec wpart[RQ_THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) {
        RequoteRec b;
        b.trading = __shfl_xor(a.trading, o, 64); b.shrt = __shfl_xor(a.shrt, o, 64); b.lng = __shfl_xor(a.lng, o, 64);
        b.capped = __shfl_xor(a.capped, o, 64); b.failed = __shfl_xor(a.failed, o, 64); b.oor = __shfl_xor(a.oor, o, 64);
        b.scale = __shfl_xor(a.scale, o, 64); b.pos = __shfl_xor(a.pos, o, 64);
        requote_merge(a, b);
    }
    __syncthreads();                                    // (the scratch may still be read from an earlier reduction)
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) for (int q = 1; q < RQ_THREADS / 64; ++q) requote_merge(a, wpart[q]);
    return a;
}

// the end of a pass: the tile's non-zero limbs to the global array; the workgroup's partial; the last workgroup folds them all
__device__ __forceinline__ void requote_finish(const unsigned long long *tile, const RequoteArgs &a, RequoteRec acc)
{
    __shared__ int last;
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * a.n; j += RQ_THREADS) { const unsigned long long v = tile[j]; if (v) atomicAdd(&a.limbs[j], v); }
    acc = requote_reduce(acc);
    if (threadIdx.x == 0) {
        unsigned long long *p = reinterpret_cast<unsigned long long *>(a.part + blockIdx.x);
        const unsigned long long v[8] = {acc.trading, acc.shrt, acc.lng, acc.capped, acc.failed, acc.oor, acc.scale, acc.pos};
#pragma unroll
        for (int q = 0; q < 8; ++q) __hip_atomic_store(p + q, v[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const unsigned long long t = atomicAdd(&a.rec->done, 1ull);
        last = t + 1 == gridDim.x;
        if (last) __threadfence();
    }
    __syncthreads();
    if (!last) return;
    RequoteRec z = requote_identity();
    for (unsigned q = threadIdx.x; q < gridDim.x; q += RQ_THREADS) {
        unsigned long long *p = reinterpret_cast<unsigned long long *>(a.part + q);
        RequoteRec b;
        b.trading = __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.shrt = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.lng = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.capped = __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.failed = __hip_atomic_load(p + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.oor = __hip_atomic_load(p + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.scale = __hip_atomic_load(p + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.pos = __hip_atomic_load(p + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        requote_merge(z, b);
    }
    z = requote_reduce(z);
    if (threadIdx.x == 0) {
        RequoteRec *r = a.rec;
        r->trading = z.trading; r->shrt = z.shrt; r->lng = z.lng; r->capped = z.capped; r->failed = z.failed; r->oor = z.oor; r->scale = z.scale; r->pos = z.pos;
    }
}

// two-asset bucket.  held: delta [2][m] | lambda [2][m] in upload order; scale: [m] in upload order
template <int KIND>
__global__ void __launch_bounds__(RQ_THREADS)
requote2_kernel(Bucket2 b, const double *__restrict__ held, double *__restrict__ scale, RequoteArgs a)
{
    extern __shared__ unsigned long long rq_tile[];
    constexpr int CLS = audit_class2(KIND);
    audit_tile_clear(rq_tile, a.n);
    RequoteRec acc = requote_identity();
    for (long long base = (long long)blockIdx.x * RQ_THREADS; base < b.m; base += (long long)gridDim.x * RQ_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            const long long o = b.perm ? b.perm[i] : i;
            const double wa = KIND == 0 ? 0.5 : (KIND == 1 ? b.param[i] : (KIND == 4 ? 1.0 - b.param[i] : 0.0));
            const double wb = KIND == 1 ? 1.0 - wa : wa;
            const double R[2] = {b.Ra[i], b.Rb[i]}, D[2] = {held[o], held[b.m + o]}, L[2] = {held[2 * b.m + o], held[3 * b.m + o]}, we[2] = {wa, wb};
            const int tok[2] = {b.ia[i], b.ib[i]};
            requote_sink<CLS, 2>(rq_tile, a, R, D, L, b.fee[i], we, KIND == 3 ? b.param[i] : 0.0, tok, o, scale, acc);
        }
    }
    requote_finish(rq_tile, a, acc);
}

// geo-mean bucket of K assets: the bucket's normalised weights.  held: delta [K][m] | lambda [K][m]
template <int K>
__global__ void __launch_bounds__(RQ_THREADS)
requoteN_kernel(BucketN b, const double *__restrict__ held, double *__restrict__ scale, RequoteArgs a)
{
    extern __shared__ unsigned long long rq_tile[];
    audit_tile_clear(rq_tile, a.n);
    RequoteRec acc = requote_identity();
    for (long long base = (long long)blockIdx.x * RQ_THREADS; base < b.m; base += (long long)gridDim.x * RQ_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            const long long o = b.perm ? b.perm[i] : i;
            double R[K], D[K], L[K], we[K];
            int tok[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                R[j] = b.R[i * K + j]; we[j] = b.w[i * K + j]; tok[j] = b.idx[i * K + j];
                D[j] = held[(size_t)j * b.m + o]; L[j] = held[(size_t)(K + j) * b.m + o];
            }
            requote_sink<AU_LOG, K>(rq_tile, a, R, D, L, b.fee[i], we, 0.0, tok, o, scale, acc);
        }
    }
    requote_finish(rq_tile, a, acc);
}

// K-asset table bucket (never permuted)
template <int KIND, int K>
__global__ void __launch_bounds__(RQ_THREADS)
requoteG_kernel(BucketG b, const double *__restrict__ held, double *__restrict__ scale, RequoteArgs a)
{
    extern __shared__ unsigned long long rq_tile[];
    constexpr int CLS = KIND == 1 ? AU_SUM : AU_STABLE;
    audit_tile_clear(rq_tile, a.n);
    RequoteRec acc = requote_identity();
    for (long long base = (long long)blockIdx.x * RQ_THREADS; base < b.m; base += (long long)gridDim.x * RQ_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            double R[K], D[K], L[K], we[K];
            int tok[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                R[j] = b.R[i * K + j]; we[j] = 0.0; tok[j] = b.idx[i * K + j];
                D[j] = held[(size_t)j * b.m + i]; L[j] = held[(size_t)(K + j) * b.m + i];
            }
            requote_sink<CLS, K>(rq_tile, a, R, D, L, b.fee[i], we, KIND == 0 ? b.param[i] : 0.0, tok, i, scale, acc);
        }
    }
    requote_finish(rq_tile, a, acc);
}

// pools of a held bucket with a non-zero tender (cfmm_hold_route's info): ten = delta [k][m] | lambda [k][m]
__global__ void __launch_bounds__(RQ_THREADS)
hold_count_kernel(const double *__restrict__ ten, long long m, int k, unsigned long long *out)
{
    unsigned long long mine = 0ull;
    for (long long i = (long long)blockIdx.x * RQ_THREADS + threadIdx.x; i < m; i += (long long)gridDim.x * RQ_THREADS) {
        bool moved = false;
        for (int j = 0; j < 2 * k; ++j) moved |= ten[(size_t)j * m + i] != 0.0;
        mine += moved ? 1ull : 0ull;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, mine);
}

}  // namespace cfmm
