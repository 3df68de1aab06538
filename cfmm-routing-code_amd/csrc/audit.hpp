// Auditing a solve's route on the device (include/cfmm.h: cfmm_audit_trades; docs/audit.md): does every pool accept the tenders
// cfmm_get_trades* would hand out, and what do they add up to, exactly?
//
// A third sink on the read-backs' per-pool code (kernels.hpp: trades2_pool / tradesn_pool; smooth.hpp: smooth_trades_pool; phik.hpp:
// tradesg_pool), next to the read-back kernels themselves and the apply passes (apply.hpp).  One templated pass per bucket family.  Per
// pool, with x_j = (R_j + gamma Delta_j) - Lambda_j (post_trade_reserve with g = gamma: the model's constraint, cfmm.h:19):
//   slack        the relative change of the trading function, >= 0 when the pool accepts the trade (audit_close: one expression per class)
//   min tender   the smallest Delta_j, Lambda_j;   min leg   the smallest x_j / max_j R_j
//   violating    slack < -tol, a tender negative or not finite, a leg that does not stay positive (constant sum: x_j < -tol sum R; a
//                fully drained leg is feasible there)
// and every non-zero Lambda_j (+) and Delta_j (-) is floored to the reproducible mode's 96-bit fixed point (fixedpoint.hpp) and added
// with integer atomics: the audited psi is a function of the tenders alone, whatever the launch geometry.
// Every expression the NumPy twin (cfmm/problem.py: audit_trades) must reproduce bit for bit is evaluated with contraction off, in the
// order written here.
//
// Geometry.  The weighted and geo-mean tender iterations stop on a wave-wide test, so the passes keep the read-back kernels' mapping
// within a wave (256 threads, pool i of a 256-pool chunk on thread i % 256, the same guard): the audit sees bitwise the tenders of
// cfmm_get_trades*.  A workgroup owns an LDS tile of 3 n 64-bit limbs (Scatter<true>'s layout) and walks many chunks, chunk-strided over a
// bounded grid: a 24 KB tile per 256 pools is not zeroed and flushed once per chunk.  It flushes the non-zero limbs with integer atomics,
// reduces its counters and minima over the wave, then over the workgroup in LDS (as apply_tally does: per-wave atomics on one record cost
// 0.4 ms there), and leaves ONE partial record; the workgroup that arrives last folds the partials into the bucket's record, so the
// smallest slack and the position that holds it stay one pair (two atomics could not keep them together).
#pragma once
#include "apply.hpp"

namespace cfmm {

constexpr int AU_THREADS = AP_THREADS;
constexpr int AU_GRID_MAX = 2048;                 // partial records per bucket slot
constexpr int AU_GRID = 512;                      // workgroups per pass by default: 2 per CU of an MI355X (docs/audit.md: measured)
constexpr int AU_MAX_TOKENS = 2560;               // 3 n limbs of 8 bytes in the 64 KB a workgroup gets without asking: n <= 2560
static_assert(AU_THREADS == GK_THREADS, "the audit passes keep the read-back kernels' thread mapping");

// the trading function's class: what `slack` is (docs/audit.md)
enum { AU_LOG = 0, AU_SUM = 1, AU_STABLE = 2, AU_POW = 3 };
constexpr int audit_class2(int kind) { return kind == 2 ? AU_SUM : kind == 3 ? AU_STABLE : kind == 4 ? AU_POW : AU_LOG; }

// AuditRec, one per bucket slot (and one partial per workgroup), and the order-preserving images audit_ord / audit_unord of its
// minima: route_rules.hpp, where the host folds them
__host__ __device__ __forceinline__ AuditRec audit_identity() { return AuditRec{0ull, 0ull, 0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0ull}; }
__host__ __device__ __forceinline__ void audit_merge(AuditRec &a, const AuditRec &b)
{
    a.trading += b.trading; a.violating += b.violating; a.oor += b.oor;
    if (b.slack < a.slack || (b.slack == a.slack && b.pos < a.pos)) { a.slack = b.slack; a.pos = b.pos; }
    a.tender = b.tender < a.tender ? b.tender : a.tender;
    a.leg = b.leg < a.leg ? b.leg : a.leg;
}

struct AuditArgs {
    int n;                            // tokens: the tile is [3][n]
    double sc;                        // 2^F (det_scales)
    double tol;                       // tol_pool
    unsigned long long *limbs;        // global [3][n], zeroed before the first pass
    AuditRec *rec, *part;             // this bucket's record; its AU_GRID_MAX partials
};

// what a pool accumulates leg by leg (sums from 0, products from 1, in leg order)
struct PoolAudit {
    double Sx = 0.0, SR = 0.0, Px = 1.0, PR = 1.0, fx = 0.0, fR = 0.0, slog = 0.0;
    double xmin = __builtin_huge_val(), Rmax = 0.0, tmin = __builtin_huge_val();
    bool moved = false, tbad = false, xnan = false, xnonpos = false;
    unsigned oor = 0;
};

// one contribution y to token tok of the workgroup's tile, as Scatter<true>::add splits it; outside the split's range: counted, left out
__device__ __forceinline__ void audit_add(unsigned long long *tile, int n, double sc, int tok, double y, unsigned &oor)
{
    const double yf = y * sc;
    if (!(fabs(yf) < 0x1p94)) { ++oor; return; }
    const FixedLimbs a = fixed_split(yf);
    atomicAdd(&tile[tok], (unsigned long long)a.a0);
    atomicAdd(&tile[n + tok], (unsigned long long)a.a1);
    atomicAdd(&tile[2 * n + tok], (unsigned long long)(long long)a.a2);
}

// leg j of a pool: reserve R, tenders D, L, fee factor g, token tok; we: its weight (AU_LOG) or the exponent 1 - t (AU_POW)
template <int CLS>
__device__ __forceinline__ void audit_leg(PoolAudit &p, unsigned long long *tile, const AuditArgs &a, int tok, double R, double D, double L, double g, double we)
{
#pragma clang fp contract(off)
    const double x = post_trade_reserve(R, g, D, L);
    p.moved |= D != 0.0 || L != 0.0;
    p.tbad |= !(D >= 0.0 && D <= 1.79769313486231570815e308) || !(L >= 0.0 && L <= 1.79769313486231570815e308);
    const double dn = D != D ? -__builtin_huge_val() : D, ln = L != L ? -__builtin_huge_val() : L;
    p.tmin = dn < p.tmin ? dn : p.tmin;
    p.tmin = ln < p.tmin ? ln : p.tmin;
    p.xnan |= x != x;
    p.xnonpos |= !(x > 0.0);
    p.xmin = x < p.xmin ? x : p.xmin;
    p.Rmax = R > p.Rmax ? R : p.Rmax;
    p.Sx = p.Sx + x; p.SR = p.SR + R;
    if (CLS == AU_STABLE) { p.Px = p.Px * x; p.PR = p.PR * R; }
    if (CLS == AU_LOG) { const double q = x / R; const double t = we * log(q); p.slog = p.slog + t; }
    if (CLS == AU_POW) { p.fx = p.fx + pow(x, we); p.fR = p.fR + pow(R, we); }
    if (L != 0.0) audit_add(tile, a.n, a.sc, tok, L, p.oor);
    if (D != 0.0) audit_add(tile, a.n, a.sc, tok, -D, p.oor);
}

// the pool is complete: its slack and verdict into the thread's record (pos: upload order)
template <int CLS>
__device__ __forceinline__ void audit_close(const PoolAudit &p, const AuditArgs &a, double param, unsigned long long pos, AuditRec &acc)
{
#pragma clang fp contract(off)
    double s;
    if (CLS == AU_LOG) s = p.slog;
    else if (CLS == AU_SUM) s = (p.Sx - p.SR) / p.SR;
    else if (CLS == AU_STABLE) {
        const double cx = param / p.Px, cR = param / p.PR;
        const double phx = p.Sx - cx, phR = p.SR - cR;
        s = (phx - phR) / (p.SR + cR);
    } else s = (p.fx - p.fR) / p.fR;
    if (!(s >= -1.79769313486231570815e308 && s <= 1.79769313486231570815e308)) s = -__builtin_huge_val();
    if (s == 0.0) s = 0.0;                              // (one zero: the order below tells -0 from +0)
    bool bad = s < -a.tol || p.tbad;
    if (CLS == AU_SUM) { const double lim = a.tol * p.SR; bad |= p.xmin < -lim; }
    else bad |= p.xnonpos;
    const double leg = p.xnan ? -__builtin_huge_val() : p.xmin / p.Rmax;
    AuditRec mine{p.moved ? 1ull : 0ull, bad ? 1ull : 0ull, (unsigned long long)p.oor, audit_ord(s), pos, audit_ord(p.tmin), audit_ord(leg), 0ull};
    audit_merge(acc, mine);
}

// every thread of the workgroup arrives; the result is thread 0's
__device__ __forceinline__ AuditRec audit_reduce(AuditRec a)
{
    __shared__ AuditRec wpart[AU_THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) {
        AuditRec b;
        b.trading = __shfl_xor(a.trading, o, 64); b.violating = __shfl_xor(a.violating, o, 64); b.oor = __shfl_xor(a.oor, o, 64);
        b.slack = __shfl_xor(a.slack, o, 64); b.pos = __shfl_xor(a.pos, o, 64);
        b.tender = __shfl_xor(a.tender, o, 64); b.leg = __shfl_xor(a.leg, o, 64);
        audit_merge(a, b);
    }
    __syncthreads();                                    // (the scratch may still be read from an earlier reduction)
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) for (int q = 1; q < AU_THREADS / 64; ++q) audit_merge(a, wpart[q]);
    return a;
}

__device__ __forceinline__ void audit_tile_clear(unsigned long long *tile, int n)
{
    for (int j = threadIdx.x; j < 3 * n; j += AU_THREADS) tile[j] = 0ull;
    __syncthreads();
}

// the end of a pass: the tile's non-zero limbs to the global array; the workgroup's partial; the last workgroup folds them all
__device__ __forceinline__ void audit_finish(const unsigned long long *tile, const AuditArgs &a, AuditRec acc)
{
    __shared__ int last;
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * a.n; j += AU_THREADS) { const unsigned long long v = tile[j]; if (v) atomicAdd(&a.limbs[j], v); }
    acc = audit_reduce(acc);
    if (threadIdx.x == 0) {
        unsigned long long *p = reinterpret_cast<unsigned long long *>(a.part + blockIdx.x);
        const unsigned long long v[7] = {acc.trading, acc.violating, acc.oor, acc.slack, acc.pos, acc.tender, acc.leg};
#pragma unroll
        for (int q = 0; q < 7; ++q) __hip_atomic_store(p + q, v[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const unsigned long long t = atomicAdd(&a.rec->done, 1ull);
        last = t + 1 == gridDim.x;
        if (last) __threadfence();
    }
    __syncthreads();
    if (!last) return;
    AuditRec z = audit_identity();
    for (unsigned q = threadIdx.x; q < gridDim.x; q += AU_THREADS) {
        unsigned long long *p = reinterpret_cast<unsigned long long *>(a.part + q);
        AuditRec b;
        b.trading = __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.violating = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.oor = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.slack = __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.pos = __hip_atomic_load(p + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.tender = __hip_atomic_load(p + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.leg = __hip_atomic_load(p + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        audit_merge(z, b);
    }
    z = audit_reduce(z);
    if (threadIdx.x == 0) {
        AuditRec *r = a.rec;
        r->trading = z.trading; r->violating = z.violating; r->oor = z.oor; r->slack = z.slack; r->pos = z.pos; r->tender = z.tender; r->leg = z.leg;
    }
}

// two-asset bucket.  mu > 0: behind a second-order solve (the gross smoothed tenders); ovr: tenders held on the host instead of the
// pool's own -- the library's kink loop's, or the caller's (delta [2][m] | lambda [2][m] in upload order)
template <int KIND>
__global__ void __launch_bounds__(AU_THREADS)
audit2_kernel(Bucket2 b, const double *__restrict__ nu, const double *__restrict__ slo, double mu, const double *__restrict__ ovr, AuditArgs a)
{
    extern __shared__ unsigned long long au_tile[];
    constexpr int CLS = audit_class2(KIND);
    audit_tile_clear(au_tile, a.n);
    AuditRec acc = audit_identity();
    for (long long base = (long long)blockIdx.x * AU_THREADS; base < b.m; base += (long long)gridDim.x * AU_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            const long long o = b.perm ? b.perm[i] : i;
            auto sink = [&](double Da, double Db, double La, double Lb) {
                const double g = b.fee[i];
                const double wa = KIND == 0 ? 0.5 : (KIND == 1 ? b.param[i] : (KIND == 4 ? 1.0 - b.param[i] : 0.0));
                const double wb = KIND == 1 ? 1.0 - wa : wa;
                PoolAudit p;
                audit_leg<CLS>(p, au_tile, a, b.ia[i], b.Ra[i], Da, La, g, wa);
                audit_leg<CLS>(p, au_tile, a, b.ib[i], b.Rb[i], Db, Lb, g, wb);
                audit_close<CLS>(p, a, KIND == 3 ? b.param[i] : 0.0, (unsigned long long)o, acc);
            };
            if (ovr) sink(ovr[o], ovr[b.m + o], ovr[2 * b.m + o], ovr[3 * b.m + o]);
            else if (mu > 0.0) smooth_trades_pool<KIND>(b, i, nu, slo, mu, sink);
            else trades2_pool<KIND>(b, i, nu, sink);
        }
    }
    audit_finish(au_tile, a, acc);
}

// geo-mean bucket of K assets: the bucket's normalised weights
template <int K>
__global__ void __launch_bounds__(AU_THREADS)
auditN_kernel(BucketN b, const double *__restrict__ nu, const double *__restrict__ slo, AuditArgs a)
{
    extern __shared__ unsigned long long au_tile[];
    audit_tile_clear(au_tile, a.n);
    AuditRec acc = audit_identity();
    for (long long base = (long long)blockIdx.x * AU_THREADS; base < b.m; base += (long long)gridDim.x * AU_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            const long long o = b.perm ? b.perm[i] : i;
            const double g = b.fee[i];
            PoolAudit p;
            tradesn_pool<K>(b, i, nu, slo, [&](int j, double R, double D, double L) {
                audit_leg<AU_LOG>(p, au_tile, a, b.idx[i * K + j], R, D, L, g, b.w[i * K + j]);
            });
            audit_close<AU_LOG>(p, a, 0.0, (unsigned long long)o, acc);
        }
    }
    audit_finish(au_tile, a, acc);
}

// K-asset table bucket (never permuted).  flags: the caller's per-leg tie flags (constant sum), as the read-back passes them;
// ovr: the caller's own tenders for this bucket (delta [K][m] | lambda [K][m])
template <int KIND, int K>
__global__ void __launch_bounds__(AU_THREADS)
auditG_kernel(BucketG b, const int *flags, const double *__restrict__ nu, const double *__restrict__ slo, double mu, const double *__restrict__ ovr, AuditArgs a)
{
    extern __shared__ unsigned long long au_tile[];
    constexpr int CLS = KIND == 1 ? AU_SUM : AU_STABLE;
    audit_tile_clear(au_tile, a.n);
    AuditRec acc = audit_identity();
    for (long long base = (long long)blockIdx.x * AU_THREADS; base < b.m; base += (long long)gridDim.x * AU_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            const double g = b.fee[i];
            PoolAudit p;
            auto sink = [&](int j, double R, double D, double L) { audit_leg<CLS>(p, au_tile, a, b.idx[i * K + j], R, D, L, g, 0.0); };
            if (ovr) { for (int j = 0; j < K; ++j) sink(j, b.R[i * K + j], ovr[(size_t)j * b.m + i], ovr[(size_t)(K + j) * b.m + i]); }
            else tradesg_pool<KIND, K>(b, i, flags, nu, slo, mu, sink);
            audit_close<CLS>(p, a, KIND == 0 ? b.param[i] : 0.0, (unsigned long long)i, acc);
        }
    }
    audit_finish(au_tile, a, acc);
}

}  // namespace cfmm
