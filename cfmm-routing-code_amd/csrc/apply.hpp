// Applying a solve's trades to the resident pools (include/cfmm.h: cfmm_apply_trades), and reading resident reserves back
// (cfmm_get_reserves2 / N / G).
//
// One templated pass per bucket family.  A pass reads a pool's columns once, gets the pool's tenders from the SAME per-pool code the
// read-backs use (kernels.hpp: trades2_pool / tradesn_pool; smooth.hpp: smooth_trades_pool; phik.hpp: tradesg_pool) and forms
//      R' = (R + g Delta) - Lambda,      g = 1 (the fee stays in the pool) or gamma (the fee is collected outside),
// every operation individually rounded -- what NumPy gives on the tenders cfmm_get_trades* returns.
//   WRITE = false   writes no pool: counts the pools that move and the pools with a leg that would not stay positive and finite, takes
//                   the smallest offending position (in upload order) and the largest new reserve into the bucket's ApplyRec
//   WRITE = true    stores the reserves and what the upload derives from them (kernels.hpp: lrw_leg; phik.hpp: gk_coupling, the warm
//                   start dropped), through the same device expressions: an applied pool is bitwise an uploaded one
// The weighted and geo-mean tender iterations stop on a wave-wide test, so a pool's last bits depend on its wave neighbours: the passes
// keep the read-back kernels' mapping (256 threads, pool i on thread i in stored order, the same guard), and both passes and
// cfmm_get_trades* see the same neighbours.
#pragma once
#include "kernels.hpp"
#include "smooth.hpp"
#include "phik.hpp"
#include "route_rules.hpp"             // ApplyRec: what a WRITE = false pass leaves per bucket

namespace cfmm {

constexpr int AP_THREADS = 256;
static_assert(AP_THREADS == GK_THREADS, "the apply passes keep the read-back kernels' thread mapping");

__device__ __forceinline__ double post_trade_reserve(double R, double g, double D, double L)
{
#pragma clang fp contract(off)
    const double in = g * D;
    const double up = R + in;
    return up - L;
}
__device__ __forceinline__ bool reserve_ok(double x) { return x > 0.0 && x <= 1.79769313486231570815e308; }

// the end of a WRITE = false pass: every thread of the workgroup arrives (threads past the bucket's end with moved = bad = false,
// mx = 0).  Reduced over the wave, then over the workgroup's waves in LDS: one thread per workgroup touches the record, and the maximum
// only when it would raise it (it only ever grows, so a stale read errs on the side of the atomic) -- per-wave atomics on one record
// serialised 1.5e4 waves of a 1e6-pool bucket into 0.4 ms
__device__ __forceinline__ void apply_tally(ApplyRec *rec, bool moved, bool bad, long long pos, double mx)
{
    __shared__ unsigned long long part[AP_THREADS / 64][4];
    unsigned long long nm = __popcll(__ballot(moved)), nb = __popcll(__ballot(bad));
    unsigned long long first = bad ? (unsigned long long)pos : ~0ull;
    unsigned long long bits = mx > 0.0 ? (unsigned long long)__double_as_longlong(mx) : 0ull;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long f = __shfl_xor(first, o, 64), v = __shfl_xor(bits, o, 64);
        first = f < first ? f : first;
        bits = v > bits ? v : bits;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[w][0] = nm; part[w][1] = nb; part[w][2] = first; part[w][3] = bits; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int q = 1; q < AP_THREADS / 64; ++q) {
        nm += part[q][0]; nb += part[q][1];
        first = part[q][2] < first ? part[q][2] : first;
        bits = part[q][3] > bits ? part[q][3] : bits;
    }
    if (nm) atomicAdd(&rec->moved, nm);
    if (nb) { atomicAdd(&rec->refused, nb); atomicMin(&rec->first, first); }
    if (bits > *(volatile unsigned long long *)&rec->maxbits) atomicMax(&rec->maxbits, bits);
}

// two-asset bucket.  mu > 0: behind a second-order solve (the gross smoothed tenders); ovr: the tenders a kink loop of the library left
// on the host (delta [2][m] | lambda [2][m] in upload order, partial fills included) instead of the pool's own
template <int KIND, bool WRITE>
__global__ void __launch_bounds__(AP_THREADS)
apply2_kernel(Bucket2 b, const double *__restrict__ nu, const double *__restrict__ slo, double mu, int aside, const double *__restrict__ ovr, ApplyRec *rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool moved = false, bad = false;
    long long o = 0;
    double mx = 0.0;
    if (i < b.m) {
        o = b.perm ? b.perm[i] : i;
        auto commit = [&](double Da, double Db, double La, double Lb) {
            const double g = aside ? b.fee[i] : 1.0;
            const double na = post_trade_reserve(b.Ra[i], g, Da, La), nb = post_trade_reserve(b.Rb[i], g, Db, Lb);
            moved = Da != 0.0 || Db != 0.0 || La != 0.0 || Lb != 0.0;
            bad = !(reserve_ok(na) && reserve_ok(nb));
            mx = fmax(na, nb);
            if (WRITE) { const_cast<double *>(b.Ra)[i] = na; const_cast<double *>(b.Rb)[i] = nb; }
        };
        if (ovr) commit(ovr[o], ovr[b.m + o], ovr[2 * b.m + o], ovr[3 * b.m + o]);
        else if (mu > 0.0) smooth_trades_pool<KIND>(b, i, nu, slo, mu, commit);
        else trades2_pool<KIND>(b, i, nu, commit);
    }
    if (!WRITE) apply_tally(rec, moved, bad, o, mx);
}

// geo-mean bucket of K assets: + lrw = log(R' / w) per leg
template <int K, bool WRITE>
__global__ void __launch_bounds__(AP_THREADS)
applyN_kernel(BucketN b, const double *__restrict__ nu, const double *__restrict__ slo, int aside, ApplyRec *rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool moved = false, bad = false;
    long long o = 0;
    double mx = 0.0;
    if (i < b.m) {
        o = b.perm ? b.perm[i] : i;
        const double g = aside ? b.fee[i] : 1.0;
        tradesn_pool<K>(b, i, nu, slo, [&](int j, double R, double D, double L) {
            const double nr = post_trade_reserve(R, g, D, L);
            moved |= D != 0.0 || L != 0.0;
            bad |= !reserve_ok(nr);
            mx = fmax(mx, nr);
            if (WRITE) {
                const_cast<double *>(b.R)[i * K + j] = nr;
                const_cast<double *>(b.lrw)[i * K + j] = lrw_leg(nr, b.w[i * K + j]);
            }
        });
    }
    if (!WRITE) apply_tally(rec, moved, bad, o, mx);
}

// K-asset table bucket (never permuted): + s_R = alpha / prod R', the evaluation tiles' warm start dropped (NaN, as at upload)
template <int KIND, int K, bool WRITE>
__global__ void __launch_bounds__(AP_THREADS)
applyG_kernel(BucketG b, const double *__restrict__ nu, const double *__restrict__ slo, double mu, int aside, ApplyRec *rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool moved = false, bad = false;
    double mx = 0.0;
    if (i < b.m) {
        const double g = aside ? b.fee[i] : 1.0;
        tradesg_pool<KIND, K>(b, i, nullptr, nu, slo, mu, [&](int j, double R, double D, double L) {
            const double nr = post_trade_reserve(R, g, D, L);
            moved |= D != 0.0 || L != 0.0;
            bad |= !reserve_ok(nr);
            mx = fmax(mx, nr);
            if (WRITE) const_cast<double *>(b.R)[i * K + j] = nr;
        });
        if (WRITE) {
            const_cast<double *>(b.sR)[i] = b.param ? gk_coupling(b.R + i * K, 1, K, b.param[i]) : 0.0;
            b.ws[i] = __builtin_nan("");
        }
    }
    if (!WRITE) apply_tally(rec, moved, bad, i, mx);
}

// ---- resident reserves back in upload order (plain gathers through perm) -----------------------------------------------------------
__global__ void __launch_bounds__(AP_THREADS)
reserves2_kernel(Bucket2 b, double *__restrict__ Ra, double *__restrict__ Rb, double *__restrict__ param)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.m) return;
    const long long o = b.perm ? b.perm[i] : i;
    Ra[o] = b.Ra[i]; Rb[o] = b.Rb[i];
    if (param) param[o] = b.param[i];
}
// pool-major legs R[i K + j] -> slot-major out[j m + o]; pcol / param: the bucket's per-pool parameter column, or null
__global__ void __launch_bounds__(AP_THREADS)
reservesK_kernel(const double *__restrict__ R, const int *__restrict__ perm, long long m, int K, double *__restrict__ out,
                 const double *__restrict__ pcol, double *__restrict__ param)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long o = perm ? perm[i] : i;
    for (int j = 0; j < K; ++j) out[(long long)j * m + o] = R[i * K + j];
    if (param) param[o] = pcol[i];
}

}  // namespace cfmm
