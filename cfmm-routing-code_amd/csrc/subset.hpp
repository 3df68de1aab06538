// Selecting pools of a solved route on the device (include/cfmm.h: cfmm_select_pools) and reading the selection back as compacted lists
// of upload-order positions (cfmm_get_selected2 / N / G).
//
// One templated pass per bucket family measures every pool by the value it takes in at the solution prices,
//      v = sum_j nu_j Delta_j      over the pool's legs in slot order, every product and every sum individually rounded,
// on the tenders of the SAME per-pool code the read-backs and the apply passes use (kernels.hpp: trades2_pool / tradesn_pool; smooth.hpp:
// smooth_trades_pool; phik.hpp: tradesg_pool) under their thread mapping (apply.hpp: 256 threads, pool i on thread i in stored order, the
// same guard): the weighted and geo-mean tender iterations stop on a wave-wide test, so only then does a pool see the neighbours the
// read-back gave it and NumPy on the read-back tenders reproduces v bit for bit.  A pool is selected iff v is finite and v > thr.
//   the mask      one bit per pool in UPLOAD order (bit o % 64 of word o / 64): a bucket stored in the caller's order writes whole ballot
//                 words, a reordered one sets its bits through perm with atomicOr into words zeroed in front of the pass
//   the tally     every workgroup leaves ONE partial (SelRec) in a slot of its own; select_fold_kernel sums a bucket's partials in a
//                 fixed order.  No atomics on shared records and nothing order-dependent inside a bucket
// The compaction is a two-pass scan over the mask words: per-workgroup popcounts, ONE single-workgroup scan of them, then every workgroup
// writes its positions behind its own offset.  No workgroup waits for another one anywhere: three launches, no look-back, no gate.
#pragma once
#include "kernels.hpp"
#include "smooth.hpp"
#include "phik.hpp"
#include "subset_rules.hpp"            // SelRec, the words and the thread counts

namespace cfmm {

constexpr int SEL_THREADS = subset::SEL_THREADS, SCAN_THREADS = subset::SCAN_THREADS;
static_assert(SEL_THREADS == GK_THREADS, "the selection passes keep the read-back kernels' thread mapping");

// v + nu D, the product and the sum rounded on their own (first leg: the product alone)
__device__ __forceinline__ double value_in_leg(bool first, double v, double nu, double D)
{
#pragma clang fp contract(off)
    const double p = nu * D;
    const double s = v + p;
    return first ? p : s;
}

struct SelArgs {
    unsigned long long *words;        // the bucket's mask
    SelRec *part;                     // one per workgroup of the pass
    double thr;
};

// the end of a pass: every thread of the workgroup arrives (threads past the bucket's end with live = false).  i: the pool's stored
// position, o: its upload position
__device__ __forceinline__ void select_commit(const SelArgs &a, bool live, long long i, long long o, long long m, bool permuted, double v)
{
    __shared__ double part[SEL_THREADS / 64][4];
    const bool fin = live && fabs(v) <= 1.79769313486231570815e308;       // (false for NaN)
    const bool sel = fin && v > a.thr;
    const unsigned long long bs = __ballot(sel);
    if (permuted) {
        if (sel) atomicOr(&a.words[o >> 6], 1ull << (o & 63));
    } else if ((threadIdx.x & 63) == 0 && i < m) a.words[i >> 6] = bs;       // (i is a multiple of 64 here: the wave's own word)
    double ns = (double)__popcll(bs), nn = (double)__popcll(__ballot(live && !fin));      // (exact: at most 256 per workgroup)
    double vt = fin ? v : 0.0, vs = sel ? v : 0.0;
    for (int s = 32; s > 0; s >>= 1) { vt += __shfl_xor(vt, s, 64); vs += __shfl_xor(vs, s, 64); }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[w][0] = ns; part[w][1] = nn; part[w][2] = vt; part[w][3] = vs; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int q = 1; q < SEL_THREADS / 64; ++q) { ns += part[q][0]; nn += part[q][1]; vt += part[q][2]; vs += part[q][3]; }
    SelRec r;
    r.selected = (unsigned long long)ns; r.non_finite = (unsigned long long)nn; r.value_total = vt; r.value_selected = vs;
    a.part[blockIdx.x] = r;
}

// two-asset bucket.  mu > 0: behind a second-order solve (the gross smoothed tenders); ovr: the tenders a kink loop of the library left
// on the host (delta [2][m] | lambda [2][m] in upload order, partial fills included) instead of the pool's own
template <int KIND>
__global__ void __launch_bounds__(SEL_THREADS)
select2_kernel(Bucket2 b, const double *__restrict__ nu, const double *__restrict__ slo, double mu, const double *__restrict__ ovr, SelArgs a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < b.m;
    long long o = i;
    double v = 0.0;
    if (live) {
        o = b.perm ? b.perm[i] : i;
        const double na = nu[b.ia[i]], nb = nu[b.ib[i]];
        auto sink = [&](double Da, double Db, double, double) { v = value_in_leg(false, value_in_leg(true, 0.0, na, Da), nb, Db); };
        if (ovr) sink(ovr[o], ovr[b.m + o], 0.0, 0.0);
        else if (mu > 0.0) smooth_trades_pool<KIND>(b, i, nu, slo, mu, sink);
        else trades2_pool<KIND>(b, i, nu, sink);
    }
    select_commit(a, live, i, o, b.m, b.perm != nullptr, v);
}

// geo-mean bucket of K assets
template <int K>
__global__ void __launch_bounds__(SEL_THREADS)
selectN_kernel(BucketN b, const double *__restrict__ nu, const double *__restrict__ slo, SelArgs a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < b.m;
    long long o = i;
    double v = 0.0;
    if (live) {
        o = b.perm ? b.perm[i] : i;
        tradesn_pool<K>(b, i, nu, slo, [&](int j, double, double D, double) { v = value_in_leg(j == 0, v, nu[b.idx[i * K + j]], D); });
    }
    select_commit(a, live, i, o, b.m, b.perm != nullptr, v);
}

// K-asset table bucket (never permuted)
template <int KIND, int K>
__global__ void __launch_bounds__(SEL_THREADS)
selectG_kernel(BucketG b, const double *__restrict__ nu, const double *__restrict__ slo, double mu, SelArgs a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < b.m;
    double v = 0.0;
    if (live)
        tradesg_pool<KIND, K>(b, i, nullptr, nu, slo, mu, [&](int j, double, double D, double) { v = value_in_leg(j == 0, v, nu[b.idx[i * K + j]], D); });
    select_commit(a, live, i, i, b.m, false, v);
}

// one workgroup per bucket slot: the slot's partials part[off[q] .. off[q + 1]) summed in a fixed order (thread t takes t, t + 256, ..;
// then a tree over the threads) into recs[q]
struct SelFold { unsigned long long off[route::SLOTS + 1]; };
__global__ void __launch_bounds__(SEL_THREADS)
select_fold_kernel(const SelRec *__restrict__ part, SelFold f, SelRec *__restrict__ recs)
{
    __shared__ SelRec sh[SEL_THREADS];
    const unsigned long long lo = f.off[blockIdx.x], hi = f.off[blockIdx.x + 1];
    SelRec r = {0ull, 0ull, 0.0, 0.0};
    for (unsigned long long p = lo + threadIdx.x; p < hi; p += SEL_THREADS) {
        const SelRec x = part[p];
        r.selected += x.selected; r.non_finite += x.non_finite; r.value_total += x.value_total; r.value_selected += x.value_selected;
    }
    sh[threadIdx.x] = r;
    __syncthreads();
    for (int s = SEL_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const SelRec x = sh[threadIdx.x + s];
            SelRec &y = sh[threadIdx.x];
            y.selected += x.selected; y.non_finite += x.non_finite; y.value_total += x.value_total; y.value_selected += x.value_selected;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) recs[blockIdx.x] = sh[0];
}

// ---- the compaction: mask words -> ascending upload-order positions ----------------------------------------------------------------
// pass 1: cnt[g] = the set bits of workgroup g's SCAN_THREADS words
__global__ void __launch_bounds__(SCAN_THREADS)
selected_count_kernel(const unsigned long long *__restrict__ words, long long nwords, unsigned *__restrict__ cnt)
{
    __shared__ unsigned wsum[SCAN_THREADS / 64];
    const long long w = (long long)blockIdx.x * SCAN_THREADS + threadIdx.x;
    unsigned c = w < nwords ? (unsigned)__popcll(words[w]) : 0u;
    for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { for (int q = 1; q < SCAN_THREADS / 64; ++q) c += wsum[q]; cnt[blockIdx.x] = c; }
}

// the workgroup's exclusive prefix of one value per thread (and the workgroup's total): wave scans, then the waves' totals in LDS
__device__ __forceinline__ unsigned block_exclusive(unsigned x, unsigned *total)
{
    __shared__ unsigned wtot[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = x;
    for (int s = 1; s < 64; s <<= 1) { const unsigned y = __shfl_up(inc, s, 64); if (lane >= s) inc += y; }
    __syncthreads();                                    // (the scratch may still be read from an earlier round)
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    unsigned base = 0, all = 0;
    for (int q = 0; q < SCAN_THREADS / 64; ++q) { if (q < w) base += wtot[q]; all += wtot[q]; }
    *total = all;
    return base + inc - x;
}

// the scan, ONE workgroup: cnt[0 .. groups) becomes its own exclusive prefix in place, cnt[groups] the total
__global__ void __launch_bounds__(SCAN_THREADS)
selected_scan_kernel(unsigned *cnt, long long groups)
{
    unsigned carry = 0;
    for (long long base = 0; base < groups; base += SCAN_THREADS) {
        const long long g = base + threadIdx.x;
        const unsigned x = g < groups ? cnt[g] : 0u;
        unsigned total;
        const unsigned ex = block_exclusive(x, &total);
        if (g < groups) cnt[g] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) cnt[groups] = carry;
}

// pass 2: every set bit's position behind the workgroup's offset, ascending; positions from `cap` on are not written
__global__ void __launch_bounds__(SCAN_THREADS)
selected_write_kernel(const unsigned long long *__restrict__ words, long long nwords, const unsigned *__restrict__ offs, int *__restrict__ out, long long cap)
{
    const long long w = (long long)blockIdx.x * SCAN_THREADS + threadIdx.x;
    unsigned long long bits = w < nwords ? words[w] : 0ull;
    unsigned total;
    long long at = (long long)offs[blockIdx.x] + block_exclusive((unsigned)__popcll(bits), &total);
    for (; bits; bits &= bits - 1, ++at)
        if (at < cap) out[at] = (int)(w * 64 + (__ffsll((long long)bits) - 1));
}

// ---- the sub-network (cfmm_subnetwork): a chosen bucket's columns gathered device to device ----------------------------------------
// sub pool t is the parent's pool list[t] (upload order; a reordered parent is addressed through the inverse of its permutation, as
// the updates address it).  Every column travels as it is -- the parent's derived columns are already bit for bit what an upload of the
// pool's current values makes (update.hpp, apply.hpp: lrw_leg, gk_coupling, 1 / fee on the device; the geo-mean bucket's log fee is the
// HOST's std::log and can only be copied) -- except the table's root-search warm start, which starts as NaN as at upload
constexpr int SUB_THREADS = 256;

__global__ void __launch_bounds__(SUB_THREADS)
subnet2_kernel(Bucket2 s, const int *__restrict__ inv, const int *__restrict__ list, long long cnt, Bucket2 d)
{
    const long long t = (long long)blockIdx.x * SUB_THREADS + threadIdx.x;
    if (t >= cnt) return;
    const int o = list[t];
    const long long p = inv ? inv[o] : o;
    const_cast<double *>(d.Ra)[t] = s.Ra[p]; const_cast<double *>(d.Rb)[t] = s.Rb[p]; const_cast<double *>(d.fee)[t] = s.fee[p];
    if (s.param) const_cast<double *>(d.param)[t] = s.param[p];
    const_cast<int *>(d.ia)[t] = s.ia[p]; const_cast<int *>(d.ib)[t] = s.ib[p];
}

template <int K>
__global__ void __launch_bounds__(SUB_THREADS)
subnetN_kernel(BucketN s, const int *__restrict__ inv, const int *__restrict__ list, long long cnt, BucketN d)
{
    const long long t = (long long)blockIdx.x * SUB_THREADS + threadIdx.x;
    if (t >= cnt) return;
    const int o = list[t];
    const long long p = inv ? inv[o] : o;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const_cast<int *>(d.idx)[t * K + j] = s.idx[p * K + j];
        const_cast<double *>(d.R)[t * K + j] = s.R[p * K + j];
        const_cast<double *>(d.w)[t * K + j] = s.w[p * K + j];
        const_cast<double *>(d.lrw)[t * K + j] = s.lrw[p * K + j];
    }
    const_cast<double *>(d.fee)[t] = s.fee[p]; const_cast<double *>(d.lfee)[t] = s.lfee[p];
}

template <int K>
__global__ void __launch_bounds__(SUB_THREADS)
subnetG_kernel(BucketG s, const int *__restrict__ list, long long cnt, BucketG d)
{
    const long long t = (long long)blockIdx.x * SUB_THREADS + threadIdx.x;
    if (t >= cnt) return;
    const long long p = list[t];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const_cast<int *>(d.idx)[t * K + j] = s.idx[p * K + j];
        const_cast<double *>(d.R)[t * K + j] = s.R[p * K + j];
    }
    const_cast<double *>(d.fee)[t] = s.fee[p];
    if (s.param) const_cast<double *>(d.param)[t] = s.param[p];
    const_cast<double *>(d.ifee)[t] = s.ifee[p]; const_cast<double *>(d.sR)[t] = s.sR[p];
    d.ws[t] = __builtin_nan("");
}

}  // namespace cfmm
