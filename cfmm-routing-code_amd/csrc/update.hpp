// In-place update of resident pools' reserves (and the stableswap alpha / power-sum t of the two-asset kinds, alpha of the
// table's stableswap pools): what a router does between two blocks, where only a small share of the pools has
// traded (include/cfmm.h: cfmm_update_pools2 / N / G).
//
// The caller names a pool by its index in the order it uploaded the bucket (the index cfmm_get_trades* reports in).  A bucket
// that the token-block ordering permuted (reorder.hpp: Bucket2::perm / BucketN::perm, position -> caller index) is addressed
// through the inverse permutation, built here once per bucket, on the device, the first time the bucket is updated.
//
// One launch per call scatters the staged records (one H2D copy: positions, then the new values, slot-major as the ABI hands
// them) into the resident columns and recomputes the derived columns from the SAME device expressions the upload uses
// (kernels.hpp: lrw_leg; phik.hpp: gk_coupling), so that an updated pool is bitwise the pool a fresh upload would have made.
// The compact mirror (ids, fee) is untouched: neither changes.  The bucket's largest reserve fixes the reproducible mode's
// fixed-point exponent: every scatter reads the value it overwrites and raises `lowered` when a reserve equal to the recorded
// maximum goes down -- only then is the bucket reduced again (upd_max_kernel); otherwise the new maximum is the larger of the
// old one and the largest new reserve, which the host knows from its validation pass.
#pragma once
#include "kernels.hpp"
#include "phik.hpp"

namespace cfmm {

constexpr int UP_THREADS = 256;

// inv[perm[p]] = p
__global__ void __launch_bounds__(UP_THREADS) upd_inverse_kernel(const int *__restrict__ perm, long long m, int *__restrict__ inv)
{
    const long long stride = (long long)gridDim.x * UP_THREADS;
    for (long long p = (long long)blockIdx.x * UP_THREADS + threadIdx.x; p < m; p += stride) inv[perm[p]] = (int)p;
}

// two-asset bucket: pos[count], Ra[count], Rb[count], param[count] or null (unchanged)
__global__ void __launch_bounds__(UP_THREADS)
upd_scatter2_kernel(Bucket2 b, int count, const int *__restrict__ pos, const double *__restrict__ Ra, const double *__restrict__ Rb,
                    const double *__restrict__ param, const int *__restrict__ inv, double mx, int *__restrict__ lowered)
{
    const int i = blockIdx.x * UP_THREADS + threadIdx.x;
    if (i >= count) return;
    const int q = pos[i];
    const long long p = inv ? inv[q] : q;
    double *ra = const_cast<double *>(b.Ra), *rb = const_cast<double *>(b.Rb);
    const double oa = ra[p], ob = rb[p], na = Ra[i], nb = Rb[i];
    if ((oa == mx && na < oa) || (ob == mx && nb < ob)) *lowered = 1;
    ra[p] = na; rb[p] = nb;
    if (param) const_cast<double *>(b.param)[p] = param[i];
}

// geo-mean bucket of K assets: R slot-major [K][count] in, pool-major legs out, + lrw = log(R / w) per leg
__global__ void __launch_bounds__(UP_THREADS)
upd_scatterN_kernel(BucketN b, int K, int count, const int *__restrict__ pos, const double *__restrict__ R, const int *__restrict__ inv,
                    double mx, int *__restrict__ lowered)
{
    const int i = blockIdx.x * UP_THREADS + threadIdx.x;
    if (i >= count) return;
    const int q = pos[i];
    const long long p = inv ? inv[q] : q;
    double *r = const_cast<double *>(b.R), *lrw = const_cast<double *>(b.lrw);
    bool low = false;
    for (int j = 0; j < K; ++j) {
        const long long leg = p * K + j;
        const double o = r[leg], v = R[(long long)j * count + i];
        low |= o == mx && v < o;
        r[leg] = v;
        lrw[leg] = lrw_leg(v, b.w[leg]);
    }
    if (low) *lowered = 1;
}

// K-asset table bucket (never permuted): R slot-major [K][count], param[count] or null; + s_R = alpha / prod R, and the
// evaluation tiles' warm start of the updated pool dropped (NaN, as at upload)
__global__ void __launch_bounds__(UP_THREADS)
upd_scatterG_kernel(BucketG b, int K, int count, const int *__restrict__ pos, const double *__restrict__ R, const double *__restrict__ param,
                    double mx, int *__restrict__ lowered)
{
    const int i = blockIdx.x * UP_THREADS + threadIdx.x;
    if (i >= count) return;
    const long long p = pos[i];
    double *r = const_cast<double *>(b.R);
    bool low = false;
    for (int j = 0; j < K; ++j) {
        const long long leg = p * K + j;
        const double o = r[leg], v = R[(long long)j * count + i];
        low |= o == mx && v < o;
        r[leg] = v;
    }
    if (low) *lowered = 1;
    double *al = const_cast<double *>(b.param);
    if (al && param) al[p] = param[i];
    const_cast<double *>(b.sR)[p] = al ? gk_coupling(R + i, count, K, param ? param[i] : al[p]) : 0.0;
    b.ws[p] = __builtin_nan("");
}

// largest value of a[0 .. na) and b[0 .. nb) (positive doubles: their bit patterns order like the values) into *out (zeroed first)
__global__ void __launch_bounds__(UP_THREADS)
upd_max_kernel(const double *__restrict__ a, long long na, const double *__restrict__ b, long long nb, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long part[UP_THREADS / 64];
    const long long stride = (long long)gridDim.x * UP_THREADS;
    unsigned long long mx = 0ull;
    for (long long i = (long long)blockIdx.x * UP_THREADS + threadIdx.x; i < na + nb; i += stride) {
        const unsigned long long v = (unsigned long long)__double_as_longlong(i < na ? a[i] : b[i - na]);
        mx = v > mx ? v : mx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(mx, o, 64);
        mx = v > mx ? v : mx;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < UP_THREADS / 64; ++w) mx = part[w] > mx ? part[w] : mx;
        atomicMax(out, mx);
    }
}

// ---- the trading TERMS of resident pools: the fee, and the weights where the family has them (cfmm_update_terms2 / N / G) ----------
// The same frame: one launch per call scatters the staged records and rewrites what the upload derives from a fee or a weight.  The
// bucket's SMALLEST fee fixes the reproducible mode's exponent like the largest reserve does: every scatter reads the fee it
// overwrites and sets `raised` when a fee equal to the recorded minimum `mn` goes up -- only then is the fee column reduced again
// (upd_min_kernel; update_rules.hpp: min_fee_after).

// two-asset bucket: pos[count], fee[count] or null, wa[count] or null (CFMM_POOL_W2's param column)
__global__ void __launch_bounds__(UP_THREADS)
upd_terms2_kernel(Bucket2 b, int count, const int *__restrict__ pos, const double *__restrict__ fee, const double *__restrict__ wa,
                  const int *__restrict__ inv, double mn, int *__restrict__ raised)
{
    const int i = blockIdx.x * UP_THREADS + threadIdx.x;
    if (i >= count) return;
    const int q = pos[i];
    const long long p = inv ? inv[q] : q;
    if (fee) {
        double *f = const_cast<double *>(b.fee);
        const double o = f[p], v = fee[i];
        if (o == mn && v > o) *raised = 1;
        f[p] = v;
    }
    if (wa) const_cast<double *>(b.param)[p] = wa[i];
}

// geo-mean bucket of K assets: fee[count] and lfee[count] = log fee as the HOST forms it (the upload's column is the host's std::log),
// or null; w slot-major [K][count] or null -> pool-major legs, + lrw = log(R / w) per leg from the resident reserve
__global__ void __launch_bounds__(UP_THREADS)
upd_termsN_kernel(BucketN b, int K, int count, const int *__restrict__ pos, const double *__restrict__ fee, const double *__restrict__ lfee,
                  const double *__restrict__ w, const int *__restrict__ inv, double mn, int *__restrict__ raised)
{
    const int i = blockIdx.x * UP_THREADS + threadIdx.x;
    if (i >= count) return;
    const int q = pos[i];
    const long long p = inv ? inv[q] : q;
    if (fee) {
        double *f = const_cast<double *>(b.fee);
        const double o = f[p], v = fee[i];
        if (o == mn && v > o) *raised = 1;
        f[p] = v;
        const_cast<double *>(b.lfee)[p] = lfee[i];
    }
    if (w) {
        double *bw = const_cast<double *>(b.w), *lrw = const_cast<double *>(b.lrw);
        for (int j = 0; j < K; ++j) {
            const long long leg = p * K + j;
            const double v = w[(long long)j * count + i];
            bw[leg] = v;
            lrw[leg] = lrw_leg(b.R[leg], v);
        }
    }
}

// K-asset table bucket (never permuted): fee[count]; + 1 / fee (phik.hpp: gk_derive_kernel's expression), and the evaluation tiles'
// warm start of the updated pool dropped (NaN, as at upload and as the reserve update does)
__global__ void __launch_bounds__(UP_THREADS)
upd_termsG_kernel(BucketG b, int count, const int *__restrict__ pos, const double *__restrict__ fee, double mn, int *__restrict__ raised)
{
    const int i = blockIdx.x * UP_THREADS + threadIdx.x;
    if (i >= count) return;
    const long long p = pos[i];
    double *f = const_cast<double *>(b.fee);
    const double o = f[p], v = fee[i];
    if (o == mn && v > o) *raised = 1;
    f[p] = v;
    const_cast<double *>(b.ifee)[p] = 1.0 / v;
    b.ws[p] = __builtin_nan("");
}

// smallest value of a[0 .. n) (positive doubles) into *out as the COMPLEMENT of its bit pattern: *out is zeroed first, and the largest
// complement is the smallest value (update_rules.hpp: fee_from_reduced)
__global__ void __launch_bounds__(UP_THREADS) upd_min_kernel(const double *__restrict__ a, long long n, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long part[UP_THREADS / 64];
    const long long stride = (long long)gridDim.x * UP_THREADS;
    unsigned long long mx = 0ull;
    for (long long i = (long long)blockIdx.x * UP_THREADS + threadIdx.x; i < n; i += stride) {
        const unsigned long long v = ~(unsigned long long)__double_as_longlong(a[i]);
        mx = v > mx ? v : mx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(mx, o, 64);
        mx = v > mx ? v : mx;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < UP_THREADS / 64; ++w) mx = part[w] > mx ? part[w] : mx;
        atomicMax(out, mx);
    }
}

}  // namespace cfmm
