// The prices the resident pools imply, fitted on the device (include/cfmm.h: cfmm_pool_prices; docs/pool_prices.md).
//
// Every pool contributes relations  log p_u - log p_v = lr  at its current resident columns (a two-asset pool one, a K-asset pool K - 1,
// leg j against leg 0); phi minimises sum (phi_u - phi_v - lr)^2, i.e. solves L phi = rhs on the multigraph Laplacian.  Four steps on the
// context's stream, none of them on the solve path:
//   1. the relation pass, SINK = 0 (one templated kernel per bucket family, as audit.hpp and apply.hpp have them): rhs through a
//      per-workgroup LDS tile of n doubles, flushed once (no per-pool global atomics on a token vector), and the dense count matrix
//      C[u][v] = relations between u and v with 32-bit integer atomics -- integers, so the matrix is exact whatever the order.  A token's
//      degree is its row sum (a relation of a token with itself counts 2 on the diagonal, as in the twin), so it needs no tile;
//   2. prices_components_kernel: min-label propagation with pointer jumping over the rows of C, one workgroup, labels in LDS.  The
//      smallest id of a component moves at least one hop per round, so it ends after at most diameter + 1 rounds on any graph;
//   3. prices_cg_kernel: Jacobi-preconditioned conjugate gradients on L = D - C from zero, one workgroup of 1024 threads, the direction
//      vector in LDS, a wave per eight rows of the matrix-vector product.  Every dot product and maximum is reduced in the workgroup in one
//      fixed order: no global atomics, no tickets, no second workgroup to wait for, and the cost of an iteration is a function of n alone;
//   4. the relation pass again, SINK = 1: phi in the tile, max and sum of squares of phi_u - phi_v - lr reduced per workgroup in LDS, one
//      partial per workgroup; the host folds them in slot and workgroup order (prices_rules.hpp).
// The lr are written in plain C++ on the upload's own columns and derived columns (lrw = log(R / w), sR = alpha / prod R), contraction off.
#pragma once
#include "audit.hpp"
#include "prices_rules.hpp"

namespace cfmm {

constexpr int PR_THREADS = prices::REL_THREADS;
constexpr int PR_ONE = 1024;                      // threads of the single-workgroup kernels (components, iteration)
constexpr int PR_ROWS = 8;                        // rows of the matrix a wave carries at once (loads in flight: one CU reads the whole matrix)
static_assert(prices::MAX_TOKENS % prices::ROW_ALIGN == 0, "a row stride never exceeds the token bound the LDS tiles are sized for");
static_assert(PR_THREADS == AP_THREADS, "the relation passes keep the route passes' thread mapping");
static_assert((size_t)prices::MAX_TOKENS * sizeof(double) <= 48 * 1024, "the tile of n doubles fits the LDS a workgroup gets without asking");

struct PricesArgs {
    int n, ld;                        // tokens; entries per matrix row
    double *rhs;                      // global [n] (SINK 0)
    unsigned *mat;                    // global [n][ld] (SINK 0)
    const double *phi;                // global [n] (SINK 1)
    double *part;                     // this bucket's partials {max, ss} per workgroup (SINK 1)
};

struct RelAcc { double mx = 0.0, ss = 0.0; };

// SINK 0: the tile is the workgroup's share of rhs, zero; SINK 1: phi
template <int SINK> __device__ __forceinline__ void prices_tile_open(double *tile, const PricesArgs &a)
{
    for (int j = threadIdx.x; j < a.n; j += PR_THREADS) tile[j] = SINK == 0 ? 0.0 : a.phi[j];
    __syncthreads();
}

// one relation log p_u - log p_v = lr
template <int SINK> __device__ __forceinline__ void prices_relation(double *tile, const PricesArgs &a, RelAcc &acc, int u, int v, double lr)
{
#pragma clang fp contract(off)
    if (SINK == 0) {
        if (lr != 0.0) { unsafeAtomicAdd(&tile[u], lr); unsafeAtomicAdd(&tile[v], -lr); }
        atomicAdd(&a.mat[(size_t)u * a.ld + v], 1u);
        atomicAdd(&a.mat[(size_t)v * a.ld + u], 1u);
    } else {
        const double e = (tile[u] - tile[v]) - lr;
        const double ae = fabs(e);
        acc.mx = ae > acc.mx ? ae : acc.mx;
        acc.ss = acc.ss + e * e;
    }
}

template <int SINK> __device__ __forceinline__ void prices_tile_close(const double *tile, const PricesArgs &a, RelAcc acc)
{
    __shared__ double wmx[PR_THREADS / 64], wss[PR_THREADS / 64];
    __syncthreads();
    if (SINK == 0) {
        for (int j = threadIdx.x; j < a.n; j += PR_THREADS) { const double v = tile[j]; if (v != 0.0) unsafeAtomicAdd(&a.rhs[j], v); }
        return;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double m = __shfl_xor(acc.mx, o, 64), s = __shfl_xor(acc.ss, o, 64);
        acc.mx = m > acc.mx ? m : acc.mx;
        acc.ss += s;
    }
    if ((threadIdx.x & 63) == 0) { wmx[threadIdx.x >> 6] = acc.mx; wss[threadIdx.x >> 6] = acc.ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < PR_THREADS / 64; ++q) { acc.mx = wmx[q] > acc.mx ? wmx[q] : acc.mx; acc.ss += wss[q]; }
        a.part[2 * blockIdx.x] = acc.mx; a.part[2 * blockIdx.x + 1] = acc.ss;
    }
}

// the marginal log-price ratio of a two-asset pool at its reserves (cfmm/problem.py: pool_prices states the same expressions)
template <int KIND> __device__ __forceinline__ double prices_lr2(const Bucket2 &b, long long i)
{
#pragma clang fp contract(off)
    if (KIND == CFMM_POOL_SUM2) return 0.0;
    const double Ra = b.Ra[i], Rb = b.Rb[i];
    if (KIND == CFMM_POOL_CP2) return log(Rb / Ra);
    const double p = b.param[i];
    if (KIND == CFMM_POOL_W2) return log(p * Rb / ((1.0 - p) * Ra));
    if (KIND == CFMM_POOL_POW2) return p * log(Rb / Ra);
    return log((1.0 + p / (Ra * Ra * Rb)) / (1.0 + p / (Ra * Rb * Rb)));
}

template <int KIND, int SINK>
__global__ void __launch_bounds__(PR_THREADS)
prices2_kernel(Bucket2 b, PricesArgs a)
{
    extern __shared__ double pr_tile[];
    prices_tile_open<SINK>(pr_tile, a);
    RelAcc acc;
    for (long long base = (long long)blockIdx.x * PR_THREADS; base < b.m; base += (long long)gridDim.x * PR_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            int u, v;
            if (b.cid != nullptr) { const unsigned pk = b.cid[i]; u = (int)(pk & 0xffffu); v = (int)(pk >> 16); }      // (the compact mirror: ia | ib << 16)
            else { u = b.ia[i]; v = b.ib[i]; }
            prices_relation<SINK>(pr_tile, a, acc, u, v, prices_lr2<KIND>(b, i));
        }
    }
    prices_tile_close<SINK>(pr_tile, a, acc);
}

// geo-mean bucket of K assets: log(w_j R_0 / (w_0 R_j)) = lrw_0 - lrw_j, the halves the upload derived
template <int K, int SINK>
__global__ void __launch_bounds__(PR_THREADS)
pricesN_kernel(BucketN b, PricesArgs a)
{
    extern __shared__ double pr_tile[];
    prices_tile_open<SINK>(pr_tile, a);
    RelAcc acc;
    for (long long base = (long long)blockIdx.x * PR_THREADS; base < b.m; base += (long long)gridDim.x * PR_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
            const int v = b.idx[i * K];
            const double l0 = b.lrw[i * K];
#pragma unroll
            for (int j = 1; j < K; ++j) prices_relation<SINK>(pr_tile, a, acc, b.idx[i * K + j], v, l0 - b.lrw[i * K + j]);
        }
    }
    prices_tile_close<SINK>(pr_tile, a, acc);
}

// K-asset table bucket: stableswap log1p(s / R_j) - log1p(s / R_0) with s = alpha / prod R (the derived column sR); constant sum 0
template <int KIND, int K, int SINK>
__global__ void __launch_bounds__(PR_THREADS)
pricesG_kernel(BucketG b, PricesArgs a)
{
    extern __shared__ double pr_tile[];
    prices_tile_open<SINK>(pr_tile, a);
    RelAcc acc;
    for (long long base = (long long)blockIdx.x * PR_THREADS; base < b.m; base += (long long)gridDim.x * PR_THREADS) {
        const long long i = base + threadIdx.x;
        if (i < b.m) {
#pragma clang fp contract(off)
            const int v = b.idx[i * K];
            const double s = KIND == CFMM_POOLK_STABLE ? b.sR[i] : 0.0;
            const double l0 = KIND == CFMM_POOLK_STABLE ? log1p(s / b.R[i * K]) : 0.0;
#pragma unroll
            for (int j = 1; j < K; ++j) {
                const double lj = KIND == CFMM_POOLK_STABLE ? log1p(s / b.R[i * K + j]) : 0.0;
                prices_relation<SINK>(pr_tile, a, acc, b.idx[i * K + j], v, lj - l0);
            }
        }
    }
    prices_tile_close<SINK>(pr_tile, a, acc);
}

// ---- the single-workgroup kernels over the count matrix -----------------------------------------------------------------------------
// sum and maximum over the workgroup in one fixed order (lanes by butterfly, waves in wave order); every thread gets the result
__device__ __forceinline__ void prices_reduce(double &s, double &m)
{
    __shared__ double ws[PR_ONE / 64], wm[PR_ONE / 64];
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(s, o, 64), x = __shfl_xor(m, o, 64);
        s += t;
        m = x > m ? x : m;
    }
    __syncthreads();                                    // (the scratch may still be read from an earlier reduction)
    if ((threadIdx.x & 63) == 0) { ws[threadIdx.x >> 6] = s; wm[threadIdx.x >> 6] = m; }
    __syncthreads();
    s = ws[0]; m = wm[0];
    for (int q = 1; q < PR_ONE / 64; ++q) { s += ws[q]; m = wm[q] > m ? wm[q] : m; }
}

// labels: every token ends on the smallest token id of its component.  LDS: cur [ld] | nxt [ld] (the tails past n are never used: their
// matrix entries are zero)
__global__ void __launch_bounds__(PR_ONE)
prices_components_kernel(const unsigned *__restrict__ mat, int n, int ld, int *__restrict__ label, PricesCg *cg)
{
    extern __shared__ int pr_lab[];
    int *cur = pr_lab, *nxt = pr_lab + ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < ld; j += PR_ONE) cur[j] = j;
    int rounds = 0;
    for (;;) {
        __syncthreads();
        for (int u0 = wave * PR_ROWS; u0 < n; u0 += (PR_ONE / 64) * PR_ROWS) {
            int m[PR_ROWS];
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) m[r] = n;
            for (int v4 = lane; v4 < ld / 4; v4 += 64) {
                const int v = 4 * v4;
                const int l0 = cur[v], l1 = cur[v + 1], l2 = cur[v + 2], l3 = cur[v + 3];
#pragma unroll
                for (int r = 0; r < PR_ROWS; ++r) {
                    const int u = u0 + r < n ? u0 + r : n - 1;                  // (a row past the end reads the last one; its label is dropped)
                    const uint4 c = reinterpret_cast<const uint4 *>(mat + (size_t)u * ld)[v4];
                    const int a = min(c.x ? l0 : n, c.y ? l1 : n), b = min(c.z ? l2 : n, c.w ? l3 : n);
                    m[r] = min(m[r], min(a, b));
                }
            }
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) {
                int x = m[r];
                for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
                const int u = u0 + r;
                if (lane == 0 && u < n) nxt[u] = min(x, cur[u]);
            }
        }
        __syncthreads();
        int changed = 0;
        for (int j = threadIdx.x; j < n; j += PR_ONE) {      // pointer jumping: nxt is only read here, cur only written
            const int c = nxt[nxt[j]];
            changed |= c != cur[j];
            cur[j] = c;
        }
        ++rounds;
        if (!__syncthreads_or(changed) || rounds > n + 1) break;
    }
    for (int j = threadIdx.x; j < n; j += PR_ONE) label[j] = cur[j];
    if (threadIdx.x == 0) cg->rounds = rounds;
}

// q = (D - C) p for the rows of this wave, PR_ROWS at a time; p in LDS (its tail up to ld zero), q to global
__device__ __forceinline__ void prices_matvec(const unsigned *__restrict__ mat, const unsigned *__restrict__ deg, int n, int ld, const double *p, double *q)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int u0 = wave * PR_ROWS; u0 < n; u0 += (PR_ONE / 64) * PR_ROWS) {
        double acc[PR_ROWS];
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) acc[r] = 0.0;
        for (int v4 = lane; v4 < ld / 4; v4 += 64) {
            const int v = 4 * v4;
            const double p0 = p[v], p1 = p[v + 1], p2 = p[v + 2], p3 = p[v + 3];
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) {
                const int u = u0 + r < n ? u0 + r : n - 1;                  // (a row past the end reads the last one; its sum is dropped)
                const uint4 c = reinterpret_cast<const uint4 *>(mat + (size_t)u * ld)[v4];
                acc[r] += ((double)c.x * p0 + (double)c.y * p1) + ((double)c.z * p2 + (double)c.w * p3);
            }
        }
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) {
            double s = acc[r];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const int u = u0 + r;
            if (lane == 0 && u < n) q[u] = (double)deg[u] * p[u] - s;
        }
    }
}

// Jacobi-preconditioned conjugate gradients from zero (cfmm/problem.py: pool_prices is the twin).  Thread t owns the entries j = t mod
// PR_ONE of phi, r and q in global memory; p is the LDS tile [ld].  deg [n] (the row sums, exact) is written for the host as well
__global__ void __launch_bounds__(PR_ONE)
prices_cg_kernel(const unsigned *__restrict__ mat, const double *__restrict__ rhs, int n, int ld, int cap, double *phi, double *r, double *q, unsigned *deg, PricesCg *cg)
{
    extern __shared__ double pr_dir[];
    double *p = pr_dir;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int u = wave; u < n; u += PR_ONE / 64) {
        unsigned s = 0u;
        const uint4 *row = reinterpret_cast<const uint4 *>(mat + (size_t)u * ld);
        for (int v4 = lane; v4 < ld / 4; v4 += 64) { const uint4 c = row[v4]; s += (c.x + c.y) + (c.z + c.w); }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) deg[u] = s;
    }
    for (int j = n + threadIdx.x; j < ld; j += PR_ONE) p[j] = 0.0;
    __syncthreads();
    double rz = 0.0, rmax = 0.0;
    for (int j = threadIdx.x; j < n; j += PR_ONE) {
        const double b = rhs[j], d = (double)max(deg[j], 1u), z = b / d;
        phi[j] = 0.0; r[j] = b; p[j] = z;
        rz += b * z;
        const double ab = fabs(b);
        rmax = ab > rmax ? ab : rmax;
    }
    prices_reduce(rz, rmax);
    const double rhs_max = rmax;
    const double stop = prices::STOP * (rhs_max > 1e-300 ? rhs_max : 1e-300);
    int it = 0, status = 0;
    while (rmax > stop) {
        if (it >= cap) { status = 1; break; }
        __syncthreads();
        prices_matvec(mat, deg, n, ld, p, q);
        __syncthreads();
        double pq = 0.0, none = 0.0;
        for (int j = threadIdx.x; j < n; j += PR_ONE) pq += p[j] * q[j];
        prices_reduce(pq, none);
        if (!(pq > 0.0)) { status = 1; break; }              // (a direction the operator does not see: nothing to gain)
        const double alpha = rz / pq;
        double rz_new = 0.0;
        rmax = 0.0;
        for (int j = threadIdx.x; j < n; j += PR_ONE) {
            const double d = (double)max(deg[j], 1u);
            phi[j] += alpha * p[j];
            const double rj = r[j] - alpha * q[j];
            r[j] = rj;
            rz_new += rj * (rj / d);
            const double ar = fabs(rj);
            rmax = ar > rmax ? ar : rmax;
        }
        prices_reduce(rz_new, rmax);
        const double beta = rz_new / rz;
        for (int j = threadIdx.x; j < n; j += PR_ONE) p[j] = r[j] / (double)max(deg[j], 1u) + beta * p[j];
        rz = rz_new;
        ++it;
    }
    if (threadIdx.x == 0) {
        cg->residual = rhs_max > 0.0 ? rmax / rhs_max : 0.0;
        cg->rhs_max = rhs_max;
        cg->iterations = it; cg->status = status;
    }
}

}  // namespace cfmm
