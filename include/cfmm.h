/* cfmm.h -- C-ABI of libcfmm_hip.so: the MI355X-native replacement for the cvxpy call pair
 *
 *        prob = cp.Problem(obj, cons); prob.solve()
 *
 * at /root/reference/arbitrage.py:81-82, liquidation.py:84-85 and two-asset.py:90-91, plus the
 * result read-back at arbitrage.py:84, liquidation.py:87, two-asset.py:94-100.
 *
 * The reference has no FFI / plugin interface of its own (it is four Python scripts that call
 * cvxpy); this header is the boundary a maintainer binds with ctypes (INTEGRATION.md shows the
 * stub).  Conventions: every entry point returns 0 on success or a negative CFMM_E* code;
 * cfmm_last_error() gives the message; no exceptions, no callbacks; the caller owns every host
 * buffer (the library copies to HBM at upload and back at get); one ctx = one GPU = one host
 * thread at a time.  All floating point is fp64 (NumPy's default in arbitrage.py:14-20), all
 * indices int32.
 *
 * Model (the reference's, arbitrage.py:51-78):
 *      maximise   U(psi)
 *      subject to psi = sum_i A_i (Lambda_i - Delta_i)                      arbitrage.py:54
 *                 phi_i(R_i + gamma_i Delta_i - Lambda_i) >= phi_i(R_i)      arbitrage.py:60,63-74
 *                 Delta_i, Lambda_i >= 0                                     arbitrage.py:51-52
 * solved in its dual-decomposition form: for prices nu every pool is an independent
 * closed-form / Newton subproblem (the HIP kernels), psi(nu) is their scatter-sum, and nu is
 * driven by an on-device projected quasi-Newton iteration in log-prices.
 */
#ifndef CFMM_H
#define CFMM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cfmm_ctx cfmm_ctx;

enum {
    CFMM_OK = 0,
    CFMM_E_ARG = -1,        /* bad argument                                   */
    CFMM_E_HIP = -2,        /* a HIP runtime call failed                      */
    CFMM_E_STATE = -3,      /* call order (e.g. solve before upload)          */
    CFMM_E_LIMIT = -4,      /* size beyond what this build supports           */
    CFMM_E_RCCL = -5,       /* an RCCL call failed                            */
    CFMM_E_NUMERIC = -6,    /* non-finite value met during the iteration      */
    CFMM_E_UNSUPPORTED = -7 /* the requested method cannot take this problem  */
};

#define CFMM_AUTO_NEWTON_MIN_STABLE 4096
/* outer iteration of cfmm_solve */
enum {
    CFMM_METHOD_AUTO = 0,       /* second order when the network holds >= CFMM_AUTO_NEWTON_MIN_STABLE stableswap pools
                                   (the near-linear case the first-order iteration crawls on at scale), else first
                                   order; a first-order run that ends without its certificates is handed on         */
    CFMM_METHOD_LBFGS = 1,      /* projected L-BFGS in log-prices, fully on-device: ONE launch per outer iteration
                                   (iter_kernel, enqueued eagerly with run-ahead on a pinned progress word; no hipGraph
                                   on this default path -- graph replay serves the two-launch iteration only: price
                                   ties, > 2048 tokens, memory > 3)                                                 */
    CFMM_METHOD_NEWTON = 2      /* barrier-smoothed dual Newton: dense n x n Hessian, blocked Cholesky on-device    */
};

/* two-asset pool families: one SoA bucket each (`param` = per-pool 4th column) */
enum {
    CFMM_POOL_CP2 = 0,      /* constant product sqrt(xy)          arbitrage.py:68-70; param = NULL  */
    CFMM_POOL_W2 = 1,       /* weighted geo-mean x^wa y^(1-wa)    arbitrage.py:65 (2 assets); param = wa */
    CFMM_POOL_SUM2 = 2,     /* constant sum x+y, x,y >= 0         arbitrage.py:73-74; param = NULL  */
    CFMM_POOL_CURVE2 = 3,   /* x + y - alpha/(xy) (StableSwap at fixed D)  not in reference; param = alpha */
    CFMM_POOL_POW2 = 4,     /* power sum x^(1-t) + y^(1-t) (YieldSpace's curve; t -> 0: constant sum, t -> 1: towards constant
                               product)  not in reference; param = t in [0.001, 0.999].  The first tenant of the GENERIC
                               bucket: it has no code of its own beyond one table entry (csrc/phi2.hpp: Phi2<4>) -- the exact
                               pool solution, the diagonal metric, the smoothed solution and the tenders all come from the
                               generic root search on that entry's forward exchange function, on both outer iterations   */
    CFMM_POOL_KINDS2 = 5
};
#define CFMM_MAX_POOL_SIZE 8    /* n-asset geo-mean pools: 3..8 assets, one bucket per size */

/* K-asset trading functions OTHER than the weighted geometric mean: the K-asset table (csrc/phik.hpp: one PhiK<KIND> struct per
 * function -- SURVEY 8(f) rank 4; "a pool is whatever constraint line is written", arbitrage.py:63-74), 3..8 assets, one
 * bucket per (kind, size).  Evaluated as wave-tiles (leg per lane, LDS psi tile) in one launch behind the main evaluation; the
 * stableswap entry enters the second-order path with its exact generalised Hessian block, the constant-sum entry with the path's own
 * log barrier on its sign constraints (csrc/phik.hpp: sum_smooth_k -- one scalar root per pool, strictly feasible tenders for every weight,
 * closed-form Hessian). */
enum {
    CFMM_POOLK_STABLE = 0,  /* n-asset stableswap  sum x - alpha / prod x  (the paper's concave form; 2 assets: CFMM_POOL_CURVE2);
                               param = alpha.  Solved by the table's generic two-level search (no closed form)              */
    CFMM_POOLK_SUM = 1,     /* n-asset constant sum  sum x, x >= 0  (arbitrage.py:73-74 with more than two tokens); param = NULL.
                               First order: the exact LP vertex on the device; an optimum ON one of its kinks (a leg drained partly, two
                               tokens tied for cheapest) needs the caller's active-set loop (cfmm_set_ties + cfmm_set_pool_flagsG:
                               cfmm/problem.py) -- or CFMM_METHOD_NEWTON, which needs none (the barrier-smoothed pool fills partly by itself) */
    CFMM_POOLK_KINDS = 2
};

/* token constraint types of the unified utility  max c'psi :  psi_k + h_k (>=, =, free) 0 */
enum { CFMM_GE = 0, CFMM_EQ = 1, CFMM_FREE = 2,
       /* the utility table: separable concave utilities beyond the reference's linear-plus-box (not in the
        * reference, whose objectives are linear: arbitrage.py:78, liquidation.py:80, two-asset.py:87).  The token's c and h carry
        * the entry's two parameters; its price has no bound.  Both outer iterations take them (the first-order one in its generic
        * two-launch form); no price ties, no batching.
        *   CFMM_ULOG   u(Psi) = c log(Psi + h),        c > 0, h >= 0
        *   CFMM_UQUAD  u(Psi) = c Psi - Psi^2 / (2 h),  c >= 0, h > 0   (cfmm_set_utility requires c >= 0 of every entry kind) */
       CFMM_ULOG = 3, CFMM_UQUAD = 4 };

typedef struct {
    double tol_gap;         /* stop when |(nu-c)'(psi+h)| / max(1,|g|)      <= tol_gap     (1e-6) */
    double tol_infeas;      /*      and  max violation / max(|psi|,|h|)     <= tol_infeas  (1e-6) */
    double armijo;          /* sufficient-decrease constant (1e-4)                                 */
    double max_step;        /* cap on one step in log-price (2.0)                                  */
    int32_t max_evals;      /* cap on dual evaluations (2000); a hand-over to the second-order method starts a fresh count */
    int32_t memory;         /* L-BFGS pairs kept, 1..8; 0 = auto (8 up to 32 tokens, else 3: no more evaluations than 4..6 on average and the cheapest update)                                        */
    int32_t iters_per_graph;/* two-launch iteration only (price ties, > 2048 tokens, memory > 3): outer iterations
                               captured per hipGraph replay (4) -- also the chunk length of the pool-sharded RCCL path; the
                               default one-launch-per-iteration path (run-ahead on a progress word) ignores it */
    int32_t pg_rule;        /* 1: stop on the projected-gradient value <= tol_gap instead (used when
                               constant-sum pools are tied: psi then lacks their fill)           */
    int32_t method;         /* CFMM_METHOD_*  (0 = auto)                                                            */
    int32_t max_newton;     /* cap on second-order steps (200)                                                      */
    double barrier_shrink;  /* factor applied to the barrier weight once a step lands near the central path (0.1)   */
} cfmm_opts;

typedef struct {
    int32_t evals;          /* dual evaluations done = passes of every pool through its kernel     */
    int32_t iters;          /* accepted quasi-Newton steps                                         */
    int32_t status;         /* 1 converged, 2 stalled (line search), 3 max_evals, <0 error         */
    int32_t n_ranks;
    double dual_value;      /* g(nu)            upper bound                                        */
    double primal_value;    /* c'psi(nu)        the reference's prob.value (arbitrage.py:84)       */
    double gap, infeas;     /* the two certificates above                                          */
    double wall_seconds;    /* host clock around the outer loop (upload / read-back excluded)      */
    double device_seconds;  /* HIP events around the same region                                   */
    double pg;              /* sum |projected reduced gradient| / max(1,|g|)                       */
    int64_t pool_subproblems;   /* evals * pools on this rank                                      */
    double barrier_mu;      /* final barrier weight of a second-order solve (0 after a first-order one): psi and the
                               tenders read back are then those of the smoothed, strictly feasible primal point     */
    int32_t newton_steps;   /* second-order steps taken (Hessian assemblies + Cholesky factorisations)             */
    int32_t method;         /* CFMM_METHOD_LBFGS or CFMM_METHOD_NEWTON: what produced the result                    */
} cfmm_stats;

/* lifetime ------------------------------------------------------------------------------ */
int cfmm_create(int device, int n_tokens, cfmm_ctx **out);
int cfmm_destroy(cfmm_ctx *ctx);
/* A second context on the same GPU that SHARES the pool columns already resident in HBM (reference-counted,
 * no copy) but has its own stream, utility, prices and solver state: several solves over one pool set --
 * the parameter sweep of two-asset.py:34-100, or independent utilities -- can then be in flight at once
 * (one per host thread), one solve's single-workgroup nu update overlapping another's evaluation kernels.
 * Pools cannot be re-uploaded while clones exist; their reserves, fees and weights can be updated in place through any of them
 * (cfmm_update_pools*, cfmm_update_terms*). */
int cfmm_clone(cfmm_ctx *src, cfmm_ctx **out);
const char *cfmm_last_error(cfmm_ctx *ctx);       /* ctx may be NULL: last error of cfmm_create */
const char *cfmm_backend(cfmm_ctx *ctx);          /* "hip:gfx950"                               */
void cfmm_default_opts(cfmm_opts *o);

/* problem object: replaces local_indices / reserves / fees (arbitrage.py:6-28) and the dense
 * A_i matrices (arbitrage.py:42-48: never materialised -- `ia/ib/idx` ARE A_i) ------------- */
int cfmm_upload_pools2(cfmm_ctx *ctx, int kind, int64_t m, const double *Ra, const double *Rb,
                       const double *fee, const double *param, const int32_t *ia, const int32_t *ib);
/* k-asset weighted geo-mean pools (arbitrage.py:65), slot-major: x[j*m + i] = slot j of pool i;
 * weights normalised to sum 1 per pool */
int cfmm_upload_poolsN(cfmm_ctx *ctx, int k, int64_t m, const int32_t *idx, const double *R,
                       const double *w, const double *fee);
/* pools of the K-asset table (CFMM_POOLK_*), k = 3..8 assets (2 is accepted too: the cross-check of the table's generic search
 * against the two-asset buckets' closed forms, tests/test_gpu_table.py): idx, R slot-major [k][m] like cfmm_upload_poolsN, fee[m],
 * param[m] (alpha for CFMM_POOLK_STABLE, NULL for CFMM_POOLK_SUM).  Replaces a constraint line such as
 * `cp.sum(new_reserves) - alpha * cp.inv_prod(new_reserves) >= ...` / `cp.sum(new_reserves) >= cp.sum(reserves)` over k > 2
 * tokens (arbitrage.py:63-74 in the reference's style; the reference itself ships the two-token forms) */
int cfmm_upload_poolsG(cfmm_ctx *ctx, int kind, int k, int64_t m, const int32_t *idx, const double *R,
                       const double *fee, const double *param);
/* In-place update of resident pools (the per-block loop of a router: between two blocks only the pools that traded change).
 * Writes new reserves -- and, where the kind has one, the parameter (CFMM_POOL_CURVE2 / CFMM_POOLK_STABLE alpha, CFMM_POOL_POW2 t;
 * param NULL = unchanged; every other kind, CFMM_POOL_W2 included, takes NULL only) -- of `count` pools of ONE bucket into the columns
 * already in HBM, and recomputes what the upload derives from them (log(R / w) of the geo-mean legs, alpha / prod R and the root-search
 * warm start of the table's pools) with the same device code: an updated pool is bitwise the pool a fresh upload would have made.  Moves
 * count x (4 + 8 k [+ 8]) bytes instead of the whole pool set.
 *   pos[count]    the pools, by their index in the order the bucket was uploaded (the index cfmm_get_trades* reports in), not by the
 *                 position the library stores them at (large buckets are reordered on the device: the update maps through the inverse)
 *   Ra, Rb        [count];  R: slot-major [k][count], like the uploads
 * Fees and weights are updated by cfmm_update_terms2 / N / G below (cfmm_update_pools2 keeps refusing a CFMM_POOL_W2 parameter).  Token
 * ids can NOT be updated (they decide the reordering): changing them, or adding / removing pools, is a re-upload.
 * Rules:
 *   - everything is checked before anything is written: a position outside [0, m) or named twice, a reserve that is not positive and
 *     finite, a parameter the bucket's upload refuses (the same rule) -> CFMM_E_ARG and the pools are left bit for bit as they were;
 *     count > 0 on an empty bucket -> CFMM_E_STATE, a k without a bucket (outside 3..8 / 2..8) -> CFMM_E_ARG; count == 0 is legal;
 *   - the bucket's largest reserve is kept exact (what a fresh upload would record: the reproducible mode's fixed-point exponent, the
 *     infeasibility floor);
 *   - the pools are shared with every cfmm_clone: an update made through any context of the set is seen by all.  Each notices it on its
 *     next call and drops what it derived from the old reserves (cached solution, the kink loop's tenders, the barrier warm start, the
 *     largest reserve) but keeps its prices, utility, ties and tie flags: cfmm_solve(ctx, NULL, ...) continues from the accepted prices,
 *     and cfmm_get_trades* before any re-solve returns the tenders of the NEW reserves at those prices;
 *   - the writes are ordered behind all work already enqueued on every context of the set, and complete when the call returns; if another
 *     context of the set is inside a solve, evaluation, batch or trade read-back at that moment the call returns CFMM_E_STATE;
 *   - pool-sharded contexts (cfmm_comm_init): positions are local to this rank's shard, and EVERY rank makes the call (count = 0 where it
 *     has nothing to update) so that the global maxima are re-reduced in step at the next solve. */
int cfmm_update_pools2(cfmm_ctx *ctx, int kind, int64_t count, const int32_t *pos,
                       const double *Ra, const double *Rb, const double *param /* NULL = unchanged */);
int cfmm_update_poolsN(cfmm_ctx *ctx, int k, int64_t count, const int32_t *pos, const double *R /* [k][count] */);
int cfmm_update_poolsG(cfmm_ctx *ctx, int kind, int k, int64_t count, const int32_t *pos,
                       const double *R /* [k][count] */, const double *param /* NULL = unchanged */);
/* The trading TERMS of resident pools, in place: the fee, and the weights where the family has them (dynamic-fee pools; liquidity-
 * bootstrapping pools, whose weights move every block).  Writes the new fee / weights of `count` pools of ONE bucket into the columns in
 * HBM and remakes what the upload derives from them, the way the upload makes it: log fee of the geo-mean pools (on the host, as the
 * upload does), log(R / w) of every leg of a pool whose weights are given, 1 / fee of the table's pools (their root-search warm start is
 * dropped), the host copy of the constant-sum bucket's fees that CFMM_METHOD_AUTO's kink loop reads, and the bucket's smallest fee
 * (exact, what a fresh upload would record: the reproducible mode's fixed-point exponent, cfmm_audit's fixed_exponent).  An updated pool
 * is bitwise the pool a fresh upload would have made.  The compact mirror of a large two-asset bucket indexes a table of the bucket's
 * distinct fees: a fee update drops it and the next call that reads the pools builds it again from the new column, so that it is
 * present exactly when a fresh upload would have it (at most 256 distinct fees).
 *   pos[count]    as for cfmm_update_pools*: upload order, mapped through the inverse of the reordering
 *   fee           [count], each in (0, 1], or NULL = unchanged (cfmm_update_termsG has nothing else to take: NULL with count > 0 is refused)
 *   wa            [count], each in (0, 1), CFMM_POOL_W2 only (any other kind: CFMM_E_ARG), or NULL = unchanged
 *   w             slot-major [k][count] like the upload's, each in (0, 1), or NULL = unchanged.  The library normalises weights no more
 *                 than the upload does: a pool's weights summing to 1 is the caller's duty
 * The contract is that of cfmm_update_pools*:
 *   - everything is checked before anything is written: a position outside [0, m) or named twice, a fee or weight the upload refuses
 *     (the same predicates), both value pointers NULL with count > 0 -> CFMM_E_ARG and the pools are left bit for bit as they were;
 *     count > 0 on an empty bucket -> CFMM_E_STATE, a k without a bucket -> CFMM_E_ARG; count == 0 is legal;
 *   - shared with every cfmm_clone, ordered behind all work enqueued on every context of the set, complete on return, CFMM_E_STATE while
 *     another context of the set is inside a solve, evaluation, batch or read-back; every context notices on its next call and drops
 *     what it drops after a reserve update (cached solution, kink tenders, barrier warm start, the extrema, captured launches) but keeps
 *     its prices, utility, ties and tie flags.  Price ties the CALLER formed from an old fee (cfmm_set_ties with an offset of
 *     +- log gamma of a constant-sum pool) are the caller's to refresh;
 *   - pool-sharded contexts: positions local to the rank's shard, and EVERY rank makes the call (count = 0 where it has nothing). */
int cfmm_update_terms2(cfmm_ctx *ctx, int kind, int64_t count, const int32_t *pos,
                       const double *fee /* [count] or NULL = unchanged */, const double *wa /* [count] or NULL; CFMM_POOL_W2 only */);
int cfmm_update_termsN(cfmm_ctx *ctx, int k, int64_t count, const int32_t *pos,
                       const double *fee /* [count] or NULL */, const double *w /* [k][count] slot-major or NULL */);
int cfmm_update_termsG(cfmm_ctx *ctx, int kind, int k, int64_t count, const int32_t *pos, const double *fee /* [count] */);
/* The router's own trades applied to the resident pools, on the device (docs/apply_trades.md): commits exactly the tenders
 * cfmm_get_trades2 / N / G would return at the moment of the call -- every bucket, at the context's accepted prices: the exact pool
 * solutions after a first-order solve or cfmm_set_nu, the gross smoothed tenders after a second-order solve (a leg may both receive and
 * pay), the tenders with their partial fills after CFMM_METHOD_AUTO's own kink loop -- as
 *      R' = (R + g Delta) - Lambda,   every operation individually rounded (what NumPy gives on the read-back tenders),
 * and recomputes what the upload derives from the reserves with the same device code: an applied pool is bitwise the pool a fresh upload
 * of the new reserves would have made, and every bucket's largest reserve is exact.
 *   - all or nothing across all buckets: a first pass writes nothing and computes every pool's new reserves; if any leg would not stay
 *     positive and finite (in practice a constant-sum pool traded at its LP vertex: Lambda = R_out) the call returns CFMM_E_UNSUPPORTED
 *     with the count and the first offender in `info`, and the pools, the generation and every context are bit for bit as they were;
 *   - sharing and ordering are those of cfmm_update_pools*: behind the work every context of the set has enqueued, CFMM_E_STATE while
 *     another one is inside a solve, evaluation, batch or read-back, seen by every clone on its next call.  The calling context keeps its
 *     prices, utility and ties and drops its cached solution, the kink loop's tenders, the barrier warm start and captured launches;
 *   - refusals: no prices yet -> CFMM_E_STATE; tie flags or price ties set by the caller (cfmm_set_pool_flags / G, cfmm_set_ties: the
 *     fills then live with the caller) or a pool-sharded context -> CFMM_E_UNSUPPORTED; another fee_mode -> CFMM_E_ARG. */
enum { CFMM_FEES_TO_POOL = 0,   /* R' = (R + Delta) - Lambda        : the fee stays in the reserves (Uniswap v2, Balancer, Curve) */
       CFMM_FEES_ASIDE   = 1 }; /* R' = (R + gamma * Delta) - Lambda: the fee is collected outside the pool; phi(R') = phi(R)      */

typedef struct {
    int64_t pools_moved;     /* pools with at least one non-zero tender                                          */
    int64_t pools_refused;   /* pools with a leg that would not stay positive and finite; 0 on success           */
    int32_t first_family;    /* of the first refused pool, in bucket order (two-asset kinds 0.., geo-mean sizes   */
    int32_t first_kind;      /*   3..8, table buckets): 0 two-asset, 1 geo-mean, 2 table; kind; size k;          */
    int32_t first_k;         /*   position in UPLOAD order  (-1 each when no pool is refused)                    */
    int32_t _pad;
    int64_t first_pos;
    double  max_reserve;     /* largest reserve resident after the call                                          */
} cfmm_apply_info;

int cfmm_apply_trades(cfmm_ctx *ctx, int fee_mode, cfmm_apply_info *info /* or NULL */);
/* the resident reserves in upload order (the order cfmm_get_trades* reports in), and the parameter column where the kind has one
 * (NULL, or a kind without one: not written); an empty bucket is CFMM_OK and writes nothing */
int cfmm_get_reserves2(cfmm_ctx *ctx, int kind, double *Ra, double *Rb, double *param /* or NULL */);   /* [m], upload order */
int cfmm_get_reservesN(cfmm_ctx *ctx, int k, double *R /* [k][m] slot-major */);
int cfmm_get_reservesG(cfmm_ctx *ctx, int kind, int k, double *R /* [k][m] */, double *param /* or NULL */);
/* measurement hook (tools/apply_timing.py): with `on`, every cfmm_apply_trades brackets each pass's launches with HIP events;
 * out2 (or NULL) receives the seconds of the last apply's checking pass and writing pass */
int cfmm_apply_timers(cfmm_ctx *ctx, int on, double *out2);
/* The route audited on the device (docs/audit.md): does every pool accept the tenders cfmm_get_trades2 / N / G would return at the moment
 * of the call -- every bucket, at the context's accepted prices: the exact pool solutions after a first-order solve or cfmm_set_nu, the
 * gross smoothed tenders after a second-order solve, the tenders with their partial fills after CFMM_METHOD_AUTO's own kink loop -- and
 * what do they add up to?  The answer is formed from the tenders alone, not from the psi the evaluation kernels summed nor from any
 * active-set bookkeeping.  Per pool, with x_j = (R_j + gamma Delta_j) - Lambda_j (every operation rounded on its own):
 *   slack       the relative change of the trading function, >= 0 when the pool accepts the trade:
 *               CFMM_POOL_CP2 / _W2 / geo-mean N   sum_j w_j log(x_j / R_j)              (w = 1/2, 1/2;  wa, 1 - wa;  the bucket's weights)
 *               CFMM_POOL_SUM2 / CFMM_POOLK_SUM    (sum x - sum R) / sum R
 *               CFMM_POOL_CURVE2 / CFMM_POOLK_STABLE   (phi(x) - phi(R)) / (sum R + alpha / prod R),  phi(x) = sum x - alpha / prod x
 *               CFMM_POOL_POW2                     (phi(x) - phi(R)) / phi(R),  phi(x) = sum x^(1 - t);     not finite: counts as -inf
 *   a pool VIOLATES if slack < -tol_pool, or a tender is negative or not finite, or a leg does not stay positive: x_j <= 0 -- for the
 *               constant-sum kinds x_j < -tol_pool sum R: a fully drained leg is feasible there (arbitrage.py:73-74)
 *   tol_pool <= 0: the default 1e-9, the stopping residual of the table's stableswap search (csrc/phik.hpp: pool_stable_k, ftol), the
 *               loosest per-pool solver.
 * psi, exactly: every non-zero Lambda_j adds +Lambda_j to its token and every non-zero Delta_j adds -Delta_j, each floored on its own to
 * the reproducible mode's 96-bit fixed point floor(y 2^F) (F: the exponent cfmm_set_deterministic would use for this context; the mode
 * itself is neither needed nor switched) and accumulated with integer atomics; a contribution that is not finite or has |y 2^F| >= 2^94 is
 * left out and counted.  limbs: the raw sums, laid out as cfmm_debug_eval_limbs'; psi[j]: their value converted once, correctly rounded.
 * Bitwise the same on every run and for any launch geometry.  value / infeas: from that psi and the utility last set (NaN without one):
 * c'psi and the violation of psi + h over max(|psi|, |h|, 1e-12 max reserve) as in cfmm_stats; for CFMM_ULOG / CFMM_UQUAD tokens the
 * entry's u(psi), and only the CFMM_GE / CFMM_EQ tokens enter infeas.
 *   own         NULL, or tenders the CALLER holds for constant-sum buckets (its own kink loop's fills; both arrays of a bucket or
 *               neither): they replace the device's tenders for that bucket.  Ignored for an empty bucket.
 * Violations are a result, not an error: the call returns CFMM_OK.  It changes nothing a later call can see (no pool column, warm start,
 * generation, price, cached solution or captured launch) and counts as a reader of the pools like cfmm_get_trades*; unlike
 * cfmm_apply_trades it serves contexts with tie flags or price ties (it audits what the read-backs return: zeros for flagged pools).
 * Refusals: no prices yet -> CFMM_E_STATE; pool-sharded context -> CFMM_E_UNSUPPORTED; out == NULL -> CFMM_E_ARG; more than 2560 tokens
 * (the workgroup's tile of 3 n limbs) -> CFMM_E_LIMIT. */
typedef struct {            /* replacement tenders the CALLER holds (its own kink loop's fills), upload order, or NULL each */
    const double *sum2_delta, *sum2_lambda;                       /* [2][m] of CFMM_POOL_SUM2                       */
    const double *sumk_delta[CFMM_MAX_POOL_SIZE + 1],             /* index k: [k][m] of the CFMM_POOLK_SUM bucket    */
                 *sumk_lambda[CFMM_MAX_POOL_SIZE + 1];            /*          of k assets                            */
} cfmm_audit_tenders;

typedef struct {
    int64_t pools, pools_trading, pools_violating, legs_out_of_range;
    int32_t worst_family, worst_kind, worst_k, fixed_exponent;    /* family / kind / k as in cfmm_apply_info; F of psi */
    int64_t worst_pos;                                            /* upload order; -1s when no pool is resident        */
    double  min_slack, min_tender, min_leg;                       /* over every pool (+inf when none is resident); min_leg: x_j / max_j R_j */
    double  value, infeas;                                        /* from the audited psi and the utility last set     */
} cfmm_audit;

int cfmm_audit_trades(cfmm_ctx *ctx, const cfmm_audit_tenders *own /* or NULL */, double tol_pool /* <= 0: default */,
                      cfmm_audit *out, double *psi /* [n] or NULL */, uint64_t *limbs /* [3][n] or NULL */);
/* test and measurement hook of the audit's launches (tools/audit_timing.py, tests/test_gpu_audit.py), not part of the product's
 * interface: with `timed`, every cfmm_audit_trades brackets its launches with HIP events; grid > 0: workgroups per pass from then on
 * (1 .. 2048; 0: leave as it is -- the audited result does not depend on it); out2 (or NULL) receives {seconds of the last audit's
 * launches, number of buckets the last audit found stored reordered (positions mapped through the upload's permutation)} */
int cfmm_debug_audit_launch(cfmm_ctx *ctx, int timed, int grid, double *out2);
/* A held route, re-quoted on the pools as they are now (docs/requote.md).  Between the quote and the execution the pools move; on chain a
 * route executes with its INPUTS fixed, and each pool pays what its curve gives at the reserves it has by then.
 *
 * cfmm_hold_route keeps, in device memory the context owns, exactly the tenders cfmm_get_trades2 / N / G would return at the moment of the
 * call, for every bucket (cfmm_apply_trades' contract: the exact pool solutions after a first-order solve or cfmm_set_nu, the gross
 * smoothed tenders after a second-order solve, the library's own kink-loop tenders with their partial fills).  Per bucket
 * delta [k][m] | lambda [k][m] in upload order, and [m] scales behind them: 16 k m + 8 m bytes per bucket.  No tender crosses the host
 * but the kink loop's, which live there.
 *   - refusals, as cfmm_apply_trades': no prices yet -> CFMM_E_STATE; tie flags or price ties set by the caller, or a pool-sharded
 *     context -> CFMM_E_UNSUPPORTED;
 *   - a second hold replaces the first.  The held route STAYS through cfmm_update_pools*, cfmm_update_terms*, cfmm_apply_trades,
 *     cfmm_solve*, cfmm_set_nu and cfmm_set_utility, through this context or any context sharing the pools.  It goes with an upload into
 *     the context's pool store (the positions no longer mean anything: later route calls return CFMM_E_STATE), cfmm_release_route and
 *     cfmm_destroy.  cfmm_clone and cfmm_subnetwork do not carry it over;
 *   - the hold changes nothing a later call can see and counts as a reader of the pools like cfmm_get_trades*.
 * cfmm_get_held2 / N / G read the held tenders back in the shapes of cfmm_get_trades*: once the pools have moved, nothing else can.
 *
 * cfmm_requote_route.  For every pool that trades in the held route, at the CURRENT resident reserves R, fee gamma and weights /
 * parameter (in-place updates and applied trades included), the inputs stay and the outputs are scaled onto the pool's curve:
 *      x_j(s) = (R_j + gamma Delta_j) - s Lambda_j,    Lambda'_j = fl(s Lambda_j)       (every operation rounded on its own)
 * with s >= 0 the root of the pool's slack as cfmm_audit_trades defines it per class: sum_j w_j log(x_j(s) / R_j) = 0 (constant product,
 * weighted, geo-mean), phi(x(s)) = phi(R) (stableswap, power sum), and the closed form s = gamma sum Delta / sum Lambda for the
 * constant-sum kinds.  The slack is concave and strictly decreasing in s and >= 0 at s = 0: the root is unique.  With one paying leg s
 * is the exact-in swap output over the quoted output; with several the outputs keep their proportions.
 *   cap       s <= s_cap = min over legs with Lambda_j > 0 of (R_j + gamma Delta_j) / Lambda_j, rounded down so that no x_j(s_cap) is
 *             negative (constant sum) or every x_j(s_cap) stays positive (the other classes); a pool whose slack is still >= 0
 *             there -- a constant-sum leg too small to pay -- pays s_cap: pools_capped
 *   special   sum Lambda = 0: s = 1;  sum Delta = 0 with a positive Lambda: s = 0;  a pool without tenders does not trade: s = 1
 *   failed    a held tender or a reserve that is negative or not finite, a slack that is not >= 0 at s = 0: s = NaN, the pool is left
 *             out of psi and counted in pools_failed
 *   search    bracketed in [0, s_cap): a bracket lo < hi with slack(lo) >= 0 and slack(hi) < 0, both evaluated; every trial lies strictly
 *             inside it (a Newton step while it does, else the midpoint) and replaces the end of its sign.  STOPPING RULE: the search
 *             ends when lo and hi are adjacent doubles and returns lo -- an s whose own slack evaluation is >= 0, and the last double for
 *             which it is: the pool accepts what the call says it pays, and nothing is left on the table beyond the slack's rounding.
 * psi, exactly, as cfmm_audit_trades': every non-zero Lambda'_j adds +Lambda'_j and every non-zero Delta_j adds -Delta_j, each floored on
 * its own to the 96-bit fixed point floor(y 2^F) (F from the CURRENT largest reserve and smallest fee) and summed with integer atomics;
 * limbs and psi have the audit's layout and its one conversion.  Given the scales, psi is a function of (held tenders, s) alone: bitwise
 * the same on every run and for any launch geometry.
 *   pools_short / pools_long   trading pools with s < 1 - tol_scale / s > 1 + tol_scale (tol_scale <= 0: the default 1e-9)
 *   min_scale                  the smallest s over the trading pools whose root was found, with the family / kind / k / upload-order
 *                              position of the pool that holds it (ties: the first bucket in bucket order, then the lowest position;
 *                              +inf and -1s when no pool qualifies)
 *   value / infeas             from the re-quoted psi and the utility last set, as cfmm_audit's (NaN without one)
 * cfmm_get_route_scale2 / N / G return the scales of the last re-quote, [m] in upload order: 1 for pools that do not trade, NaN for failed
 * ones (CFMM_E_STATE before the first re-quote of the held route).  The re-quoted tenders are (Delta, fl(s Lambda)).
 * The call touches nothing a later call can see (no pool column, warm start of the table's search, generation, price, cached solution or
 * captured launch) and counts as a reader of the store; an in-place update through a sharer is refused meanwhile.
 * Refusals: no held route (or one an upload has outdated) -> CFMM_E_STATE; out == NULL -> CFMM_E_ARG; more than 2560 tokens (the audit's
 * tile) -> CFMM_E_LIMIT; a pool-sharded context -> CFMM_E_UNSUPPORTED. */
typedef struct {
    int64_t pools, pools_trading;         /* resident pools; those with a non-zero held tender */
    int64_t bytes;                        /* device memory the held route takes                */
} cfmm_route_info;

typedef struct {
    int64_t pools, pools_trading, pools_short, pools_long, pools_capped, pools_failed, legs_out_of_range;
    int32_t min_family, min_kind, min_k, fixed_exponent;          /* family / kind / k as in cfmm_apply_info; F of psi */
    int64_t min_pos;                                              /* upload order; -1s when no trading pool has a root */
    double  min_scale;
    double  value, infeas;                                        /* from the re-quoted psi and the utility last set   */
} cfmm_requote;

int cfmm_hold_route(cfmm_ctx *ctx, cfmm_route_info *info /* or NULL */);
int cfmm_release_route(cfmm_ctx *ctx);                            /* CFMM_OK without a held route too */
int cfmm_get_held2(cfmm_ctx *ctx, int kind, double *delta /* [2][m] or NULL */, double *lambda /* [2][m] or NULL */);
int cfmm_get_heldN(cfmm_ctx *ctx, int k, double *delta /* [k][m] or NULL */, double *lambda /* [k][m] or NULL */);
int cfmm_get_heldG(cfmm_ctx *ctx, int kind, int k, double *delta, double *lambda);
int cfmm_requote_route(cfmm_ctx *ctx, double tol_scale /* <= 0: default */, cfmm_requote *out,
                       double *psi /* [n] or NULL */, uint64_t *limbs /* [3][n] or NULL */);
int cfmm_get_route_scale2(cfmm_ctx *ctx, int kind, double *s /* [m], upload order */);
int cfmm_get_route_scaleN(cfmm_ctx *ctx, int k, double *s /* [m] */);
int cfmm_get_route_scaleG(cfmm_ctx *ctx, int kind, int k, double *s /* [m] */);
/* test and measurement hook of the re-quote's launches (tools/requote_timing.py, tests/test_gpu_requote.py), shaped like
 * cfmm_debug_audit_launch: `timed` brackets the launches with HIP events; grid > 0: workgroups per pass from then on (1 .. 2048; the
 * result does not depend on it); out2 (or NULL): {seconds of the last re-quote's launches, buckets it found stored reordered} */
int cfmm_debug_requote_launch(cfmm_ctx *ctx, int timed, int grid, double *out2);
/* Selecting pools of the route on the device (docs/subnetwork.md): every resident pool is measured by the value it takes in at the
 * context's accepted prices,
 *      v_i = sum_j nu_j Delta_ij     over the pool's legs in slot order, every product and every sum rounded on its own,
 * on exactly the tenders cfmm_get_trades2 / N / G would return at the moment of the call (the exact pool solutions after a first-order
 * solve or cfmm_set_nu, the gross smoothed tenders after a second-order solve, the tenders with their partial fills after
 * CFMM_METHOD_AUTO's own kink loop): NumPy on the read-back tenders and cfmm_get_nu's prices reproduces v_i bit for bit.  A pool is
 * selected iff v_i is finite and v_i > min_value_in (strict: 0 selects exactly the pools that take something in).  v_i is what the pool
 * receives, not its surplus nu'(Lambda - Delta): a constant-sum pool filled on its kink has no surplus and a real fill.
 *   - the selection stays with the context, one bit per pool per bucket in upload order, until the tenders it was made of go: a solve,
 *     cfmm_set_nu, new tie flags or price ties, an upload, or an in-place update or apply through any context sharing the pools.
 *     It changes nothing else a later call can see, and counts as a reader of the pools like cfmm_get_trades*;
 *   - info: counts per bucket slot and in total; value_in_total / value_in_selected are plain double sums (per workgroup, then per
 *     bucket, then over the slots, each in a fixed order: the same on every run, but not the sum NumPy forms in its own order -- compare
 *     to a relative 1e-12, not bitwise).  Pools with a non-finite v_i are counted in non_finite and enter neither sum;
 *   - refusals, as cfmm_apply_trades': no prices yet -> CFMM_E_STATE; tie flags or price ties set by the caller or a pool-sharded
 *     context -> CFMM_E_UNSUPPORTED; a NaN threshold -> CFMM_E_ARG.
 * A bucket slot: two-asset kind `kind` -> kind; the geo-mean bucket of k assets -> CFMM_POOL_KINDS2 + k; the K-asset table's bucket
 * (kind, k) -> CFMM_POOL_KINDS2 + (CFMM_MAX_POOL_SIZE + 1) * (1 + kind) + k -- the bucket order of cfmm_apply_info and cfmm_audit. */
#define CFMM_BUCKET_SLOTS 32    /* CFMM_POOL_KINDS2 + (CFMM_MAX_POOL_SIZE + 1) * (1 + CFMM_POOLK_KINDS) */
typedef struct {
    int64_t pools, selected, non_finite;
    double  value_in_total, value_in_selected;
    int64_t slot_pools[CFMM_BUCKET_SLOTS], slot_selected[CFMM_BUCKET_SLOTS];
} cfmm_select_info;

int cfmm_select_pools(cfmm_ctx *ctx, double min_value_in, cfmm_select_info *info /* or NULL */);
/* the selected pools of one bucket as ascending upload-order positions: *count receives how many the bucket has, idx the first
 * min(*count, cap) of them (idx may be NULL with cap 0: the count alone).  An empty bucket: CFMM_OK, *count = 0.  CFMM_E_STATE without a
 * selection (cfmm_select_pools first, and nothing since that dropped it); count == NULL, cap < 0, a kind or k without a bucket -> CFMM_E_ARG */
int cfmm_get_selected2(cfmm_ctx *ctx, int kind, int32_t *idx, int64_t cap, int64_t *count);
int cfmm_get_selectedN(cfmm_ctx *ctx, int k, int32_t *idx, int64_t cap, int64_t *count);
int cfmm_get_selectedG(cfmm_ctx *ctx, int kind, int k, int32_t *idx, int64_t cap, int64_t *count);
/* A sub-network on the device (docs/subnetwork.md): a NEW context on src's device, with src's n_tokens (token ids are unchanged, so prices
 * and utilities carry over one to one) and a pool store of its OWN, whose buckets hold the chosen pools of src in ascending upload order.
 * Every column is gathered device to device from src's resident columns as they are NOW (in-place updates and applied trades included):
 * no pool column crosses the host.  The new context is bit for bit the one a caller would get by uploading the same pools' current
 * values: the same columns, the derived columns, every bucket's largest reserve and smallest fee reduced on the device, the token-block
 * ordering left pending exactly where a fresh upload of that many pools would have it, the host copy of a small constant-sum bucket.
 *   lists       per bucket slot (see cfmm_select_info) `count` upload-order positions, strictly ascending and in range; a slot with
 *               count 0 takes no pool of that bucket.  Checked on the host before anything is allocated: a list that breaks the rule,
 *               or names a bucket src does not hold -> CFMM_E_ARG, *out stays NULL and nothing is created.  NULL: src's current
 *               selection (cfmm_select_pools; CFMM_E_STATE without one).  An empty choice gives a context with no pools.
 *   carried     src's utility (as last set), its accepted prices (cfmm_solve(sub, NULL, ..) then starts warm from them) and the
 *               reproducible mode.  NOT carried: tie flags, price ties, the solution and anything derived from it.
 * Afterwards the two contexts are independent: either may be destroyed, updates through one do not reach the other.  The call reads
 * src's pools like cfmm_get_trades* and changes nothing of src a later call can see; CFMM_E_STATE while another context sharing src's
 * pools is inside a solve, evaluation or read-back.  An in-place update or apply through a sharer holds the store's lock from its
 * first check to its last write, so a call that meets one WAITS for it (it is not refused) and gathers the updated pools.  A
 * pool-sharded src -> CFMM_E_UNSUPPORTED.
 * Bit for bit: the columns, the derived columns, the extrema, the reproducible mode's results, and every tender of a sub-bucket that
 * keeps the caller's order.  A sub-bucket large enough for the token-block ordering (16 384 two-asset, 65 536 geo-mean pools) is stored
 * in an order atomics settle, which differs between any two uploads of the same pools; the one tender that depends on a pool's wave
 * neighbours -- CFMM_POOL_W2's, through a wave-uniform choice of series -- then agrees to 1e-14 of the reserve, as between two uploads. */
typedef struct {
    const int32_t *pos[CFMM_BUCKET_SLOTS];    /* [count] each, or NULL with count 0 */
    int64_t count[CFMM_BUCKET_SLOTS];
} cfmm_pool_lists;
int cfmm_subnetwork(cfmm_ctx *src, const cfmm_pool_lists *lists /* or NULL */, cfmm_ctx **out);
/* The prices the resident pools imply (docs/pool_prices.md).  Every pool contributes relations  log p_u - log p_v = lr  at its CURRENT
 * resident reserves, fees and weights: a two-asset pool one, (ia, ib); a k-asset pool k - 1, leg j against leg 0.  lr is the pool's
 * marginal log-price ratio at zero trade: log(Rb / Ra) (constant product), log(wa Rb / ((1 - wa) Ra)) (weighted), 0 (constant sum, two
 * assets or k), t log(Rb / Ra) (power sum), log((1 + alpha / (Ra Ra Rb)) / (1 + alpha / (Ra Rb Rb))) (two-asset stableswap),
 * log(w_j R_0 / (w_0 R_j)) (geo-mean), log1p(s / R_j) - log1p(s / R_0) with s = alpha / prod R (k-asset stableswap).  Every pool
 * counts, with unit weight, tie flags or not (flags describe a solve, not the reserves).
 *   phi       minimises sum (phi_u - phi_v - lr)^2: L phi = rhs on the multigraph Laplacian, zero mean on every connected component
 *             of the token graph; a token no pool lists is a component of its own with phi = 0.  Solved on the device by
 *             Jacobi-preconditioned conjugate gradients from zero, stopped at max |r| <= 1e-12 max |rhs| or after 4 n + 100 iterations
 *             (status 1; the prices are still returned).
 *   anchor    anchor[j] > 0 and finite: the price of token j is known; 0 (or anchor == NULL): unknown.  On a component with anchored
 *             tokens log p = phi + off, off the mean of log anchor - phi over its anchored tokens summed in token order, and anchored
 *             tokens are returned bit for bit as given; a component without one returns exp(phi) (geometric-mean price 1).
 *   prices    [n], required.  log_potential: the gauged phi.  component: labels 0.., numbered by each component's first token.
 * Needs uploaded pools only -- no utility, no prices, no solve; a context without pools is served (every token its own component).
 * The call reads the pools like cfmm_get_trades* and changes nothing a later call can see: no pool column, no warm start of the table's
 * root search, no generation, no accepted prices, no cached solution, no barrier warm start, no Cholesky factor, no captured launch;
 * its scratch is its own (grow-only, made at the first call, freed by cfmm_destroy).  An in-place update through a context sharing the
 * pools is refused meanwhile; a call made after an update sees the updated pools.  One synchronisation, one staged copy back.
 * Refusals: prices == NULL, or an anchor entry that is negative, NaN or infinite -> CFMM_E_ARG; a pool-sharded context ->
 * CFMM_E_UNSUPPORTED; more than 6144 tokens (the workgroup's tile of the direction vector) or 2^32 relations -> CFMM_E_LIMIT. */
typedef struct {
    int64_t relations;            /* 1 per two-asset pool, k - 1 per k-asset pool */
    int32_t components;           /* unlisted tokens count one each */
    int32_t components_anchored;
    int32_t tokens_unlisted;
    int32_t iterations;           /* of the iterative solve (0 if direct) */
    int32_t status;               /* 0 converged; 1 iteration cap reached */
    double residual;              /* max |L phi - rhs| / max |rhs| at return (the iteration's own residual); 0 when rhs == 0 */
    double misfit_max, misfit_ss; /* max and sum of squares of phi_u - phi_v - lr over all relations */
} cfmm_prices_info;

int cfmm_pool_prices(cfmm_ctx *ctx, const double *anchor /* [n] or NULL */,
                     double *prices /* [n] */,
                     double *log_potential /* [n] or NULL */,
                     int32_t *component /* [n] or NULL: labels 0.., numbered by first token */,
                     cfmm_prices_info *info /* or NULL */);
/* measurement hook of the call's launches (tools/prices_timing.py), not part of the product's interface: with `timed`, every
 * cfmm_pool_prices brackets its phases with HIP events; out5 (or NULL) receives the seconds of the last timed call's {clear, relation
 * pass, components, iteration, misfit pass} */
int cfmm_debug_prices_launch(cfmm_ctx *ctx, int timed, double *out5);
/* constant-sum pools sitting on their kink are `tied` (flag 1): they are skipped by the
 * kernels and their fill fraction is assigned by the host's primal recovery */
int cfmm_set_pool_flags(cfmm_ctx *ctx, int kind, const int32_t *flags /* [m] or NULL */);
/* the same for the K-asset table's constant-sum bucket of k tokens, per LEG (slot-major [k][m] like the bucket's columns, or NULL):
 * a flagged leg j of a pool sits on the kink gamma nu_j = nu_cheapest (arbitrage.py:73-74 over more than two tokens: that token is
 * partially drained at the optimum); it is left out of the evaluation and the tenders, the caller ties the two prices
 * (cfmm_set_ties) and adds the partial fill theta R_j itself */
int cfmm_set_pool_flagsG(cfmm_ctx *ctx, int k, const int32_t *flags);

/* utility: replaces obj + the psi constraints (arbitrage.py:57,77; liquidation.py:57,77-80;
 * two-asset.py:66,86).  ctype NULL = all CFMM_GE, h NULL = 0. */
int cfmm_set_utility(cfmm_ctx *ctx, const double *c, const double *h, const int32_t *ctype);
/* price ties: log nu_j = s[grp[j]] + off[j]; NULL, NULL = none */
int cfmm_set_ties(cfmm_ctx *ctx, int n_groups, const int32_t *grp, const double *off);

/* one dual evaluation = every pool's subproblem once + the reduction:  psi(nu), sum_i arb_i,
 * optionally the diagonal metric.  This is the unit BASELINE.json's metric counts. */
int cfmm_eval_dual(cfmm_ctx *ctx, const double *nu, double *arb_sum, double *psi, double *diag /* or NULL */);

/* the barrier-smoothed evaluation behind CFMM_METHOD_NEWTON: every direction of every two-asset pool solves
 *      max_{D > 0}  nu_out L(D) - nu_in D + mu log D        (constant sum: + mu log(R_out/gamma - D))
 * (k-asset geo-mean pools enter unsmoothed, with their exact solution and generalised Hessian);
 * value = sum of those optima, trade = sum nu'(L - D), psi[n] = sum A_i (L - D), and -- if H is not NULL -- the
 * n x n Hessian of `value` in log-prices minus its diag(nu * psi) term, column-major, LOWER triangle only. */
int cfmm_eval_smooth(cfmm_ctx *ctx, const double *nu, double mu, double *value, double *trade, double *psi, double *H);

/* test hook: the dense Cholesky solve of the second-order method on a caller-supplied SPD system (A: n x n
 * column-major, ONLY the lower triangle read: what lies above may be zero, the mirror image or anything else; n must
 * equal the context's token count).  *info = 0, or non-zero: A is not positive definite (a pivot <= 0, NaN or +inf met);
 * the value is not a position (everything behind a failed pivot is NaN and flags too), and x is then meaningless.  A
 * failed call leaves the context fit for the next one. */
int cfmm_debug_cholesky(cfmm_ctx *ctx, int n, const double *A, const double *b, double *x, int32_t *info);
/* test hook: x = A^-1 b for a NEW right-hand side through the factor and inverse factor the last cfmm_debug_cholesky left
 * (the two matrix-vector products of the second-order iteration's chord steps) */
int cfmm_debug_cholesky_apply(cfmm_ctx *ctx, int n, const double *b, double *x);

/* Reproducible mode.  By default psi is scatter-added with fp64 atomics, whose order -- lanes, waves, workgroups -- varies
 * from run to run: psi, and with it the path of a solve, is reproducible to rounding only.  With `on` != 0 every pool's
 * contribution y is floored to the 96-bit fixed-point integer floor(y * 2^F) -- exactly, for tendered (negative) and received
 * amounts alike; F is chosen from the largest reserve and the smallest fee so that |y * 2^F| < 2^84, and only the fraction
 * below 2^-F is dropped -- and accumulated with integer atomics (associative: any order gives the same bits),
 * all-reduced as integers when pool-sharded, and converted back in a fixed order:
 * psi, the iterates and the evaluation count are then BITWISE identical from run to run and for any number of pool
 * shards / GPUs.  Cost, measured (DESIGN.md "Reproducible mode"): the evaluation kernel +20..30 % (three LDS atomics per leg
 * instead of one: 20.1 against 16.6 us at 1e6 mixed pools), the outer iteration +24..30 % (one small extra launch per
 * evaluation).  First-order path and cfmm_eval_dual; needs <= ~2600 tokens; fees >= 1e-3.  Also: CFMM_DETERMINISTIC=1. */
int cfmm_set_deterministic(cfmm_ctx *ctx, int on);
/* test hook of the reproducible mode: one dual evaluation returning the RAW integer limbs of psi ([3][n], limb-major, value =
 * (limb2 2^64 + limb1 2^32 + limb0) / 2^F, limb2 a wrapped signed 64-bit sum, limb0 and limb1 sums of values in [0, 2^32)) with
 * the fixed-point exponent F derived from (ref_reserve, ref_fee) instead of this context's own largest reserve / smallest fee
 * -- so that the limbs of the S shards of a network, added as integers on the host, can be compared bit for bit with the
 * unsharded network's. */
int cfmm_debug_eval_limbs(cfmm_ctx *ctx, const double *nu, double ref_reserve, double ref_fee, uint64_t *limbs);
/* test hook of the reproducible mode: the device's fixed-point split alone.  Contribution y[i] is added to token tok[i]
 * (0 <= tok[i] < the context's token count, i < count) exactly as an evaluation adds a pool's, into a zeroed [3][n] limb
 * array (layout as above) with the exponent F cfmm_debug_eval_limbs derives from the same (ref_reserve, ref_fee); every
 * |y[i] * 2^F| must be below 2^95.  limbs[.][j] is then the sum over tok[i] == j of the limbs of floor(y[i] * 2^F). */
int cfmm_debug_scatter_limbs(cfmm_ctx *ctx, int64_t count, const int32_t *tok, const double *y,
                             double ref_reserve, double ref_fee, uint64_t *limbs /* [3][n] */);

/* prob.solve(): nu0 = start prices.  NULL: continue from cfmm_set_nu / the previous solution -- after a second-order
 * solve that includes (a multiple of) its final barrier weight: the warm start of a parametric sweep (two-asset.py:34-100).
 * Constant-sum pools (arbitrage.py:12,20,28,72-74) can end PARTIALLY filled -- a kink of the dual that prices alone do not resolve.
 * With CFMM_METHOD_AUTO on a network of the reference's size (what cfmm_solve_sweep serves; linear-box utility, one GPU, no ties set by
 * the caller) the library runs the active-set loop over such kinks itself (round 6): stats.primal_value, cfmm_get_psi / _solution and
 * cfmm_get_trades2 return the point WITH the fills (arbitrage.py's pool 4: 38.6 %), stats.method = CFMM_METHOD_LBFGS.  Elsewhere AUTO
 * falls back on the second-order method, which needs no active set; an explicit CFMM_METHOD_LBFGS leaves the kinks to the caller
 * (cfmm_set_ties, cfmm_set_pool_flags: what cfmm/problem.py does for networks of any size). */
int cfmm_solve(cfmm_ctx *ctx, const double *nu0, const cfmm_opts *opts, cfmm_stats *out);

/* `nb` prob.solve() calls over the SAME pools in lock-step: the loop body of the parametric sweep, two-asset.py:34-100
 * (the pools, reserves and fees of lines 7-32 stay, only the utility of line 66 / 86 changes with t), or independent
 * baskets over one pool set.  ctxs[0] is the context the pools were uploaded to, ctxs[1..] its cfmm_clone()s, each with
 * its own cfmm_set_utility; nu0[b] (or nu0 itself) may be NULL = continue from that context's prices.  Every outer
 * iteration reads every pool column ONCE and solves each pool at all nb price vectors (first-order method; no price
 * ties or tie flags, linear-plus-box utilities, not pool-sharded, not reproducible); out[b] are the statistics of solve b
 * (wall / device seconds: of the whole batch).  nb <= cfmm_batch_capacity(n_tokens) (8 up to ~1100 tokens; bounded by the
 * LDS tile beyond).  Every pool family rides along: the stableswap / power-sum two-asset buckets and the K-asset table's
 * buckets through batched launches of their own behind the main one.  Constant-sum pools, two-asset or of the table, are
 * evaluated at their LP vertex: an optimum on one of their kinks is left to the caller (cfmm_set_ties, cfmm_solve).  The
 * table's stableswap search warm-starts from a slab of the batch's own, cleared at every call: a call's result is a function
 * of its inputs alone.
 * Afterwards every context is read back as after cfmm_solve (cfmm_get_solution, cfmm_get_trades*). */
int cfmm_solve_batch(cfmm_ctx *const *ctxs, int nb, const double *const *nu0, const cfmm_opts *opts, cfmm_stats *out);
/* one dual evaluation at nb price vectors in ONE pass over the pools (what cfmm_solve_batch iterates on):
 * ctxs as for cfmm_solve_batch; nu[b]: [n]; arb_sum[nb]; psi[b]: [n].  No metric.  Refusals: those of cfmm_solve_batch that
 * concern the pools and the mode (ties, sharded, reproducible); needs no utility.  The prices become every context's point, as
 * after cfmm_set_nu. */
int cfmm_eval_dual_batch(cfmm_ctx *const *ctxs, int nb, const double *const *nu, double *arb_sum, double *const *psi);
int cfmm_batch_capacity(int n_tokens);

/* The reference's OWN sweep as one call: two-asset.py:34-100 solves the same 5-pool network (constant-sum pool included,
 * two-asset.py:7-32) under 50 utilities (current_assets = [t, 0, 0], :41-45; psi + current_assets >= 0, :86) and reads value,
 * psi and every pool's tenders at each (:93-100).  B utilities over ONE tiny network -- what one workgroup evaluates: <= 64 tokens,
 * <= 64 wave-tiles, no stableswap / generic / K-asset table pools, one GPU -- are solved in lock-step: a round is ONE launch with
 * one workgroup per unfinished point (the whole first-order solve of a point inside its workgroup), and the active-set loop over the
 * kinks of the constant-sum pools (arbitrage.py:73-74: tie the two prices of a pool found on its kink, re-solve, recover the fill
 * fraction, release ties whose fill leaves (0, 1)) runs inside the library between the rounds.
 *   c, h, ctype, nu0        [B][n]: utility (cfmm_set_utility's arrays; h / ctype may be NULL = 0 / CFMM_GE) and start prices per point
 *   m_sum, sum_*            the constant-sum bucket's columns as uploaded (the host half of the loop reads them); m_sum = 0: none
 *   kink_tol, max_rounds    <= 0: the defaults (1e-3, 6)
 *   nu, psi                 [B][n]: accepted prices and the DEVICE's net trade there (tied pools excluded)
 *   theta, tsgn             [B][m_sum]: fill fraction in (0, 1) and kink direction (+1: tender the first token, drain the second; -1:
 *                           the reverse) of every pool that ended tied on its kink, NaN / 0 elsewhere: psi_total = psi + sum theta d
 *   trades                  NULL, or [B][T]: per point, for every non-empty bucket in the order two-asset kinds 0.., then sizes 3..8,
 *                           delta [k][m] then lambda [k][m] (tied pools: zeros -- their tenders are theta x their full fill)
 *   out, rounds             [B] statistics (evals / iters summed over the rounds; wall / device seconds: of the whole sweep), rounds per point.
 *                           primal_value / dual_value / infeas of a point with tied pools are those of the point WITHOUT the tied pools' fills
 *                           (psi likewise): the caller adds theta x the full fill of each -- the objective is then c'psi */
int cfmm_solve_sweep(cfmm_ctx *ctx, int B, const double *c, const double *h, const int32_t *ctype, const double *nu0,
                     int64_t m_sum, const int32_t *sum_ia, const int32_t *sum_ib, const double *sum_fee, const double *sum_Ra, const double *sum_Rb,
                     const cfmm_opts *opts, double kink_tol, int max_rounds,
                     double *nu, double *psi, double *theta, int32_t *tsgn, double *trades, cfmm_stats *out, int32_t *rounds);

/* read-back (arbitrage.py:84 prob.value is stats.primal_value; psi.value; deltas/lambdas.value) */
int cfmm_get_nu(cfmm_ctx *ctx, double *nu);
int cfmm_set_nu(cfmm_ctx *ctx, const double *nu);
int cfmm_get_psi(cfmm_ctx *ctx, double *psi);
int cfmm_get_solution(cfmm_ctx *ctx, double *nu, double *psi);     /* both with one synchronisation; either may be NULL */
/* tenders at the accepted prices; slot-major [2][m] / [k][m]; either pointer may be NULL */
int cfmm_get_trades2(cfmm_ctx *ctx, int kind, double *delta, double *lambda);
int cfmm_get_tradesN(cfmm_ctx *ctx, int k, double *delta, double *lambda);
int cfmm_get_tradesG(cfmm_ctx *ctx, int kind, int k, double *delta, double *lambda);      /* K-asset table buckets, [k][m] */

/* pool-sharding over the GPUs of a node: one process per GPU, one RCCL all-reduce of
 * [psi | sum arb] per dual evaluation.  `uid` is the 128-byte ncclUniqueId made by rank 0. */
int cfmm_comm_unique_id(void *uid128);
int cfmm_comm_init(cfmm_ctx *ctx, int n_ranks, int rank, const void *uid128);
/* (cfmm_update_pools* on a pool-sharded context: positions local to the rank's shard, and every rank makes the call -- count = 0 where
 *  it has nothing to update -- so that the global maxima are re-reduced in step at the next solve) */

/* One-shot all-reduce over the xGMI mesh for the iteration's 8-50 KB messages (csrc/oneshot.hpp): every rank stores its
 * vector straight into a mailbox in each peer's HBM, one hop instead of a ring's 2 (R - 1); reduced in rank order, so every
 * rank holds the same bits.  RCCL (cfmm_comm_init) stays the default and carries whatever does not fit a mailbox.
 *   cfmm_oneshot_export: allocates this rank's mailbox, returns its 64-byte hipIpcMemHandle_t;
 *   cfmm_oneshot_import: all ranks' handles ([n_ranks][64], own entry ignored) -> the collectives above use the mailboxes;
 *   cfmm_oneshot_attach / cfmm_oneshot_mailbox: the same with raw device pointers, for ranks living in ONE process
 *     (several contexts on one GPU: how the exchange is tested where a second GPU is not available). */
int cfmm_oneshot_export(cfmm_ctx *ctx, void *handle64);
int cfmm_oneshot_import(cfmm_ctx *ctx, int n_ranks, int rank, const void *handles);
int cfmm_oneshot_attach(cfmm_ctx *ctx, int n_ranks, int rank, void *const *mailboxes);
/* with mailboxes attached AND an RCCL communicator: route the collectives through the one-shot exchange (1) or back through
 * RCCL (0).  Must be called with the same value on every rank (the one-shot epochs advance only while it is on).  Used by
 * cfmm.distributed's start-up check, which compares the two paths on the real peers before trusting the one-shot one. */
int cfmm_oneshot_enable(cfmm_ctx *ctx, int on);
void *cfmm_oneshot_mailbox(cfmm_ctx *ctx);

/* measurement hooks (bench.py): time `reps` back-to-back launches of the fused evaluation kernel
 * with HIP events on the library's stream, over every bucket (kind = CFMM_TIME_ALL: exactly the
 * launch one dual evaluation makes) or restricted to one bucket (kind = CFMM_POOL_*, or -k for
 * the k-asset bucket); returns the average seconds per launch in *sec_per_launch. */
#define CFMM_TIME_ALL 100
#define CFMM_TIME_TABLE 200      /* the K-asset table's own launch alone (every table bucket: table_eval_kernel) */
int cfmm_time_eval_kernel(cfmm_ctx *ctx, int kind, int reps, double *sec_per_launch);
/* the two pool-sharded pieces of an outer iteration, timed the same way (bench.py's per-iteration split): `reps`
 * back-to-back launches of the accumulator-slice fold, and `reps` back-to-back RCCL all-reduces of [psi | sum arb]
 * (n + 1 doubles) -- the latter only on a context with a communicator, and then EVERY rank must make this call */
int cfmm_time_collective(cfmm_ctx *ctx, int reps, double *fold_sec, double *allreduce_sec);
/* measurement: what it costs to hand `np` doubles from ONE workgroup per XCD to the other workgroups of that XCD through its L2 (store,
   acknowledge, flag, spin, load into LDS) -- the price of running iter_kernel's update once per XCD instead of once per workgroup
   (DESIGN (d) "tried and rejected").  out7: median, max over `reps` launches of the slowest follower's [data ready -> data in LDS] in us;
   median [ready -> flag seen]; workgroups whose XCC id is not blockIdx % 8; followers that failed; XCDs without a publisher; the XCC
   ids of workgroups 0 .. 7 as eight decimal digits.
   No reference counterpart (arbitrage.py:82 is one cvxpy call). */
int cfmm_time_xcd_handoff(cfmm_ctx *ctx, int np, int reps, double *out7);
/* the kernels of one second-order step (bench.py --config C5), each timed over `reps` launches at the current prices and
 * barrier weight mu: out4 = seconds per {smoothed evaluation with Hessian assembly, smoothed evaluation alone, dense
 * factorisation (all its launches), back substitution} */
/* NOTE: the hook overwrites the Hessian, the pin mask and the warm starts of the smoothed per-direction solves; a following
 * cfmm_solve(nu0 = NULL) therefore starts its barrier path afresh instead of continuing the previous one */
int cfmm_time_newton_kernels(cfmm_ctx *ctx, double mu, int reps, double *out4);
/* Shader-clock probe (bench.py: roofline.effective_clock_ghz_live).  MI355X clocks to its power budget, so a launch duration alone
 * cannot tell a slower binary from a slower clock.  cfmm_clock_probe_start puts ONE sleeping wave on a stream of its own that, every
 * `period_us`, stores {shader cycles (s_memtime), ticks of the constant 100 MHz counter (s_memrealtime)} into mapped pinned memory
 * until cfmm_clock_probe_stop, `max_ms`, or 8192 samples -- while whatever the caller enqueues on the library's stream runs beside
 * it.  cfmm_clock_probe_read copies the samples so far (no synchronisation; out[2 i] cycles, out[2 i + 1] ticks, oldest first);
 * the clock over an interval = (delta cycles) / (delta ticks x 10 ns).  Replaces nothing in the reference (a measurement hook). */
int cfmm_clock_probe_start(cfmm_ctx *ctx, double period_us, double max_ms);
int cfmm_clock_probe_read(cfmm_ctx *ctx, int64_t *out, int cap, int *count);
int cfmm_clock_probe_stop(cfmm_ctx *ctx, int64_t *out, int cap, int *count);
/* the chain of dependent v_fma_f64 the probe runs in front of its first sample: out3 = {shader cycles, 100 MHz ticks, links} -- cycles per
 * link is a pipeline constant, which shows that the first counter counts shader cycles */
int cfmm_clock_probe_chain(cfmm_ctx *ctx, int64_t *out3);
/* checks the cross-lane primitives of the update kernels (DPP / v_permlane*_swap / ds_swizzle butterflies and the
 * 64-value reduce-scatter) against exact integer sums on this device; 0 = pass */
int cfmm_selftest(cfmm_ctx *ctx);
/* kernel-tuning hook: 32 {shader-cycle, 100 MHz wall-clock} stamp pairs written by the last
 * evaluation / update kernels of a build made with -DCFMM_PHASE_TIMERS (zeros otherwise), then a
 * per-wave tile log and per-block start/end clocks of the last evaluation; `out` holds
 * 64 + 8 * 4096 + 2048 int64 */
int cfmm_debug_timers(cfmm_ctx *ctx, int64_t *out);
#ifdef CFMM_SMOOTH_HIST        /* tuning builds only (tools/build_variants.sh): iteration histogram of the smoothed per-direction solves */
int cfmm_debug_smooth_hist(cfmm_ctx *ctx, uint64_t *out128, int reset);
int cfmm_debug_smooth_samples(cfmm_ctx *ctx, double *out768);
#endif
int64_t cfmm_pool_count(cfmm_ctx *ctx);
/* measurement hook: bytes of pool columns one dual evaluation loads AS STORED (behind the first evaluation / solve: large
 * two-asset buckets then carry a compact mirror of their ids and fee, 21 B per constant-product pool instead of the 32 B
 * SURVEY 8(d) counts) */
int64_t cfmm_eval_bytes(cfmm_ctx *ctx);
void *cfmm_stream(cfmm_ctx *ctx);                 /* the hipStream_t the library launches on */

#ifdef __cplusplus
}
#endif
#endif
