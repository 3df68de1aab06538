"""The exact reference of the pool-price fit (docs/pool_prices.md) and the instances its tests share.

reference(net) builds the instance's multigraph Laplacian L (integers) and right-hand side (the twin's fp64 lr as they stand, summed at
50 digits) in NumPy and solves L phi = rhs EXACTLY: per connected component the first token is grounded, the grounded system is solved by
iterative refinement whose residuals and iterates are mpmath numbers at 50 digits (the float factor only preconditions it; the loop runs
until the 50-digit residual is below 1e-40 of the right-hand side), then the mean is taken off.  No float pinv enters phi.

The tolerance is derived per instance:
    tol = |L+|_inf (1e-12 max|rhs| + 8 eps max_j(deg_j sum_{relations at j} |lr|))
the first term the iteration's stopping rule, the second the rounding of the logs and of the unordered sums.  |L+|_inf comes from a float
inverse of L + sum_c 1_c 1_c' / n_c (a magnitude, not a solution).  The NumPy twin is held to the first term alone."""
import functools

import mpmath
import numpy as np

from cfmm import synthetic
from cfmm.problem import pack, pool_relations

EPS = float(np.finfo(np.float64).eps)

# the 11-pool, 6-token network with one pool of every kind and size (tests/test_subset_host.py)
IDX = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, 1, 2], [1, 2, 3, 4], [2, 3, 4], [0, 2, 4, 5], [1, 5], [0, 5]]
RES = [[10, 20], [30, 40], [5, 6], [7, 8], [9, 11], [1, 2, 3], [4, 5, 6, 7], [8, 9, 10], [11, 12, 13, 14], [3, 4], [6, 7]]
KINDS = ["geomean", "geomean", "sum", "curve", "powersum", "geomean", "geomean", "curve", "sum", "geomean", "geomean"]
WEIGHTS = [None, [0.3, 0.7], None, None, None, None, [1, 2, 3, 4], None, None, None, [0.8, 0.2]]
PARAMS = [None, None, None, 50.0, 0.4, None, None, 20.0, None, None, None]
FEES = [0.997, 0.99, 0.999, 0.9996, 0.995, 0.997, 0.998, 0.9994, 0.9999, 0.9970, 0.98]


def every_kind():
    return pack(6, IDX, RES, FEES, KINDS, WEIGHTS, PARAMS)[0]


def pools_network(n, idx, res, kinds=None, weights=None, params=None, fee=0.997):
    m = len(idx)
    return pack(n, idx, res, [fee] * m, kinds or ["geomean"] * m, weights or [None] * m, params or [None] * m)[0]


def chain(n):
    """n tokens in a line of constant-product pools: the worst conditioning a connected graph of n tokens has"""
    rng = np.random.default_rng(n)
    return pools_network(n, [[j, j + 1] for j in range(n - 1)], [list(rng.uniform(50.0, 150.0, 2)) for _ in range(n - 1)])


def three_components():
    """9 tokens: {0, 1, 2, 3} (a cycle whose pools disagree), {4, 5} (two-asset stableswap and constant sum), {6, 7} (a 3-asset pool
    would not fit: one weighted pool), and token 8 that no pool lists"""
    idx = [[0, 1], [1, 2], [2, 3], [3, 0], [0, 2], [4, 5], [5, 4], [6, 7]]
    res = [[10, 21], [30, 41], [50, 66], [70, 12], [5, 9], [100, 120], [80, 90], [3, 14]]
    kinds = ["geomean"] * 5 + ["curve", "sum", "geomean"]
    weights = [None] * 7 + [[0.25, 0.75]]
    params = [None] * 5 + [4.0e5, None, None]
    return pools_network(9, idx, res, kinds, weights, params)


def single_family(family, m, n, seed=0):
    """m pools of one family over n tokens (n >= 2; pools of k assets take min(k, n) ... the families of more than two assets need n >= k)"""
    rng = np.random.default_rng(1000 * m + n + seed)
    k = {"cp2": 2, "w2": 2, "sum2": 2, "curve2": 2, "pow2": 2, "gn8": 8, "gn3": 3, "stable3": 3, "sumk4": 4}[family]
    idx = [list(rng.choice(n, size=k, replace=False)) for _ in range(m)]
    res = [list(rng.uniform(10.0, 1000.0, k)) for _ in range(m)]
    kind = {"cp2": "geomean", "w2": "geomean", "sum2": "sum", "curve2": "curve", "pow2": "powersum", "gn8": "geomean", "gn3": "geomean",
            "stable3": "curve", "sumk4": "sum"}[family]
    weights = [list(rng.uniform(0.2, 0.8, 1)) for _ in range(m)] if family == "w2" else [None] * m
    weights = [[w[0], 1.0 - w[0]] for w in weights] if family == "w2" else weights
    if family in ("gn8", "gn3"):
        weights = [list(rng.uniform(0.5, 2.0, k)) for _ in range(m)]
    params = [None] * m
    if kind == "curve":
        params = [float(np.prod(r) * np.mean(r) * rng.uniform(0.5, 2.0)) for r in res]
    if kind == "powersum":
        params = [float(rng.uniform(0.1, 0.9)) for _ in range(m)]
    return pools_network(n, idx, res, [kind] * m, weights, params)


def mixed(n, m, zipf=None, seed=0):
    """about m pools of all families over n tokens; zipf: token popularity ~ rank^-zipf (one token then has thousands of relations)"""
    rng = np.random.default_rng(seed + n + m)
    p = None
    if zipf is not None:
        p = 1.0 / np.arange(1, n + 1) ** zipf
        p /= p.sum()
    fams = [("geomean", 2), ("w", 2), ("sum", 2), ("curve", 2), ("powersum", 2), ("geomean", 3), ("geomean", 5), ("geomean", 8), ("curve", 3), ("sum", 4)]
    share = np.array([30, 15, 5, 10, 10, 8, 6, 4, 7, 5], dtype=float)
    pick = rng.choice(len(fams), size=m, p=share / share.sum())
    idx, res, kinds, weights, params = [], [], [], [], []
    for f in pick:
        kind, k = fams[f]
        ids = list(rng.choice(n, size=k, replace=False, p=p))
        r = list(rng.uniform(10.0, 1000.0, k))
        idx.append(ids); res.append(r)
        if kind == "w":
            w = float(rng.uniform(0.2, 0.8))
            kinds.append("geomean"); weights.append([w, 1.0 - w]); params.append(None)
        elif kind == "geomean":
            kinds.append("geomean"); weights.append(list(rng.uniform(0.5, 2.0, k)) if k > 2 else None); params.append(None)
        elif kind == "curve":
            kinds.append("curve"); weights.append(None); params.append(float(np.prod(r) * np.mean(r) * rng.uniform(0.5, 2.0)))
        elif kind == "powersum":
            kinds.append("powersum"); weights.append(None); params.append(float(rng.uniform(0.1, 0.9)))
        else:
            kinds.append("sum"); weights.append(None); params.append(None)
    return pack(n, idx, res, [0.997] * m, kinds, weights, params)[0]


def shipped(name):
    """the reference project's shipped instances (oracle/instances.py) as packed networks"""
    from oracle import instances as I
    inst = {"arbitrage": I.arbitrage, "liquidation": I.liquidation, "two_asset": lambda: I.two_asset(0.0)}[name]()
    return pack(inst["n_tokens"], inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], inst["weights"])[0]


INSTANCES = {
    "every_kind": every_kind,
    "three_components": three_components,
    "chain65": lambda: chain(65),
    "chain257": lambda: chain(257),
    "arbitrage": lambda: shipped("arbitrage"),
    "liquidation": lambda: shipped("liquidation"),
    "two_asset": lambda: shipped("two_asset"),
    "c3_small": lambda: synthetic.config("C3", scale=0.002),
    "zipf300": lambda: mixed(300, 3000, zipf=1.1),
    "sparse1000": lambda: mixed(1000, 5000),
    "sparse2049": lambda: mixed(2049, 5000),
}


@functools.lru_cache(maxsize=None)
def instance(name):
    return INSTANCES[name]()


def components(n, eu, ev):
    """labels 0.., numbered by each component's first token"""
    label = np.arange(n)
    while len(eu):
        new = label.copy()
        np.minimum.at(new, eu, label[ev])
        np.minimum.at(new, ev, label[eu])
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    return np.unique(label, return_inverse=True)[1]


def reference(net):
    """dict(phi, comp, L, rhs, deg, tol, tol_stop, misfit_max, misfit_ss, misfit_l1, relations): the exact fit of `net` and its bounds"""
    mpmath.mp.dps = 50
    n = int(net["n_tokens"])
    eu, ev, lr = pool_relations(net)
    comp = components(n, eu, ev)
    L = np.zeros((n, n), dtype=np.int64)
    np.add.at(L, (eu, eu), 1); np.add.at(L, (ev, ev), 1)
    np.add.at(L, (eu, ev), -1); np.add.at(L, (ev, eu), -1)
    deg = np.bincount(eu, minlength=n) + np.bincount(ev, minlength=n)
    rhs = [mpmath.mpf(0)] * n
    for u, v, x in zip(eu.tolist(), ev.tolist(), lr.tolist()):
        rhs[u] = rhs[u] + mpmath.mpf(x)
        rhs[v] = rhs[v] - mpmath.mpf(x)
    phi = [mpmath.mpf(0)] * n
    for c in range(int(comp.max()) + 1 if n else 0):
        tok = np.flatnonzero(comp == c)
        if len(tok) < 2:
            continue
        g = tok[1:]                                            # grounded at the component's first token
        A = L[np.ix_(g, g)]
        Ainv = np.linalg.inv(A.astype(np.float64))
        rows, cols = np.nonzero(A)
        vals = A[rows, cols].tolist()
        rows, cols = rows.tolist(), cols.tolist()
        b = [rhs[j] for j in g.tolist()]
        bmax = max(abs(x) for x in b)
        x = [mpmath.mpf(0)] * len(g)
        for _ in range(40):
            r = list(b)
            for i, j, a in zip(rows, cols, vals):
                r[i] = r[i] - a * x[j]
            if max(abs(t) for t in r) <= mpmath.mpf(10) ** -40 * bmax:
                break
            d = Ainv @ np.array([float(t) for t in r])
            x = [xi + mpmath.mpf(float(di)) for xi, di in zip(x, d)]
        else:
            raise AssertionError("the refinement of the exact reference did not converge")
        full = [mpmath.mpf(0)] + x
        mean = sum(full) / len(full)
        for j, t in zip(tok.tolist(), full):
            phi[j] = t - mean
    mis = [phi[u] - phi[v] - mpmath.mpf(x) for u, v, x in zip(eu.tolist(), ev.tolist(), lr.tolist())]
    # |L+|_inf: L+ = (L + sum_c 1_c 1_c' / n_c)^-1 - sum_c 1_c 1_c' / n_c
    P = np.zeros((n, n))
    for c in range(int(comp.max()) + 1 if n else 0):
        tok = np.flatnonzero(comp == c)
        P[np.ix_(tok, tok)] = 1.0 / len(tok)
    Lp = np.linalg.inv(L.astype(np.float64) + P) - P
    lnorm = float(np.abs(Lp).sum(axis=1).max()) if n else 0.0
    rhs_f = np.array([float(t) for t in rhs])
    rmax = float(np.abs(rhs_f).max()) if n else 0.0
    alr = np.bincount(eu, weights=np.abs(lr), minlength=n) + np.bincount(ev, weights=np.abs(lr), minlength=n)
    tol_stop = lnorm * 1e-12 * rmax
    tol = lnorm * (1e-12 * rmax + 8 * EPS * float((deg * alr).max() if n else 0.0))
    return dict(phi=np.array([float(t) for t in phi]), comp=comp, L=L, rhs=rhs_f, deg=deg, tol=tol, tol_stop=tol_stop, lnorm=lnorm,
                misfit_max=float(max([abs(t) for t in mis], default=0)), misfit_ss=float(sum(t * t for t in mis)),
                misfit_l1=float(sum(abs(t) for t in mis)), relations=len(eu))


@functools.lru_cache(maxsize=None)
def reference_of(name):
    return reference(instance(name))


def anchored_prices(ref, anchor):
    """the definition's prices from the exact phi"""
    phi, comp = ref["phi"], ref["comp"]
    nc = int(comp.max()) + 1
    known = anchor > 0
    logp = phi.copy()
    for c in range(nc):
        k = known & (comp == c)
        if k.any():
            logp[comp == c] += float(np.mean(np.log(anchor[k]) - phi[k]))
    out = np.exp(logp)
    out[known] = anchor[known]
    return out
