"""Host-side mirror of the reference's problem object and of its `cp.Problem(...).solve()` call.

The reference (/root/reference/arbitrage.py, liquidation.py, two-asset.py) has no functions or
classes: a "problem" is the module-level data `local_indices`, `reserves`, `fees`
(arbitrage.py:6-28), the constraint lines that pick a trading function per pool
(arbitrage.py:63-74), and a utility (arbitrage.py:57,77 / liquidation.py:57,77-80 /
two-asset.py:66,86); the result surface is `prob.value`, `psi.value`, `deltas[i].value`,
`lambdas[i].value` (arbitrage.py:84, two-asset.py:94-100).  `Problem` keeps exactly that
vocabulary and hands the work to libcfmm_hip.so (include/cfmm.h).  There is no CPU path here:
without the HIP extension and a gfx950 device `solve()` raises.

Host logic that stays in Python (tiny, O(n) or O(#constant-sum pools)):
  * packing pools into per-kind SoA buckets (the dense A_i of arbitrage.py:42-48 become int32 ids);
  * start prices for utilities that do not name a price for every token;
  * constant-sum pools on their kink: tying the two prices (a linear equality in log-price),
    re-solving on the device, and recovering the fill fraction (primal recovery).
"""
import os
import sys
import numpy as np

from . import _lib
from ._lib import GE, EQ, FREE, ULOG, UQUAD, POOL_CP2, POOL_W2, POOL_SUM2, POOL_CURVE2, POOL_POW2, MAX_POOL_SIZE, CfmmError

KIND2 = dict(cp2=POOL_CP2, w2=POOL_W2, sum2=POOL_SUM2, curve2=POOL_CURVE2, pow2=POOL_POW2)
# the name of a two-asset bucket's parameter column (None: the kind has none)
PARAM2 = dict(cp2=None, w2="wa", sum2=None, curve2="alpha", pow2="t")


# ------------------------------------------------------------------------------- utilities
class Utility:
    """maximise c'psi  s.t.  psi_k + h_k >= 0 (GE) | = 0 (EQ) | unconstrained (FREE) -- the reference's utilities (arbitrage.py:57,77;
    liquidation.py:57,77-80; two-asset.py:66,86).  Beyond them, per token, an entry of the utility table:
    ctype ULOG: + c_k log(psi_k + h_k);  UQUAD: + c_k psi_k - psi_k^2 / (2 h_k)   (include/cfmm.h; both outer iterations take them: the
    generic two-launch first-order iteration, and the second-order path -- which `method="auto"` falls back to when the first-order
    run ends without its certificates)."""

    def __init__(self, c, h=None, ctype=None):
        self.c = np.asarray(c, dtype=np.float64)
        n = len(self.c)
        self.h = np.zeros(n) if h is None else np.asarray(h, dtype=np.float64)
        self.ctype = np.zeros(n, dtype=np.int32) if ctype is None else np.asarray(ctype, dtype=np.int32)


def Arbitrage(market_value):
    """max market_value @ psi, psi >= 0                      (arbitrage.py:57,77)"""
    return Utility(market_value)


def Liquidate(current_assets, target):
    """max psi[target], psi[k] + current_assets[k] == 0, k != target   (liquidation.py:57,77-80)"""
    h = np.asarray(current_assets, dtype=np.float64).copy()
    n = len(h)
    c = np.zeros(n); c[target] = 1.0
    h[target] = 0.0
    ctype = np.full(n, EQ, dtype=np.int32); ctype[target] = FREE
    return Utility(c, h, ctype)


def LogUtility(weights, holdings):
    """max sum_k weights[k] log(psi_k + holdings[k]): a logarithmic (Kelly / Cobb-Douglas) utility of the post-trade holdings.
    Not in the reference (its objectives are linear); tokens with weight 0 are held at psi_k + holdings[k] >= 0 and worth nothing."""
    a = np.asarray(weights, dtype=np.float64)
    h = np.asarray(holdings, dtype=np.float64)
    ctype = np.where(a > 0, ULOG, GE).astype(np.int32)
    return Utility(a, h, ctype)


def QuadraticUtility(marginal_value, depth):
    """max sum_k marginal_value[k] psi_k - psi_k^2 / (2 depth[k]): a linear value with quadratic impact (an external order book of
    finite depth behind every token).  depth[k] = inf is the linear-arbitrage token (psi_k >= 0 at value c_k).
    marginal_value >= 0 (what cfmm_set_utility accepts for every entry kind: include/cfmm.h)."""
    c = np.asarray(marginal_value, dtype=np.float64)
    if np.any(c < 0):
        raise ValueError("QuadraticUtility: marginal_value must be >= 0")
    d = np.asarray(depth, dtype=np.float64)
    fin = np.isfinite(d)
    return Utility(c, np.where(fin, d, 0.0), np.where(fin, UQUAD, GE).astype(np.int32))


def Swap(current_assets, target):
    """max psi[target], psi + current_assets >= 0            (two-asset.py:66,86)"""
    h = np.asarray(current_assets, dtype=np.float64)
    c = np.zeros(len(h)); c[target] = 1.0
    return Utility(c, h)


# ------------------------------------------------------------------------------- packing
def pack(n_tokens, local_indices, reserves, fees, kinds=None, weights=None, params=None):
    """Ragged pool list (reference vocabulary) -> SoA buckets + `where[i] = (bucket, position)`.

    kinds[i]: "geomean" (default) | "sum" | "curve" | "powersum";  weights[i]: geo-mean exponents (None =
    equal, i.e. Uniswap v2 for two assets);  params[i]: alpha of a curve pool, the exponent t of a power-sum pool
    (x^(1-t) + y^(1-t): the generic bucket's first tenant, include/cfmm.h CFMM_POOL_POW2).
    "sum" and "curve" pools over 3..8 tokens go to the K-asset table's buckets (net["gk"][(kind, k)]: csrc/phik.hpp,
    include/cfmm.h CFMM_POOLK_*): `where` then holds (("stable" | "sum", k), position)."""
    m = len(local_indices)
    kinds = ["geomean"] * m if kinds is None else list(kinds)
    weights = [None] * m if weights is None else list(weights)
    params = [None] * m if params is None else list(params)
    rows = dict(cp2=[], w2=[], sum2=[], curve2=[], pow2=[])
    rows_n = {}
    rows_g = {}
    where = []
    for i in range(m):
        l = np.asarray(local_indices[i], dtype=np.int64)
        R = np.asarray(reserves[i], dtype=np.float64)
        k = len(l)
        if len(R) != k:
            raise ValueError(f"pool {i}: {k} indices but {len(R)} reserves")
        if len(set(l.tolist())) != k or l.min() < 0 or l.max() >= n_tokens:
            raise ValueError(f"pool {i}: token ids must be distinct and in [0, {n_tokens})")
        if not np.all(R > 0) or not (0 < fees[i] <= 1):
            raise ValueError(f"pool {i}: reserves must be > 0 and the fee in (0, 1]")
        kind = kinds[i]
        if kind == "geomean":
            w = np.ones(k) if weights[i] is None else np.asarray(weights[i], dtype=np.float64)
            if len(w) != k or not np.all(w > 0):
                raise ValueError(f"pool {i}: bad weights")
            w = w / w.sum()
            if k == 2:
                if w[0] == w[1]:
                    where.append(("cp2", len(rows["cp2"])))
                    rows["cp2"].append((R[0], R[1], fees[i], 0.0, l[0], l[1]))
                else:
                    where.append(("w2", len(rows["w2"])))
                    rows["w2"].append((R[0], R[1], fees[i], w[0], l[0], l[1]))
            elif 3 <= k <= MAX_POOL_SIZE:
                b = rows_n.setdefault(k, [])
                where.append((k, len(b)))
                b.append((l, R, w, fees[i]))
            else:
                raise ValueError(f"pool {i}: geo-mean pools hold 2..{MAX_POOL_SIZE} tokens, got {k}")
        elif kind == "sum":
            if k == 2:
                where.append(("sum2", len(rows["sum2"])))
                rows["sum2"].append((R[0], R[1], fees[i], 0.0, l[0], l[1]))
            elif 3 <= k <= MAX_POOL_SIZE:                  # arbitrage.py:73-74 over more than two tokens: the K-asset table
                b = rows_g.setdefault(("sum", k), [])
                where.append((("sum", k), len(b)))
                b.append((l, R, fees[i], 0.0))
            else:
                raise ValueError(f"pool {i}: constant-sum pools hold 2..{MAX_POOL_SIZE} tokens, got {k}")
        elif kind == "curve":
            if params[i] is None or not (float(params[i]) > 0):
                raise ValueError(f"pool {i}: curve pools need params[i] = alpha > 0")
            if k == 2:
                where.append(("curve2", len(rows["curve2"])))
                rows["curve2"].append((R[0], R[1], fees[i], float(params[i]), l[0], l[1]))
            elif 3 <= k <= MAX_POOL_SIZE:                  # sum x - alpha / prod x over more than two tokens: the K-asset table
                b = rows_g.setdefault(("stable", k), [])
                where.append((("stable", k), len(b)))
                b.append((l, R, fees[i], float(params[i])))
            else:
                raise ValueError(f"pool {i}: curve pools hold 2..{MAX_POOL_SIZE} tokens, got {k}")
        elif kind == "powersum":
            if k != 2 or params[i] is None or not (1e-3 <= float(params[i]) <= 0.999):
                raise ValueError(f"pool {i}: power-sum pools are two-asset and need params[i] = t in [0.001, 0.999]")
            where.append(("pow2", len(rows["pow2"])))
            rows["pow2"].append((R[0], R[1], fees[i], float(params[i]), l[0], l[1]))
        else:
            raise ValueError(f"pool {i}: unknown kind {kind!r}")
    net = dict(n_tokens=int(n_tokens))
    pname = PARAM2
    for key, rr in rows.items():
        if not rr:
            continue
        a = np.array(rr, dtype=np.float64)
        b = dict(Ra=a[:, 0].copy(), Rb=a[:, 1].copy(), fee=a[:, 2].copy(),
                 ia=a[:, 4].astype(np.int32), ib=a[:, 5].astype(np.int32))
        if pname[key]:
            b[pname[key]] = a[:, 3].copy()
        net[key] = b
    if rows_n:
        net["gn"] = {}
        for k, rr in rows_n.items():
            net["gn"][k] = dict(idx=np.array([r[0] for r in rr], dtype=np.int32).T.copy(),
                                R=np.array([r[1] for r in rr]).T.copy(),
                                w=np.array([r[2] for r in rr]).T.copy(),
                                fee=np.array([r[3] for r in rr], dtype=np.float64))
    if rows_g:
        net["gk"] = {}
        for key, rr in rows_g.items():
            net["gk"][key] = dict(idx=np.array([r[0] for r in rr], dtype=np.int32).T.copy(),
                                  R=np.array([r[1] for r in rr]).T.copy(),
                                  fee=np.array([r[2] for r in rr], dtype=np.float64),
                                  param=np.array([r[3] for r in rr], dtype=np.float64))
    return net, where


def _param_rule(kind_key, i, x):
    """the parameter rule of pack() for a bucket whose pools carry one (None: fine), with pack's message"""
    if kind_key in ("curve2", "stable"):
        if x is None or not (float(x) > 0):
            return f"pool {i}: curve pools need params[i] = alpha > 0"
    elif kind_key == "pow2":
        if x is None or not (1e-3 <= float(x) <= 0.999):
            return f"pool {i}: power-sum pools are two-asset and need params[i] = t in [0.001, 0.999]"
    elif x is not None:
        return f"pool {i}: this kind of pool has no parameter to update"
    return None


def route_updates(net, where, pools, reserves, params=None):
    """New reserves of some pools of a packed network, routed to their buckets: `pools` are indices into the reference's pool
    list (arbitrage.py:6-28 order, `where` as pack() returned it), reserves[i] the new reserve vector of pools[i], params[i] (or
    params None) the new alpha / t of a curve / power-sum pool (None: unchanged).  Checks lengths, positivity, parameters (with
    pack's messages), range and duplicates; raises ValueError.  Returns {bucket key: (positions int32[count], R [k][count],
    param [count] or None)} with slot-major R, positions ascending, the key as bucket_trades takes it ('cp2'..'pow2', a size k,
    ('stable' | 'sum', k)).  An entry without a new parameter in a bucket where another entry has one keeps its current value."""
    pools = [int(i) for i in pools]
    if len(reserves) != len(pools):
        raise ValueError(f"{len(pools)} pools but {len(reserves)} reserve vectors")
    if params is not None and len(params) != len(pools):
        raise ValueError(f"{len(pools)} pools but {len(params)} parameters")
    if len(set(pools)) != len(pools):
        raise ValueError("a pool is named twice")
    rows = {}
    for e, i in enumerate(pools):
        if not 0 <= i < len(where):
            raise ValueError(f"pool {i}: outside [0, {len(where)})")
        key, pos = where[i]
        R = np.asarray(reserves[e], dtype=np.float64).ravel()
        k = key if isinstance(key, int) else (key[1] if isinstance(key, tuple) else 2)
        if len(R) != k:
            raise ValueError(f"pool {i}: {k} indices but {len(R)} reserves")
        if not np.all(np.isfinite(R)) or not np.all(R > 0):
            raise ValueError(f"pool {i}: reserves must be > 0 and finite")
        x = None if params is None else params[e]
        msg = _param_rule(key[0] if isinstance(key, tuple) else key, i, x) if x is not None else None
        if msg:
            raise ValueError(msg)
        rows.setdefault(key, []).append((pos, R, None if x is None else float(x)))
    out = {}
    for key, rr in rows.items():
        rr.sort(key=lambda r: r[0])
        pos = np.array([r[0] for r in rr], dtype=np.int32)
        R = np.array([r[1] for r in rr], dtype=np.float64).T.copy()
        param = None
        if any(r[2] is not None for r in rr):
            cur = _bucket_param(net, key)
            param = np.array([cur[r[0]] if r[2] is None else r[2] for r in rr], dtype=np.float64)
        out[key] = (pos, R, param)
    return out


def route_terms(net, where, pools, fees=None, weights=None):
    """New fees and / or weights of some pools of a packed network, routed to their buckets, beside route_updates: `pools` are indices
    into the reference's pool list, fees[i] the new fee of pools[i], weights[i] its new geo-mean exponents (either list may be None, or
    hold None for "unchanged").  Weights are normalised as pack() does (w / w.sum()).  Checks lengths, the fee in (0, 1], weights positive
    (with pack's messages), range and duplicates; a two-asset pool that pack() put into 'cp2' takes no weights (unequal ones would move it
    to another bucket: a re-upload), a 'w2' pool may take equal ones and stays where it is; raises ValueError.  Returns {bucket key: (positions
    int32[count], fee [count] or None, w or None)}, positions ascending; w is slot-major [k][count] for a geo-mean bucket and the first
    token's weight wa [count] for 'w2'.  An entry without a new fee (weights) in a bucket where another entry has one keeps its current."""
    pools = [int(i) for i in pools]
    for what, col in (("fees", fees), ("weight vectors", weights)):
        if col is not None and len(col) != len(pools):
            raise ValueError(f"{len(pools)} pools but {len(col)} {what}")
    if len(set(pools)) != len(pools):
        raise ValueError("a pool is named twice")
    rows = {}
    for e, i in enumerate(pools):
        if not 0 <= i < len(where):
            raise ValueError(f"pool {i}: outside [0, {len(where)})")
        key, pos = where[i]
        f = None if fees is None or fees[e] is None else float(fees[e])
        if f is not None and not (0 < f <= 1):
            raise ValueError(f"pool {i}: the fee must be in (0, 1], got {f!r}")
        w = None if weights is None or weights[e] is None else np.asarray(weights[e], dtype=np.float64).ravel()
        if w is not None:
            if key == "cp2":
                raise ValueError(f"pool {i}: a constant-product pool (bucket 'cp2': equal weights) holds no weight column; giving it unequal weights is a re-upload")
            if key != "w2" and not isinstance(key, int):
                raise ValueError(f"pool {i}: this kind of pool has no weights to update")
            k = 2 if key == "w2" else key
            if len(w) != k or not np.all(w > 0) or not np.all(np.isfinite(w)):
                raise ValueError(f"pool {i}: bad weights")
            w = w / w.sum()
            if not np.all((w > 0) & (w < 1)):
                raise ValueError(f"pool {i}: bad weights")
        if f is not None or w is not None:
            rows.setdefault(key, []).append((pos, f, w))
    out = {}
    for key, rr in rows.items():
        rr.sort(key=lambda r: r[0])
        b, fam = _bucket_of(net, key)
        pos = np.array([r[0] for r in rr], dtype=np.int32)
        fee = w = None
        if any(r[1] is not None for r in rr):
            fee = np.array([b["fee"][r[0]] if r[1] is None else r[1] for r in rr], dtype=np.float64)
        if any(r[2] is not None for r in rr):
            if key == "w2":
                w = np.array([b["wa"][r[0]] if r[2] is None else r[2][0] for r in rr], dtype=np.float64)
            else:
                w = np.array([b["w"][:, r[0]] if r[2] is None else r[2] for r in rr], dtype=np.float64).T.copy()
        out[key] = (pos, fee, w)
    return out


def post_trade_reserves(R, delta, lam, fee, fees="pool"):
    """Reserves of pools after their tenders are executed: R' = (R + g delta) - lam, every operation individually rounded -- the
    expression cfmm_apply_trades evaluates on the device (docs/apply_trades.md).  g = 1 with fees="pool" (the fee stays in the
    reserves: Uniswap v2, Balancer, Curve), g = the pool's fee factor gamma with fees="aside" (the fee is collected outside the pool:
    phi(R') = phi(R)).  R, delta, lam: [k][m] slot-major (or [m]); fee: [m].  Gross tenders (a leg that both receives and pays, as
    after a second-order solve) are taken as they are, in this order."""
    if fees not in _lib.FEE_MODES:
        raise ValueError(f"fees {fees!r}: expected one of {sorted(_lib.FEE_MODES)}")
    R, delta, lam = (np.asarray(a, dtype=np.float64) for a in (R, delta, lam))
    g = 1.0 if fees == "pool" else np.asarray(fee, dtype=np.float64)
    return (R + g * delta) - lam


# ------------------------------------------------------------------------------- the route audited (docs/audit.md)
AUDIT_TOL_POOL = 1e-9      # the stopping residual of the K-asset table's stableswap search (csrc/phik.hpp: pool_stable_k), the loosest per-pool solver


def audit_buckets(net):
    """every non-empty bucket of a packed network in the order of the library's bucket records (two-asset kinds, geo-mean sizes 3..8,
    the table's stableswap then constant-sum sizes): dicts with key (as bucket_trades takes it), family / kind / k (as cfmm_apply_info
    names them), cls ('log' | 'sum' | 'stable' | 'pow': what the slack is), idx, R [k][m], fee [m], and w [k][m] (cls 'log': the
    normalised weights), e [m] (cls 'pow': 1 - t) or alpha [m] (cls 'stable')"""
    out = []
    cls2 = dict(cp2="log", w2="log", sum2="sum", curve2="stable", pow2="pow")
    for key, kind in KIND2.items():
        b = net.get(key)
        if b is None or not len(b["Ra"]):
            continue
        m = len(b["Ra"])
        rec = dict(key=key, family=0, kind=kind, k=2, cls=cls2[key], idx=np.stack([b["ia"], b["ib"]]).astype(np.int64),
                   R=np.stack([b["Ra"], b["Rb"]]).astype(np.float64), fee=np.asarray(b["fee"], dtype=np.float64))
        if key == "cp2":
            rec["w"] = np.full((2, m), 0.5)
        elif key == "w2":
            wa = np.asarray(b["wa"], dtype=np.float64)
            rec["w"] = np.stack([wa, 1.0 - wa])
        elif key == "curve2":
            rec["alpha"] = np.asarray(b["alpha"], dtype=np.float64)
        elif key == "pow2":
            rec["e"] = 1.0 - np.asarray(b["t"], dtype=np.float64)
        out.append(rec)
    for k in sorted(net.get("gn", {})):
        b = net["gn"][k]
        if b["R"].shape[1]:
            w = np.asarray(b["w"], dtype=np.float64)
            out.append(dict(key=k, family=1, kind=0, k=k, cls="log", idx=np.asarray(b["idx"], dtype=np.int64), R=np.asarray(b["R"], dtype=np.float64),
                            fee=np.asarray(b["fee"], dtype=np.float64), w=w / w.sum(axis=0)))
    for name, kind in sorted(_lib.POOLK.items(), key=lambda kv: kv[1]):
        for k in range(2, MAX_POOL_SIZE + 1):
            b = net.get("gk", {}).get((name, k))
            if b is None or not b["R"].shape[1]:
                continue
            rec = dict(key=(name, k), family=2, kind=kind, k=k, cls="stable" if name == "stable" else "sum", idx=np.asarray(b["idx"], dtype=np.int64),
                       R=np.asarray(b["R"], dtype=np.float64), fee=np.asarray(b["fee"], dtype=np.float64))
            if name == "stable":
                rec["alpha"] = np.asarray(b["param"], dtype=np.float64)
            out.append(rec)
    return out


def audit_exponent(net):
    """F of the fixed point y 2^F: what the reproducible mode derives from the largest reserve and the smallest fee (csrc/cfmm_hip.hip: det_scales)"""
    import math
    mr, mf = 0.0, 1.0
    for b in audit_buckets(net):
        mr = max(mr, float(b["R"].max())); mf = min(mf, float(b["fee"].min()))
    return 84 - math.frexp(max(mr, 1e-300) / max(mf, 1e-3))[1]


def _fixed_limbs(y, F):
    """the three limbs (uint64, uint64, int64 arrays) of floor(y 2^F), exactly, for doubles with |y 2^F| < 2^94: y = m 2^e with m a signed
    53-bit integer, and m 2^(e + F) is shifted in integer arithmetic (csrc/fixedpoint.hpp: fixed_split gives the same limbs)"""
    mant, exp = np.frexp(np.asarray(y, dtype=np.float64))
    m = np.ldexp(mant, 53).astype(np.int64)
    s = exp.astype(np.int64) - 53 + F
    M32 = np.int64(0xFFFFFFFF)
    # s < 0: an arithmetic shift floors (beyond 63 places: 0 or -1)
    v = m >> np.minimum(np.maximum(-s, 0), 63)
    neg = (v & M32, (v >> 32) & M32, v >> 63)                          # (the sign fills the top limb)
    # s >= 0 (<= 41): m = mh 2^32 + ml, shifted by r = s mod 32 in two pieces, then by whole limbs
    sp = np.maximum(s, 0)
    r, a = sp & 31, sp >> 5
    ml, mh = (m & M32).astype(np.uint64), m >> 32
    t0 = ml << r.astype(np.uint64)
    l0 = (t0 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    t1 = (mh << r) + (t0 >> np.uint64(32)).astype(np.int64)
    l1, l2 = t1 & M32, t1 >> 32
    pos = (np.where(a == 0, l0, 0), np.where(a == 0, l1, l0), np.where(a == 0, l2, l1 + (l2 << 32)))
    lo = s < 0
    return (np.where(lo, neg[0], pos[0]).astype(np.uint64), np.where(lo, neg[1], pos[1]).astype(np.uint64), np.where(lo, neg[2], pos[2]))


def audit_trades(net, trades, utility=None, tol_pool=AUDIT_TOL_POOL, exponent=None):
    """Does every pool accept this route, and what does it add up to?  The NumPy twin of cfmm_audit_trades (include/cfmm.h,
    docs/audit.md), the host path of pool-sharded problems and the reference of the tests.  trades: {bucket key: (delta, lambda)}, slot-major
    [k][m] in upload order, as Problem.bucket_trades hands them out.  Per pool, x_j = (R_j + gamma Delta_j) - Lambda_j, each operation
    rounded on its own; slack: the relative change of the trading function (>= 0: accepted); a pool violates with slack < -tol_pool, a
    tender negative or not finite, or a leg that does not stay positive (constant sum: x_j < -tol_pool sum R).  psi is summed EXACTLY:
    every non-zero Lambda_j (+) and Delta_j (-) floored on its own to the 96-bit fixed point floor(y 2^F), as Python integers.
    exponent: F; None derives it from this network's largest reserve and smallest fee (audit_exponent), which is what the device does
    for an unsharded context -- the shards of a pool-sharded network pass the exponent of the WHOLE network, so that their integers add.
    Returns the fields of cfmm_audit plus psi [n], psi_int (n Python integers: psi 2^F before the one rounding), limbs ([3][n] uint64: the
    layout of cfmm_debug_eval_limbs) and slack ({key: [m]})."""
    import math
    n = int(net["n_tokens"])
    tol = float(tol_pool) if tol_pool is not None and tol_pool > 0 else AUDIT_TOL_POOL
    F = audit_exponent(net) if exponent is None else int(exponent)
    L0 = np.zeros(n, dtype=np.uint64); L1 = np.zeros(n, dtype=np.uint64); L2 = np.zeros(n, dtype=np.int64)
    rep = dict(pools=0, pools_trading=0, pools_violating=0, legs_out_of_range=0, worst_family=-1, worst_kind=-1, worst_k=-1,
               fixed_exponent=F, worst_pos=-1, min_slack=np.inf, min_tender=np.inf, min_leg=np.inf, value=np.nan, infeas=np.nan)
    slacks = {}
    ninf = -np.inf
    with np.errstate(all="ignore"):
        for b in audit_buckets(net):
            D, L = (np.asarray(a, dtype=np.float64) for a in trades[b["key"]])
            R, g, k = b["R"], b["fee"], b["k"]
            m = R.shape[1]
            x = (R + g * D) - L
            Sx = np.zeros(m); SR = np.zeros(m)
            for j in range(k):
                Sx = Sx + x[j]; SR = SR + R[j]
            if b["cls"] == "log":
                s = np.zeros(m)
                for j in range(k):
                    s = s + b["w"][j] * np.log(x[j] / R[j])
            elif b["cls"] == "sum":
                s = (Sx - SR) / SR
            elif b["cls"] == "stable":
                Px = np.ones(m); PR = np.ones(m)
                for j in range(k):
                    Px = Px * x[j]; PR = PR * R[j]
                cx, cR = b["alpha"] / Px, b["alpha"] / PR
                s = ((Sx - cx) - (SR - cR)) / (SR + cR)
            else:
                fx = np.zeros(m); fR = np.zeros(m)
                for j in range(k):
                    fx = fx + np.power(x[j], b["e"]); fR = fR + np.power(R[j], b["e"])
                s = (fx - fR) / fR
            s = np.where(np.isfinite(s), s, ninf) + 0.0
            tbad = (~(np.isfinite(D) & (D >= 0.0)) | ~(np.isfinite(L) & (L >= 0.0))).any(axis=0)
            xmin = np.fmin.reduce(x, axis=0)                                   # (NaN legs are told apart below)
            bad = (s < -tol) | tbad
            bad |= (xmin < -(tol * SR)) if b["cls"] == "sum" else ~(x > 0.0).all(axis=0)
            leg = np.where(np.isnan(x).any(axis=0), ninf, xmin / R.max(axis=0))
            tmin = min(float(np.where(np.isnan(D), ninf, D).min()), float(np.where(np.isnan(L), ninf, L).min()))
            rep["pools"] += m
            rep["pools_trading"] += int(((D != 0.0) | (L != 0.0)).any(axis=0).sum())
            rep["pools_violating"] += int(bad.sum())
            i = int(np.argmin(s))                                              # (the first of equals: the lowest upload position)
            if rep["worst_pos"] < 0 or s[i] < rep["min_slack"]:                # (strictly: ties go to the first bucket)
                rep.update(min_slack=float(s[i]), worst_family=b["family"], worst_kind=b["kind"], worst_k=k, worst_pos=i)
            rep["min_tender"] = min(rep["min_tender"], tmin)
            rep["min_leg"] = min(rep["min_leg"], float(leg.min()))
            slacks[b["key"]] = s
            for y, sign in ((L, 1.0), (D, -1.0)):
                sel = y != 0.0
                yv, tok = sign * y[sel], b["idx"][sel]
                ok = np.abs(np.ldexp(yv, F)) < 2.0 ** 94                       # (false for values that are not finite)
                rep["legs_out_of_range"] += int((~ok).sum())
                a0, a1, a2 = _fixed_limbs(yv[ok], F)
                np.add.at(L0, tok[ok], a0); np.add.at(L1, tok[ok], a1); np.add.at(L2, tok[ok], a2)
    limbs = np.stack([L0, L1, L2.view(np.uint64)])
    psi_int = [(int(L2[j]) << 64) + (int(L1[j]) << 32) + int(L0[j]) for j in range(n)]
    psi = np.array([math.ldexp(float(v), -F) for v in psi_int], dtype=np.float64).reshape(n)
    rep.update(psi=psi, psi_int=psi_int, limbs=limbs, slack=slacks)
    if utility is not None:
        c, h, ct = utility.c, utility.h, utility.ctype
        r = psi + h
        lin = ct <= FREE
        with np.errstate(all="ignore"):
            terms = np.where(ct == ULOG, c * np.log(np.where(ct == ULOG, r, 1.0)),
                             np.where(ct == UQUAD, c * psi - psi * psi / (2.0 * np.where(ct == UQUAD, h, 1.0)), c * psi))
        value = 0.0
        for t in terms.tolist():
            value += t
        viol = float(np.where(ct == GE, np.maximum(-r, 0.0), np.where(ct == EQ, np.abs(r), 0.0)).max()) if n else 0.0
        scale = max(float(np.abs(psi).max()) if n else 0.0, float(np.abs(h[lin]).max()) if lin.any() else 0.0)
        mr = max((float(b["R"].max()) for b in audit_buckets(net)), default=0.0)
        rep["value"] = value
        rep["infeas"] = viol / max(scale, 1e-12 * mr, 1e-300)
    return rep


# ------------------------------------------------------------------------------- a held route re-quoted (docs/requote.md)
REQUOTE_TOL_SCALE = 1e-9   # the default tol_scale: the audit's tol_pool


def requote_slack(b, up, L, s):
    """the slack of every pool of one bucket (a record of audit_buckets) at the scales s [m]: the audit's expression per class on
    x = up - s L with up = R + gamma Delta already formed, every operation rounded on its own, sums and products in leg order"""
    R, k = b["R"], b["k"]
    m = R.shape[1]
    with np.errstate(all="ignore"):
        x = up - s * L
        Sx = np.zeros(m); SR = np.zeros(m)
        for j in range(k):
            Sx = Sx + x[j]; SR = SR + R[j]
        if b["cls"] == "log":
            F = np.zeros(m)
            for j in range(k):
                F = F + b["w"][j] * np.log(x[j] / R[j])
        elif b["cls"] == "sum":
            F = (Sx - SR) / SR
        elif b["cls"] == "stable":
            Px = np.ones(m); PR = np.ones(m)
            for j in range(k):
                Px = Px * x[j]; PR = PR * R[j]
            cx, cR = b["alpha"] / Px, b["alpha"] / PR
            F = ((Sx - cx) - (SR - cR)) / (SR + cR)
        else:
            fx = np.zeros(m); fR = np.zeros(m)
            for j in range(k):
                fx = fx + np.power(x[j], b["e"]); fR = fR + np.power(R[j], b["e"])
            F = (fx - fR) / fR
    return F


def _take(b, sel):
    """the pools `sel` of a bucket record"""
    out = dict(b)
    for key in ("R", "w", "idx"):
        if key in b:
            out[key] = b[key][:, sel]
    for key in ("fee", "alpha", "e"):
        if key in b:
            out[key] = b[key][sel]
    return out


def requote_bucket(b, D, L, scales=None):
    """one bucket of requote_route: (s [m], trading, capped, failed -- boolean [m]).  The cap, the special cases and the verdicts are the
    device's (csrc/requote.hpp); the root, with scales=None, is found by bisection on the bracket [0, s_cap] down to adjacent doubles
    and is the lower one: the last s whose own slack evaluation is >= 0"""
    R, g = b["R"], b["fee"]
    m = R.shape[1]
    fin = lambda a: np.isfinite(a) & (a >= 0.0)
    with np.errstate(all="ignore"):
        up = R + g * D
        trading = ((D != 0.0) | (L != 0.0)).any(axis=0)
        ok = (fin(D) & fin(L) & fin(up)).all(axis=0)
        SD = np.zeros(m); SL = np.zeros(m)
        for j in range(b["k"]):
            SD = SD + D[j]; SL = SL + L[j]
        c = up / L
        for _ in range(6):
            over = (c * L > up) if b["cls"] == "sum" else (c * L >= up)          # (only a constant-sum leg may be drained to zero)
            c = np.where((L > 0.0) & (c > 0.0) & over, np.nextafter(c, 0.0), c)
        cap = np.where(L > 0.0, c, np.inf).min(axis=0)
        failed = trading & (~ok | ((SL > 0.0) & ~fin(cap)))
        live = trading & ~failed
        s = np.ones(m)
        s[live & (SL > 0.0) & ~(SD > 0.0)] = 0.0
        act = live & (SL > 0.0) & (SD > 0.0)
        capped = np.zeros(m, dtype=bool)
        if b["cls"] == "sum":
            sv = (g * SD) / SL
            bad = act & ~fin(sv)
            capped = act & ~bad & (sv > cap)
            s = np.where(act, np.where(capped, cap, sv), s)
            failed |= bad
        else:
            bad = act & ~(requote_slack(b, up, L, np.zeros(m)) >= 0.0)
            capped = act & ~bad & (requote_slack(b, up, L, np.where(act, cap, 0.0)) >= 0.0)
            s = np.where(capped, cap, s)
            failed |= bad
            idx = np.flatnonzero(act & ~bad & ~capped)
            if scales is None and len(idx):
                bb, ub, Lb = _take(b, idx), up[:, idx], L[:, idx]
                lo, hi = np.zeros(len(idx)), cap[idx].copy()
                for _ in range(2400):
                    mid = lo + 0.5 * (hi - lo)
                    inside = (mid > lo) & (mid < hi)
                    if not inside.any():
                        break
                    above = requote_slack(bb, ub, Lb, mid) >= 0.0
                    lo = np.where(inside & above, mid, lo); hi = np.where(inside & ~above, mid, hi)
                s[idx] = lo
        s = np.where(failed, np.nan, s)
        if scales is not None:
            s = np.asarray(scales, dtype=np.float64).copy()
    return s, trading, capped, failed


def psi_worth(net, psi, utility):
    """(value, infeas) of a net trade under a utility: the host expression of cfmm_audit / cfmm_requote (csrc/route_rules.hpp: psi_worth)"""
    n = len(psi)
    c, h, ct = utility.c, utility.h, utility.ctype
    r = psi + h
    lin = ct <= FREE
    with np.errstate(all="ignore"):
        terms = np.where(ct == ULOG, c * np.log(np.where(ct == ULOG, r, 1.0)),
                         np.where(ct == UQUAD, c * psi - psi * psi / (2.0 * np.where(ct == UQUAD, h, 1.0)), c * psi))
    value = 0.0
    for t in terms.tolist():
        value += t
    viol = float(np.where(ct == GE, np.maximum(-r, 0.0), np.where(ct == EQ, np.abs(r), 0.0)).max()) if n else 0.0
    scale = max(float(np.abs(psi).max()) if n else 0.0, float(np.abs(h[lin]).max()) if lin.any() else 0.0)
    mr = max((float(b["R"].max()) for b in audit_buckets(net)), default=0.0)
    return value, viol / max(scale, 1e-12 * mr, 1e-300)


def requote_route(net, held, utility=None, scales=None, tol_scale=REQUOTE_TOL_SCALE, exponent=None):
    """What does a held route pay on the pools as they are now?  The NumPy twin of cfmm_requote_route (include/cfmm.h, docs/requote.md),
    the host path of Problem.requote and the reference of the tests.  net: the packed network at its CURRENT reserves, fees and weights;
    held: {bucket key: (delta, lambda)}, slot-major [k][m] in upload order, as Problem._trades builds it.  Per trading pool the inputs
    stay and the outputs are scaled onto the curve: x_j(s) = (R_j + gamma Delta_j) - s Lambda_j with s the root of the audit's slack,
    Lambda'_j = fl(s Lambda_j).  scales=None: every root is found here in fp64 by bisection to the last bit that changes the slack's
    sign; scales = {key: s [m]} (the device's): they are used as they are and only the tenders, the integers, limbs, psi and the report
    are formed -- bit for bit the device's.  exponent: F of the fixed point (None: audit_exponent(net)).
    Returns the fields of cfmm_requote plus psi [n], psi_int, limbs [3][n] uint64, scale {key: [m]} and lambdas {key: [k][m]}."""
    import math
    n = int(net["n_tokens"])
    tol = float(tol_scale) if tol_scale is not None and tol_scale > 0 else REQUOTE_TOL_SCALE
    F = audit_exponent(net) if exponent is None else int(exponent)
    L0 = np.zeros(n, dtype=np.uint64); L1 = np.zeros(n, dtype=np.uint64); L2 = np.zeros(n, dtype=np.int64)
    rep = dict(pools=0, pools_trading=0, pools_short=0, pools_long=0, pools_capped=0, pools_failed=0, legs_out_of_range=0,
               min_family=-1, min_kind=-1, min_k=-1, fixed_exponent=F, min_pos=-1, min_scale=np.inf, value=np.nan, infeas=np.nan)
    scale, lambdas = {}, {}
    with np.errstate(all="ignore"):
        for b in audit_buckets(net):
            key = b["key"]
            D, L = (np.asarray(a, dtype=np.float64) for a in held[key])
            s, trading, capped, failed = requote_bucket(b, D, L, None if scales is None else scales[key])
            live = trading & ~failed
            Lp = s * L
            scale[key], lambdas[key] = s, Lp
            rep["pools"] += len(s)
            rep["pools_trading"] += int(trading.sum())
            rep["pools_short"] += int((live & (s < 1.0 - tol)).sum())
            rep["pools_long"] += int((live & (s > 1.0 + tol)).sum())
            rep["pools_capped"] += int(capped.sum())
            rep["pools_failed"] += int(failed.sum())
            if live.any():
                sl = np.where(live, s, np.inf)
                i = int(np.argmin(sl))                                         # (the first of equals: the lowest upload position)
                if sl[i] < rep["min_scale"]:                                   # (strictly: ties go to the first bucket)
                    rep.update(min_scale=float(sl[i]), min_family=b["family"], min_kind=b["kind"], min_k=b["k"], min_pos=i)
            for y, sign in ((Lp, 1.0), (D, -1.0)):
                sel = (y != 0.0) & live[None, :]
                yv, tok = sign * y[sel], b["idx"][sel]
                ok = np.abs(np.ldexp(yv, F)) < 2.0 ** 94
                rep["legs_out_of_range"] += int((~ok).sum())
                a0, a1, a2 = _fixed_limbs(yv[ok], F)
                np.add.at(L0, tok[ok], a0); np.add.at(L1, tok[ok], a1); np.add.at(L2, tok[ok], a2)
    limbs = np.stack([L0, L1, L2.view(np.uint64)])
    psi_int = [(int(L2[j]) << 64) + (int(L1[j]) << 32) + int(L0[j]) for j in range(n)]
    psi = np.array([math.ldexp(float(v), -F) for v in psi_int], dtype=np.float64).reshape(n)
    rep.update(psi=psi, psi_int=psi_int, limbs=limbs, scale=scale, lambdas=lambdas)
    if utility is not None:
        rep["value"], rep["infeas"] = psi_worth(net, psi, utility)
    return rep


def apply_path(theta, dev_ties, sharded):
    """where Problem.apply_trades forms the new reserves: "device" (cfmm_apply_trades: no host leg) unless fills are held on the
    host (`theta`: the Python kink loop's), price ties / tie flags sit on the device, or the pools are sharded -- then "host\""""
    return "host" if (theta or dev_ties or sharded) else "device"


def _bucket_of(net, key):
    """(bucket dict, 'two' | 'gn' | 'gk') of a bucket key as bucket_trades takes it"""
    if isinstance(key, str):
        if key not in KIND2 or key not in net:
            raise ValueError(f"no bucket {key!r} in this network")
        return net[key], "two"
    if isinstance(key, tuple):
        if key not in net.get("gk", {}):
            raise ValueError(f"no bucket {key!r} in this network")
        return net["gk"][key], "gk"
    if int(key) not in net.get("gn", {}):
        raise ValueError(f"no bucket {key!r} in this network")
    return net["gn"][int(key)], "gn"


def _bucket_param(net, key):
    b, fam = _bucket_of(net, key)
    if fam == "two":
        return b[PARAM2[key]] if PARAM2[key] else None
    return b["param"] if fam == "gk" and key[0] == "stable" else None


def subset_network(net, positions_by_key):
    """The host network of a choice of pools: {bucket key: strictly ascending positions} (keys as bucket_trades takes them; a bucket
    not named, or named with no position, is left out) -> a network holding copies of those pools' columns in that order, equal array
    for array to what pack makes of the same pool sub-list.  Everything that is not a bucket (n_tokens, c, prices) is carried over."""
    out = {k: v for k, v in net.items() if not str(k).startswith("_") and k not in KIND2 and k not in ("gn", "gk")}
    for key, pos in positions_by_key.items():
        b, fam = _bucket_of(net, key)
        m = len(b["Ra"]) if fam == "two" else b["R"].shape[1]
        p = np.asarray(pos, dtype=np.int64).reshape(-1)
        if len(p) and (p[0] < 0 or p[-1] >= m or np.any(np.diff(p) <= 0)):
            raise ValueError(f"bucket {key!r}: positions must be strictly ascending and in [0, {m})")
        if len(p) == 0:
            continue
        sub = {name: (col[p].copy() if col.ndim == 1 else np.ascontiguousarray(col[:, p])) for name, col in b.items() if isinstance(col, np.ndarray)}
        if fam == "two":
            out[key] = sub
        else:
            out.setdefault(fam, {})[key if fam == "gk" else int(key)] = sub
    # (bucket order as pack and the uploads have it: the two-asset kinds, then the sizes in the parent's order)
    ordered = {k: v for k, v in out.items() if k not in KIND2 and k not in ("gn", "gk")}
    for key in KIND2:
        if key in out:
            ordered[key] = out[key]
    for fam in ("gn", "gk"):
        if fam in out:
            ordered[fam] = {k: out[fam][k] for k in net[fam] if k in out[fam]}
    return ordered


def network_pool_count(net):
    m = sum(len(net[k]["Ra"]) for k in KIND2 if k in net)
    m += sum(b["R"].shape[1] for b in net.get("gn", {}).values())
    m += sum(b["R"].shape[1] for b in net.get("gk", {}).values())
    return m


def shard_range(m, rank, world):
    """the contiguous slice [lo, hi) of a bucket of m pools that rank `rank` of `world` holds (shard_network)"""
    return (m * rank) // world, (m * (rank + 1)) // world


def shard_updates(m, rank, world, positions, R, param=None):
    """The entries of a bucket update given in GLOBAL positions (over all m pools of the bucket) that fall in this rank's slice,
    with positions local to it: what a pool-sharded Problem's update_bucket takes on each rank.  Every rank calls update_bucket
    with its part, an empty one included.  Returns (positions, R [k][count], param or None)."""
    lo, hi = shard_range(m, rank, world)
    pos = np.asarray(positions, dtype=np.int64).ravel()
    sel = (pos >= lo) & (pos < hi)
    R = np.asarray(R, dtype=np.float64)
    return pos[sel] - lo, R[:, sel], (None if param is None else np.asarray(param, dtype=np.float64)[sel])


def shard_terms(m, rank, world, positions, fee=None, w=None):
    """shard_updates for the per-pool columns of a terms update (Problem.update_bucket_terms): the entries given in GLOBAL positions
    that fall in this rank's slice of a bucket of m pools, with positions local to it.  Every rank calls update_bucket_terms with its
    part, an empty one included.  Returns (positions, fee [count] or None, w or None); w is [k][count] or, for 'w2', [count]."""
    lo, hi = shard_range(m, rank, world)
    pos = np.asarray(positions, dtype=np.int64).ravel()
    sel = (pos >= lo) & (pos < hi)
    return (pos[sel] - lo, None if fee is None else np.asarray(fee, dtype=np.float64)[sel],
            None if w is None else np.asarray(w, dtype=np.float64)[..., sel])


def shard_network(net, rank, world):
    """Pool-sharding: contiguous equal-count slices of every bucket; tokens,
    prices and the utility stay replicated."""
    out = {k: v for k, v in net.items() if k not in KIND2 and k not in ("gn", "gk") and not str(k).startswith("_")}      # (not the per-network caches: _price_relations, _potentials)

    def sl(m):
        return slice(*shard_range(m, rank, world))
    for key in KIND2:
        if key in net:
            b = net[key]; s = sl(len(b["Ra"]))
            out[key] = {c: v[s] for c, v in b.items()}
    if "gn" in net:
        out["gn"] = {}
        for k, b in net["gn"].items():
            s = sl(b["R"].shape[1])
            out["gn"][k] = dict(idx=b["idx"][:, s], R=b["R"][:, s], w=b["w"][:, s], fee=b["fee"][s])
    if "gk" in net:
        out["gk"] = {}
        for key, b in net["gk"].items():
            s = sl(b["R"].shape[1])
            out["gk"][key] = dict(idx=b["idx"][:, s], R=b["R"][:, s], fee=b["fee"][s], param=b["param"][s])
    return out


# ------------------------------------------------------------------------------- start prices
def _is_general(util):
    """does the utility hold entries of the utility table (ULOG / UQUAD)?  Kept with the utility object like the other facts derived
    from its arrays (Problem.set_utility drops them when the object is re-sent): three array scans less per solve"""
    g = getattr(util, "_general", None)
    if g is None:
        g = bool((util.ctype >= ULOG).any())
        try:
            util._general = g
        except AttributeError:
            pass
    return g


def start_prices(net, util):
    """Prices for every token: c where the utility names one, otherwise propagated through the
    pools' marginal prices at their current reserves (breadth-first, averaged in log space).
    The propagation depends on the pools and on c alone: its result is kept with the utility object (a re-solve with
    another basket h -- or the same one -- skips the ~2 ms walk over a 1000-token network)."""
    c = util.c
    if _is_general(util):           # the utility table: a token starts at the price at which it would not trade (u'(0))
        c = c.copy()
        lg, qd = util.ctype == ULOG, util.ctype == UQUAD
        with np.errstate(divide="ignore"):
            c[lg] = np.where(util.h[lg] > 0, util.c[lg] / np.where(util.h[lg] > 0, util.h[lg], 1.0), 0.0)
        c[qd] = util.c[qd]
        known = c > 0
        return c if known.all() else _propagate_prices(net, c, known)
    if getattr(util, "_all_priced", None) is None:       # (kept with the utility object: Problem.set_utility drops it when the object is re-sent)
        try:
            util._all_priced = bool((c > 0).all())
        except AttributeError:
            pass
    known = c > 0 if getattr(util, "_all_priced", None) is None else None
    if getattr(util, "_all_priced", None) or (known is not None and known.all()):
        return c.copy()
    if known is None:
        known = c > 0
    memo = getattr(util, "_start_memo", None)
    gen = net.get("_generation", 0)              # (Problem.update_bucket: the reserves the guess was propagated through changed)
    if memo is not None and memo[0] is net and memo[3] == gen and np.array_equal(memo[1], c):
        return memo[2].copy()
    out = _propagate_prices(net, c, known)
    try:
        util._start_memo = (net, c.copy(), out.copy(), gen)
    except AttributeError:
        pass
    return out


def _price_relations(net):
    """(eu, ev, lr): log p_eu - log p_ev = lr, the pools' marginal prices at their current reserves -- a property of the
    network alone, built once per network (kept in the dict under a private key; shard_network builds new dicts)."""
    rel = net.get("_price_relations")
    if rel is not None:
        return rel
    n = net["n_tokens"]
    eu, ev, elr = [], [], []
    # a rough guess is all this has to be (the solvers start by repairing it): on large networks every bucket is
    # thinned to an evenly strided sample, ~64 price relations per token in all
    total = sum(len(net[k]["Ra"]) for k in KIND2 if k in net) + \
        sum((kk - 1) * b["R"].shape[1] for kk, b in net.get("gn", {}).items()) + \
        sum((key[1] - 1) * b["R"].shape[1] for key, b in net.get("gk", {}).items())
    stride = max(1, total // (64 * n))
    for key in KIND2:
        if key not in net:
            continue
        b = net[key]
        sl = slice(0, None, stride)
        Ra, Rb = b["Ra"][sl], b["Rb"][sl]
        if key == "cp2":
            lr = np.log(Rb / Ra)
        elif key == "w2":
            wa = b["wa"][sl]
            lr = np.log(wa * Rb / ((1 - wa) * Ra))
        elif key == "sum2":
            lr = np.zeros(len(Ra))
        elif key == "pow2":
            lr = b["t"][sl] * np.log(Rb / Ra)
        else:
            al = b["alpha"][sl]
            lr = np.log((1 + al / (Ra * Ra * Rb)) / (1 + al / (Ra * Rb * Rb)))
        eu.append(b["ia"][sl]); ev.append(b["ib"][sl]); elr.append(lr)
    for k, b in net.get("gn", {}).items():
        sl = slice(0, None, stride)
        for j in range(1, k):
            eu.append(b["idx"][j][sl]); ev.append(b["idx"][0][sl])
            elr.append(np.log(b["w"][j][sl] * b["R"][0][sl] / (b["w"][0][sl] * b["R"][j][sl])))
    # the K-asset table's pools (csrc/phik.hpp): a token the utility leaves unpriced and that hangs on the rest through such pools
    # alone would otherwise be a component of its own and start at price 1.  Stableswap: the marginal ratio
    # (1 + s / R_j) / (1 + s / R_0), s = alpha / prod R; constant sum: equal prices
    for (kind, k), b in net.get("gk", {}).items():
        sl = slice(0, None, stride)
        R = b["R"][:, sl]
        if kind == "stable":
            sR = b["param"][sl] / np.prod(R, axis=0)
            lm = np.log1p(sR[None, :] / R)
        else:
            lm = np.zeros_like(R)
        for j in range(1, k):
            eu.append(b["idx"][j][sl]); ev.append(b["idx"][0][sl]); elr.append(lm[j] - lm[0])
    if eu:
        rel = (np.concatenate(eu).astype(np.int64), np.concatenate(ev).astype(np.int64), np.concatenate(elr))
    else:
        rel = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    net["_price_relations"] = rel
    return rel


def _potentials(net):
    """(phi, comp): log-price potentials of the tokens, the least-squares fit  min sum (phi_u - phi_v - lr)^2  over the
    network's price relations (one free constant per connected component), and the component of every token.  A property of
    the pools alone: solved once per network (sparse conjugate gradients; a few ms at 1000 tokens), after which the start prices of
    ANY utility cost O(n).  (Round 3 walked the relations breadth-first from the utility's priced tokens on every new utility:
    2-3 ms of host time per config-5 solve, hidden behind a per-utility memo.)"""
    pot = net.get("_potentials")
    if pot is not None:
        return pot
    n = net["n_tokens"]
    eu, ev, lr = _price_relations(net)
    if not len(eu):
        pot = (np.zeros(n), np.arange(n))
        net["_potentials"] = pot
        return pot
    # connected components: min-label propagation with pointer jumping (O(log n) rounds of two scatter-mins)
    comp = np.arange(n)
    while True:
        new = comp.copy()
        np.minimum.at(new, eu, comp[ev])
        np.minimum.at(new, ev, comp[eu])
        new = new[new]
        if np.array_equal(new, comp):
            break
        comp = new
    comp = np.unique(comp, return_inverse=True)[1]
    deg = (np.bincount(eu, minlength=n) + np.bincount(ev, minlength=n)).astype(float)

    def adj(x):                                            # A x for the (multi-)graph's adjacency matrix: two gathers, two scatter-adds
        return np.bincount(eu, weights=x[ev], minlength=n) + np.bincount(ev, weights=x[eu], minlength=n)
    rhs = np.bincount(eu, weights=lr, minlength=n) - np.bincount(ev, weights=lr, minlength=n)
    # Jacobi-preconditioned conjugate gradients on the graph Laplacian L = D - A (singular by one constant per component; the
    # right-hand side is orthogonal to those, and the iteration started at zero never leaves their complement)
    dinv = 1.0 / np.maximum(deg, 1.0)
    phi = np.zeros(n)
    r = rhs.copy()
    z = dinv * r
    pdir = z.copy()
    rz = float(r @ z)
    stop = 1e-12 * max(float(np.abs(rhs).max()), 1e-300)
    for _ in range(4 * n + 100):
        if float(np.abs(r).max()) <= stop:
            break
        q = deg * pdir - adj(pdir)
        alpha = rz / float(pdir @ q)
        phi += alpha * pdir
        r -= alpha * q
        z = dinv * r
        rz_new = float(r @ z)
        pdir = z + (rz_new / rz) * pdir
        rz = rz_new
    nc = int(comp.max()) + 1                              # gauge: zero mean per component
    phi -= (np.bincount(comp, weights=phi, minlength=nc) / np.bincount(comp, minlength=nc))[comp]
    pot = (phi, comp)
    net["_potentials"] = pot
    return pot


def _propagate_prices(net, c, known):
    """unpriced tokens from the network's potentials (above), shifted per connected component to agree on average with the
    prices the utility names there; a component the utility prices nowhere gets 1"""
    n = net["n_tokens"]
    phi, comp = _potentials(net)
    nc = int(comp.max()) + 1
    lc = np.log(np.where(known, c, 1.0))
    cnt = np.bincount(comp[known], minlength=nc)
    off = np.bincount(comp[known], weights=(lc - phi)[known], minlength=nc) / np.maximum(cnt, 1)
    logp = np.where(cnt[comp] > 0, phi + off[comp], 0.0)
    return np.where(known, c, np.exp(logp))


# ------------------------------------------------------------------------------- the prices the pools imply
def start_anchor(util):
    """the prices a utility names, 0 where it names none: start_prices' `c` (entries of the utility table start at the price at which
    they would not trade, u'(0)) -- the anchors of pool_prices for solve(nu0="pools")"""
    c = util.c
    if _is_general(util):
        c = c.copy()
        lg, qd = util.ctype == ULOG, util.ctype == UQUAD
        with np.errstate(divide="ignore"):
            c[lg] = np.where(util.h[lg] > 0, util.c[lg] / np.where(util.h[lg] > 0, util.h[lg], 1.0), 0.0)
        c[qd] = util.c[qd]
    return np.where(c > 0, c, 0.0)


def pool_relations(net):
    """(eu, ev, lr) of EVERY pool at the network's current reserves, fees and weights: log p_eu - log p_ev = lr, one relation per
    two-asset pool (ia, ib), k - 1 per k-asset pool (leg j against leg 0), in bucket order.  _price_relations' formulas at stride 1;
    reads and writes none of its caches"""
    eu, ev, elr = [], [], []
    for key in KIND2:
        if key not in net:
            continue
        b = net[key]
        Ra, Rb = b["Ra"], b["Rb"]
        if key == "cp2":
            lr = np.log(Rb / Ra)
        elif key == "w2":
            lr = np.log(b["wa"] * Rb / ((1 - b["wa"]) * Ra))
        elif key == "sum2":
            lr = np.zeros(len(Ra))
        elif key == "pow2":
            lr = b["t"] * np.log(Rb / Ra)
        else:
            lr = np.log((1 + b["alpha"] / (Ra * Ra * Rb)) / (1 + b["alpha"] / (Ra * Rb * Rb)))
        eu.append(b["ia"]); ev.append(b["ib"]); elr.append(lr)
    for k, b in net.get("gn", {}).items():
        for j in range(1, k):
            eu.append(b["idx"][j]); ev.append(b["idx"][0])
            elr.append(np.log(b["w"][j] * b["R"][0] / (b["w"][0] * b["R"][j])))
    for (kind, k), b in net.get("gk", {}).items():
        R = b["R"]
        lm = np.log1p((b["param"] / np.prod(R, axis=0))[None, :] / R) if kind == "stable" else np.zeros_like(R)
        for j in range(1, k):
            eu.append(b["idx"][j]); ev.append(b["idx"][0]); elr.append(lm[j] - lm[0])
    if not eu:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(eu).astype(np.int64), np.concatenate(ev).astype(np.int64), np.concatenate(elr).astype(np.float64)


def pool_prices(net, anchor=None):
    """The prices the pools imply (docs/pool_prices.md; the pure NumPy twin of cfmm_pool_prices).  phi minimises
    sum (phi_u - phi_v - lr)^2 over every pool's relations (unit weights, no thinning): L phi = rhs on the multigraph Laplacian by
    Jacobi-preconditioned conjugate gradients from zero, stopped at max |r| <= 1e-12 max |rhs| or after 4 n + 100 iterations, then
    zero mean per connected component.  anchor[j] > 0: a known price.  A component with anchored tokens gets log p = phi + off, off
    the mean of log anchor - phi over them in token order, and its anchored tokens come back as given; one without returns exp(phi).
    Returns (prices, info): info has cfmm_prices_info's fields, and phi (gauged) and comp (labels 0.., numbered by first token)."""
    n = int(net["n_tokens"])
    eu, ev, lr = pool_relations(net)
    if anchor is not None:
        anchor = np.asarray(anchor, dtype=np.float64)
        if anchor.shape != (n,) or not np.all(np.isfinite(anchor) & (anchor >= 0)):
            raise ValueError("pool_prices: anchor holds n entries, each 0 (unknown) or a positive finite price")
    deg = (np.bincount(eu, minlength=n) + np.bincount(ev, minlength=n)).astype(np.float64)
    label = np.arange(n)
    while len(eu):                                            # min-label propagation with pointer jumping
        new = label.copy()
        np.minimum.at(new, eu, label[ev])
        np.minimum.at(new, ev, label[eu])
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    comp = np.unique(label, return_inverse=True)[1].astype(np.int32)       # (labels are first tokens: ascending labels = by first token)
    nc = int(comp.max()) + 1 if n else 0

    def adj(x):
        return np.bincount(eu, weights=x[ev], minlength=n) + np.bincount(ev, weights=x[eu], minlength=n)
    rhs = np.bincount(eu, weights=lr, minlength=n) - np.bincount(ev, weights=lr, minlength=n)
    dinv = 1.0 / np.maximum(deg, 1.0)
    phi = np.zeros(n)
    r = rhs.copy()
    pdir = dinv * r
    rz = float(r @ pdir)
    rhs_max = float(np.abs(rhs).max()) if n else 0.0
    stop = 1e-12 * max(rhs_max, 1e-300)
    it, status = 0, 0
    rmax = rhs_max
    while rmax > stop:
        if it >= 4 * n + 100:
            status = 1
            break
        q = deg * pdir - adj(pdir)
        pq = float(pdir @ q)
        if not pq > 0.0:
            status = 1
            break
        alpha = rz / pq
        phi += alpha * pdir
        r -= alpha * q
        z = dinv * r
        rz_new = float(r @ z)
        rmax = float(np.abs(r).max())
        pdir = z + (rz_new / rz) * pdir
        rz = rz_new
        it += 1
    cnt = np.bincount(comp, minlength=nc)
    phi = phi - (np.bincount(comp, weights=phi, minlength=nc) / cnt)[comp]
    known = anchor > 0 if anchor is not None else np.zeros(n, dtype=bool)
    ka = np.bincount(comp[known], minlength=nc)
    off = np.zeros(nc)
    if known.any():
        off = np.bincount(comp[known], weights=(np.log(anchor[known]) - phi[known]), minlength=nc) / np.maximum(ka, 1)
    prices = np.exp(phi + off[comp])
    if known.any():
        prices[known] = anchor[known]
    mis = phi[eu] - phi[ev] - lr
    info = dict(relations=int(len(eu)), components=nc, components_anchored=int((ka > 0).sum()), tokens_unlisted=int((deg == 0).sum()),
                iterations=it, status=status, residual=(rmax / rhs_max if rhs_max > 0 else 0.0),
                misfit_max=float(np.abs(mis).max()) if len(mis) else 0.0, misfit_ss=float(mis @ mis), phi=phi, comp=comp)
    return prices, info


# ------------------------------------------------------------------------------- ties (kinks)
class _Ties:
    """Weighted union-find over tokens: log nu_j = s[group(j)] + off[j]."""

    def __init__(self, n):
        self.parent = np.arange(n)
        self.off = np.zeros(n)           # log nu_j - log nu_root(j)

    def find(self, j):
        path = []
        while self.parent[j] != j:
            path.append(j); j = self.parent[j]
        root = j
        # compress, accumulating offsets from the top of the path down
        for node in reversed(path):
            p = self.parent[node]
            if p != root:
                self.off[node] += self.off[p]
            self.parent[node] = root
        return root

    def tie(self, a, b, delta):
        """impose log nu_a - log nu_b = delta; False if it contradicts existing ties"""
        ra, rb = self.find(a), self.find(b)
        if ra == rb:
            return abs((self.off[a] - self.off[b]) - delta) < 1e-12
        # attach ra under rb: off[ra] = log nu_ra - log nu_rb
        self.off[ra] = delta + self.off[b] - self.off[a]
        self.parent[ra] = rb
        return True

    def groups(self):
        n = len(self.parent)
        roots = np.array([self.find(j) for j in range(n)])
        uniq, grp = np.unique(roots, return_inverse=True)
        return grp.astype(np.int32), self.off.copy(), len(uniq)


# ------------------------------------------------------------------------------- pool-sharded agreement
class HostComm:
    """The host-side agreement a pool-sharded solve needs (cfmm.distributed): every decision that changes the
    number or order of device collectives -- start prices, which method runs, which constant-sum pools are tied --
    must be the SAME on every rank, so it is taken on global quantities exchanged here.  Tiny and off the hot path
    (a few n-vectors per solve); wraps an initialised torch.distributed (nccl on the GPUs, gloo in the CPU tests)."""

    def __init__(self, dist):
        self.dist = dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        import torch
        self._torch = torch
        self._dev = "cuda" if dist.get_backend() == "nccl" else "cpu"

    def _t(self, a):
        return self._torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy()).to(self._dev)

    def broadcast(self, a, src=0):
        t = self._t(a)
        self.dist.broadcast(t, src=src)
        return t.cpu().numpy()

    def allreduce_sum(self, a):
        t = self._t(a)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return t.cpu().numpy()

    def allgather(self, obj):
        box = [None] * self.world
        self.dist.all_gather_object(box, obj)
        return box

    def assert_identical(self, a, what):
        """every rank must hold bit-identical `a` (different prices on different ranks would make the all-reduced
        psi a sum of shards evaluated at different points: silently wrong, or a hang)"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        t = self._t(np.concatenate([a, -a]))
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        mx = t.cpu().numpy()
        if not (np.array_equal(mx[:len(a)], a) and np.array_equal(-mx[len(a):], a)):
            raise CfmmError(f"pool-sharded solve: {what} differ between ranks")


# ------------------------------------------------------------------------------- Problem
AUTO_NEWTON_MIN_STABLE = 4096      # include/cfmm.h: CFMM_AUTO_NEWTON_MIN_STABLE
# solve_many's default (batch=None) over networks with curve2 / pow2 / table stableswap pools: the batched path or the clone path.
# Opt-in until tools/batch_timing.py --mix has shown the batched path faster (see the solve_many docstring).
BATCH_SEARCH_POOLS_BY_DEFAULT = False


def _drain_leg(code):
    """the leg a K-asset drain record flags, from the last field of its key: j itself, or 200 + 10 t + j for the record of the SAME leg paid
    for by another of the pool's cheapest tokens (leg t): Problem._split_payers"""
    return code if code < 100 else (code - 200) % 10


class Problem:
    """Drop-in for the reference's `prob = cp.Problem(obj, cons); prob.solve()`.

        p = Problem(n_tokens, local_indices, reserves, fees, kinds, weights, utility=Arbitrage(mv))
        p.solve()            # -> objective value (what arbitrage.py:84 prints)
        p.value, p.status, p.psi, p.deltas[i], p.lambdas[i], p.nu, p.gap, p.stats
    """

    def __init__(self, n_tokens, local_indices=None, reserves=None, fees=None, kinds=None, weights=None,
                 params=None, utility=None, device=0, network=None, deterministic=False):
        self.n = int(n_tokens)
        if network is not None:
            self.net, self.where = network, None
        else:
            self.net, self.where = pack(self.n, local_indices, reserves, fees, kinds, weights, params)
        self.m = network_pool_count(self.net)
        self.utility = utility
        self.device = device
        self.deterministic = bool(deterministic)      # bitwise-reproducible psi (include/cfmm.h: cfmm_set_deterministic)
        self.ctx = None
        self._uploaded = False
        self.value = None; self.status = None; self.psi = None; self.nu = None
        self._held_route = None            # hold_route: where the held route is kept, with psi and value of that moment
        self.gap = None; self.infeas = None; self.dual_value = None; self.stats = None
        self._theta = {}
        self._trade_cache = None
        self.audit_report = None       # the report of the last solve(audit=True)
        self._comm = None              # (n_ranks, rank) once the library's RCCL communicator is up
        self._host = None              # HostComm of a pool-sharded problem (cfmm.distributed.sharded_problem)
        self._dev_utility = None       # the Utility object whose data sits on the device
        self._dev_ties = False         # price ties / pool flags are set on the device

    @classmethod
    def from_network(cls, net, utility=None, device=0, deterministic=False):
        return cls(net["n_tokens"], utility=utility, device=device, network=net, deterministic=deterministic)

    def clone(self, utility=None):
        """A Problem over the SAME pools -- they stay where they are in HBM, nothing is uploaded again --
        with its own utility, prices and solver state (cfmm_clone).  Clones may be solved concurrently from
        different host threads: `solve_many`."""
        ctx = self._ensure_ctx()
        q = Problem(self.n, utility=utility if utility is not None else self.utility, device=self.device, network=self.net,
                    deterministic=self.deterministic)        # (cfmm_clone hands the mode on to the new context)
        q.where = self.where
        q.ctx = ctx.clone()
        q._uploaded = True
        return q

    def solve_many(self, utilities, concurrency=2, nu0s=None, warm_start=False, batch=None, **kw):
        """Solve the same pools under many utilities (the two-asset.py:34-100 sweep; independent baskets).  Returns one
        dict per utility, in order: value, status, psi, nu, gap, infeas, stats.

        Batched (first-order method, no constant-sum pools, linear-plus-box utilities, one GPU: `_batch_applies`):
        `batch` solves at a time (default: as many as the LDS tile takes, 8 up to ~1100 tokens) run in lock-step through
        cfmm_solve_batch -- every outer iteration reads every pool column once for all of them.  With warm_start the
        solves of one group start from the prices the same slot reached in the previous group.
        Networks with curve2 / pow2 pools or stableswap buckets of the K-asset table are taken too, under method="lbfgs" and
        under "auto" below AUTO_NEWTON_MIN_STABLE stableswap pools (from there on "auto" means the second-order method: an
        explicit `batch=` raises); under "auto" a member that ends without its certificates is re-solved alone, which hands it on
        to the second-order method as `solve` does.  For these networks the batched path is opt-in (`batch=8`): it has not yet
        been measured against the clone path (tools/batch_timing.py --mix), and becomes the default
        (BATCH_SEARCH_POOLS_BY_DEFAULT) only once it is shown faster; batch=None keeps them on the clone path until then.
        Otherwise (`batch=0`, or a network the batched path does not take): `concurrency` clones work through the list
        from as many host threads."""
        utilities = list(utilities)
        ctx = self._ensure_ctx()
        if batch is None and nu0s is None and self._sweep_applies(ctx, utilities, kw):
            # (the test above mirrors the library's own -- tile sizes, the one-workgroup path switched on -- and cannot know a build or
            #  an environment that differs, CFMM_TINY=0, another WT_LIGHT: a library that declines falls through to the paths below
            #  instead of failing a call they would serve; ADVICE r5.  warm_start and concurrency mean nothing to the one-call sweep.)
            try:
                return self._solve_sweep(utilities, **kw)
            except CfmmError as e:
                if getattr(e, "code", None) != _lib.E_UNSUPPORTED:
                    raise
        can_batch = hasattr(ctx, "solve_batch") and self._batch_applies(utilities, kw)
        if batch is None:
            batch = ctx.batch_capacity() if can_batch and (BATCH_SEARCH_POOLS_BY_DEFAULT or not self._search_pools()) else 0
        if batch and not can_batch:
            raise ValueError("solve_many(batch=...): the batched path takes first-order solves of networks without constant-sum pools on "
                             "one GPU (method=\"auto\" means first order below AUTO_NEWTON_MIN_STABLE stableswap pools)")
        if batch:
            return self._solve_batched(utilities, int(batch), nu0s, warm_start, **kw)
        import threading
        workers = [self] + [self.clone() for _ in range(max(1, int(concurrency)) - 1)]
        results = [None] * len(utilities)
        errors = []
        lock = threading.Lock()
        nxt = [0]

        def run(p):
            try:
                first = True
                while True:
                    with lock:
                        i = nxt[0]; nxt[0] += 1
                    if i >= len(utilities):
                        return
                    p.set_utility(utilities[i])
                    p.solve(nu0=None if nu0s is None else nu0s[i], warm_start=warm_start and not first, **kw)
                    first = False
                    results[i] = p._result()
            except Exception as e:       # surfaced in the caller's thread
                errors.append(e)

        threads = [threading.Thread(target=run, args=(p,)) for p in workers]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for p in workers[1:]:
            p.close()
        if errors:
            raise errors[0]
        return results

    def _stable_count(self):
        """stableswap pools as `solve` counts them for method="auto": curve2 plus the table's stableswap buckets"""
        return ((len(self.net["curve2"]["Ra"]) if "curve2" in self.net else 0)
                + sum(b["R"].shape[1] for (kd, _), b in self.net.get("gk", {}).items() if kd == "stable"))

    def _search_pools(self):
        """the network holds pools whose subproblem is a root search: curve2, pow2, the table's stableswap buckets"""
        return "curve2" in self.net or "pow2" in self.net or any(kd == "stable" for kd, _ in self.net.get("gk", {}))

    def _batch_applies(self, utilities, kw):
        """Does cfmm_solve_batch take these solves?  Reads the network, the utilities and the options only (no device).
        Constant-sum pools (sum2 and the table's ("sum", k) buckets) stay out: their kinks need the tie loop.  curve2, pow2 and
        ("stable", k) buckets ride along under method="lbfgs", and under "auto" while the stableswap count is below
        AUTO_NEWTON_MIN_STABLE -- from there on "auto" means the second-order method, which is not batched."""
        if "sum2" in self.net or any(kd == "sum" for kd, _ in self.net.get("gk", {})):
            return False
        if self._host is not None or self.deterministic or any(_is_general(x) for x in utilities):
            return False
        method = kw.get("method", "auto")
        if method == "lbfgs":
            return True
        return method == "auto" and (not self._search_pools() or self._stable_count() < AUTO_NEWTON_MIN_STABLE)

    # -- the reference's own sweep (two-asset.py:34-100): tiny networks, constant-sum pools included, one library call --------
    _WT = dict(cp2=128, sum2=128, w2=64)               # pools per wave-tile (csrc/kernels.hpp: wave_tile_pools)

    def _sweep_applies(self, ctx, utilities, kw):
        """cfmm_solve_sweep serves what ONE workgroup evaluates: <= 64 tokens, <= 64 wave-tiles, linear-box utilities, first-order
        method, one GPU (csrc/tiny.hpp)"""
        if not hasattr(ctx, "solve_sweep") or self._host is not None or self.deterministic or self.n > 64 or not utilities:
            return False
        if kw.get("method", "auto") not in ("auto", "lbfgs") or any(k in self.net for k in ("curve2", "pow2", "gk")):
            return False
        if set(kw) - {"tol", "max_evals", "memory", "method", "kink_tol", "max_rounds"}:
            return False
        tiles = sum(-(-len(self.net[k]["Ra"]) // wt) for k, wt in self._WT.items() if k in self.net)
        tiles += sum(-(-b["R"].shape[1] // (64 // k)) for k, b in self.net.get("gn", {}).items())
        return 1 <= tiles <= 64 and not any(_is_general(u) for u in utilities)

    def _trade_layout(self):
        """(key, legs, pools, offset) of every non-empty bucket in cfmm_solve_sweep's tender layout, and the doubles per point"""
        lay, off = [], 0
        for key in KIND2:                                # (dict order = kind order 0..4)
            if key in self.net and len(self.net[key]["Ra"]):
                m = len(self.net[key]["Ra"]); lay.append((key, 2, m, off)); off += 4 * m
        for k in sorted(self.net.get("gn", {})):
            m = self.net["gn"][k]["R"].shape[1]
            if m:
                lay.append((k, k, m, off)); off += 2 * k * m
        return lay, off

    def _solve_sweep(self, utilities, tol=1e-6, max_evals=2000, memory=0, method="auto", kink_tol=1e-3, max_rounds=6):
        ctx = self._ensure_ctx()
        n, B = self.n, len(utilities)
        C_ = np.stack([u.c for u in utilities]); H = np.stack([u.h for u in utilities]); CT = np.stack([u.ctype for u in utilities]).astype(np.int32)
        # start prices: a function of the pools and of c alone (problem.py: start_prices) -- the points of a sweep mostly share c
        memo, NU0 = {}, np.empty((B, n))
        for b, u in enumerate(utilities):
            key = u.c.tobytes()
            if key not in memo:
                memo[key] = start_prices(self.net, u)
            NU0[b] = memo[key]
        lay, T = self._trade_layout()
        s2 = self.net.get("sum2")
        nu, psi, theta, tsgn, trades, sts, rounds = ctx.solve_sweep(C_, H, CT, NU0, s2, T, kink_tol, max_rounds, tol=tol, max_evals=max_evals,
                                                                    memory=memory, method=_lib.METHODS["lbfgs"])
        # fills of the pools that ended tied on their kink: psi_total = psi + sum theta d, their tenders = theta x the full fill
        tied = np.isfinite(theta) if s2 is not None else None
        if s2 is not None and tied.any():
            m2 = len(s2["Ra"])
            ya = np.where(tsgn > 0, -s2["Rb"] / s2["fee"], s2["Ra"]) * np.where(tied, theta, 0.0)      # [B][m2]: the pool's first token
            yb = np.where(tsgn > 0, s2["Rb"], -s2["Ra"] / s2["fee"]) * np.where(tied, theta, 0.0)      #          its second
            psi = psi.copy()
            np.add.at(psi, (np.arange(B)[:, None], s2["ia"][None, :]), ya)
            np.add.at(psi, (np.arange(B)[:, None], s2["ib"][None, :]), yb)
        # certificates, as Problem._finish computes them, for all points at once
        r = psi + H
        value = (C_ * psi).sum(axis=1)
        cs = ((nu - C_) * r).sum(axis=1)
        dual = ((nu - C_) * H).sum(axis=1) + (nu * psi).sum(axis=1)
        gap = np.abs(cs) / np.maximum(1.0, np.abs(dual))
        viol = np.where(CT == GE, np.maximum(-r, 0.0), np.where(CT == EQ, np.abs(r), 0.0)).max(axis=1)
        scale = np.maximum(np.maximum(np.abs(psi).max(axis=1), np.abs(H).max(axis=1)), max(1e-12 * self._max_reserve(), 1e-300))
        infeas = viol / scale
        tolx = max(tol, 1e-12) * (1 + 1e-6) + 1e-15
        good = (gap <= tolx) & (infeas <= tolx)
        collapsed = ((CT == EQ) & (H > 0) & ~self._listed_tokens()[None, :]).any(axis=1)      # (a token that must be sold and that no pool lists: _finish)
        results = []
        for b in range(B):
            st = sts[b]
            status = "optimal" if good[b] else ("infeasible" if collapsed[b] else
                                                 ("inaccurate" if st["status"] == 1 else _lib.STATUS.get(st["status"], f"error {st['status']}")))
            st.update(rounds=int(rounds[b]), batch=B, pool_subproblems=st["evals"] * self.m)
            res = dict(value=float(value[b]), status=status, psi=psi[b], nu=nu[b], gap=float(gap[b]), infeas=float(infeas[b]),
                       dual_value=float(dual[b]), stats=st)
            if trades is not None:
                tr = {}
                for key, k, m, off in lay:
                    blk = trades[b, off:off + 2 * k * m].reshape(2, k, m)
                    tr[key] = (blk[0], blk[1])
                if s2 is not None and tied[b].any():
                    d, l = tr["sum2"]
                    for i in np.flatnonzero(tied[b]):
                        y = np.array([ya[b, i], yb[b, i]])
                        d[:, i] = np.maximum(-y, 0.0); l[:, i] = np.maximum(y, 0.0)
                res["trades"] = tr
            results.append(res)
        # a point the sweep did not bring to its certificates takes the one-at-a-time path, second-order fall-back included
        if method == "auto":
            for b in np.flatnonzero(~good):
                self.set_utility(utilities[b])
                self.solve(tol=tol, max_evals=max_evals, memory=memory, kink_tol=kink_tol, max_rounds=max_rounds)
                res = self._result()
                res["trades"] = {k: v for k, v in self._trades().items()}
                results[int(b)] = res
        return results

    def tenders_of(self, result):
        """(deltas, lambdas) per pool, in the order of the pool list, of one result of a swept solve_many (two-asset.py:94,98)"""
        if self.where is None:
            raise CfmmError("per-pool lists need a Problem built from pool lists")
        tr = result["trades"]
        return ([tr[key][0][:, pos].copy() for key, pos in self.where], [tr[key][1][:, pos].copy() for key, pos in self.where])

    def _result(self):
        return dict(value=self.value, status=self.status, psi=self.psi, nu=self.nu, gap=self.gap, infeas=self.infeas,
                    dual_value=self.dual_value, stats=self.stats)

    def _solve_batched(self, utilities, batch, nu0s, warm_start, tol=1e-6, max_evals=2000, memory=0, method="auto", **kw):
        if kw:
            raise TypeError(f"solve_many: unknown option(s) {sorted(kw)}")
        ctx = self._ensure_ctx()
        batch = max(1, min(batch, ctx.batch_capacity(), len(utilities) or 1))
        workers = getattr(self, "_batch_workers", None) or [self]
        while len(workers) < batch:
            workers.append(self.clone())
        self._batch_workers = workers          # (kept: the next sweep over these pools reuses the clones' state buffers)
        results = []
        for g0 in range(0, len(utilities), batch):
            group = utilities[g0:g0 + batch]
            ws = workers[:len(group)]
            starts = []
            for k, (p, u) in enumerate(zip(ws, group)):
                p.utility = u
                p.ctx.set_utility(u.c, u.h, u.ctype)
                p._dev_utility = u
                p._theta = {}; p._trade_cache = None; p._tol = tol
                given = None if nu0s is None else nu0s[g0 + k]
                if given is not None:
                    starts.append(given)
                elif warm_start and p.nu is not None:
                    starts.append(p.nu)
                else:
                    starts.append(start_prices(self.net, u))
            sts = ws[0].ctx.solve_batch([p.ctx for p in ws[1:]], starts, tol=tol, max_evals=max_evals, memory=memory,
                                        method=_lib.METHODS["lbfgs"])
            for p, st in zip(ws, sts):
                nu, psi = p.ctx.get_solution()
                total = dict(evals=st["evals"], iters=st["iters"], wall_seconds=st["wall_seconds"], device_seconds=st["device_seconds"],
                             rounds=1, batch=len(group))
                p._finish(st, nu, psi, total)
                if method == "auto" and p.status != "optimal" and self._search_pools():
                    # what `solve` does for such a network: hand the member on to the second-order method, from where it stands
                    p.solve(tol=tol, max_evals=max_evals, memory=memory, warm_start=True, method="auto")
                    p.stats["batch"] = len(group)
                results.append(p._result())
        return results

    # -- device plumbing ---------------------------------------------------------------------
    def _ensure_ctx(self):
        if self.ctx is None:
            self.ctx = _lib.Context(self.n, self.device)      # raises without HIP lib / gfx950
            if self.deterministic:
                self.ctx.set_deterministic(True)
        if not self._uploaded:
            for key, kind in KIND2.items():
                if key in self.net:
                    b = self.net[key]
                    param = b.get(PARAM2[key]) if PARAM2[key] else None
                    self.ctx.upload_pools2(kind, b["Ra"], b["Rb"], b["fee"], b["ia"], b["ib"], param)
            for k, b in self.net.get("gn", {}).items():
                self.ctx.upload_poolsN(b["idx"], b["R"], b["w"], b["fee"])
            for (kind, k), b in self.net.get("gk", {}).items():       # the K-asset table's buckets (csrc/phik.hpp)
                self.ctx.upload_poolsG(_lib.POOLK[kind], b["idx"], b["R"], b["fee"], b["param"] if kind == "stable" else None)
            self._uploaded = True
        return self.ctx

    def set_utility(self, utility):
        self.utility = utility       # (a new object, or the same object mutated: call this to re-send it)
        self._dev_utility = None
        for attr in ("_all_priced", "_plain", "_start_memo", "_general"):        # (what was derived from its arrays)
            try:
                setattr(utility, attr, None)
            except AttributeError:
                pass

    def _send_utility(self):
        """the device-side utility is re-sent only when it changed (each call is a synchronisation).  Everything that
        runs a solve on the raw context (Problem.solve, cfmm.distributed.attach_oneshot_checked) goes through here:
        cfmm_solve refuses a context that never received a utility (CFMM_E_STATE)."""
        if self.utility is None:
            raise ValueError("no utility set")
        ctx = self._ensure_ctx()
        u = self.utility
        if self._dev_utility is not u:
            if self._host:
                # the utility is replicated: every rank must hold the same one (checked when it is sent to the device, once
                # per utility object -- the host-side collectives of a solve are off its steady-state path)
                self._host.assert_identical(np.concatenate([u.c, u.h, u.ctype.astype(np.float64)]), "the utilities")
            ctx.set_utility(u.c, u.h, u.ctype)
            self._dev_utility = u

    def init_comm(self, n_ranks, rank, uid):
        """pool-sharding: this process holds one shard; see cfmm.distributed"""
        self._ensure_ctx().comm_init(n_ranks, rank, uid)
        self._comm = (n_ranks, rank)

    def eval_dual(self, nu, want_diag=False):
        return self._ensure_ctx().eval_dual(nu, want_diag)

    # -- in-place updates (include/cfmm.h: cfmm_update_pools*) ---------------------------------
    def update_reserves(self, pools, reserves, params=None):
        """New reserves of some pools, written into the resident columns in place (nothing else is uploaded again): `pools` index the
        pool list the Problem was built from, reserves[i] is the new reserve vector of pools[i], params[i] the new alpha / t of a
        curve / power-sum pool (None: unchanged).  Fees and weights have their own calls (update_fees, update_weights); token ids
        stay (changing them, or adding / removing pools, is a new Problem).  The per-block loop of a router:

            p.solve()
            for block in blocks:
                p.update_reserves(block.pools, block.reserves)
                p.solve(warm_start=True)          # from the prices of the previous block
        """
        if self.where is None:
            raise CfmmError("update_reserves needs a Problem built from pool lists; use update_bucket()")
        for key, (pos, R, param) in route_updates(self.net, self.where, pools, reserves, params).items():
            self.update_bucket(key, pos, R, param)

    def update_bucket(self, key, positions, R, param=None):
        """New reserves R ([k][count], slot-major; k = 2 for the two-asset buckets) of the pools `positions` of one bucket (`key` as
        bucket_trades takes it: 'cp2' .. 'pow2', a size k, ('stable' | 'sum', k)), and of its parameter where it has one (None:
        unchanged), in place on the device and in self.net (shared with this Problem's clones, which notice the change too).  A
        pool-sharded Problem takes positions local to its rank's shard, and every rank makes the call for every bucket any rank updates
        (empty `positions` where its slice is untouched): shard_updates(m, rank, world, global_positions, R, param) picks a rank's part
        of an update given over the whole bucket of m pools."""
        b, fam = _bucket_of(self.net, key)
        pos = np.ascontiguousarray(positions, dtype=np.int64).ravel()
        m = len(b["Ra"]) if fam == "two" else b["R"].shape[1]
        k = 2 if fam == "two" else b["R"].shape[0]
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.ndim == 1 and len(pos) == 0:
            R = R.reshape(k, 0)
        if R.shape != (k, len(pos)):
            raise ValueError(f"bucket {key!r}: reserves of shape {R.shape}, expected ({k}, {len(pos)})")
        if len(pos) and (pos.min() < 0 or pos.max() >= m):
            raise ValueError(f"bucket {key!r}: a position outside [0, {m})")
        if len(np.unique(pos)) != len(pos):
            raise ValueError(f"bucket {key!r}: a position is named twice")
        if not np.all(np.isfinite(R)) or not np.all(R > 0):
            raise ValueError(f"bucket {key!r}: reserves must be > 0 and finite")
        cur = _bucket_param(self.net, key)
        if param is not None:
            param = np.ascontiguousarray(param, dtype=np.float64).ravel()
            if cur is None or (fam == "two" and key == "w2"):
                raise ValueError(f"bucket {key!r}: no parameter to update")
            if len(param) != len(pos):
                raise ValueError(f"bucket {key!r}: {len(pos)} positions but {len(param)} parameters")
            for i, x in zip(pos, param):
                msg = _param_rule(key[0] if isinstance(key, tuple) else key, int(i), x)
                if msg:
                    raise ValueError(msg)
        if self.ctx is not None and self._uploaded:
            p32 = pos.astype(np.int32)
            if fam == "two":
                self.ctx.update_pools2(KIND2[key], p32, R[0], R[1], param)
            elif fam == "gn":
                self.ctx.update_poolsN(p32, R)
            else:
                self.ctx.update_poolsG(_lib.POOLK[key[0]], p32, R, param)
        if fam == "two":
            b["Ra"][pos] = R[0]; b["Rb"][pos] = R[1]
        else:
            b["R"][:, pos] = R
        if param is not None:
            cur[pos] = param
        self._reserves_changed()

    # -- in-place updates of fees and weights (include/cfmm.h: cfmm_update_terms*) --------------
    def update_fees(self, pools, fees):
        """New fees of some pools (dynamic-fee pools), in place: `pools` index the pool list the Problem was built from."""
        if self.where is None:
            raise CfmmError("update_fees needs a Problem built from pool lists; use update_bucket_terms()")
        for key, (pos, fee, w) in route_terms(self.net, self.where, pools, fees=fees).items():
            self.update_bucket_terms(key, pos, fee, w)

    def update_weights(self, pools, weights):
        """New geo-mean exponents of some pools (liquidity-bootstrapping pools), in place; normalised as pack() does.  A two-asset pool
        with equal weights lives in the constant-product bucket and has no weight column: giving it unequal weights is a new Problem."""
        if self.where is None:
            raise CfmmError("update_weights needs a Problem built from pool lists; use update_bucket_terms()")
        for key, (pos, fee, w) in route_terms(self.net, self.where, pools, weights=weights).items():
            self.update_bucket_terms(key, pos, fee, w)

    def update_bucket_terms(self, key, positions, fee=None, w=None):
        """New fees ([count], each in (0, 1]; None: unchanged) and / or weights (None: unchanged; [k][count] slot-major for a geo-mean
        bucket, the first token's weight wa [count] for 'w2', each in (0, 1) and NOT normalised here: update_weights does that) of the
        pools `positions` of one bucket, in place on the device and in self.net -- update_bucket's keys, sharing and pool-sharded rule
        (local positions, every rank calls; shard_terms picks a rank's part)."""
        b, fam = _bucket_of(self.net, key)
        pos = np.ascontiguousarray(positions, dtype=np.int64).ravel()
        m = len(b["Ra"]) if fam == "two" else b["R"].shape[1]
        if len(pos) and (pos.min() < 0 or pos.max() >= m):
            raise ValueError(f"bucket {key!r}: a position outside [0, {m})")
        if len(np.unique(pos)) != len(pos):
            raise ValueError(f"bucket {key!r}: a position is named twice")
        if fee is None and w is None and len(pos):
            raise ValueError(f"bucket {key!r}: neither fees nor weights given")
        if fee is not None:
            fee = np.ascontiguousarray(fee, dtype=np.float64).ravel()
            if len(fee) != len(pos):
                raise ValueError(f"bucket {key!r}: {len(pos)} positions but {len(fee)} fees")
            if not np.all((fee > 0) & (fee <= 1)):
                raise ValueError(f"bucket {key!r}: the fee must be in (0, 1]")
        if w is not None:
            if key != "w2" and fam != "gn":
                raise ValueError(f"bucket {key!r}: no weights to update" + (" (unequal weights for a constant-product pool are a re-upload)" if key == "cp2" else ""))
            w = np.ascontiguousarray(w, dtype=np.float64)
            shape = (len(pos),) if key == "w2" else (b["R"].shape[0], len(pos))
            if w.size == 0 and len(pos) == 0:
                w = w.reshape(shape)
            if w.shape != shape:
                raise ValueError(f"bucket {key!r}: weights of shape {w.shape}, expected {shape}")
            if not np.all((w > 0) & (w < 1)):
                raise ValueError(f"bucket {key!r}: weights must be in (0, 1)")
        if self.ctx is not None and self._uploaded:
            call = getattr(self.ctx, {"two": "update_terms2", "gn": "update_termsN", "gk": "update_termsG"}[fam], None)
            if call is None:
                raise CfmmError(f"this context ({getattr(self.ctx, 'backend', type(self.ctx).__name__)}) has no in-place update of fees and weights "
                                "(cfmm_update_terms*): build a new Problem")
            p32 = pos.astype(np.int32)
            if fam == "two":
                call(KIND2[key], p32, fee, w)
            elif fam == "gn":
                call(int(key), p32, fee, w)
            else:
                call(_lib.POOLK[key[0]], key[1], p32, fee)
        if fee is not None:
            b["fee"][pos] = fee
        if w is not None:
            if key == "w2":
                b["wa"][pos] = w
            else:
                b["w"][:, pos] = w
        self._reserves_changed()         # (the start-price relations, the kink fills and the trade cache depend on fees and weights too)

    def _reserves_changed(self):
        """what was derived from the old reserves goes: start-price relations (and the start prices memoised on them), the largest
        reserve, the read-back caches -- of this Problem and of its clones, through the generation stamp on the network they share"""
        net = self._net
        for kk in ("_price_relations", "_potentials"):
            net.pop(kk, None)
        net["_generation"] = net.get("_generation", 0) + 1
        self._pools_seen()

    # -- the router's own trades applied to the pools (include/cfmm.h: cfmm_apply_trades; docs/apply_trades.md) -----------------
    @property
    def net(self):
        """the packed network; a host copy that apply_trades(sync_host=False) left behind the device is refreshed on first use"""
        n = self._net
        if n.get("_stale") and self.ctx is not None and self._uploaded and not self._hold_refresh:
            self._refresh_net()
        return n

    _hold_refresh = False          # inside solve(nu0="pools"): the solve reads the network's shape alone, the reserves stay on the device

    @net.setter
    def net(self, network):
        self._net = network

    def _apply_path(self):
        return apply_path(self._theta, self._dev_ties, self._host is not None or self._comm is not None)

    def bucket_reserves(self, key):
        """resident reserves [k][m] (slot-major, upload order; k = 2 for the two-asset buckets) of one bucket, read back from the device"""
        b, fam = _bucket_of(self._net, key)
        ctx = self._ensure_ctx()
        if fam == "two":
            return np.stack(ctx.get_reserves2(KIND2[key], len(b["Ra"])))
        if fam == "gn":
            return ctx.get_reservesN(int(key), b["R"].shape[1])
        return ctx.get_reservesG(_lib.POOLK[key[0]], key[1], b["R"].shape[1])

    def reserves(self):
        """{bucket key: resident reserves [k][m]} of every bucket, read back from the device (keys as bucket_trades takes them)"""
        net = self._net
        keys = [k for k in KIND2 if k in net] + list(net.get("gn", {})) + list(net.get("gk", {}))
        return {key: self.bucket_reserves(key) for key in keys}

    def _refresh_net(self):
        net = self._net
        net.pop("_stale", None)
        for key, R in self.reserves().items():
            b, fam = _bucket_of(net, key)
            if fam == "two":
                b["Ra"][:] = R[0]; b["Rb"][:] = R[1]
            else:
                b["R"][:] = R

    def apply_trades(self, fees="pool", sync_host=True):
        """Execute the route: every pool's tenders at the accepted prices (what deltas / lambdas / bucket_trades return now) are
        committed to the resident reserves, R' = (R + g delta) - lam with g = 1 (fees="pool": the fee stays in the pool) or the pool's
        gamma (fees="aside").  All or nothing: a pool that would be drained (a constant-sum pool traded at its vertex) raises ValueError
        and neither the device nor self.net changes.  Sequential orders, each seeing the pools as the previous one left them:

            for order in orders:
                p.set_utility(order); p.solve(warm_start=True); p.apply_trades()

        Without host-held fills, device ties or sharding the reserves move on the device (no host leg) and self.net is refreshed from
        there -- at once, or with sync_host=False on its first use; otherwise they are formed here from the tenders, fills included, and
        sent through update_bucket.  Returns the number of pools that moved."""
        if fees not in _lib.FEE_MODES:
            raise ValueError(f"fees {fees!r}: expected one of {sorted(_lib.FEE_MODES)}")
        ctx = self._ensure_ctx()
        self._pools_seen()
        if self._apply_path() == "device":
            rc, info = ctx.apply_trades(fees, check=False)
            if rc == _lib.E_UNSUPPORTED and info["pools_refused"] > 0:
                raise ValueError(ctx.L.cfmm_last_error(ctx.h).decode())
            ctx._chk(rc)
            self._net["_stale"] = True
            self._reserves_changed()
            self._rmax = float(info["max_reserve"])      # (the network's largest new reserve, exact: what _max_reserve would read back)
            if sync_host:
                self._refresh_net()
            return int(info["pools_moved"])
        net = self.net
        new = {}
        for key, (d, l) in self._trades().items():          # (every bucket is checked before the first write)
            b, fam = _bucket_of(net, key)
            R = np.stack([b["Ra"], b["Rb"]]) if fam == "two" else b["R"]
            Rn = post_trade_reserves(R, d, l, b["fee"], fees)
            bad = ~(np.isfinite(Rn) & (Rn > 0)).all(axis=0)
            if bad.any():
                raise ValueError(f"bucket {key!r}: pool {int(np.flatnonzero(bad)[0])} would be left with a reserve that is not positive and finite; nothing was changed")
            pos = np.flatnonzero(((d != 0) | (l != 0)).any(axis=0))
            new[key] = (pos, np.ascontiguousarray(Rn[:, pos]))
        sharded = self._host is not None or self._comm is not None
        for key, (pos, Rn) in new.items():
            if len(pos) or sharded:                          # (pool-sharded: every rank makes the call)
                self.update_bucket(key, pos, Rn)
        return int(sum(len(pos) for pos, _ in new.values()))

    def _pools_seen(self):
        """drop what was derived from reserves that an update through this Problem or a clone (they share self.net) has replaced"""
        g = self._net.get("_generation", 0)
        if getattr(self, "_net_generation", 0) != g:
            self._net_generation = g
            self._rmax = None
            self._theta = {}
            self._trade_cache = None

    # -- solve -------------------------------------------------------------------------------
    def solve(self, tol=1e-6, nu0=None, max_evals=2000, memory=0, iters_per_graph=8, kink_tol=1e-3,
              max_rounds=6, warm_start=False, method="auto", audit=False):
        """`method`: "lbfgs" (first order, on-device), "newton" (barrier-smoothed second order: the remedy for
        stableswap / constant-sum pools at scale; k-asset pools enter it unsmoothed) or "auto" (second order when the
        network holds stableswap pools; otherwise first order, with the host-side active-set loop for constant-sum
        kinks and the second-order method as its fall-back).
        `audit`: audit the route the solve ends on (Problem.audit, docs/audit.md) and keep the report as self.audit_report; a status of
        "optimal" becomes "inaccurate" when a pool refuses its tenders, a contribution falls outside the fixed point, or the audited
        psi disagrees with the reported one -- or misses the certificates -- beyond the solve's tolerance."""
        if isinstance(nu0, str) and nu0 != "pools":
            raise ValueError(f"nu0 {nu0!r}: start prices, None, or \"pools\" (fitted on the device to the resident pools, pool_prices)")
        # nu0="pools" on a host copy an apply left behind the device: nothing the solve reads of it but its shape, unless constant-sum
        # pools (whose kink loop reads the host's reserves) are present or the largest reserve is not known -- then it is refreshed as ever
        self._pools_seen()
        self._hold_refresh = (isinstance(nu0, str) and self._host is None and self._comm is None and bool(self._net.get("_stale"))
                              and getattr(self, "_rmax", None) is not None and "sum2" not in self._net
                              and not any(kd == "sum" for kd, _ in self._net.get("gk", {})))
        try:
            value = self._solve(tol, nu0, max_evals, memory, iters_per_graph, kink_tol, max_rounds, warm_start, method)
        finally:
            self._hold_refresh = False
        self.audit_report = None
        if audit and self.psi is not None and np.all(np.isfinite(self.psi)):
            rep = self.audit_report = self.audit()
            tolx = max(self._tol, 1e-12) * (1 + 1e-6) + 1e-15          # (_finish's bar)
            if self.status == "optimal" and (rep["pools_violating"] > 0 or rep["legs_out_of_range"] > 0
                                             or not (rep["psi_mismatch"] <= tolx and rep["infeas"] <= tolx and rep["gap"] <= tolx)):
                self.status = "inaccurate"
        return value

    def audit(self, tol_pool=AUDIT_TOL_POOL):
        """Does every pool accept the route this object hands out (deltas / lambdas / bucket_trades), and does it add up?  The report
        of cfmm_audit_trades (docs/audit.md) as a dict, with psi (summed exactly from the tenders alone), plus
          psi_mismatch   max |psi_audit - self.psi| / max(|psi_audit|_inf, 1e-12 max reserve)
          gap            |self.dual_value - value| / max(1, |self.dual_value|): the audited point against the solve's dual value
        On the device unless the pools are sharded or the tenders were repaired on the host (a worthless component taken out): then
        the NumPy twin (audit_trades) on the tenders read back.  Fills the Python kink loop holds (constant-sum pools tied on a kink)
        travel as the caller's own tenders."""
        ctx = self._ensure_ctx()
        self._pools_seen()
        if self.utility is not None:
            self._send_utility()
        if self._host is not None or self._comm is not None or (self.stats or {}).get("worthless_tokens"):
            exponent = None
            if self._host is not None:                 # the fixed-point exponent of the WHOLE network: the shards' integers then add
                import math
                mf = min([1.0] + [float(b["fee"].min()) for b in audit_buckets(self.net)])
                mf = float(min(self._host.allgather(mf)))
                exponent = 84 - math.frexp(max(self._max_reserve(), 1e-300) / max(mf, 1e-3))[1]
            rep = audit_trades(self.net, self._trades(), self.utility, tol_pool, exponent=exponent)
            rep = {k: v for k, v in rep.items() if k not in ("psi_int", "limbs", "slack")}
            rep["path"] = "host"
        else:
            own = None
            if self._theta:
                tr = self._trades()
                own = {key: tr[key] for key in tr if key == "sum2" or (isinstance(key, tuple) and key[0] == "sum")}
            rep = ctx.audit(own=own, tol_pool=tol_pool)
            rep["path"] = "device"
        psi = rep["psi"]
        if self.psi is not None:
            rep["psi_mismatch"] = float(np.abs(psi - self.psi).max()) / max(float(np.abs(psi).max()), 1e-12 * self._max_reserve(), 1e-300)
        else:
            rep["psi_mismatch"] = float("nan")
        dv = getattr(self, "dual_value", None)
        rep["gap"] = abs(dv - rep["value"]) / max(1.0, abs(dv)) if dv is not None else float("nan")
        return rep

    # -- the pools moved before the route landed (include/cfmm.h: cfmm_hold_route, cfmm_requote_route; docs/requote.md) -----------
    def _bucket_keys(self):
        net = self._net
        return [k for k in KIND2 if k in net] + list(net.get("gn", {})) + list(net.get("gk", {}))

    def hold_route(self):
        """Keep the route this object hands out now (deltas / lambdas / bucket_trades) through whatever happens to the pools next --
        update_reserves / update_fees / update_weights, apply_trades, another solve, through this Problem or a clone -- together with
        self.psi and self.value of this moment.  On the device (cfmm_hold_route: no tender crosses the host) unless fills are held in
        Python, ties sit on the device or the pools are sharded: then the tenders are kept here.  Returns the info record."""
        ctx = self._ensure_ctx()
        self._pools_seen()
        kept = dict(psi=None if self.psi is None else np.array(self.psi, copy=True), value=self.value)
        if self._apply_path() == "device":
            info = ctx.hold_route()
            kept["path"] = "device"
        else:
            tr = {key: (d.copy(), l.copy()) for key, (d, l) in self._trades().items()}
            kept.update(path="host", trades=tr)
            info = dict(pools=int(sum(d.shape[1] for d, _ in tr.values())),
                        pools_trading=int(sum(((d != 0) | (l != 0)).any(axis=0).sum() for d, l in tr.values())),
                        bytes=int(sum(d.nbytes + l.nbytes for d, l in tr.values())))
        self._held_route = kept
        return info

    def release_route(self):
        """let the held route go (a no-op without one)"""
        if self._held_route is not None and self._held_route["path"] == "device" and self.ctx is not None:
            self.ctx.release_route()
        self._held_route = None

    def held_trades(self):
        """{bucket key: (delta, lambda)} of the held route, read back from where it is kept"""
        kept = self._held_route
        if kept is None:
            raise CfmmError("no route is held (hold_route first)", code=_lib.E_STATE)
        if kept["path"] == "host":
            return kept["trades"]
        ctx, out = self._ensure_ctx(), {}
        for key in self._bucket_keys():
            b, fam = _bucket_of(self._net, key)
            if fam == "two":
                out[key] = ctx.held2(KIND2[key], len(b["Ra"]))
            elif fam == "gn":
                out[key] = ctx.heldN(int(key), b["R"].shape[1])
            else:
                out[key] = ctx.heldG(_lib.POOLK[key[0]], key[1], b["R"].shape[1])
        return out

    def requote(self, tol_scale=REQUOTE_TOL_SCALE):
        """What does the held route pay on the pools as they are NOW, which pools fall short, and is it still worth sending?  The
        report of cfmm_requote_route (docs/requote.md) as a dict with psi, plus
          shortfall    psi_held - psi: what the route delivers less (per token) than when it was quoted
          value_held   self.value at the hold
          scale        {bucket key: s [m]}: 1 = not trading, NaN = failed
          lambdas      the re-quoted outputs fl(s Lambda) -- in the order of self.lambdas for a Problem built from pool lists, else
                       {bucket key: [k][m]}; deltas: the inputs, the held ones unchanged, in the same order (self.deltas itself
                       follows the pools: once they have moved it hands out another route)
        On the device unless the route is held here (hold_route): then the NumPy twin (requote_route) on the reserves read back."""
        kept = self._held_route
        if kept is None:
            raise CfmmError("no route is held (hold_route first)", code=_lib.E_STATE)
        ctx = self._ensure_ctx()
        self._pools_seen()
        if self.utility is not None:
            self._send_utility()
        if kept["path"] == "host":
            net = dict(self._net)
            for key, R in self.reserves().items():
                b, fam = _bucket_of(self._net, key)
                nb = dict(b)
                if fam == "two":
                    nb["Ra"], nb["Rb"] = R[0], R[1]
                    net[key] = nb
                else:
                    nb["R"] = R
                    net["gn" if fam == "gn" else "gk"] = dict(net["gn" if fam == "gn" else "gk"])
                    net["gn" if fam == "gn" else "gk"][int(key) if fam == "gn" else key] = nb
            rep = requote_route(net, kept["trades"], self.utility, None, tol_scale)
            rep = {k: v for k, v in rep.items() if k not in ("psi_int", "limbs")}
            rep["path"] = "host"
            lam, held = rep["lambdas"], kept["trades"]
        else:
            rep = ctx.requote(tol_scale=tol_scale)
            rep["path"] = "device"
            held, scale, lam = self.held_trades(), {}, {}
            for key in self._bucket_keys():
                b, fam = _bucket_of(self._net, key)
                if fam == "two":
                    scale[key] = ctx.route_scale2(KIND2[key], len(b["Ra"]))
                elif fam == "gn":
                    scale[key] = ctx.route_scaleN(int(key), b["R"].shape[1])
                else:
                    scale[key] = ctx.route_scaleG(_lib.POOLK[key[0]], key[1], b["R"].shape[1])
                lam[key] = scale[key] * held[key][1]
            rep["scale"] = scale
        dlt = {key: d for key, (d, _) in held.items()}
        if self.where is not None:
            lam = [lam[key][:, pos].copy() for key, pos in self.where]
            dlt = [dlt[key][:, pos].copy() for key, pos in self.where]
        rep["lambdas"], rep["deltas"] = lam, dlt
        rep["value_held"] = kept["value"]
        rep["shortfall"] = kept["psi"] - rep["psi"] if kept["psi"] is not None else None
        return rep

    def pool_prices(self, anchor=None):
        """What is every token worth according to the resident pools, and how far do the pools disagree?  cfmm_pool_prices on the
        device (docs/pool_prices.md), at the reserves, fees and weights the pools hold NOW -- after update_* and
        apply_trades(sync_host=False) included; self.net is not read.  anchor: [n] known prices, 0 = unknown.  Returns (prices, info)
        as the NumPy twin cfmm.problem.pool_prices does, info carrying phi and comp.  Needs no utility and no solve."""
        if self._host is not None or self._comm is not None:
            raise ValueError("pool_prices: pool-sharded problems are not served (cfmm.problem.pool_prices on the gathered network)")
        return self._ensure_ctx().pool_prices(anchor, want_potential=True)

    def select(self, min_value=0.0):
        """Which pools of the route are worth executing?  Every pool is measured on the device by the value it takes in at the accepted
        prices, v = sum_j nu_j delta_j on the tenders deltas / lambdas / bucket_trades hand out now, and selected iff v > min_value
        (strict: 0 selects the pools that trade; docs/subnetwork.md).  Only the selected positions cross to the host.  Returns the
        report of cfmm_select_pools as a dict (pools, selected, non_finite, value_in_total, value_in_selected, per-slot counts), plus
          positions   {bucket key: ascending upload-order positions of the bucket's selected pools} (keys as bucket_trades takes them)
          pools       the selected pools' indices in the pool lists this Problem was built from, ascending (None without lists)
        Refused (CfmmError) while fills are held on the host, ties sit on the device or the pools are sharded, as apply_trades'
        device path is: the selection is of the device's own tenders."""
        ctx = self._ensure_ctx()
        self._pools_seen()
        if self._apply_path() != "device":
            raise CfmmError("select: fills held on the host, device ties or sharded pools -- the device's tenders are not the route")
        net = self._net
        out = ctx.select_pools(min_value)
        pos = {}
        cap = lambda key: out["slot_selected"][self._slot_of(key)]      # (the count is known: one compaction per bucket, none where it is 0)
        for key, kind in KIND2.items():
            if key in net:
                pos[key] = ctx.get_selected2(kind, cap(key))[0] if cap(key) else np.zeros(0, dtype=np.int32)
        for k in net.get("gn", {}):
            pos[k] = ctx.get_selectedN(k, cap(k))[0] if cap(k) else np.zeros(0, dtype=np.int32)
        for (kind, k) in net.get("gk", {}):
            pos[(kind, k)] = ctx.get_selectedG(_lib.POOLK[kind], k, cap((kind, k)))[0] if cap((kind, k)) else np.zeros(0, dtype=np.int32)
        out["positions"] = pos
        out["pools"] = None
        if self.where is not None:
            chosen = {key: set(p.tolist()) for key, p in pos.items()}
            out["pools"] = np.array([i for i, (key, p) in enumerate(self.where) if int(p) in chosen.get(key, ())], dtype=np.int64)
        return out

    @staticmethod
    def _slot_of(key):
        if isinstance(key, str):
            return _lib.bucket_slot(KIND2[key])
        return _lib.bucket_slot(("table", _lib.POOLK[key[0]], key[1])) if isinstance(key, tuple) else _lib.bucket_slot(("gn", int(key)))

    def subproblem(self, pools=None, buckets=None):
        """A Problem over a choice of this one's pools, built on the device (cfmm_subnetwork, docs/subnetwork.md): the chosen pools'
        resident columns -- as in-place updates and applied trades left them -- are gathered device to device into a pool store of
        its own; nothing is uploaded.  The choice: `pools` (indices of the pool lists this Problem was built from, no duplicates),
        or `buckets` ({bucket key: strictly ascending upload-order positions}), or neither = the current selection (select()).
        The new Problem has this one's utility and, as its warm start, this one's prices (solve(warm_start=True)); its net / where are
        the subset of this one's host copy (refreshed first if the device has moved it), and it carries
          parent_positions   {bucket key: positions in this Problem's buckets}
          parent_pools       this Problem's pool-list indices, ascending: sub.deltas[i] belongs to pool parent_pools[i] (None without lists)
        Afterwards the two are independent: updates through one do not reach the other, either may be closed."""
        if pools is not None and buckets is not None:
            raise ValueError("subproblem: pools or buckets, not both")
        if self._host is not None or self._comm is not None:
            raise CfmmError("subproblem: pool-sharded problems are not served")
        ctx = self._ensure_ctx()
        self._pools_seen()
        net = self.net                                   # (refreshed when an apply left it behind the device)
        if pools is not None:
            if self.where is None:
                raise CfmmError("subproblem(pools=...) needs a Problem built from pool lists; use buckets=")
            pp = np.sort(np.asarray(pools, dtype=np.int64).reshape(-1))
            if len(pp) and (pp[0] < 0 or pp[-1] >= len(self.where) or np.any(np.diff(pp) == 0)):
                raise ValueError(f"subproblem: pools must be distinct and in [0, {len(self.where)})")
            positions = {}
            for i in pp:
                positions.setdefault(self.where[i][0], []).append(self.where[i][1])
        elif buckets is not None:
            positions = dict(buckets)
        else:
            positions = {}
            for key in [k for k in KIND2 if k in net] + list(net.get("gn", {})) + list(net.get("gk", {})):
                got = (ctx.get_selected2(KIND2[key]) if isinstance(key, str) else
                       ctx.get_selectedG(_lib.POOLK[key[0]], key[1]) if isinstance(key, tuple) else ctx.get_selectedN(key))[0]
                if len(got):
                    positions[key] = got
        positions = {key: np.asarray(p, dtype=np.int64).reshape(-1) for key, p in positions.items()}
        sub_net = subset_network(net, positions)         # (checks the lists as the library does: ValueError)
        lists = {self._slot_of(key): p for key, p in positions.items() if len(p)}
        q = Problem(self.n, utility=self.utility, device=self.device, network=sub_net, deterministic=self.deterministic)
        q.ctx = ctx.subnetwork(lists)
        q._uploaded = True
        q._dev_utility = self._dev_utility               # (what the library carried over: the utility last sent)
        q.nu = None if self.nu is None else np.array(self.nu, dtype=np.float64)
        q.parent_positions = positions
        q.parent_pools = None
        if self.where is not None:
            rank = {key: {int(p): r for r, p in enumerate(pos)} for key, pos in positions.items()}
            keep = [(i, key, rank[key][int(p)]) for i, (key, p) in enumerate(self.where) if int(p) in rank.get(key, ())]
            q.parent_pools = np.array([i for i, _, _ in keep], dtype=np.int64)
            q.where = [(key, r) for _, key, r in keep]
        return q

    def sparsify(self, min_value=0.0, solve=True, **solve_kw):
        """Drop the dust and route again: select(min_value), the selected pools as a subproblem() built on the device, and (solve=True)
        its solve, warm from this Problem's prices -- the fixed-cost heuristic's second pass, so that the smaller route is itself
        optimal and feasible over the pools it uses.  Returns the new Problem, with the selection's report as .selection"""
        rep = self.select(min_value)
        q = self.subproblem(buckets={key: p for key, p in rep["positions"].items() if len(p)})      # (the lists select() read: no second read)
        q.selection = rep
        if solve:
            solve_kw.setdefault("warm_start", True)
            q.solve(**solve_kw)
        return q

    def _solve(self, tol=1e-6, nu0=None, max_evals=2000, memory=0, iters_per_graph=8, kink_tol=1e-3,
               max_rounds=6, warm_start=False, method="auto"):
        if self.utility is None:
            raise ValueError("no utility set")
        ctx = self._ensure_ctx()
        u = self.utility
        self._send_utility()
        if self._dev_ties:
            self._clear_ties(ctx)
        nu0_given = nu0
        host = self._host
        rank = host.rank if host else 0
        # global pool counts: the branches below change the sequence of device collectives, so a pool-sharded solve
        # takes them on what ALL ranks hold, never on its own shard
        cnt = getattr(self, "_global_counts", None)
        if cnt is None:                               # (the pools of a Problem never change: one collective per Problem, not per solve)
            gk = self.net.get("gk", {})
            cnt = np.array([(len(self.net["curve2"]["Ra"]) if "curve2" in self.net else 0) + sum(b["R"].shape[1] for (kd, _), b in gk.items() if kd == "stable"),
                            (len(self.net["sum2"]["Ra"]) if "sum2" in self.net else 0) + sum(b["R"].shape[1] for (kd, _), b in gk.items() if kd == "sum")],
                           dtype=np.float64)
            if host:
                cnt = host.allreduce_sum(cnt)
            self._global_counts = cnt
        n_stable, n_sum = int(cnt[0]), int(cnt[1])
        if isinstance(nu0, str):                      # "pools": fitted on the device to the resident pools; pool-sharded: the host path
            anchor = start_anchor(u)
            nu0 = None if host or self._comm is not None else (anchor.copy() if np.all(anchor > 0) else ctx.pool_prices(anchor)[0])
            nu0_given = nu0
            warm_start = False
        if nu0 is None:
            if warm_start and self.nu is not None and np.all(np.isfinite(self.nu)) and np.all(np.asarray(self.nu) > 0.0):
                nu0 = self.nu                     # (a previous solve that ended on collapsed / non-finite prices is no warm start: cold instead)
            elif host and not np.all(u.c > 0):
                # start prices are a guess propagated through THIS rank's pools: rank 0's guess is everyone's
                nu0 = host.broadcast(start_prices(self.net, u) if rank == 0 else np.zeros(self.n), src=0)
            else:
                nu0 = start_prices(self.net, u)
        # start prices: derived from the (verified) utility, broadcast from rank 0, or the previous solution of an identical
        # solve -- identical on every rank by construction; prices the CALLER supplies are verified every time
        if host and nu0_given is not None:
            host.assert_identical(nu0, "the start prices")
        self._theta = {}
        self._trade_cache = None
        self._tol = tol
        kw = dict(max_evals=max_evals, memory=memory, iters_per_graph=iters_per_graph)
        total = dict(evals=0, iters=0, wall_seconds=0.0, device_seconds=0.0, rounds=0)
        general = _is_general(u)      # entries of the utility table: generic first-order iteration or the second-order path; no ties
        # (round 5 refused such a utility over ANY network with constant-sum pools, the K-asset table's included, for every method: what
        #  cannot be had is the tie loop -- a plain first-order leg and the second-order path, which smooths these pools, need no ties)
        # (the K-asset table's pools are in the second-order path too: the stableswap entry with its exact Hessian block, the constant-sum
        #  entry smoothed in price space -- csrc/phik.hpp: table_newton_kernel, gk_sum_newton_kernel)
        can_second = getattr(ctx, "second_order", False)
        if method not in _lib.METHODS:
            raise ValueError(f"method {method!r}: expected one of {sorted(_lib.METHODS)}")
        # auto: many stableswap pools -> second order straight away (first order needs thousands of evaluations there);
        # otherwise first order (with the active-set loop over constant-sum kinks), second order if that fails
        many_stable = n_stable >= AUTO_NEWTON_MIN_STABLE
        second_order = method == "newton" or (method == "auto" and can_second and many_stable)
        def first_order_leg(nu_from):
            """the first-order iteration from `nu_from` (with the active-set loop where the network has constant-sum pools), finished"""
            if n_sum == 0 or general:
                st = self._run(ctx, nu_from, total, tol=tol, method=_lib.METHODS["lbfgs"], **kw)
                nu, psi = self._solution_of(ctx, st, nu_from)
            else:
                self._kinks_settled = False
                st, nu, psi = self._solve_kinks(ctx, nu_from, tol, dict(kw, method=_lib.METHODS["lbfgs"]), kink_tol, max_rounds, total)
                if st["status"] == 1 and not self._kinks_settled:
                    st = dict(st, status=2)       # (the last leg converged on a REDUCED dual whose ties did not yield their fills: not a solution)
            self._finish(st, nu, psi, total)
            return st

        retry_near = False
        if not second_order:
            st = first_order_leg(nu0)
            # what decides is the CERTIFICATES of the point the run ended on (recomputed here, the worthless-component repair included), not
            # the device's verdict: a run that "stalled" at 1e-44 prices on a value-0 instance is optimal, and a run that reported
            # convergence while a whole region's prices collapsed (the device's test is value-weighted) is not (tools/fuzz_small.py,
            # fuzz_mid.py).  Uncertified: the second-order path from the start prices -- unless the device had converged and the
            # miss is a near one ("inaccurate", with its figures)
            near = st["status"] == 1 and max(self.gap, self.infeas) <= 100.0 * max(tol, 1e-12)
            # (a near miss on a SMALL network goes on all the same: a second-order solve of <= 512 tokens costs a millisecond or two, and
            #  "inaccurate at 1.02 x the tolerance" is what the round-6 table campaign's one failure in 360 was -- seed 703; should the
            #  second-order path not certify it either, the first-order point is solved for again below)
            retry_near = near and self.n <= 512
            if not (method == "auto" and can_second and self.status not in ("optimal", "infeasible") and (not near or retry_near)):
                return self.value
            second_order = True
            if self._dev_ties:
                self._clear_ties(ctx)
            self._theta = {}; self._trade_cache = None
        # warm start after a second-order solve on this context: nu0 = NULL tells the library to continue from its
        # own previous solution -- the prices AND (a multiple of) the final barrier weight, which is what turns the
        # ~18 steps of a cold solve into 4-7 (the parametric sweep of two-asset.py:34-100)
        cont = warm_start and nu0_given is None and self.nu is not None and (self.stats or {}).get("method") == _lib.METHODS["newton"]
        st = self._run(ctx, None if cont else nu0, total, tol=tol, method=_lib.METHODS["newton"], **kw)
        nu, psi = self._solution_of(ctx, st, nu0)
        self._finish(st, nu, psi, total)
        if method == "auto" and self.status not in ("optimal", "infeasible") and psi is not None and not retry_near and st.get("newton_steps", 0) > 0:
            # the second-order path ended without its certificates: ONE continuation from where it stopped -- the prices and a multiple of the
            # barrier weight it reached (cfmm_solve with nu0 = NULL).  Its end game on a partially filled constant-sum pool moves prices
            # below fp64 resolution, and whether the last steps centre or stall is decided by summation noise (tools/fuzz_table.py seeds
            # 1389, 1401: the same instance ends optimal in one run and stalled in the next); re-centring at a larger weight settles it.
            st2 = self._run(ctx, None, total, tol=tol, method=_lib.METHODS["newton"], **kw)
            nu2, psi2 = self._solution_of(ctx, st2, nu)
            if psi2 is not None:
                self._finish(st2, nu2, psi2, total)
        if method == "auto" and retry_near and self.status != "optimal":
            if self._dev_ties:
                self._clear_ties(ctx)
            self._theta = {}; self._trade_cache = None
            first_order_leg(nu0)                  # (the near miss stands: its point again, so that the device holds what this object reports)
            return self.value
        if method == "newton" and self.status not in ("optimal", "infeasible") and psi is not None and not general:
            # The barrier path asked for BY NAME and ended without its certificates (round 6; tools/fuzz_small.py seeds 1387, 1501): optima
            # where nothing trades, or a partially filled constant-sum pool decides, are what the first-order leg with its active-set
            # loop is for -- `auto` sends such problems there first; an explicit "newton" now hands it the prices the path ended on.
            # Kept only if that leg ends certified or at least closer: otherwise the path's own point is solved for again (the device's
            # buffers must hold the point this object reports).
            worst = lambda: max(abs(self.gap) / tol, self.infeas / tol) if np.isfinite(self.gap) and np.isfinite(self.infeas) else np.inf
            w_path, newton_steps = worst(), (self.stats or {}).get("newton_steps", 0)
            first_order_leg(np.asarray(nu, dtype=np.float64).copy())
            if self.status == "optimal" or worst() < w_path:
                self.stats["newton_steps"] = newton_steps
            else:
                if self._dev_ties:
                    self._clear_ties(ctx)
                self._theta = {}; self._trade_cache = None
                st = self._run(ctx, nu0, total, tol=tol, method=_lib.METHODS["newton"], **kw)
                nu, psi = self._solution_of(ctx, st, nu0)
                self._finish(st, nu, psi, total)
        return self.value

    @staticmethod
    def _solution_of(ctx, st, nu_start):
        """(nu, psi) of the run `st` -- or, for a run that ended in the library's numeric error, the start prices and NO net trade: the
        device's buffers then still hold the PREVIOUS solve's point, which must not be certified in this one's name"""
        if "numeric_error" in st:
            return np.asarray(nu_start, dtype=np.float64).copy(), None
        return ctx.get_solution()

    @staticmethod
    def _run(ctx, nu, total, **kw):
        try:
            st = ctx.solve(nu, **kw)
        except CfmmError as e:
            # an iteration that ran into non-finite numbers (a degenerate instance: prices hundreds of orders of magnitude apart) is a
            # solve that did not converge, not a crash of the caller: reported as "stalled", and `method="auto"` goes on to the
            # second-order path (tools/fuzz_table.py)
            # (ONLY the library's CFMM_E_NUMERIC -- "dual value is not finite", "non-finite value in the second-order iteration": an argument
            #  check that happens to mention "finite" -- a start price that is not positive and finite -- is the caller's error and is raised.
            #  the substring test swallowed those too, and _finish then certified the PREVIOUS solve's point)
            numeric = getattr(e, "code", None) == _lib.E_NUMERIC or (getattr(e, "code", None) is None and
                                                                     ("dual value is not finite" in str(e) or "non-finite value in the second-order iteration" in str(e)))
            if not numeric:
                raise
            st = dict(evals=0, iters=0, status=2, n_ranks=1, dual_value=float("nan"), primal_value=float("nan"), gap=float("inf"), infeas=float("inf"),
                      wall_seconds=0.0, device_seconds=0.0, pg=float("nan"), pool_subproblems=0, barrier_mu=0.0, newton_steps=0,
                      method=kw.get("method", 0), numeric_error=str(e))
        total["evals"] += st["evals"]; total["iters"] += st["iters"]; total["rounds"] += 1
        total["wall_seconds"] += st["wall_seconds"]; total["device_seconds"] += st["device_seconds"]
        return st

    def _clear_ties(self, ctx):
        ctx.set_ties(None, None)
        if "sum2" in self.net:
            ctx.set_pool_flags(POOL_SUM2, None)
        for (kd, k) in self.net.get("gk", {}):
            if kd == "sum" and hasattr(ctx, "set_pool_flagsG"):
                ctx.set_pool_flagsG(k, None)
        self._dev_ties = False

    def _kink_candidates(self, nu, kink_tol, banned, tied, loose=False):
        """constant-sum pools whose price ratio sits on one of their kinks: nearest kink, within kink_tol and well inside its half
        (`loose`: anywhere within kink_tol of it -- a guess for a leg that would not converge; see _solve_kinks).
        Two-asset pools: log nu_a - log nu_b = +-log gamma.  Pools of the K-asset table (arbitrage.py:73-74 over k > 2 tokens): with `lo`
        the pool's cheapest token, leg j is partially drained where gamma nu_j = nu_lo -- the same record with a = lo, b = j, tender a.
        Returns {(rank, k, pool, leg): record} (k = 2, leg = 0: the two-asset bucket): the pool's data travels with its key, so that
        every rank of a pool-sharded solve can build the same ties and the same fill recovery from the union of all ranks' candidates.
        A K-asset record carries the pool's WHOLE token list and reserves (`pidx`, `pR`): whether its kink still stands, what a switch
        record pays and the drain -> switch conversion are then functions of the record alone -- on every rank the same, whoever owns
        the pool (round 5 looked them up in the local bucket under the record's pool index: another rank's pool, or none -- ADVICE r5)."""
        rank = self._host.rank if self._host else 0
        out = {}
        if "sum2" in self.net:
            b = self.net["sum2"]
            r = np.log(nu[b["ia"]]) - np.log(nu[b["ib"]])
            lg = np.log(b["fee"])
            sgn = np.where(r < 0, 1, -1)                 # a->b kink at r = lg < 0, b->a kink at r = -lg > 0
            dist = np.abs(r - sgn * lg)
            near = (dist < kink_tol) & ((dist < 0.5 * np.abs(lg)) | (lg == 0.0) | loose)
            for i in np.flatnonzero(near):               # (only the pools on a kink: the scan itself is vectorised)
                i = int(i)
                key = (rank, 2, i, 0)
                if key not in tied and (key, int(sgn[i])) not in banned:
                    out[key] = dict(sgn=int(sgn[i]), ia=int(b["ia"][i]), ib=int(b["ib"][i]), fee=float(b["fee"][i]),
                                    Ra=float(b["Ra"][i]), Rb=float(b["Rb"][i]), loose=bool(loose))
        for (kd, k), b in self.net.get("gk", {}).items():
            if kd != "sum":
                continue
            lnu = np.log(nu[b["idx"]])                   # [k][m]
            lo = np.argmin(lnu, axis=0)
            m = lnu.shape[1]
            lg = np.log(b["fee"])
            r = lnu[lo, np.arange(m)][None, :] - lnu     # log nu_lo - log nu_j  (<= 0)
            dist = np.abs(r - lg[None, :])
            near = (dist < kink_tol) & ((dist < 0.5 * np.abs(lg)[None, :]) | (lg == 0.0)[None, :] | loose)
            near[lo, np.arange(m)] = False
            for j, i in zip(*np.nonzero(near)):
                i, j = int(i), int(j)
                key = (rank, k, i, j)
                if key not in tied and (key, 1) not in banned:
                    out[key] = dict(sgn=1, ia=int(b["idx"][lo[i], i]), ib=int(b["idx"][j, i]), fee=float(b["fee"][i]),
                                    Ra=float(b["R"][lo[i], i]), Rb=float(b["R"][j, i]), loose=bool(loose), leg_lo=int(lo[i]),
                                    pidx=[int(x) for x in b["idx"][:, i]], pR=[float(x) for x in b["R"][:, i]])
            # the pool's OTHER kind of kink: two tokens tied for cheapest (nu_a = nu_b) -- which of them pays for the drained tokens
            # switches there, and the whole payment with it; at the optimum it is split.  Record: a = the token the device makes pay (the
            # first of the equals), b = the other; "sgn" 0 marks it; the amount P / gamma is filled in when the fills are recovered
            srt = np.argsort(lnu, axis=0, kind="stable")
            a1, a2 = srt[0], srt[1]
            gap = lnu[a2, np.arange(m)] - lnu[a1, np.arange(m)]
            # (only where the pool PAYS something at these prices -- some token worth more than the cheapest after the fee: a pool that
            #  does not trade has no kink there, and tying its two cheapest prices only takes a degree of freedom from the dual)
            pays = (lnu + lg[None, :] > lnu[a1, np.arange(m)][None, :] + 1e-12).sum(axis=0) > 0
            sw = pays & (gap < kink_tol) & ((gap < 0.5 * np.abs(lg)) | (lg == 0.0) | loose)
            for i in np.flatnonzero(sw):
                i = int(i)
                ja, jb = sorted((int(a1[i]), int(a2[i])))         # (equal prices: the device takes the lower leg as the payer)
                key = (rank, k, i, 100 + 10 * ja + jb)
                if key not in tied and (key, 0) not in banned:
                    out[key] = dict(sgn=0, ia=int(b["idx"][ja, i]), ib=int(b["idx"][jb, i]), fee=float(b["fee"][i]), Ra=0.0, Rb=0.0,
                                    loose=bool(loose), leg_a=ja, leg_b=jb, pool=i, k=k,
                                    pidx=[int(x) for x in b["idx"][:, i]], pR=[float(x) for x in b["R"][:, i]])
        if self._host:                                   # the union over ranks, identical everywhere
            merged = {}
            for part in self._host.allgather(out):
                merged.update(part)
            out = merged
        return dict(sorted(out.items()))

    def _solve_kinks(self, ctx, nu, tol, kw, kink_tol, max_rounds, total):
        """A constant-sum pool whose optimum is a partial fill sits on a kink of the dual (all three
        shipped scripts do this).  Active-set loop: run the device solver in short legs; tie the two
        prices of every pool found on a kink (a linear equality in log-price) and skip it in the
        kernels; once the (now smooth) reduced dual has converged recover the fill fractions;
        release ties whose fill leaves (0,1).  Pool-sharded: every decision below is a function of the
        all-reduced prices / psi and of the all-gathered candidates, hence identical on every rank.
        Round 5: the K-asset table's constant-sum pools take part leg by leg (a tied LEG is left out of the evaluation)."""
        rank = self._host.rank if self._host else 0
        m2 = len(self.net["sum2"]["Ra"]) if "sum2" in self.net else 0
        gks = {k: b["R"].shape for (kd, k), b in self.net.get("gk", {}).items() if kd == "sum"}
        tied, banned = {}, set()
        # legs: short on small networks (a solve stuck on a kink gains nothing from more evaluations: the reference's own
        # instances spent 300 of their 315 evaluations that way), longer where an evaluation covers many pools
        budget = min(kw["max_evals"], 40 if self.m <= 1000 else 100)
        st = None
        psi = None
        for _ in range(8 * max_rounds):
            if total["evals"] >= 4 * kw["max_evals"]:
                break
            ties = _Ties(self.n)
            flags = np.zeros(m2, dtype=np.int32)
            flagsg = {k: np.zeros(shp, dtype=np.int32) for k, shp in gks.items()}
            for key, rec in list(tied.items()):
                if ties.tie(rec["ia"], rec["ib"], rec["sgn"] * np.log(rec["fee"])):
                    if key[0] == rank:
                        if key[1] == 2:
                            flags[key[2]] = 1
                        elif key[3] < 100 or key[3] >= 200:           # (a switch record ties two prices and flags nothing)
                            flagsg[key[1]][_drain_leg(key[3]), key[2]] = 1
                else:
                    del tied[key]; banned.add((key, rec["sgn"]))
            self._dev_ties = True
            if tied:
                grp, off, ng = ties.groups()
                ctx.set_ties(grp, off)
                if m2:
                    ctx.set_pool_flags(POOL_SUM2, flags)
                for k, f in flagsg.items():
                    ctx.set_pool_flagsG(k, f)
                st = self._run(ctx, nu, total, tol=0.01 * tol, pg_rule=1, **dict(kw, max_evals=budget))
            else:
                ctx.set_ties(None, None)
                if m2:
                    ctx.set_pool_flags(POOL_SUM2, None)
                for k in flagsg:
                    ctx.set_pool_flagsG(k, None)
                st = self._run(ctx, nu, total, tol=tol, **dict(kw, max_evals=budget))
            if "numeric_error" in st:
                return st, nu, None        # (the leg ran into non-finite numbers: its start prices, no net trade -- _finish reports "stalled")
            nu, psi = ctx.get_solution()
            if not (np.all(np.isfinite(nu)) and np.all(nu > 0.0)):
                break                      # a price has collapsed (a token to sell that no pool lists: the dual is unbounded) -- _finish says "infeasible"
            if st["status"] == 1:
                if not tied:
                    self._kinks_settled = True
                    return st, nu, psi
                # a K-asset record is a statement about the pool's CHEAPEST token (leg j drained where gamma nu_j = nu_lo; the two
                # cheapest tied): if the prices have since made another token the cheapest, the flagged leg is no longer on a kink --
                # it would be drained outright through the new cheapest token, value the reduced dual does not see (tools/fuzz_table.py:
                # a "certified" optimum below SLSQP's feasible point).  Such ties are dropped and the leg repeated
                stale = [k for k, rec in tied.items() if k[1] != 2 and not self._kink_still_stands(nu, k, rec)]
                if stale:
                    for k in stale:
                        del tied[k]
                    continue
                tied = self._canonical_switches(tied, banned)
                n_before = len(tied)
                tied = self._split_payers(tied, banned)
                if len(tied) != n_before:     # (new records tie new prices: a leg with them first)
                    continue
                self._refresh_switches(nu, tied)
                theta, ok = self._recover_fills(nu, psi, tied, tol)
                if os.environ.get("CFMM_KINK_TRACE"):
                    print("[kinks] status", st["status"], "ok", ok, "records", [(k[1:], r["sgn"], r["ia"], r["ib"], round(float(r.get("Rb", 0.0)), 4), round(float(theta[k]), 6)) for k, r in tied.items()], file=sys.stderr)
                bad = [k for k in tied if not (1e-9 < theta[k] < 1 - 1e-9) or (tied[k]["sgn"] == 0 and not tied[k]["Rb"] > 0.0)]      # (a switch record with nothing to move)
                # Switch records of ONE pool that move its payment away from the SAME leg share that payment: their fills live on a
                # simplex, sum theta < 1, not in a box.  Three tokens tied for cheapest (two records from one leg) came back from the
                # box-bounded least squares with fills 0.40 + 0.91: the leg "paid" -30 % of the payment, i.e. received a token it tenders,
                # fee-free -- every token balanced, both certificates met, and a value 1.3e-3 ABOVE the optimum (round 6, the dual
                # referee on tools/fuzz_table.py seeds 1059, 1358: the first FALSELY CERTIFIED points it found).  Such a group means
                # its source leg is not a payer at all: its records are released like any fill outside (0, 1).
                groups = {}
                for k in tied:
                    if tied[k]["sgn"] == 0 and k not in bad:
                        groups.setdefault((k[0], k[1], k[2], tied[k]["ia"]), []).append(k)
                for k in tied:            # ... and so do the records of ONE leg paid for by several of the pool's cheapest tokens
                    if tied[k]["sgn"] == 1 and k[1] != 2 and k not in bad:
                        groups.setdefault((k[0], k[1], k[2], "leg", _drain_leg(k[3])), []).append(k)
                for ks in groups.values():
                    if len(ks) > 1 and sum(theta[k] for k in ks) >= 1 - 1e-9:
                        bad.extend(ks)
                if ok and not bad:
                    self._theta = {k: (tied[k], theta[k]) for k in tied}
                    self._kinks_settled = True
                    return st, nu, psi
                if bad:                   # fully on / fully off after all: back to bang-bang
                    for k in bad:
                        rec = tied.pop(k)
                        banned.add((k, rec["sgn"]))
                        # a guessed kink that carries no trade: the pool's fee band is narrower than the leg could
                        # resolve and the optimum sits on its OTHER kink (arbitrage.py / liquidation.py: fee 0.999)
                        if k[1] == 2 and rec.get("loose") and theta[k] <= 1e-9 and (k, -rec["sgn"]) not in banned:
                            tied[k] = dict(rec, sgn=-rec["sgn"], loose=False)
                        # the K-asset analogue: a guessed DRAIN kink (gamma nu_j = nu_lo) that carries no trade -- inside the fee band the
                        # pool's other kink on that pair is the SWITCH (nu_j = nu_lo: j pays alongside lo), tools/fuzz_table.py seed 256
                        elif k[1] != 2 and rec["sgn"] == 1 and k[3] < 100 and theta[k] <= 1e-9:
                            ja, jb = sorted((rec["leg_lo"], k[3]))
                            k2 = (k[0], k[1], k[2], 100 + 10 * ja + jb)
                            if k2 not in tied and (k2, 0) not in banned:
                                tied[k2] = dict(sgn=0, ia=int(rec["pidx"][ja]), ib=int(rec["pidx"][jb]), fee=rec["fee"], Ra=0.0, Rb=0.0,
                                                loose=False, leg_a=ja, leg_b=jb, pool=k[2], k=k[1], pidx=rec["pidx"], pR=rec["pR"])
                    tied = dict(sorted(tied.items()))
                    continue
            new = self._kink_candidates(nu, kink_tol, banned, tied)
            # nothing within the tolerance although the leg did not converge: look further out before spending another leg
            # (a wrongly tied pool shows as a fill outside (0,1) and is released again)
            wide = kink_tol
            while not new and st["status"] != 1 and wide < 0.05:
                wide *= 10
                new = self._kink_candidates(nu, wide, banned, tied, loose=True)
            if new:
                tied.update(new)
                tied = dict(sorted(tied.items()))
                banned = {bn for bn in banned if bn[0] in new}     # bans expire when the active set changes
            elif st["status"] == 3 and budget < kw["max_evals"]:
                budget = min(kw["max_evals"], 2 * budget)           # no kink in sight: longer legs
            elif kink_tol < 0.05:
                kink_tol *= 10
            else:
                break
        return st, nu, psi

    def _kink_still_stands(self, nu, key, rec):
        lnu = np.log(nu[np.asarray(rec["pidx"], dtype=np.int64)])        # (the pool's own token list: the record's, not a local bucket's)
        lo = float(lnu.min())
        legs = (rec["leg_a"], rec["leg_b"]) if rec["sgn"] == 0 else (rec["leg_lo"],)
        return all(lnu[j] <= lo + 1e-9 for j in legs)

    @staticmethod
    def _canonical_switches(tied, banned):
        """A K-asset constant-sum pool with SEVERAL tokens tied for cheapest: the switch records that tie them were found pair by pair, in
        rounds whose cheapest token differed -- (0, 3) in one, (2, 3) in another.  The device makes ONE leg pay, the lowest of the tied
        legs (csrc/phik.hpp: "ties: the first"), and a record moves a share of THAT leg's payment: a record rooted at another leg moves
        a payment that leg never made (round 6, tools/fuzz_table.py seed 1358: leg 2 "paid" -57 %, every token balanced, both
        certificates met, the value 1.1e-3 above the optimum -- caught by the dual referee).  Canonical form: for the tied legs T of a
        pool, one record (min T -> t) per t in T; same union of tied tokens, so the price ties on the device are what they were."""
        pools = {}
        for k, rec in tied.items():
            if rec["sgn"] == 0:
                pools.setdefault((k[0], k[1], k[2]), []).append(k)
        out = dict(tied)
        for (r, kk, i), ks in pools.items():
            legs = sorted({tied[k]["leg_a"] for k in ks} | {tied[k]["leg_b"] for k in ks})
            want = {(r, kk, i, 100 + 10 * legs[0] + t): t for t in legs[1:]}
            if set(want) == set(ks):
                continue
            proto = tied[ks[0]]
            for k in ks:
                del out[k]
            for k2, t in want.items():
                if (k2, 0) in banned:
                    continue
                out[k2] = dict(proto, ia=int(proto["pidx"][legs[0]]), ib=int(proto["pidx"][t]), leg_a=legs[0], leg_b=t, Ra=0.0, Rb=0.0, loose=False)
        return dict(sorted(out.items()))

    @staticmethod
    def _split_payers(tied, banned):
        """A K-asset constant-sum pool on BOTH kinds of kink at once: leg j partly drained (gamma nu_j = nu_lo) while several tokens are tied
        for cheapest.  The drain record says who pays for the fill -- ONE token, the cheapest when the kink was found -- but at the optimum
        the payment may be split between the tied tokens, and the switch record cannot do it: what it moves is the payment for the legs
        drained OUTRIGHT, which is zero here (round 6, tools/fuzz_table.py seed 2595: the loop cycled through four tie sets, each
        unbalanced, for 48 rounds).  So the leg gets one record per cheapest token that could pay for it: the same fill vector with
        another payer, key 200 + 10 t + j; their fills share the leg, sum theta < 1 (the simplex test below)."""
        pools = {}
        for k, rec in tied.items():
            if rec["sgn"] == 0:
                pools.setdefault((k[0], k[1], k[2]), set()).update((rec["leg_a"], rec["leg_b"]))
        if not pools:
            return tied
        out = dict(tied)
        for k, rec in tied.items():
            if rec["sgn"] != 1 or k[1] == 2 or (k[0], k[1], k[2]) not in pools:
                continue
            T, j = pools[(k[0], k[1], k[2])], _drain_leg(k[3])
            if rec["leg_lo"] not in T:
                continue
            for t in sorted(T):
                k2 = (k[0], k[1], k[2], 200 + 10 * t + j)
                if t in (rec["leg_lo"], j) or k2 in out or (k2, 1) in banned or (k[0], k[1], k[2], j) in out and out[(k[0], k[1], k[2], j)]["leg_lo"] == t:
                    continue
                out[k2] = dict(rec, ia=int(rec["pidx"][t]), Ra=float(rec["pR"][t]), leg_lo=t, loose=False)
        return dict(sorted(out.items()))

    def _refresh_switches(self, nu, tied):
        """the payment a K-asset constant-sum pool's cheapest token makes at the prices nu (what the device evaluated): the reserves of
        every token drained there over the fee, tied legs' fills aside -- the amount a `switch` record moves to the other cheapest token"""
        for key, rec in tied.items():
            if rec["sgn"] != 0:
                continue
            i = rec["pool"]
            p = nu[np.asarray(rec["pidx"], dtype=np.int64)]
            R = np.asarray(rec["pR"], dtype=np.float64)
            lo = rec["leg_a"]
            drained = rec["fee"] * p > p[lo]
            drained[lo] = False
            for k2, r2 in tied.items():                           # legs of this pool tied on a drain kink: left out by the device
                if r2["sgn"] == 1 and k2[0] == key[0] and k2[1] == rec["k"] and k2[2] == i:
                    drained[_drain_leg(k2[3])] = False
            rec["Rb"] = float(R[drained].sum() / rec["fee"])

    def _fill_vector(self, rec):
        """net trade of the tied constant-sum pool `rec` at full fill in its kink's direction"""
        d = np.zeros(self.n)
        a, bb, g = rec["ia"], rec["ib"], rec["fee"]
        if rec["sgn"] == 0:   # a K-asset pool whose two cheapest tokens are tied: the payment P / gamma moves from a to b
            d[a] = rec["Rb"]; d[bb] = -rec["Rb"]                  # (Rb holds P / gamma: _refresh_switches)
            return d
        if rec["sgn"] > 0:    # tender a, drain b
            d[a] = -rec["Rb"] / g; d[bb] = rec["Rb"]
        else:                 # tender b, drain a
            d[bb] = -rec["Ra"] / g; d[a] = rec["Ra"]
        return d

    def _recover_fills(self, nu, psi, tied, tol):
        """theta in [0,1]^K with  (psi + h + sum_k theta_k d_k)_j = 0 on every token that must balance
        (EQ tokens, GE tokens priced above their bound) and >= 0 on GE tokens at their bound."""
        u = self.utility
        keys = list(tied)
        D = np.stack([self._fill_vector(tied[k]) for k in keys], axis=1)       # n x K
        r = psi + u.h
        at_bound = (u.ctype == GE) & (nu <= u.c * (1 + 1e-9))
        must = (u.ctype == EQ) | ((u.ctype == GE) & ~at_bound)
        touched = np.abs(D).sum(axis=1) > 0
        rows = must & touched
        A = D[rows] * nu[rows, None]
        rhs = -r[rows] * nu[rows]
        if A.shape[0] == 0:
            th = np.full(len(keys), 0.5)
        elif len(keys) == 1:              # one tied pool (every shipped script): the bounded least squares in closed form
            a1 = A[:, 0]
            th = np.array([min(1.0, max(0.0, float(a1 @ rhs) / max(float(a1 @ a1), 1e-300)))])
        else:
            th = np.linalg.lstsq(A, rhs, rcond=None)[0]
            if th.min() < 0.0 or th.max() > 1.0:          # a bound is active: the bounded problem proper
                try:
                    from scipy.optimize import lsq_linear
                    th = lsq_linear(A, rhs, bounds=(0.0, 1.0), tol=1e-14).x
                except Exception:
                    th = np.clip(th, 0.0, 1.0)
        tot = r + D @ th
        scale = max(1.0, float(np.abs(nu * (np.abs(psi) + np.abs(u.h))).sum()))
        res_eq = np.abs(nu[must] * tot[must]).sum() / scale if must.any() else 0.0
        ge_b = at_bound
        res_ge = np.maximum(-(nu[ge_b] * tot[ge_b]), 0.0).sum() / scale if ge_b.any() else 0.0
        ok = (res_eq <= 10 * tol) and (res_ge <= 10 * tol)
        return dict(zip(keys, th)), ok

    def _listed_tokens(self):
        """per token: some pool (of any rank) lists it"""
        ls = getattr(self, "_listed", None)
        if ls is None:
            ls = np.zeros(self.n, dtype=bool)
            for _, idx in self._pool_token_arrays():
                ls[idx.ravel()] = True
            if self._host:
                ls = np.any(np.stack(self._host.allgather(ls)), axis=0)
            self._listed = ls
        return ls

    def _max_reserve(self):
        """largest reserve of the network (all ranks of a pool-sharded problem: the floor of a relative figure must not differ between them)"""
        self._pools_seen()
        mr = getattr(self, "_rmax", None)
        if mr is None:
            mr = 0.0
            for key in KIND2:
                if key in self.net and len(self.net[key]["Ra"]):
                    mr = max(mr, float(self.net[key]["Ra"].max()), float(self.net[key]["Rb"].max()))
            for b in list(self.net.get("gn", {}).values()) + list(self.net.get("gk", {}).values()):
                if b["R"].size:
                    mr = max(mr, float(b["R"].max()))
            if self._host:
                mr = float(max(self._host.allgather(mr)))
            self._rmax = mr
        return mr

    def _pool_token_arrays(self):
        """(key, idx [k][m]) of every non-empty bucket: the token ids of its pools, leg by leg"""
        out = []
        for key in KIND2:
            if key in self.net and len(self.net[key]["Ra"]):
                out.append((key, np.stack([self.net[key]["ia"], self.net[key]["ib"]])))
        for k, b in self.net.get("gn", {}).items():
            if b["R"].shape[1]:
                out.append((k, b["idx"]))
        for key, b in self.net.get("gk", {}).items():
            if b["R"].shape[1]:
                out.append((key, b["idx"]))
        return out

    def _recover_worthless(self, st, nu, psi, total):
        """Tokens worth NOTHING at the optimum -- no chain of pools leads from them to anything the utility values: a disconnected
        component, a target no pool lists -- have prices that run to zero TOGETHER: the dual is flat along that ray, the ratios between
        them never settle, and the pools among them trade at whatever ratio the last iterate had (found by tools/fuzz_small.py: such
        instances came back "infeasible" although the program is feasible -- cvxpy solves them).  The primal side of that degeneracy
        is simple: a pool ALL of whose tokens are worthless can be left untouched at no cost in the objective, and a worthless token that
        must leave the trader's hands (an equality, liquidation.py:77-80) can be given to any pool that lists it (Delta > 0 with
        Lambda = 0 only raises the pool's trading function: arbitrage.py:60,63-74).  Done here, on the host, on the tenders read back;
        accepted only if the certificates then hold.  Returns True if they do (and _finish has been re-run on the repaired point)."""
        u = self.utility
        if _is_general(u):
            return False
        # "worthless": a price far below the largest.  How far is not knowable in advance (the iteration stops somewhere down the
        # ray) -- and need not be: the repair is accepted only if BOTH certificates hold afterwards, and leaving out a pool whose
        # arbitrage value is not negligible breaks the gap.  So: the strictest threshold first, looser ones after it
        for thr in (1e-9, 1e-7, 1e-5):
            W = nu <= thr * float(nu.max())
            if W.any() and self._recover_worthless_at(W, st, nu, psi, total):
                return True
        return False

    def _recover_worthless_at(self, W, st, nu, psi, total):
        u = self.utility
        tr = self._trades()                               # (the tied pools' fills included)
        # psi of the repaired point is re-summed from the tenders that are handed out, not patched: down a flat ray the prices end
        # tens of orders of magnitude apart, and there the evaluation's psi and the tender kernel's need not agree on a worthless pool
        psi2 = np.zeros(self.n)
        psi_dropped = np.zeros(self.n)                    # net trade of the pools left untouched: their arbitrage value stays in the DUAL
        zeroed, lister = {}, {}
        arrays = self._pool_token_arrays()
        for key, idx in arrays:
            allw = W[idx].all(axis=0)
            for leg in range(idx.shape[0]):               # a pool to give token j to: the first that lists it
                for pos in np.flatnonzero(W[idx[leg]]):
                    lister.setdefault(int(idx[leg, pos]), (key, leg, int(pos)))
            d, l = tr[key]
            keep = ~allw
            np.add.at(psi2, idx[:, keep].ravel(), (l - d)[:, keep].ravel())
            if allw.any():
                zeroed[key] = allw
                np.add.at(psi_dropped, idx[:, allw].ravel(), (l - d)[:, allw].ravel())
        r = psi2 + u.h
        give = np.where(W & (u.ctype == EQ) & (r > 0.0), r, 0.0)
        for j in np.flatnonzero(give):
            if int(j) not in lister:
                return False                              # (no pool lists it: truly infeasible)
        if not zeroed and not give.any():
            return False
        # the dual value at nu counts EVERY pool's arbitrage value, the untouched ones' included: the repaired point's gap is taken against
        # that, not against a dual rebuilt from the repaired psi (with the zeroed pools' nu'(L - D) missing from both sides a
        # repair at the loosest threshold could pass the gap test it should fail)
        self._repair_dual = float((nu - u.c) @ u.h + nu @ (psi2 + psi_dropped))
        psi2 = psi2 - give
        saved = (self._theta, self._trade_cache)
        names = ("value", "dual_value", "gap", "infeas", "nu", "psi", "status", "stats")
        before = {k: getattr(self, k, None) for k in names}
        self._theta = {}                                  # (psi2 already holds the fills)
        self._finish(st, nu, psi2, total, _recovering=True)
        self._repair_dual = None
        if self.status != "optimal":                      # not a repair: everything back as the solve left it
            self._theta, self._trade_cache = saved
            for k, v in before.items():
                setattr(self, k, v)
            return False
        # the tenders of the repaired point: the untouched pools at zero, the gifts on top
        tr = {key: (d.copy(), l.copy()) for key, (d, l) in tr.items()}
        for key, allw in zeroed.items():
            tr[key][0][:, allw] = 0.0; tr[key][1][:, allw] = 0.0
        for j in np.flatnonzero(give):
            key, leg, pos = lister[int(j)]
            tr[key][0][leg, pos] += give[j]
        self._theta = saved[0]
        self._trade_cache = tr
        self.stats["worthless_tokens"] = int(W.sum())
        return True

    def _finish(self, st, nu, psi, total, _recovering=False):
        u = self.utility
        if psi is None:                       # a run that ended in a numeric error: nothing to certify
            self.value = self.dual_value = float("nan")
            self.gap = self.infeas = float("inf")
            self.nu, self.psi = nu, np.full(self.n, np.nan)
            self.status = "stalled"
            self.stats = dict(st); self.stats.update(total)
            self.stats["pool_subproblems"] = total["evals"] * self.m
            return self
        if self._theta:
            psi = psi.copy()
            for rec, th in self._theta.values():
                psi += th * self._fill_vector(rec)
        if _is_general(u):
            # a utility with entries of the table: value, dual value and certificates are the device's (Fenchel-Young gap of
            # the pair (nu, psi): csrc/lbfgs_rules.hpp); recomputed here in NumPy only by the tests
            self.value = float(st["primal_value"]); self.dual_value = float(st["dual_value"])
            self.gap = abs(float(st["gap"])); self.infeas = float(st["infeas"])
            self.nu, self.psi = nu, psi
            self.status = _lib.STATUS.get(st["status"], f"error {st['status']}")
            tolx = max(self._tol, 1e-12) * (1 + 1e-6) + 1e-15
            if self.status == "optimal" and not (self.gap <= tolx and self.infeas <= tolx):
                self.status = "inaccurate"
            self.stats = dict(st)
            self.stats.update(total)
            return
        plain = getattr(u, "_plain", None)
        if plain is None:                    # h == 0 and psi >= 0 everywhere (arbitrage.py:57,77): a shorter certificate check
            plain = u._plain = bool(not u.h.any() and not u.ctype.any())
        r = psi if plain else psi + u.h
        self.value = float(u.c @ psi)
        nu_psi = float(nu @ psi) if plain else None           # (plain: (nu - c)'psi = nu'psi - c'psi, two dot products serve three quantities)
        cs = nu_psi - self.value if plain else float((nu - u.c) @ r)      # complementary slackness (nu - c)'(psi + h)
        if st.get("method") == _lib.METHODS["newton"]:
            # psi is the barrier-smoothed primal point (strictly inside every pool's trading set); the dual value
            # and the gap against it were computed on the device from an exact evaluation at nu
            self.dual_value = float(st["dual_value"])
            self.gap = abs(float(st["gap"]))
            if _recovering:                   # (a repaired primal point: the duality gap against the device's exact dual value at nu)
                self.gap = abs(self.dual_value - self.value) / max(1.0, abs(self.dual_value))
        else:
            # sum_i arb_i = nu'psi_pools; tied pools trade value-neutrally at their kink prices
            self.dual_value = nu_psi if plain else float((nu - u.c) @ u.h + nu @ psi)
            self.gap = abs(cs) / max(1.0, abs(self.dual_value))
            if _recovering and getattr(self, "_repair_dual", None) is not None:      # (a repaired primal point against the dual value of ALL pools)
                self.dual_value = self._repair_dual
                self.gap = abs(self.dual_value - self.value) / max(1.0, abs(self.dual_value))
        floor = 1e-12 * self._max_reserve()       # (trades of rounding size at a no-arbitrage optimum: noise over noise is not an infeasibility)
        if plain:
            lo, hi = float(psi.min()), float(psi.max())
            viol = max(-lo, 0.0)
            scale = max(hi, -lo, floor, 1e-300)
        else:
            viol = float(np.where(u.ctype == GE, np.maximum(-r, 0.0), np.where(u.ctype == EQ, np.abs(r), 0.0)).max())
            scale = max(float(np.abs(psi).max()), float(np.abs(u.h).max()), floor, 1e-300)
        self.infeas = viol / scale
        self.nu, self.psi = nu, psi
        self.status = _lib.STATUS.get(st["status"], f"error {st['status']}")
        # "optimal" means what the caller asked for: both certificates at the requested tolerance (the recomputation
        # above repeats the device's sums in another order: allow it rounding, not a looser bar)
        tolx = max(self._tol, 1e-12) * (1 + 1e-6) + 1e-15
        if self.gap <= tolx and self.infeas <= tolx:
            self.status = "optimal"
        elif not _recovering and self._host is None and self._recover_worthless(st, nu, psi, total):
            return self                       # (the certificates hold once the worthless component is taken out: _finish has run again)
        else:
            # the certificates do not hold.  A token that MUST leave the trader's hands (an equality with h > 0, liquidation.py:77-80)
            # and that no pool lists cannot: the program is infeasible, and is reported as that.  (Round 5: this used to be read off a
            # price collapsing to zero -- which is also what a WORTHLESS token's price does in a feasible program; any listed token can be
            # given to a pool, so the structural test is the whole of it.)  Otherwise the device's verdict stands, or "inaccurate" if it
            # believed it had converged
            stuck = (u.ctype == EQ) & (u.h > 0) & ~self._listed_tokens()
            if stuck.any():
                self.status = "infeasible"
            elif self.status == "optimal":
                self.status = "inaccurate"
        self.stats = dict(st)
        self.stats.update(total)
        self.stats["pool_subproblems"] = total["evals"] * self.m
        return self

    # -- result read-back (arbitrage.py:84, two-asset.py:94-100) --------------------------------
    def _trades(self):
        self._pools_seen()
        if self._trade_cache is None:
            ctx = self._ensure_ctx()
            tr = {}
            for key, kind in KIND2.items():
                if key in self.net:
                    tr[key] = ctx.get_trades2(kind, len(self.net[key]["Ra"]))
            for k, b in self.net.get("gn", {}).items():
                tr[k] = ctx.get_tradesN(k, b["R"].shape[1])
            for (kind, k), b in self.net.get("gk", {}).items():
                tr[(kind, k)] = ctx.get_tradesG(_lib.POOLK[kind], k, b["R"].shape[1])
            if self._theta:
                rank = self._host.rank if self._host else 0
                for (r, k, i, j), (rec, th) in self._theta.items():
                    if r != rank:                      # (another rank's pool: its tenders are read back there)
                        continue
                    full = self._fill_vector(rec)
                    if k == 2 and "sum2" in tr:
                        d, l = tr["sum2"]
                        y = th * np.array([full[rec["ia"]], full[rec["ib"]]])
                        d[:, i] = np.maximum(-y, 0.0); l[:, i] = np.maximum(y, 0.0)
                    elif ("sum", k) in tr and rec["sgn"] == 0:      # two cheapest tokens tied: theta of the payment moves from leg a to leg b
                        d, l = tr[("sum", k)]
                        d[rec["leg_a"], i] -= th * rec["Rb"]
                        d[rec["leg_b"], i] += th * rec["Rb"]
                    elif ("sum", k) in tr:             # a tied LEG of a K-asset pool: theta R_j received, paid for by the pool's cheapest token
                        d, l = tr[("sum", k)]
                        l[_drain_leg(j), i] += th * rec["Rb"]
                        d[rec["leg_lo"], i] += th * rec["Rb"] / rec["fee"]
            self._trade_cache = tr
        return self._trade_cache

    def bucket_trades(self, key):
        """(delta, lambda), slot-major [k][m], of one bucket ('cp2', 'w2', 'sum2', 'curve2', 'pow2' or a pool size)"""
        return self._trades()[key]

    def _per_pool(self, which):
        if self.where is None:
            raise CfmmError("per-pool lists need a Problem built from pool lists; use bucket_trades()")
        tr = self._trades()
        return [tr[key][which][:, pos].copy() for key, pos in self.where]

    @property
    def deltas(self):
        return self._per_pool(0)

    @property
    def lambdas(self):
        return self._per_pool(1)

    def close(self):
        for p in (getattr(self, "_batch_workers", None) or [])[1:]:
            p.close()
        self._batch_workers = None
        if self.ctx is not None:
            self.ctx.close(); self.ctx = None; self._uploaded = False
            self._dev_utility = None; self._dev_ties = False
