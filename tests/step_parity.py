"""Step-by-step parity of the projected L-BFGS iteration: shared by tests/test_step_parity_host.py (no GPU) and
tests/test_gpu_step_parity.py (docs/step_parity.md).

A SCENARIO is everything the iteration's trajectory depends on: a small network, a utility, price ties or none, a start, a memory.
From it the twin (oracle/cfmm_oracle.c: oracle_step, driven through Oracle.solve_sharded) gives one RECORD per evaluation budget
k = 1 .. K -- what a solve with max_evals = k ends on: (evals, iters, status), the accepted prices and the five values.  The
iteration is deterministic and the budget only ends it, so the records of all budgets are read off ONE run of K evaluations
(test_budget_records_are_budget_runs checks that against K separate runs); the device runs its K solves from scratch.

The TOLERANCE of a scenario, per budget and per quantity, is measured on the twin alone: 8 x the largest deviation from the
unperturbed run over SEEDS runs whose reduced buffer [psi | sum arb] is perturbed by the bound to which device and twin evaluate the
same function (1e-11 of |psi|_inf on psi, 1e-11 relative on the value: tests/test_gpu.py: test_eval_dual_matches_oracle).  A quantity
the perturbation does not reach at a budget (the accepted prices at budget 1 ARE the clamped start; an infeasibility of exactly zero)
would get the tolerance zero, which asks of two exp / log implementations that they agree bit for bit; so no tolerance is below
FLOOR_ULPS units in the last place of the quantity (of max(1, |value|); for the prices: of max(1, max |log nu|)).
"""
import ctypes as C
import functools
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (python tests/step_parity.py prints the table of the document)
for _p in (ROOT, os.path.join(ROOT, "cfmm-routing-code_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from cfmm import synthetic  # noqa: E402
from oracle import c_oracle  # noqa: E402
from oracle.c_oracle import Oracle  # noqa: E402

K_DEFAULT = 14                      # budgets 1 .. K; K >= memory + 6 for every memory <= 8
TOL = 1e-13                         # the stopping tolerance of every run: none of the scenarios gets there within K evaluations
SEEDS = 8                           # perturbed twin runs per scenario
PERTURB = 1e-11                     # the bound of test_eval_dual_matches_oracle
MARGIN = 8.0                        # eight samples underestimate a maximum
SEPARATION = 100.0                  # a wrong-rule twin deviates by at least this many tolerances
FLOOR_ULPS = 16.0
EPS = float(np.finfo(np.float64).eps)
QUANTITIES = ("lognu", "dual_value", "primal_value", "gap", "infeas", "pg")
GE, EQ, FREE, ULOG, UQUAD = 0, 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------------------------ scenarios
@dataclass(frozen=True)
class Scenario:
    """n tokens; `utility` in arbitrage | liquidate | swap | table (a ULOG / UQUAD / linear mix); the start is
    prices x exp(N(0, sigma)) (relative to the target's price for liquidate / swap); ties: the first n // 8 pairs of tokens tied"""
    n: int
    utility: str = "arbitrage"
    sigma: float = 0.2
    memory: int = 3
    ties: bool = False
    seed: int = 3
    start_seed: int = 0
    K: int = K_DEFAULT
    rejecting: bool = False          # the twin must reject trial points
    capped: bool = False             # the step cap must be active

    @property
    def name(self):
        return (f"n{self.n}-{self.utility}-s{self.sigma:g}-M{self.memory}" + ("-ties" if self.ties else "") +
                (f"-q{self.start_seed}" if self.start_seed else ""))


def pool_counts(n):
    """a few hundred pools, up to ~10^4 at 2049 tokens: four constant-product pools per token, so that every token is listed (an unlisted
    token's step hangs on the sign of the noise on its psi = 0: test_step_parity_host.py asserts there is none).  At 70 tokens the
    network the step-parity scenarios were first measured on; <= 64 tokens: few enough wave-tiles for the one-launch solve (tiny.hpp:
    TINY_MAX_TILES)"""
    if n == 70:
        return dict(m_cp2=600, m_w2=200, m_gn=100)
    if n <= 64:
        return dict(m_cp2=max(12, 4 * n), m_w2=max(6, 2 * n), m_gn=max(4, n))
    return dict(m_cp2=max(600, 4 * n), m_w2=max(200, n // 2), m_gn=max(100, n // 4))


@functools.lru_cache(maxsize=None)
def network(n, seed):
    hi = min(8, n)
    return synthetic.make_network(n, seed=seed, gn_sizes=(3, hi), **pool_counts(n))


@dataclass
class Built:
    sc: Scenario
    net: dict
    c: np.ndarray
    h: np.ndarray
    ctype: np.ndarray
    nu0: np.ndarray
    grp: np.ndarray = None
    off: np.ndarray = None
    _oracle: Oracle = field(default=None, repr=False)


def utility_arrays(sc, net):
    """(c, h, ctype, reference price) of the scenario's utility"""
    n = sc.n
    pi = net["prices"]
    rng = np.random.default_rng([sc.seed, 101])
    if sc.utility == "arbitrage":
        return net["c"].copy(), np.zeros(n), np.zeros(n, dtype=np.int32), 1.0
    target = n // 2
    sell = rng.choice(np.delete(np.arange(n), target), size=min(6, n - 1), replace=False)
    h = np.zeros(n)
    h[sell] = 200.0 / pi[sell] * np.exp(rng.normal(0.0, 0.5, len(sell)))      # ~200 units of value each: a fraction of a pool
    c = np.zeros(n); c[target] = 1.0
    if sc.utility == "liquidate":                      # psi + h == 0 off the target (prices free), the target's price fixed
        ctype = np.full(n, EQ, dtype=np.int32); ctype[target] = FREE
        return c, h, ctype, pi[target]
    if sc.utility == "swap":                           # psi + h >= 0 everywhere: lower bound log c on the target alone
        return c, h, np.zeros(n, dtype=np.int32), pi[target]
    if sc.utility == "table":                          # a third ULOG, a third UQUAD, the rest linear arbitrage
        c = net["c"].copy(); h = np.zeros(n); ctype = np.zeros(n, dtype=np.int32)
        kind = rng.integers(0, 3, n)
        lg, qd = kind == 1, kind == 2
        ctype[lg] = ULOG; ctype[qd] = UQUAD
        hold = 50.0 / pi                               # holdings worth 50 each: u = c log(P + h) with u'(0) = the market price
        h[lg] = hold[lg]; c[lg] = (net["c"] * hold)[lg]
        h[qd] = (500.0 / pi ** 2)[qd]                  # depth: a trade worth 500 moves the marginal value by its own size
        return c, h, ctype, 1.0
    raise ValueError(sc.utility)


@functools.lru_cache(maxsize=None)
def build(sc):
    net = network(sc.n, sc.seed)
    n = sc.n
    c, h, ctype, ref = utility_arrays(sc, net)
    rng = np.random.default_rng([sc.seed, 202, sc.start_seed])
    nu0 = net["prices"] / ref * np.exp(rng.normal(0.0, sc.sigma, n))
    b = Built(sc, net, c, h, ctype, nu0)
    if sc.ties:
        # tokens 2 i and 2 i + 1 share a price up to the ratio of their latent prices, for the first n // 8 pairs: ng < n, groups
        # of two at the front and of one behind them
        T = max(1, n // 8)
        grp = np.zeros(n, dtype=np.int32); off = np.zeros(n)
        for i in range(T):
            grp[2 * i] = grp[2 * i + 1] = i
            off[2 * i + 1] = np.log(net["prices"][2 * i + 1] / net["prices"][2 * i])
        grp[2 * T:] = T + np.arange(n - 2 * T)
        b.grp, b.off = grp, off
    return b


def oracle_of(b):
    if b._oracle is None:
        o = Oracle(b.sc.n)
        o.add_network(b.net)
        o.set_utility(b.c, b.h, b.ctype)
        if b.grp is not None:
            o.set_ties(b.grp, b.off)
        b._oracle = o
    return b._oracle


# ------------------------------------------------------------------------------------------------------------------ the twin
def _state(o):
    st = c_oracle.Stats()
    nu = np.zeros(o.n)
    o.L.oracle_get(o.h, None, c_oracle._d(nu), C.byref(st))
    return dict(evals=st.evals, iters=st.iters, status=st.status, nu=nu, dual_value=st.dual_value, primal_value=st.primal_value,
                gap=st.gap, infeas=st.infeas, pg=st.pg)


def twin_records(sc, memory=None, armijo=1e-4, max_step=2.0, seed=None, K=None):
    """records[k - 1]: what the twin's solve with max_evals = k ends on, k = 1 .. K.  seed: perturb the reduced buffer (module
    docstring).  One run: the callback of evaluation k + 1 reads the state that step k left -- the end of the budget-k run but for its
    status, which is 3 (out of budget) where the run was still going."""
    b = build(sc)
    o = oracle_of(b)
    n = sc.n
    K = sc.K if K is None else K
    rng = None if seed is None else np.random.default_rng([977, seed])
    recs = []
    calls = [0]

    def allreduce(buf):
        if calls[0]:
            r = _state(o)
            r["status"] = 3
            recs.append(r)
        calls[0] += 1
        if rng is not None:
            buf[:n] += PERTURB * np.abs(buf[:n]).max() * rng.uniform(-1.0, 1.0, n)
            buf[n] *= 1.0 + PERTURB * rng.uniform(-1.0, 1.0)

    r = o.solve_sharded(b.nu0, allreduce, tol=TOL, max_evals=K, memory=sc.memory if memory is None else memory, armijo=armijo, max_step=max_step)
    last = {k: r[k] for k in ("evals", "iters", "status", "nu", "dual_value", "primal_value", "gap", "infeas", "pg")}
    recs.append(last)
    while len(recs) < K:             # ended before the budget (converged, stalled): every larger budget ends the same
        recs.append(last)
    return recs


def twin_budget_run(sc, k):
    """the record of budget k from a run of its own (what twin_records reads off one run)"""
    b = build(sc)
    r = oracle_of(b).solve_sharded(b.nu0, lambda buf: None, tol=TOL, max_evals=k, memory=sc.memory)
    return {q: r[q] for q in ("evals", "iters", "status", "nu", "dual_value", "primal_value", "gap", "infeas", "pg")}


def integers(rec):
    return (rec["evals"], rec["iters"], rec["status"])


def deviation(a, b):
    """{quantity: |a - b|}; the prices as max_j |log(nu_a / nu_b)|"""
    d = {q: abs(a[q] - b[q]) for q in QUANTITIES[1:]}
    d["lognu"] = float(np.abs(np.log(a["nu"] / b["nu"])).max())
    return d


def floor_of(rec):
    f = {q: FLOOR_ULPS * EPS * max(1.0, abs(rec[q])) for q in QUANTITIES[1:]}
    f["lognu"] = FLOOR_ULPS * EPS * max(1.0, float(np.abs(np.log(rec["nu"])).max()))
    return f


@dataclass
class Reference:
    """the unperturbed twin's records, the perturbed runs' and the tolerance per budget and quantity"""
    records: list
    perturbed: list                 # [seed][k - 1]
    noise: list                     # [k - 1] {quantity: largest perturbation deviation}
    tol: list                       # [k - 1] {quantity: tolerance}


@functools.lru_cache(maxsize=None)
def reference(sc):
    recs = twin_records(sc)
    pert = [twin_records(sc, seed=s) for s in range(SEEDS)]
    noise, tol = [], []
    for k in range(sc.K):
        devs = [deviation(p[k], recs[k]) for p in pert]
        mx = {q: max(d[q] for d in devs) for q in QUANTITIES}
        fl = floor_of(recs[k])
        noise.append(mx)
        tol.append({q: max(MARGIN * mx[q], fl[q]) for q in QUANTITIES})
    return Reference(recs, pert, noise, tol)


def wrong_rule_twins(sc):
    """{name: twin_records kwargs} of the rules a layout could get wrong and still converge"""
    w = {}
    if sc.memory >= 2:
        w["memory-1"] = dict(memory=sc.memory - 1)
        w["memory+1"] = dict(memory=sc.memory + 1)
    if sc.rejecting:
        w["armijo=0.5"] = dict(armijo=0.5)
    if sc.capped:
        w["max_step*2"] = dict(max_step=4.0)
    return w


def separation(sc, kwargs):
    """(multiple of the tolerance, budget, quantity) of the largest deviation of a wrong-rule twin from the true one; a budget at which
    the integer records differ separates outright (inf)"""
    ref = reference(sc)
    wrong = twin_records(sc, **kwargs)
    best = (0.0, 0, "")
    for k in range(sc.K):
        if integers(wrong[k]) != integers(ref.records[k]):
            return (float("inf"), k + 1, "integers")
        d = deviation(wrong[k], ref.records[k])
        for q in QUANTITIES:
            r = d[q] / ref.tol[k][q]
            if r > best[0]:
                best = (r, k + 1, q)
    return best


def compare(sc, device_records):
    """device_records[k - 1] against the twin: (failures, worst), failures a list of readable lines (empty: parity), worst the largest
    deviation as a fraction of its tolerance with its budget and quantity.  Every budget is compared."""
    ref = reference(sc)
    assert len(device_records) == sc.K
    fails, worst = [], (0.0, 0, "")
    for k in range(sc.K):
        dv, tw = device_records[k], ref.records[k]
        if integers(dv) != integers(tw):
            fails.append(f"budget {k + 1}: (evals, iters, status) device {integers(dv)} twin {integers(tw)}")
            continue
        d = deviation(dv, tw)
        for q in QUANTITIES:
            frac = d[q] / ref.tol[k][q]
            if frac > worst[0]:
                worst = (frac, k + 1, q)
            if not d[q] <= ref.tol[k][q]:
                fails.append(f"budget {k + 1}: {q} deviates by {d[q]:.3e}, tolerance {ref.tol[k][q]:.3e}")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------------ the scenarios
def S(n, **kw):
    return Scenario(n, **kw)


FAR_ARB = dict(sigma=2.5, rejecting=True, capped=True)        # a start far from the market: rejected trial points, the step cap active
FAR_LIQ = dict(utility="liquidate", sigma=1.0, rejecting=True)

# every scenario a GPU case runs (tests/test_gpu_step_parity.py picks from here by name), so that the host test proves each of them
# stable and separated
SCENARIOS = {}


def _add(*scs):
    for sc in scs:
        SCENARIOS[sc.name] = sc


# the one-launch solves: 5 .. 64 tokens, every memory, ties, the three linear utilities
_add(S(5, memory=8), S(6, utility="swap", memory=8), S(7, utility="liquidate", memory=3), S(20, memory=1), S(20, memory=3, ties=True),
     S(33, memory=4), S(33, **FAR_ARB), S(33), S(64, memory=3), S(64, memory=8), S(64, utility="liquidate", memory=3, ties=True))
# the grid-wide layouts at the lane and dispatch edges
for _n in (65, 127, 128, 129, 1024, 1025, 2048, 2049):
    _add(S(_n, memory=3), S(_n, memory=1))
for _n in (65, 129, 1024, 1025, 2048):
    _add(S(_n, memory=4))
for _n in (65, 129, 1024, 1025, 2049):
    _add(S(_n, memory=8))
# (the far starts: a start seed whose twin rejects trial points, is stable under the perturbation and leaves the trajectory under every
#  wrong rule -- test_step_parity_host.py holds them to all three)
_add(S(70, **FAR_ARB), S(70, **FAR_LIQ), S(70, utility="swap"), S(70, utility="liquidate"), S(70),
     S(129, ties=True), S(1025, ties=True), S(2049, ties=True), S(129, **FAR_ARB), S(129, **FAR_LIQ),
     S(1025, start_seed=3, **FAR_ARB), S(2049, start_seed=7, **FAR_ARB), S(1024, **FAR_LIQ),
     S(129, utility="table", memory=8), S(1024, utility="table", memory=3), S(1025, utility="table", memory=8))
# the batched solve: eight starts on one network
BATCH_STARTS = [S(70, memory=m, start_seed=q) for m in (3, 8) for q in range(8)]
SWEEP_STARTS = [S(20, memory=8, start_seed=q) for q in range(4)]
_add(*BATCH_STARTS, *SWEEP_STARTS)


def tolerance_table():
    """the table of docs/step_parity.md: per scenario the largest perturbation deviation over the budgets (log-price and dual value),
    the tolerance made of it, and the smallest separation of its wrong-rule twins"""
    rows = ["| scenario | evals, iters at K | noise, log-price | tolerance, log-price | tolerance, dual value | smallest separation (x tolerance) |",
            "|---|---|---|---|---|---|"]
    for name in sorted(SCENARIOS, key=lambda s: (SCENARIOS[s].n, s)):
        sc = SCENARIOS[name]
        ref = reference(sc)
        seps = [(separation(sc, kw)[0], w) for w, kw in wrong_rule_twins(sc).items()]
        sep = "--" if not seps else "{:.1e} ({})".format(*min(seps)) if min(seps)[0] < float("inf") else "integers differ (all)"
        last = ref.records[-1]
        rows.append(f"| {name} | {last['evals']}, {last['iters']} | {max(x['lognu'] for x in ref.noise):.1e} | {max(x['lognu'] for x in ref.tol):.1e} | "
                    f"{max(x['dual_value'] for x in ref.tol):.1e} | {sep} |")
    return "\n".join(rows)


if __name__ == "__main__":
    print(tolerance_table())
