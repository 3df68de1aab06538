"""The second-order path's records over a fixed list of instances, under both hand-off modes (CFMM_NEWTON_IO=lean / blit):
    python tools/newton_path_records.py [out.json] [traces.txt]
One cfmm_solve with method = CFMM_METHOD_NEWTON per instance and mode, straight through the binding (no finisher of cfmm.Problem behind
it): status, newton_steps, evals, barrier_mu, value (the primal value) and the chord-step count of the trace's last line.  CFMM_LIB
selects the library: tests/golden/newton_path_records.json is this tool's output on the build BEFORE solve_newton was divided into
phases (three runs, identical integers), and tests/test_gpu_newton.py holds every later build to it."""
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "cfmm-routing-code_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import cfmm
from cfmm import synthetic, _lib
from helpers import problem_of, random_instance, shipped_cases, table_instance

MODES = ("lean", "blit")


def _basket(net, seed=1, k=10):               # (tests/test_gpu_newton.py: _basket)
    n = net["n_tokens"]
    rng = np.random.default_rng(seed)
    h = np.zeros(n); idx = rng.choice(n, min(k, n - 1), replace=False)
    h[idx] = np.exp(rng.normal(2, 0.5, len(idx))) / net["prices"][idx] * 10
    tgt = int(rng.integers(0, n)); h[tgt] = 0
    return h, tgt


def _traced(f):
    """f() with CFMM_NEWTON_TRACE on and the library's stderr lines returned beside its result"""
    os.environ["CFMM_NEWTON_TRACE"] = "1"
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = f()
        finally:
            os.dup2(keep, 2); os.close(keep)
            os.environ.pop("CFMM_NEWTON_TRACE", None)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def _solve(p, nu0="start", **kw):
    """one explicit second-order solve on p's context -> (record, trace)"""
    ctx = p._ensure_ctx()
    p._send_utility()
    if isinstance(nu0, str):
        nu0 = cfmm.start_prices(p.net, p.utility)

    def run():
        try:
            return ctx.solve(nu0, method="newton", **kw)
        except _lib.CfmmError as e:
            if e.code != _lib.E_NUMERIC:
                raise
            return dict(status=int(_lib.E_NUMERIC), newton_steps=-1, evals=-1, barrier_mu=0.0, primal_value=0.0)
    st, trace = _traced(run)
    last = re.findall(r"\[newton\] (\d+) steps, (\d+) of them chord steps", trace)
    rec = dict(status=int(st["status"]), newton_steps=int(st["newton_steps"]), evals=int(st["evals"]), barrier_mu=float(st["barrier_mu"]),
               value=float(st["primal_value"]), chord_steps=int(last[-1][1]) if last else -1)
    return rec, trace


def _no_arbitrage_problem():
    """two-asset constant-product pools whose reserves sit exactly on the market prices: with a fee, nothing trades at nu = c"""
    rng = np.random.default_rng(77)
    n, m = 6, 14
    price = np.exp(rng.normal(0, 0.5, n))
    L, R = [], []
    for _ in range(m):
        l = rng.choice(n, 2, replace=False); val = np.exp(rng.normal(3, 1))
        L.append(l.tolist()); R.append((val / price[l]).tolist())
    return cfmm.Problem(n, L, R, [0.997] * m, ["geomean"] * m, [[1.0, 1.0]] * m, utility=cfmm.Arbitrage(price)), price


def _mixed_network(seed=0, n=60, m=1500):     # (tests/test_gpu_newton.py: _mixed_network)
    net = synthetic.make_network(n, m_cp2=m, m_w2=m, m_curve2=m, seed=seed)
    rng = np.random.default_rng(seed + 99)
    ms = m // 2
    ia = rng.integers(0, n, ms); ib = (ia // 4) * 4 + (ia % 4 + rng.integers(1, 4, ms)) % 4
    ib = np.minimum(ib, n - 1); ib = np.where(ib == ia, (ia // 4) * 4, ib)
    keep = ia != ib
    ia, ib = ia[keep].astype(np.int32), ib[keep].astype(np.int32)
    L = np.exp(rng.normal(np.log(1e3), 1.0, len(ia)))
    net["sum2"] = dict(Ra=L / net["prices"][ia], Rb=L / net["prices"][ia] * np.exp(rng.normal(0, 0.05, len(ia))),
                       fee=np.full(len(ia), 0.999), ia=ia, ib=ib)
    return net


def cases():
    """(name, function returning (record, trace)) -- each builds its problem afresh (the hand-off mode is read when a context is created)"""
    def one(make, **kw):
        def run():
            p = make()
            try:
                return _solve(p, **kw)
            finally:
                p.close()
        return run
    out = []
    for name, inst in shipped_cases():
        out.append((name, one(lambda inst=inst: problem_of(inst), tol=1e-9)))
    for seed in range(400, 412):
        out.append((f"rand{seed}", one(lambda seed=seed: problem_of(random_instance(seed, n_tokens=6, n_pools=14)), tol=1e-8)))

    def mixed():
        net = _mixed_network(seed=3)
        h, t = _basket(net)
        return cfmm.Problem.from_network(net, utility=cfmm.Liquidate(h, t))
    out.append(("mixed3_basket", one(mixed, tol=1e-8)))

    def c5():
        net = synthetic.config("C5", scale=0.1)
        n = net["n_tokens"]
        rng = np.random.default_rng(2)
        h = np.zeros(n); idx = rng.choice(n, 6, replace=False); h[idx] = rng.uniform(1.0, 20.0, 6)
        return cfmm.Problem.from_network(net, utility=cfmm.Liquidate(h, int(np.setdiff1d(np.arange(n), idx)[0])))
    out.append(("c5_tenth_basket", one(c5, tol=1e-7)))
    for seed, kw in ((1132, dict(n_tokens=7, n_pools=5, with_sum=False, with_curve=False, with_power=False, utility="swap")),
                     (1099, dict(n_tokens=4, n_pools=5, with_sum=True, with_curve=True, with_power=False, utility="swap")),
                     (1329, dict(n_tokens=5, n_pools=4, with_sum=True, with_curve=False, with_power=False, utility="arbitrage"))):
        out.append((f"unlisted{seed}", one(lambda seed=seed, kw=kw: problem_of(random_instance(seed, **kw)), tol=1e-8)))

    def unsellable(seed=5):
        net = synthetic.make_network(7, m_cp2=60, m_curve2=60, seed=seed)
        net["n_tokens"] = 8
        net["prices"] = np.append(net["prices"], 1.0); net["c"] = np.append(net["c"], 1.0)
        h = np.zeros(8); h[7] = 3.0; h[2] = 1.0
        return cfmm.Problem.from_network(net, utility=cfmm.Liquidate(h, 0))
    out.append(("unsellable9", one(lambda: unsellable(9))))      # (seeds 5 .. 8 end on a value that differs from run to run by more than 1e-9)

    def no_arb_at_c():
        p, price = _no_arbitrage_problem()
        try:
            return _solve(p, nu0=price.copy(), tol=1e-8)
        finally:
            p.close()

    def no_arb_perturbed():
        p, price = _no_arbitrage_problem()
        try:
            return _solve(p, nu0=price * np.exp(np.random.default_rng(5).normal(0, 0.05, len(price))), tol=1e-8)
        finally:
            p.close()
    out.append(("no_arbitrage_from_c", no_arb_at_c))
    out.append(("no_arbitrage_perturbed", no_arb_perturbed))

    def ulog():
        net = synthetic.config("C3", scale=0.03, seed=4)
        n = net["n_tokens"]
        rng = np.random.default_rng(9)
        hold = np.exp(rng.normal(3, 0.5, n)) / net["prices"]
        return cfmm.Problem.from_network(net, utility=cfmm.LogUtility(np.exp(rng.normal(0, 0.3, n)), hold))
    out.append(("ulog_far", one(ulog, tol=1e-7)))

    def table4():
        net = synthetic.make_network(120, m_cp2=3000, m_gk_stable=4000, gk_sizes=(3, 4), seed=11, peg=4)
        return cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    out.append(("table_3_4_asset", one(table4, tol=1e-8)))

    def warm(seed=2):
        net = synthetic.config("C5", scale=0.1)
        h, t = _basket(net, seed=seed)
        p = cfmm.Problem.from_network(net, utility=cfmm.Liquidate(h, t))
        try:
            _solve(p)
            p.set_utility(cfmm.Liquidate(h * 1.05, t))
            return _solve(p, nu0=None)         # (continues from the context's own point and barrier weight)
        finally:
            p.close()
    out.append(("c5_tenth_warm_resolve", warm))

    def fuzz_small(seed):                      # (tools/fuzz_small.py's instance of a seed)
        rng = np.random.default_rng(seed)
        kw = dict(n_tokens=int(rng.integers(3, 9)), n_pools=int(rng.integers(4, 24)), with_sum=bool(seed % 2), with_curve=bool((seed // 2) % 2),
                  with_power=bool((seed // 4) % 3 == 0), utility=["arbitrage", "swap", "liquidate"][seed % 3])
        return problem_of(random_instance(seed, **kw))
    for seed in (1434,):
        out.append((f"small_seed{seed}", one(lambda seed=seed: fuzz_small(seed), tol=1e-8)))
    out.append(("liquidation_max_newton_3", one(lambda: problem_of(dict(shipped_cases())["liquidation"]), tol=1e-9, max_newton=3)))
    for seed in (12, 733):                     # (tools/fuzz_table.py seeds the rules' comments name: certified where the path stalled; a forced shrink)
        out.append((f"table_seed{seed}", one(lambda seed=seed: problem_of(table_instance(seed)[0]), tol=1e-7)))
    return out


def records(traces=None):
    out = {}
    for name, run in cases():
        out[name] = {}
        for io in MODES:
            os.environ["CFMM_NEWTON_IO"] = io
            try:
                rec, trace = run()
            finally:
                os.environ.pop("CFMM_NEWTON_IO", None)
            out[name][io] = rec
            if traces is not None:
                traces.write(f"==== {name} {io}\n{trace}")
    return out


if __name__ == "__main__":
    tf = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    rec = records(tf)
    text = json.dumps(rec, indent=1, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
