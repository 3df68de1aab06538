"""GPU suite (-m gpu): the HIP path through the C-ABI against the oracle on the same seeded inputs,
against the golden fixtures, and -- at BASELINE's full sizes -- through size-independent
properties.  Tolerances: per-pool trades and psi 1e-11 relative to the reserves / to |psi|_inf
(fp64, different libm + summation order); objectives 1e-6 relative (the north-star bar)."""
import os
import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib
from oracle import instances as I
from helpers import golden, shipped_cases, problem_of, random_instance, normalise_with_params, utility_of

pytestmark = pytest.mark.gpu


def _oracle_for(oracle_lib, net, threads=4):
    o = oracle_lib.Oracle(net["n_tokens"], threads=threads)
    o.add_network(net)
    o.set_utility(net["c"])
    return o


def test_cross_lane_primitives_selftest():
    """wave butterflies (DPP, v_permlane16/32_swap) and the 64-value reduce-scatter, exact integer sums"""
    ctx = _lib.Context(8)
    ctx.selftest()
    ctx.close()


def test_backend_is_gfx950():
    ctx = _lib.Context(8)
    assert ctx.backend.startswith("hip:gfx950")
    ctx.close()


@pytest.mark.parametrize("cfg,scale", [("C2", 1.0), ("C3", 0.05), ("C5", 0.05), ("C4shard", 0.1)])
def test_eval_dual_matches_oracle(oracle_lib, cfg, scale):
    net = synthetic.config(cfg, scale=scale, seed=1)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    o = _oracle_for(oracle_lib, net)
    rng = np.random.default_rng(2)
    for sig in (0.0, 0.03, 0.3):
        nu = net["c"] * np.exp(rng.normal(0, sig, net["n_tokens"]))
        f1, psi1, d1 = p.eval_dual(nu, want_diag=True)
        f0, psi0, d0 = o.eval(nu, want_diag=True)
        # scale of the terms summed into psi_j: the gross flow, not the (cancelling) net
        assert abs(f1 - f0) <= 1e-11 * max(abs(f0), 1.0)
        gross = max(np.abs(psi0).max(), 1.0)
        assert np.abs(psi1 - psi0).max() <= 1e-10 * gross * 10
        assert np.abs(d1 - d0).max() <= 1e-11 * np.abs(d0).max()
    p.close()


@pytest.mark.parametrize("cfg", ["C3", "C4shard", "C4", "C5"])
def test_full_size_eval_dual_matches_oracle(oracle_lib, cfg):
    """BASELINE configs 3, 4 (one GPU's shard AND the whole 1e7-pool set) and 5 at FULL size: one dual evaluation,
    GPU vs the C oracle on the same seeded input -- sum arb, every entry of psi, the diagonal metric"""
    net = synthetic.config(cfg, seed=0)
    n = net["n_tokens"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    o = _oracle_for(oracle_lib, net, threads=16)
    rng = np.random.default_rng(12)
    for sig in (0.01, 0.2):
        nu = net["c"] * np.exp(rng.normal(0, sig, n))
        f1, psi1, d1 = p.eval_dual(nu, want_diag=True)
        f0, psi0, d0 = o.eval(nu, want_diag=True)
        assert abs(f1 - f0) <= 1e-11 * max(abs(f0), 1.0)
        # psi_j is a sum of ~2 m / n terms of either sign: the yardstick is the gross flow, not the cancelling net
        assert np.abs(psi1 - psi0).max() <= 1e-10 * max(np.abs(psi0).max(), 1.0)
        assert np.abs(d1 - d0).max() <= 1e-11 * np.abs(d0).max()
    p.close()


@pytest.mark.parametrize("cfg", ["C3", "C4shard", "C4"])
def test_full_size_solve_matches_oracle_solver(oracle_lib, cfg):
    """... and the converged solve (the configuration bench.py times, and both forms of config 4): objective, dual
    value and prices against the C oracle running the same iteration to the same 1e-6 certificates"""
    net = synthetic.config(cfg, seed=0)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    o = _oracle_for(oracle_lib, net, threads=16)
    v = p.solve(tol=1e-6)
    r = o.solve(net["c"], tol=1e-6)
    assert p.status == "optimal" and p.gap <= 1e-6 and p.infeas <= 1e-6 and r["status"] == 1
    assert abs(v - r["primal_value"]) <= 2e-6 * abs(v)              # both within 1e-6 of the optimum
    assert abs(p.dual_value - r["dual_value"]) <= 2e-6 * abs(v)
    assert p.stats["evals"] <= 2 * r["evals"] + 16
    f0, psi0 = o.eval(p.nu)                                       # the oracle's evaluation AT the GPU's prices
    assert np.abs(p.psi - psi0).max() <= 1e-9 * max(np.abs(psi0).max(), 1.0)
    assert abs(net["c"] @ psi0 - v) <= 1e-9 * abs(v)
    p.close()


@pytest.mark.parametrize("cfg,scale", [("C2", 1.0), ("C3", 0.1), ("C3", 1.0)])
def test_full_size_optimum_against_the_independent_dual_referee(cfg, scale):
    """... and against an optimiser that is NOT the device's iteration restated (at full size the HIP path was
    compared with the C twin, whose update mirrors the device's by design, and with its own certificates).  oracle/dual_np.py:
    solve_dual_network minimises the dual with SciPy's L-BFGS-B -- its own line search, its own stopping rule -- over the vectorised NumPy
    restatements of the pools (pinned pool by pool elsewhere).  By weak duality its value bounds the optimum from above; the device's
    certified primal value bounds it from below: the two must meet within the tolerances both sides stop at.  BASELINE config 3 at FULL
    size (1e6 pools / 1000 tokens) is ~0.1 s per NumPy evaluation: about twenty seconds of the referee."""
    from oracle import dual_np
    net = synthetic.config(cfg, scale=scale, seed=0)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    v = p.solve(tol=1e-7)
    assert p.status == "optimal" and p.gap <= 1e-7 and p.infeas <= 1e-7
    d = dual_np.solve_dual_network(net, net["c"])
    assert v <= d["value"] + 1e-7 * abs(v)                               # weak duality: no certified primal value above an independent dual bound
    assert d["value"] - v <= 3e-6 * abs(v), (v, d["value"], d["pg"])     # ... and the bound is tight: the two optimisers agree on the optimum
    # the referee's prices are an optimum too: the device's evaluation there is feasible to the referee's own accuracy
    f, psi = p.eval_dual(d["nu"])[:2]
    assert abs(f - d["value"]) <= 1e-9 * abs(f)                          # (same dual function: device evaluation = NumPy evaluation at the same prices)
    p.close()


def test_trades_match_oracle_pool_by_pool(oracle_lib):
    net = synthetic.config("C3", scale=0.02, seed=4)
    cv = synthetic.config("C5", scale=0.01, seed=4)
    net["curve2"] = cv["curve2"]
    net["curve2"]["ia"] = net["curve2"]["ia"] % net["n_tokens"]; net["curve2"]["ib"] = net["curve2"]["ib"] % net["n_tokens"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    o = _oracle_for(oracle_lib, net)
    nu = net["c"] * np.exp(np.random.default_rng(3).normal(0, 0.05, net["n_tokens"]))
    p._ensure_ctx().set_nu(nu)
    names = [k for k, _ in o.b2]
    for key in ("cp2", "w2", "curve2"):
        d, l = p.bucket_trades(key)
        ya, yb = o.trades2(names.index(key), nu)
        b = net[key]
        assert np.all(d >= 0) and np.all(l >= 0) and np.all(d * l == 0)
        tol = (1e-9 if key == "curve2" else 1e-12) * (b["Ra"] + b["Rb"])
        assert np.all(np.abs((l - d)[0] - ya) <= tol) and np.all(np.abs((l - d)[1] - yb) <= tol), key
    sizes = [k for k, _ in o.bn]
    for k in net["gn"]:
        d, l = p.bucket_trades(k)
        y = o.tradesN(sizes.index(k), nu)
        assert np.abs((l - d) - y).max() <= 1e-12 * net["gn"][k]["R"].max()
    p.close()


def test_invariants_preserved_and_psi_is_scatter_of_trades():
    """size-independent properties at BASELINE config 3's full size (1e6 pools / 1000 tokens)"""
    net = synthetic.config("C3", seed=0)
    n = net["n_tokens"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    v = p.solve(tol=1e-6)
    assert p.status == "optimal" and p.gap <= 1e-6 and p.infeas <= 1e-6
    assert p.stats["evals"] < 200
    psi = np.zeros(n)
    value = 0.0
    for key in ("cp2", "w2"):
        b = net[key]
        d, l = p.bucket_trades(key)
        y = l - d
        assert np.all(d * l == 0)
        psi += np.bincount(b["ia"], weights=y[0], minlength=n) + np.bincount(b["ib"], weights=y[1], minlength=n)
        wa = b["wa"] if key == "w2" else 0.5
        xa = b["Ra"] + b["fee"] * d[0] - l[0]; xb = b["Rb"] + b["fee"] * d[1] - l[1]
        inv = wa * np.log(xa / b["Ra"]) + (1 - wa) * np.log(xb / b["Rb"])
        assert np.abs(inv).max() <= 1e-12            # phi(R + gamma D - L) == phi(R)
        assert np.all(p.nu[b["ia"]] * y[0] + p.nu[b["ib"]] * y[1] >= -1e-9)   # arb_i >= 0
    for k, b in net["gn"].items():
        d, l = p.bucket_trades(k)
        y = l - d
        for j in range(k):
            psi += np.bincount(b["idx"][j], weights=y[j], minlength=n)
        x = b["R"] + b["fee"][None, :] * d - l
        assert np.abs((b["w"] * np.log(x / b["R"])).sum(0)).max() <= 1e-12
    assert np.abs(psi - p.psi).max() <= 1e-9 * max(1.0, np.abs(psi).max())
    assert abs(net["c"] @ psi - v) <= 1e-9 * abs(v)
    # certificate: weak duality sandwich
    assert p.dual_value >= v - 1e-9 * abs(v)
    assert (p.dual_value - v) <= 2e-6 * abs(v)
    p.close()


@pytest.mark.parametrize("cfg,scale", [("C2", 1.0), ("C3", 0.1), ("C4shard", 0.2)])
def test_solve_matches_oracle_solver(oracle_lib, cfg, scale):
    net = synthetic.config(cfg, scale=scale, seed=0)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    o = _oracle_for(oracle_lib, net)
    v = p.solve(tol=1e-6)
    r = o.solve(net["c"], tol=1e-6)
    assert p.status == "optimal" and r["status"] == 1
    assert abs(v - r["primal_value"]) <= 2e-6 * abs(v)
    assert abs(p.dual_value - r["dual_value"]) <= 2e-6 * abs(v)
    assert p.stats["evals"] <= 2 * r["evals"] + 16
    # tighter tolerance: both converge to the same prices
    v9 = p.solve(tol=1e-9)
    r9 = o.solve(net["c"], tol=1e-9)
    assert abs(v9 - r9["primal_value"]) <= 1e-8 * abs(v9)
    assert np.abs(p.nu / r9["nu"] - 1).max() <= 1e-6
    p.close()


@pytest.mark.parametrize("name,inst", shipped_cases())
def test_shipped_instances_through_hip(name, inst):
    """arbitrage.py / liquidation.py / two-asset.py on the GPU: objective, psi, every pool's tenders"""
    g = golden()[name]
    p = problem_of(inst)
    v = p.solve(tol=1e-10)
    assert p.status == "optimal"
    assert abs(v - g["survey"]["value"]) <= 1e-6 * max(1, abs(v))          # the north-star tolerance
    assert abs(v - g["survey"]["value"]) <= 1e-8 * max(1, abs(v))          # ... and what we actually reach
    assert abs(v - g["kkt"]["value"]) <= 1e-9 * max(1, abs(v))             # (against the 50-digit KKT solution)
    assert p.gap <= 1e-10 and p.infeas <= 1e-10
    # psi and EVERY pool's tenders against the 50-digit KKT solution: 1e-6 absolute is the bar
    assert np.abs(p.psi - np.asarray(g["kkt"]["psi"])).max() <= 5e-8
    for d, l, y in zip(p.deltas, p.lambdas, g["kkt"]["y"]):
        assert np.all(d >= 0) and np.all(l >= 0) and np.all(d * l == 0)
        assert np.abs((l - d) - np.asarray(y)).max() <= 1e-6
        assert np.abs((l - d) - np.asarray(y)).max() <= 5e-8
    if "cvxpy" in g:            # the reference's own output, where the fixture was made with cvxpy installed (oracle/make_golden.py --cvxpy)
        cv = g["cvxpy"]
        assert abs(v - cv["value"]) <= 1e-6 * max(1, abs(v))                 # BASELINE.json: "objective within 1e-6 relative of cvxpy"
        assert np.abs(p.psi - np.asarray(cv["psi"])).max() <= 1e-4 * max(np.abs(np.asarray(y)).max() for y in g["kkt"]["y"])
    p.close()


def test_two_asset_sweep_warm_started():
    """two-asset.py:40-100 -- the 50-point sweep, each solve warm-started from its neighbour"""
    p = problem_of(I.two_asset(0.0))
    vals = []
    for t in I.two_asset_sweep():
        p.set_utility(cfmm.Swap([t, 0, 0], 2))
        vals.append(p.solve(tol=1e-9, warm_start=True))
        assert p.status == "optimal"
    vals = np.array(vals)
    g = golden()
    for j in (0, 1, 10, 25, 49):
        assert abs(vals[j] - g[f"two_asset_{j}"]["kkt"]["value"]) <= 1e-7
    assert np.all(np.diff(vals) > 0)
    p.close()


def test_two_asset_sweep_in_one_call_all_five_pools():
    """two-asset.py:34-100 UNMODIFIED -- all five pools, the constant-sum pool included (two-asset.py:21-22, 82-83) -- swept at
    its 50 points through ONE library call (cfmm_solve_sweep: one workgroup per point and round, the kink loop inside the library):
    value, psi and EVERY pool's tenders (two-asset.py:93-100) against the 50-digit KKT fixture at j in {0, 1, 10, 25, 49}, the value
    against the one-at-a-time path at every point; and the wall time of the whole sweep"""
    import time
    ts = I.two_asset_sweep()
    p = problem_of(I.two_asset(0.0))
    utils = [cfmm.Swap([t, 0, 0], 2) for t in ts]
    res = p.solve_many(utils, tol=1e-10)
    assert len(res) == 50 and all(r["status"] == "optimal" and r["gap"] <= 1e-10 and r["infeas"] <= 1e-10 for r in res)
    assert all(r["stats"]["batch"] == 50 for r in res)                      # the swept path, not 50 solves
    vals = np.array([r["value"] for r in res])
    assert np.all(np.diff(vals) > 0)
    g = golden()
    for j in (0, 1, 10, 25, 49):
        k = g[f"two_asset_{j}"]["kkt"]
        assert abs(vals[j] - k["value"]) <= 1e-9 * max(1.0, abs(k["value"]))
        assert np.abs(res[j]["psi"] - np.asarray(k["psi"])).max() <= 5e-8
        d, l = p.tenders_of(res[j])
        for dd, ll, y in zip(d, l, k["y"]):
            assert np.all(dd >= 0) and np.all(ll >= 0) and np.all(dd * ll == 0)
            assert np.abs((ll - dd) - np.asarray(y)).max() <= 5e-8
    # the partially filled constant-sum pool of j = 10 came out of the library's own kink loop
    assert res[10]["stats"]["rounds"] >= 2 and 0.0 < abs((p.tenders_of(res[10])[1][4] - p.tenders_of(res[10])[0][4])[0]) < 10.0
    q = problem_of(I.two_asset(0.0))
    for j in range(0, 50, 7):
        q.set_utility(utils[j])
        v = q.solve(tol=1e-10)
        assert q.status == "optimal" and abs(v - vals[j]) <= 1e-8 * max(1.0, abs(v))
    q.close()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter(); p.solve_many(utils, tol=1e-8); best = min(best, time.perf_counter() - t0)
    print(f"two-asset.py sweep, 50 points, all five pools: {1e3 * best:.2f} ms")
    assert best <= 2e-3                                                     # (VERDICT r4 item 4's bar; 13 ms in round 4; measured 0.68: profiles/r05_small.json)
    p.close()


@pytest.mark.parametrize("seed,util", [(0, "arbitrage"), (1, "swap"), (2, "liquidate"), (3, "arbitrage"), (4, "swap"), (5, "liquidate")])
def test_swept_solves_match_one_at_a_time_on_random_tiny_networks(seed, util):
    """random networks of the reference's size with SEVERAL constant-sum pools (ties that chain through shared tokens, fills that
    leave (0, 1) and are released again) under a dozen utilities: the swept path (the library's own active-set loop) against the
    one-at-a-time path (the host's loop in cfmm/problem.py) -- same optimum, certificates of every point, tenders that add up to psi"""
    inst = random_instance(40 + seed, n_tokens=5 + seed % 3, n_pools=10 + 2 * seed, with_sum=True, utility=util)
    rng = np.random.default_rng(seed)
    # make sure there are a few constant-sum pools
    for i in range(3):
        a, b = rng.choice(inst["n_tokens"], 2, replace=False)
        inst["local_indices"].append([int(a), int(b)]); inst["reserves"].append([float(np.exp(rng.normal(2, 0.5)))] * 2)
        inst["fees"].append(float(rng.choice([0.997, 0.999, 0.99]))); inst["kinds"].append("sum"); inst["weights"].append(None); inst["params"].append(None)
    p = problem_of(inst)
    u0 = utility_of(inst)
    utils = []
    for k in range(12):
        if util == "arbitrage":
            utils.append(cfmm.Arbitrage(u0.c * np.exp(rng.normal(0, 0.02 * (1 + k), inst["n_tokens"]))))
        else:
            h = u0.h * (0.25 + 0.5 * k)
            utils.append(cfmm.Swap(h, inst["utility"]["t"]) if util == "swap" else cfmm.Liquidate(h, inst["utility"]["t"]))
    res = p.solve_many(utils, tol=1e-9)
    q = problem_of(inst)
    nsum = sum(1 for k in inst["kinds"] if k == "sum")
    for u, r in zip(utils, res):
        q.set_utility(u)
        v = q.solve(tol=1e-9)
        assert r["status"] == q.status
        if q.status != "optimal":
            continue
        assert r["gap"] <= 1e-9 and r["infeas"] <= 1e-9
        assert abs(r["value"] - v) <= 1e-7 * max(1.0, abs(v))
        assert np.abs(r["psi"] - q.psi).max() <= 1e-5 * max(1.0, np.abs(q.psi).max())
        d, l = p.tenders_of(r)
        tot = np.zeros(inst["n_tokens"])
        for li, dd, ll in zip(inst["local_indices"], d, l):
            np.add.at(tot, li, ll - dd)
        assert np.abs(tot - r["psi"]).max() <= 1e-9 * max(1.0, np.abs(r["psi"]).max())        # A (Lambda - Delta) summed IS psi (arbitrage.py:54)
    assert nsum >= 3
    p.close(); q.close()


@pytest.mark.parametrize("seed,util", [(0, "arbitrage"), (1, "swap"), (2, "liquidate"), (3, "arbitrage"), (4, "swap"), (5, "liquidate"), (6, "arbitrage"), (7, "swap")])
def test_c_abi_solve_settles_constant_sum_kinks_itself_on_small_networks(seed, util):
    """cfmm_solve with the DEFAULT method (CFMM_METHOD_AUTO: what a raw C-ABI caller gets) on networks of the reference's size with
    several constant-sum pools: the library's own active-set loop (round 6: the degenerate sweep of one point) ends on the optimum of
    the host's loop in cfmm/problem.py, with the fills folded into psi, the certificates and cfmm_get_trades2 -- sum of tenders = psi
    (arbitrage.py:54), as prob.solve() of arbitrage.py:82 returns a partially filled pool with no ceremony"""
    from cfmm import _lib
    inst = random_instance(140 + seed, n_tokens=5 + seed % 3, n_pools=10 + 2 * seed, with_sum=True, utility=util)
    rng = np.random.default_rng(seed)
    for i in range(3):
        a, b = rng.choice(inst["n_tokens"], 2, replace=False)
        inst["local_indices"].append([int(a), int(b)]); inst["reserves"].append([float(np.exp(rng.normal(2, 0.5)))] * 2)
        inst["fees"].append(float(rng.choice([0.997, 0.999, 0.99]))); inst["kinds"].append("sum"); inst["weights"].append(None); inst["params"].append(None)
    q = problem_of(inst)
    v = q.solve(tol=1e-9)
    p = problem_of(inst)
    u = utility_of(inst)
    ctx = p._ensure_ctx(); ctx.set_utility(u.c, u.h, u.ctype)
    st = ctx.solve(cfmm.start_prices(p.net, u), tol=1e-9)                 # default opts: method 0
    if q.status == "optimal":
        assert st["status"] == 1 and st["gap"] <= 1.001e-9 and st["infeas"] <= 1.001e-9, st
        assert abs(st["primal_value"] - v) <= 1e-7 * max(1.0, abs(v))
        nu, psi = ctx.get_solution()
        assert np.abs(psi - q.psi).max() <= 1e-5 * max(1.0, np.abs(q.psi).max())
        if st["method"] == _lib.METHODS["lbfgs"]:                         # (the library's loop: exact tenders that add up to psi)
            tot = np.zeros(inst["n_tokens"])
            for key in ("cp2", "w2", "sum2", "curve2", "pow2"):
                if key in p.net and len(p.net[key]["Ra"]):
                    b = p.net[key]
                    d, l = ctx.get_trades2(cfmm.problem.KIND2[key], len(b["Ra"]))
                    np.add.at(tot, b["ia"], l[0] - d[0]); np.add.at(tot, b["ib"], l[1] - d[1])
            for k, b in p.net.get("gn", {}).items():
                d, l = ctx.get_tradesN(k, b["R"].shape[1])
                for j in range(k):
                    np.add.at(tot, b["idx"][j], l[j] - d[j])
            assert np.abs(tot - psi).max() <= 1e-9 * max(1.0, np.abs(psi).max())
    p.close(); q.close()


def _sweep_record_cases():
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.join(root, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(root, "tools"))
    import sweep_records
    with open(os.path.join(root, "tests", "golden", "sweep_records.json")) as f:
        want = json.load(f)["cases"]
    cases = dict(sweep_records.cases())
    assert set(want) <= set(cases) and "two_asset_50" in want and sum(1 for k in want if k.startswith("tiny")) >= 4
    return [(name, cases[name], want[name]) for name in sorted(want)]


@pytest.mark.parametrize("name,run,want", [pytest.param(*c, id=c[0]) for c in _sweep_record_cases()])
def test_swept_solve_repeats_the_recorded_rounds(name, run, want):
    """tools/sweep_records.py: cfmm_solve_sweep straight through the binding on the two-asset sweep at its 50 points, the six random
    tiny networks of the test above under their dozen utilities, a network without constant-sum pools (one leg per point), and the
    shipped arbitrage instance through cfmm_solve with the default method (the library's one-point sweep).  The golden file holds what
    the build BEFORE cfmm_solve_sweep was divided into rules (sweep_rules.hpp) and phases recorded in TEN runs (the first three agreed
    bit for bit on a case that the later ones moved).  Per point the status, evaluations, iterations, rounds, method and the tied pools'
    signs are those exactly.  The network without constant-sum pools is left out: its evaluation counts did not repeat on that build.
    Theta, the dual value and psi: the one-workgroup solve is NOT run-to-run deterministic where several waves add into the LDS tile.
    Two cases (tiny0_arbitrage, the arbitrage instance) repeated bit for bit in all runs and are held to that.  The others spread by up
    to 1.1e-13 in psi, 3.6e-14 in the value and 1.3e-15 in theta -- 6.8e-4 in tiny2_liquidate, whose tied pools share tokens so that
    the fills are not unique -- and each quantity is held to ten times its own case's spread (a quantity that happened to repeat in a
    case that did not: ten times the case's largest spread).  The file's header and per-case `spread` hold the figures."""
    import sweep_records
    got = run()
    assert len(got) == len(want["points"])
    val = lambda h: np.array([float.fromhex(x) for x in h])
    for b, (g, w) in enumerate(zip(got, want["points"])):
        print(name, b, {k: g[k] for k in sweep_records.INTS}, g["theta"])
        for k in sweep_records.INTS:
            assert g[k] == w[k], (name, b, k, g, w)
        for q in sweep_records.RAW:
            tol = want["tolerance"][q]
            if tol == 0.0:
                assert g["raw"][q] == w["raw"][q], (name, b, q, g, w)
            else:
                vg, vw = val(g["raw"][q]), val(w["raw"][q])
                assert np.array_equal(np.isnan(vg), np.isnan(vw)) and np.nanmax(np.abs(vg - vw), initial=0.0) <= tol, (name, b, q, g, w)


def _kink_network(seed):
    """constant-product and constant-sum pools only (what cfmm_solve_batch takes) of the reference's size, three constant-sum pools
    more, as in test_c_abi_solve_settles_constant_sum_kinks_itself_on_small_networks"""
    inst = random_instance(140 + seed, n_tokens=5 + seed % 3, n_pools=10 + 2 * seed, with_sum=True, two_asset_only=True)
    inst["weights"] = [None] * len(inst["kinds"])                         # (every geo-mean pool constant-product)
    rng = np.random.default_rng(seed)
    for i in range(3):
        a, b = rng.choice(inst["n_tokens"], 2, replace=False)
        inst["local_indices"].append([int(a), int(b)]); inst["reserves"].append([float(np.exp(rng.normal(2, 0.5)))] * 2)
        inst["fees"].append(float(rng.choice([0.997, 0.999, 0.99]))); inst["kinds"].append("sum"); inst["weights"].append(None); inst["params"].append(None)
    return inst


def _solved_in_the_kink_loop(inst):
    """a context of `inst` after a default-method solve that the library's own kink loop settled (it left its tenders)"""
    p = problem_of(inst)
    u = utility_of(inst)
    ctx = p._ensure_ctx(); ctx.set_utility(u.c, u.h, u.ctype)
    st = ctx.solve(cfmm.start_prices(p.net, u), tol=1e-9)
    assert st["status"] == 1 and st["method"] == _lib.METHODS["lbfgs"], st
    return p, u, ctx


def _trades2_of(ctx, net):
    return {key: ctx.get_trades2(cfmm.problem.KIND2[key], len(net[key]["Ra"])) for key in cfmm.problem.KIND2 if key in net and len(net[key]["Ra"])}


def test_batch_solve_after_the_kink_loop_reads_back_its_own_tenders():
    """the kink loop's tenders describe the point of the solve that left them: after a batch solve moves the context to other prices,
    cfmm_get_trades2 returns the tenders at THOSE prices -- bit for bit what a fresh context returns there -- and they add up to the
    batch's psi (cfmm.h: "afterwards every context is read back as after cfmm_solve")"""
    inst = _kink_network(0)
    p, u, ctx = _solved_in_the_kink_loop(inst)
    ctx.set_utility(np.asarray(u.c) * np.exp(np.random.default_rng(1).normal(0, 0.05, inst["n_tokens"])))
    ctx.solve_batch([], tol=1e-9)
    nu, psi = ctx.get_solution()
    fresh = problem_of(inst)
    f = fresh._ensure_ctx(); f.set_nu(nu)
    got, want = _trades2_of(ctx, p.net), _trades2_of(f, p.net)
    assert set(got) == {"cp2", "sum2"}
    tot = np.zeros(inst["n_tokens"])
    for key, (d, l) in got.items():
        assert np.array_equal(d, want[key][0]) and np.array_equal(l, want[key][1]), key
        np.add.at(tot, p.net[key]["ia"], l[0] - d[0]); np.add.at(tot, p.net[key]["ib"], l[1] - d[1])
    assert np.abs(tot - psi).max() <= 1e-9 * max(1.0, np.abs(psi).max())
    p.close(); fresh.close()


def test_tie_flags_after_the_kink_loop_apply_to_the_read_back():
    """cfmm_set_pool_flags after a solve the kink loop settled: the read-back follows the new flags, as a fresh context's does at the
    same prices"""
    inst = _kink_network(0)
    p, _, ctx = _solved_in_the_kink_loop(inst)
    nu, _ = ctx.get_solution()
    flags = np.ones(len(p.net["sum2"]["Ra"]), dtype=np.int32)
    ctx.set_pool_flags(_lib.POOL_SUM2, flags)
    fresh = problem_of(inst)
    f = fresh._ensure_ctx(); f.set_nu(nu); f.set_pool_flags(_lib.POOL_SUM2, flags)
    got, want = _trades2_of(ctx, p.net), _trades2_of(f, p.net)
    assert set(got) == {"cp2", "sum2"}
    for key, (d, l) in got.items():
        assert np.array_equal(d, want[key][0]) and np.array_equal(l, want[key][1]), key
    p.close(); fresh.close()


def test_sweep_call_refuses_what_it_cannot_index():
    """cfmm_solve_sweep's host half indexes the prices with the constant-sum columns handed in: ids out of range, a non-positive
    reserve, a fee outside (0, 1], a non-finite offset, a utility-table entry, a count that differs from the upload -- each is an
    error with its reason, not a read past the price vector; an empty sweep is an error too"""
    from cfmm import _lib
    inst = I.two_asset(0.0)
    p = problem_of(inst)
    ctx, n = p._ensure_ctx(), inst["n_tokens"]
    s2 = {k: np.array(v, copy=True) for k, v in p.net["sum2"].items() if k in ("ia", "ib", "fee", "Ra", "Rb")}
    c = np.zeros((2, n)); c[:, 2] = 1.0
    h = np.zeros((2, n)); h[:, 0] = 5.0
    ct = np.zeros((2, n), dtype=np.int32)
    nu0 = np.ones((2, n))
    ok = ctx.solve_sweep(c, h, ct, nu0, sum2=s2, tol=1e-8)
    assert all(st["status"] == 1 for st in ok[5])
    def bad(msg, **kw):
        args = dict(c=c, h=h, ctype=ct, nu0=nu0, sum2=s2); args.update(kw)
        with pytest.raises(_lib.CfmmError, match=msg):
            ctx.solve_sweep(args["c"], args["h"], args["ctype"], args["nu0"], sum2=args["sum2"])
    bad("out of range", sum2=dict(s2, ia=np.array([n], dtype=np.int32)))
    bad("out of range", sum2=dict(s2, ib=s2["ia"]))
    bad("fee", sum2=dict(s2, fee=np.array([1.5])))
    bad("reserves", sum2=dict(s2, Rb=np.array([0.0])))
    bad("handed in", sum2=None)
    hh = h.copy(); hh[1, 1] = np.inf
    bad("not finite", h=hh)
    cc = c.copy(); cc[0, 0] = -1.0
    bad("c\\[0\\] < 0", c=cc)
    nn = nu0.copy(); nn[1, 2] = 0.0
    bad("positive finite price", nu0=nn)
    tt = ct.copy(); tt[0, 1] = 3
    bad("utility table", ctype=tt)
    bad("no points", c=c[:0], h=h[:0], ctype=ct[:0], nu0=nu0[:0])
    p.close()


@pytest.mark.parametrize("seed", range(4))
def test_tiny_one_launch_solve_matches_the_grid_path(seed, monkeypatch):
    """networks of the reference's own size (<= 64 tokens, <= 64 wave-tiles) are solved by ONE workgroup in ONE launch
    (tiny.hpp: tiles stay in LDS, the update is one wave); CFMM_TINY=0 sends the same instance through the grid-wide
    kernels: same optimum, same certificates, comparable evaluation counts -- price ties (a constant-sum pool on its
    kink) included"""
    inst = random_instance(seed, n_tokens=5 + seed, n_pools=8 + 3 * seed, with_sum=True, utility=("arbitrage", "liquidate", "swap", "arbitrage")[seed])
    res = {}
    for tiny in ("1", "0"):
        monkeypatch.setenv("CFMM_TINY", tiny)
        p = problem_of(inst)
        v = p.solve(tol=1e-9)
        res[tiny] = (v, p.status, p.psi.copy(), p.stats["evals"], p.gap, p.infeas)
        p.close()
    (v1, s1, psi1, e1, g1, i1), (v0, s0, psi0, e0, g0, i0) = res["1"], res["0"]
    assert s1 == s0 == "optimal" and max(g1, g0, i1, i0) <= 1e-9
    assert abs(v1 - v0) <= 1e-8 * max(1.0, abs(v0))
    assert np.abs(psi1 - psi0).max() <= 1e-6 * max(1.0, np.abs(psi0).max())
    assert e1 <= 2 * e0 + 20 and e0 <= 2 * e1 + 20


@pytest.mark.parametrize("seed", range(6))
def test_random_small_instances_vs_primal(seed):
    from oracle.primal_scipy import solve_primal
    util = ["arbitrage", "swap", "liquidate"][seed % 3]
    inst = random_instance(200 + seed, n_tokens=6, n_pools=14, with_sum=True, with_curve=True, utility=util)
    p = problem_of(inst)
    v = p.solve(tol=1e-9)
    r = solve_primal(normalise_with_params(inst))
    if p.status == "infeasible":          # a token to sell that no pool lists: SLSQP fails on it too
        assert not r["success"]
        return
    assert p.status == "optimal" and p.gap <= 1e-8 and p.infeas <= 1e-8       # self-certifying
    assert r["value"] <= v + 2e-6 * max(1, abs(v))                            # weak duality vs SLSQP's point
    if r["success"]:
        assert abs(v - r["value"]) <= 2e-6 * max(1, abs(v)), (v, r["value"])
    p.close()


@pytest.mark.parametrize("seed,kw,value", [
    (1313, dict(n_tokens=7, n_pools=10, with_sum=True, with_curve=False, with_power=False, utility="liquidate"), 24.4327269044),
    (1367, dict(n_tokens=8, n_pools=8, with_sum=True, with_curve=True, with_power=False, utility="liquidate"), 0.0),
    (1387, dict(n_tokens=7, n_pools=4, with_sum=True, with_curve=True, with_power=False, utility="swap"), 0.0),
    (1091, dict(n_tokens=6, n_pools=5, with_sum=True, with_curve=True, with_power=False, utility="liquidate"), None),
])
def test_worthless_components_found_by_the_fuzz_campaign(seed, kw, value):
    """tools/fuzz_small.py's finds.  Tokens from which no chain of pools leads to anything the utility values (a disconnected
    component; a target no pool lists) have prices that run to zero together -- the dual is flat along that ray and the pools among them
    trade at whatever ratio the last iterate had.  The program is FEASIBLE (a pool all of whose tokens are worthless can be left alone, a
    worthless token that must go can be GIVEN to a pool that lists it: Delta > 0, Lambda = 0 -- cvxpy solves these, SLSQP too) and used
    to come back "infeasible".  Now: optimal, SLSQP's value, tenders that add up to psi and keep every pool feasible.  Seed 1091 has a
    token to sell that NO pool lists: that one IS infeasible, and says so instead of raising on a collapsed price."""
    from oracle.primal_scipy import solve_primal
    inst = random_instance(seed, **kw)
    p = problem_of(inst)
    v = p.solve(tol=1e-9)
    if value is None:
        assert p.status == "infeasible"
        p.close()
        return
    assert p.status == "optimal" and p.gap <= 1e-9 and p.infeas <= 1e-9, (p.status, p.gap, p.infeas)
    assert abs(v - value) <= 1e-8 * max(1.0, abs(value)) and p.stats["worthless_tokens"] >= 2
    r = solve_primal(normalise_with_params(inst))
    assert r["success"] and abs(r["value"] - v) <= 2e-6 * max(1.0, abs(v))
    tot = np.zeros(inst["n_tokens"])
    for li, R, g, kind, dd, ll in zip(inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], p.deltas, p.lambdas):
        np.add.at(tot, li, ll - dd)
        assert np.all(dd >= 0) and np.all(ll >= 0)
        x = np.asarray(R) + g * dd - ll
        assert np.all(x > 0) or kind == "sum"
        if kind == "sum":
            assert np.all(x >= -1e-9) and x.sum() >= np.sum(R) * (1 - 1e-12)
    assert np.abs(tot - p.psi).max() <= 1e-9 * max(1.0, np.abs(p.psi).max())
    u = utility_of(inst)
    rr = p.psi + u.h
    assert np.all(np.where(u.ctype == 1, np.abs(rr), np.maximum(-rr, 0.0)) <= 1e-8 * max(1.0, np.abs(u.h).max()))
    p.close()


@pytest.mark.parametrize("seed,kw", [
    (1132, dict(n_tokens=7, n_pools=5, with_sum=False, with_curve=False, with_power=False, utility="swap")),
    (1099, dict(n_tokens=4, n_pools=5, with_sum=True, with_curve=True, with_power=False, utility="swap")),
    (1329, dict(n_tokens=5, n_pools=4, with_sum=True, with_curve=False, with_power=False, utility="arbitrage")),
])
def test_second_order_path_with_tokens_no_pool_lists(seed, kw):
    """more of the campaign's finds: a token that NO pool lists and whose offset is zero has nothing on its row of the second-order
    system but the barrier's -mu (the step ran away: "infeasible" after 200 steps) -- pinned now; and the diagonal's own term
    nu_j (psi_j + h_j) is taken without the barrier's -mu (it vanished exactly at a barrier token's optimum: singular rows).
    method="newton" and the default path reach the same certified optimum"""
    inst = random_instance(seed, **kw)
    p = problem_of(inst)
    v = p.solve(tol=1e-9)
    assert p.status == "optimal", (p.status, p.gap, p.infeas)
    v2 = p.solve(tol=1e-8, method="newton")
    assert p.status == "optimal" and p.stats["newton_steps"] <= 80 and abs(v2 - v) <= 1e-6 * max(1.0, abs(v)), (p.status, v, v2, p.stats)
    p.close()


def test_generic_bucket_power_sum_pools_end_to_end(oracle_lib):
    """SURVEY 8(f) rank 4 on the device: a trading function that exists in the library as ONE table entry (csrc/phi2.hpp:
    Phi2<4>, the power sum x^(1-t) + y^(1-t)) and rides in the generic two-asset bucket.  Its exact pool solution, its share of
    the diagonal metric, its tenders, its barrier-smoothed solution and Hessian term all come from the generic code on that
    entry; the oracle's closed form (which the device never uses) is the independent check.  20 000 such pools among
    28 000 pools of the reference's kinds, 200 tokens."""
    from oracle import barrier_np
    net = synthetic.config("G4", seed=2)
    n = net["n_tokens"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    p._ensure_ctx().selftest()             # includes pool_generic2 on the three closed-form kinds, started from D = 0
    o = _oracle_for(oracle_lib, net)
    nu = net["c"] * np.exp(np.random.default_rng(7).normal(0, 0.04, n))
    f, psi, diag = p.eval_dual(nu, want_diag=True)
    f0, psi0, diag0 = o.eval(nu, True)
    assert abs(f - f0) <= 1e-10 * abs(f0) and np.abs(psi - psi0).max() <= 1e-10 * np.abs(psi0).max()
    assert np.abs(diag - diag0).max() <= 1e-10 * np.abs(diag0).max()
    # the pool-by-pool tenders of the generic bucket, and the invariant they preserve
    p.ctx.set_nu(nu)
    d, l = p.bucket_trades("pow2")
    ya, yb = o.trades2([k for k, _ in o.b2].index("pow2"), nu)
    b = net["pow2"]
    assert np.all(d >= 0) and np.all(l >= 0) and np.all(d * l == 0)
    assert np.abs((l - d)[0] - ya).max() <= 1e-10 * b["Ra"].max() and np.abs((l - d)[1] - yb).max() <= 1e-10 * b["Rb"].max()
    q = 1.0 - b["t"]
    xa, xb = b["Ra"] + b["fee"] * d[0] - l[0], b["Rb"] + b["fee"] * d[1] - l[1]
    assert np.abs((xa ** q + xb ** q) / (b["Ra"] ** q + b["Rb"] ** q) - 1).max() <= 1e-12
    assert ((l - d)[0] != 0).mean() > 0.5
    # the solve, first order and second order, against the oracle's solver
    r = o.solve(net["c"], tol=1e-6)
    v1 = p.solve(tol=1e-6, method="lbfgs")
    assert p.status == "optimal" and abs(v1 - r["primal_value"]) <= 2e-6 * abs(v1)
    v2 = p.solve(tol=1e-6, method="newton")
    assert p.status == "optimal" and abs(v2 - r["primal_value"]) <= 2e-6 * abs(v2) and p.stats["newton_steps"] >= 2
    # the smoothed evaluation (value, psi, Hessian) against its NumPy restatement
    small = synthetic.make_network(40, m_cp2=300, m_pow2=500, seed=9)
    ps = cfmm.Problem.from_network(small, utility=cfmm.Arbitrage(small["c"]))
    nus = small["prices"] * np.exp(np.random.default_rng(1).normal(0, 0.03, 40))
    for mu in (1e-2, 1e-6):
        val, tr, psm, H = ps._ensure_ctx().eval_smooth(nus, mu, want_hessian=True)
        ref = barrier_np.smooth_eval(small, nus, mu, hessian=True)
        assert abs(val - ref["value"]) <= 1e-9 * max(1.0, abs(ref["value"])) and np.abs(psm - ref["psi"]).max() <= 1e-9 * np.abs(ref["psi"]).max()
        assert np.abs(np.tril(H) - np.tril(ref["H"])).max() <= 1e-7 * np.abs(ref["H"]).max()
    ps.close(); p.close()


@pytest.mark.parametrize("seed", range(4))
def test_random_small_instances_with_power_sum_pools_vs_primal(seed):
    """the generic bucket on the reference's own scale: 5 tokens / 10 pools with power-sum pools among geo-mean ones,
    both outer iterations, against the primal program solved by SciPy with the same phi"""
    from oracle.primal_scipy import solve_primal
    inst = random_instance(30 + seed, n_tokens=5, n_pools=10, with_sum=False, with_power=True, utility=["arbitrage", "swap"][seed % 2])
    r = solve_primal(normalise_with_params(inst))
    p = problem_of(inst)
    for method in ("lbfgs", "newton"):
        v = p.solve(tol=1e-9, method=method)
        assert p.status == "optimal", (method, p.status)
        assert abs(v - r["value"]) <= 2e-6 * max(1.0, abs(v)), (method, v, r["value"])
        for d, l, y in zip(p.deltas, p.lambdas, r["y"]):
            assert np.abs((l - d) - y).max() <= 2e-4 * max(1.0, np.abs(y).max())
    p.close()


def test_error_behaviour():
    ctx = _lib.Context(4)
    with pytest.raises(cfmm.CfmmError, match="token ids"):
        ctx.upload_pools2(_lib.POOL_CP2, [1.0], [1.0], [0.99], [0], [7])
    with pytest.raises(cfmm.CfmmError, match="pool size"):
        ctx.upload_poolsN(np.zeros((9, 1), dtype=np.int32), np.ones((9, 1)), np.ones((9, 1)) / 9, [0.99])
    with pytest.raises(cfmm.CfmmError, match="set_utility"):
        ctx.solve(np.ones(4))
    ctx.set_utility(np.ones(4))
    with pytest.raises(cfmm.CfmmError, match="no pools"):
        ctx.solve(np.ones(4))
    ctx.upload_pools2(_lib.POOL_CP2, [1.0], [1.0], [0.99], [0], [1])
    with pytest.raises(cfmm.CfmmError, match="positive finite"):
        ctx.solve(np.array([1.0, -1.0, 1.0, 1.0]))
    with pytest.raises(cfmm.CfmmError, match="fee"):
        ctx.upload_pools2(_lib.POOL_CP2, [1.0], [1.0], [1.5], [0], [1])
    with pytest.raises(cfmm.CfmmError, match="reserve"):
        ctx.upload_pools2(_lib.POOL_CP2, [1.0], [-2.0], [0.99], [0], [1])
    with pytest.raises(cfmm.CfmmError, match="weight"):
        ctx.upload_pools2(_lib.POOL_W2, [1.0], [1.0], [0.99], [0], [1], param=[1.0])
    with pytest.raises(cfmm.CfmmError, match="reserve|weight"):
        ctx.upload_poolsN(np.array([[0], [1], [2]], dtype=np.int32), np.array([[1.0], [0.0], [1.0]]), np.ones((3, 1)) / 3, [0.99])
    # empty bucket upload is allowed and clears the bucket
    ctx.upload_pools2(_lib.POOL_W2, [], [], [], [], [], param=[])
    assert ctx.pool_count() == 1
    ctx.close()
    with pytest.raises(cfmm.CfmmError, match="LDS-staged limit"):
        _lib.Context(50_000)


def test_hub_tokens_zipf_stress(oracle_lib):
    """heavy-tailed token popularity: most pools touch a few hub tokens (LDS atomic contention)"""
    net = synthetic.make_network(500, m_cp2=200_000, seed=5, zipf_s=1.1)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    o = _oracle_for(oracle_lib, net)
    nu = net["c"] * np.exp(np.random.default_rng(0).normal(0, 0.02, 500))
    f1, psi1 = p.eval_dual(nu)
    f0, psi0 = o.eval(nu)
    assert abs(f1 - f0) <= 1e-11 * abs(f0)
    assert np.abs(psi1 - psi0).max() <= 1e-9 * np.abs(psi0).max()
    p.close()


def test_integration_md_ctypes_stub_runs():
    """the raw ctypes stub printed in INTEGRATION.md section 3 is executed verbatim"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    md = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", md, re.S)
    stub = [b for b in blocks if "cfmm_create" in b]
    assert len(stub) == 2 and "cfmm_solve_sweep" in stub[1]
    ns = {}
    assert "o.method" not in stub[0].split("cfmm_default_opts")[1].split("cfmm_solve")[0].replace("(o.method stays", "")     # the DEFAULT method (round 6)
    exec(stub[0].replace("<repo>", root), ns)
    st = ns["st"]
    # the full five-pool instance of arbitrage.py through the raw ABI: prob.value of arbitrage.py:84 -- with CFMM_METHOD_AUTO the library's
    # own active-set loop settles the constant-sum pool's kink (first order: stats.method 1, no barrier weight) ...
    assert st.method == 1 and st.barrier_mu == 0.0
    assert st.status == 1 and st.gap <= 1e-9 and st.infeas <= 1e-9
    assert abs(st.primal_value - 21.4998087635) <= 1e-7 and abs(st.primal_value - golden()["arbitrage"]["kkt"]["value"]) <= 1e-7
    assert np.all(ns["psi"] >= -1e-8 * np.abs(ns["psi"]).max())
    assert np.abs(ns["psi"] - np.asarray(golden()["arbitrage"]["kkt"]["psi"])).max() <= 1e-6
    # ... and the partially filled constant-sum pool's net tender (38.6 % of its reserve, arbitrage.py:12,20,28)
    y = ns["lam"] - ns["dlt"]
    assert np.abs(y[:, 0] - np.asarray(golden()["arbitrage"]["kkt"]["y"][4])).max() <= 1e-6
    assert 0.386 < abs(y[0, 0]) / 10.0 < 0.3875 and 0.386 < abs(y[1, 0]) / 10.0 < 0.3875      # (the 38.6 % fill, read from cfmm_get_trades2)
    # ... and the same point through the barrier path asked for by name (what the stub did before round 6)
    ns2 = {}
    exec(stub[0].replace("<repo>", root).replace("o.tol_gap, o.tol_infeas = 1e-9, 1e-9", "o.method, o.tol_gap, o.tol_infeas = 2, 1e-9, 1e-9"), ns2)
    assert ns2["st"].status == 1 and ns2["st"].method == 2 and abs(ns2["st"].primal_value - st.primal_value) <= 1e-7
    assert np.abs((ns2["lam"] - ns2["dlt"]) - y).max() <= 1e-6
    # section 3b (continues the same namespace): two-asset.py's 50-point sweep, all five pools, as ONE raw call
    exec(stub[1], ns)
    assert all(ns["stats"][j].status == 1 for j in range(50)) and np.all(np.diff(ns["all_values"]) > 0)
    assert ns["on_kink"].sum() >= 5                                        # (the constant-sum pool is partially filled at many points)
    for j in (0, 1, 10, 25, 49):
        k = golden()[f"two_asset_{j}"]["kkt"]
        assert abs(ns["all_values"][j] - k["value"]) <= 1e-8 * max(1.0, abs(k["value"]))
        assert np.abs(ns["psi_all"][j] - np.asarray(k["psi"])).max() <= 5e-8


def test_full_size_c4_single_gpu_streams_from_hbm():
    """BASELINE config 4's whole pool set (1e7 constant-product pools / 2000 tokens, 320 MB: larger than
    the Infinity Cache) on ONE GPU: solve to the certificates, then size-independent checks"""
    net = synthetic.config("C4", seed=0)
    n = net["n_tokens"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    v = p.solve(tol=1e-6)
    assert p.status == "optimal" and p.gap <= 1e-6 and p.infeas <= 1e-6 and p.stats["evals"] < 200
    b = net["cp2"]
    d, l = p.bucket_trades("cp2")
    y = l - d
    assert np.all(d * l == 0) and np.all(d >= 0) and np.all(l >= 0)
    psi = np.bincount(b["ia"], weights=y[0], minlength=n) + np.bincount(b["ib"], weights=y[1], minlength=n)
    assert np.abs(psi - p.psi).max() <= 1e-9 * np.abs(psi).max()
    xa = b["Ra"] + b["fee"] * d[0] - l[0]; xb = b["Rb"] + b["fee"] * d[1] - l[1]
    assert np.abs(0.5 * np.log(xa / b["Ra"]) + 0.5 * np.log(xb / b["Rb"])).max() <= 1e-12
    # weak duality: the dual value bounds the objective of every FEASIBLE psi from above; this psi satisfies psi >= 0 only to
    # the 1e-6 certificate, so it may overshoot the bound by that much
    assert -1e-6 * abs(v) <= p.dual_value - v <= 2e-6 * abs(v)
    p.close()


@pytest.mark.parametrize("kind", ["liquidate", "swap"])
def test_basket_utilities_at_scale_match_oracle(oracle_lib, kind):
    """liquidation.py:57,77-80 / two-asset.py:66,86 utilities on a 1e5-pool mixed network"""
    net = synthetic.config("C3", scale=0.1, seed=2)
    n = net["n_tokens"]
    rng = np.random.default_rng(7)
    h = np.zeros(n); idx = rng.choice(n, 10, replace=False)
    h[idx] = np.exp(rng.normal(2, 0.5, 10)) / net["prices"][idx] * 10
    t = int(rng.integers(0, n)); h[t] = 0.0
    u = cfmm.Liquidate(h, t) if kind == "liquidate" else cfmm.Swap(h, t)
    p = cfmm.Problem.from_network(net, utility=u)
    v = p.solve(tol=1e-7)
    o = oracle_lib.Oracle(n, threads=4); o.add_network(net); o.set_utility(u.c, u.h, u.ctype)
    r = o.solve(cfmm.start_prices(net, u), tol=1e-7)
    assert p.status == "optimal" and r["status"] == 1
    assert abs(v - r["primal_value"]) <= 2e-6 * abs(v)
    res = p.psi + u.h
    if kind == "liquidate":
        mask = np.arange(n) != t
        assert np.abs(res[mask]).max() <= 1e-6 * max(np.abs(p.psi).max(), h.max())
    else:
        assert res.min() >= -1e-6 * max(np.abs(p.psi).max(), h.max())
    # ... and the independent dual referee (round 6: SciPy L-BFGS-B over the NumPy pools, nothing of the device's iteration in it): weak
    # duality holds against its bound, and the bound is tight
    from oracle import dual_np
    d = dual_np.solve_dual_network(net, u.c, u.h, u.ctype, nu0=cfmm.start_prices(net, u))
    assert v <= d["value"] + 1e-6 * max(1.0, abs(v)) and d["value"] - v <= 2e-5 * max(1.0, abs(v)), (v, d["value"], d["pg"], d["evals"])
    p.close()


def test_virtual_shards_on_the_gpu_sum_to_the_unsharded_evaluation():
    """pool-sharding without a second GPU: S shards evaluated one after the other on
    the device and summed on the host equal the unsharded dual evaluation"""
    net = synthetic.config("C3", scale=0.05, seed=4)
    n = net["n_tokens"]
    nu = net["c"] * np.exp(np.random.default_rng(0).normal(0, 0.02, n))
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    f, psi = p.eval_dual(nu)
    p.close()
    for S in (2, 8):
        fs, ps = 0.0, np.zeros(n)
        for r in range(S):
            q = cfmm.Problem.from_network(cfmm.distributed.rank_network(net, r, S), utility=cfmm.Arbitrage(net["c"]))
            fr, pr = q.eval_dual(nu)
            fs += fr; ps += pr
            q.close()
        assert abs(fs - f) <= 1e-11 * abs(f)
        assert np.abs(ps - psi).max() <= 1e-10 * np.abs(psi).max()


@pytest.mark.parametrize("fused", [None, "0"], ids=["default", "two_launch"])
def test_eager_iteration_path_matches_graph_path(tmp_path, fused):
    """the pool-sharded build enqueues its iterations eagerly (RCCL between the kernels) instead of
    replaying a captured graph; CFMM_NO_GRAPH=1 drives the same control flow on one GPU.
    (On this network the one-launch iteration applies, which is enqueued eagerly whatever CFMM_NO_GRAPH says: `two_launch` sets
    CFMM_FUSED=0 on both sides, so that the chunk driver replays the graph on one and enqueues on the other.)"""
    import subprocess, sys, json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import cfmm; from cfmm import synthetic; "
            "net = synthetic.config('C3', scale=0.05, seed=0); p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net['c'])); "
            "v = p.solve(tol=1e-6); print(json.dumps(dict(v=v, status=p.status, evals=p.stats['evals'], nu=p.nu.tolist())))"
            % (root, os.path.join(root, "cfmm-routing-code_amd")))
    out = {}
    for mode in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_NO_GRAPH=mode, **({} if fused is None else {"CFMM_FUSED": fused})),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["0"]["status"] == out["1"]["status"] == "optimal"
    assert out["0"]["evals"] == out["1"]["evals"]
    assert abs(out["0"]["v"] - out["1"]["v"]) <= 1e-9 * abs(out["0"]["v"])


@pytest.mark.parametrize("allreduce", ["rccl", "oneshot"])
def test_pool_sharded_path_with_a_one_rank_communicator(allreduce):
    """the whole N > 1 code path on ONE GPU: torch.distributed(nccl) rendezvous, communicator id broadcast,
    cfmm_comm_init (RCCL resolved at run time, warm-up all-reduce), eager iterations with fold + ncclAllReduce
    + update -- a communicator of one rank runs exactly what every rank of an 8-GPU job runs"""
    import subprocess, sys, json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = '''
import sys, os, json
sys.path[:0] = [%r, %r]
import torch, torch.distributed as dist
import cfmm
from cfmm import synthetic
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
net = synthetic.config("C3", scale=0.05, seed=0)
p = cfmm.distributed.sharded_problem(net, cfmm.Arbitrage(net["c"]), dist=dist, device=0, allreduce=%r)
v = p.solve(tol=1e-6)
f, psi = p.eval_dual(p.nu)
q = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
w = q.solve(tol=1e-6)
f2, psi2 = q.eval_dual(p.nu)
print(json.dumps(dict(v=v, w=w, status=p.status, evals=p.stats["evals"], evals1=q.stats["evals"], ranks=p.stats["n_ranks"],
                      df=abs(f - f2) / abs(f2), dpsi=float(abs(psi - psi2).max() / abs(psi2).max()))))
dist.destroy_process_group()
''' % (root, os.path.join(root, "cfmm-routing-code_amd"), allreduce)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["status"] == "optimal" and out["ranks"] == 1
    assert out["evals"] == out["evals1"]
    assert abs(out["v"] - out["w"]) <= 1e-9 * abs(out["w"])
    assert out["df"] <= 1e-12 and out["dpsi"] <= 1e-10


@pytest.mark.parametrize("deterministic", [False, True])
def test_clones_share_pools_and_solve_many_matches_sequential(deterministic):
    """cfmm_clone: several solves in flight over ONE resident pool set give the same answers as one after
    the other; re-uploading pools while clones exist is refused.  In reproducible mode "the same" is bitwise."""
    net = synthetic.config("C3", scale=0.1, seed=3)
    n = net["n_tokens"]
    rng = np.random.default_rng(11)
    utils = [cfmm.Arbitrage(net["c"] * np.exp(rng.normal(0, 0.01, n))) for _ in range(6)]
    h = np.zeros(n); idx = rng.choice(n, 5, replace=False); h[idx] = 50.0 / net["prices"][idx]
    utils.append(cfmm.Swap(h, int(rng.integers(0, n))))
    p = cfmm.Problem.from_network(net, utility=utils[0], deterministic=deterministic)
    seq = []
    for u in utils:
        p.set_utility(u); p.solve(tol=1e-7)
        seq.append((p.value, p.status, p.psi.copy(), p.stats["evals"]))
    for conc in (1, 3):
        res = p.solve_many(utils, concurrency=conc, tol=1e-7, batch=0)         # (host threads over clones; the batched path is tested below)
        for (v, st, psi, ev), r in zip(seq, res):
            assert r["status"] == st == "optimal"
            if deterministic:
                assert r["value"] == v and r["stats"]["evals"] == ev and np.array_equal(r["psi"], psi)
            else:
                # (fp64 atomics are order-nondeterministic: two runs agree to the solver tolerance, not bitwise)
                assert abs(r["value"] - v) <= 5e-7 * abs(v)
                assert np.abs(r["psi"] - psi).max() <= 1e-4 * np.abs(psi).max()
    q = p.clone()
    with pytest.raises(cfmm.CfmmError, match="shared with a clone"):
        p.ctx.upload_pools2(_lib.POOL_CP2, [1.0], [1.0], [0.99], [0], [1])
    q.close()
    p.ctx.upload_pools2(_lib.POOL_SUM2, [1.0], [1.0], [0.99], [0], [1])      # fine again once the clone is gone
    p.close()


# ---------------------------------------------------------------------------------------------------------------
# batched solves (cfmm_solve_batch): B price vectors per pool read
# ---------------------------------------------------------------------------------------------------------------
def _mixed_utilities(net, rng, count):
    """arbitrage under perturbed market values, liquidations and swaps of random baskets (arbitrage.py:57,77,
    liquidation.py:57,77-80, two-asset.py:66,86): solves that need different numbers of iterations"""
    n = net["n_tokens"]
    out = []
    for k in range(count):
        if k % 3 == 0:
            out.append(cfmm.Arbitrage(net["c"] * np.exp(rng.normal(0, 0.003 * (1 + k), n))))
        else:
            h = np.zeros(n); idx = rng.choice(n, 4 + k, replace=False)
            h[idx] = np.exp(rng.normal(2, 0.5, idx.size)) / net["prices"][idx] * 10
            t = int(rng.integers(0, n)); h[t] = 0.0
            out.append(cfmm.Liquidate(h, t) if k % 3 == 1 else cfmm.Swap(h, t))
    return out


@pytest.mark.parametrize("n_tokens,memory,count", [(1000, 0, 8), (300, 8, 5), (1500, 0, 4), (3000, 0, 2)])
def test_batched_solves_match_the_oracle_and_single_solves(oracle_lib, n_tokens, memory, count):
    """B solves in lock-step over one pool set -- one pool read per iteration for all of them -- reach the optimum of the
    oracle's solver and of the single-solve path, each with its own certificates, whatever iteration each one ends at;
    every instantiation of the batched update (Gram form, register form 2 / 4 per thread, generic) is covered"""
    net = synthetic.make_network(n_tokens, m_cp2=60_000, m_w2=20_000, m_gn=10_000, seed=21)
    rng = np.random.default_rng(5)
    utils = _mixed_utilities(net, rng, count)
    p = cfmm.Problem.from_network(net, utility=utils[0])
    assert p._ensure_ctx().batch_capacity() >= min(count, 2)
    res = p.solve_many(utils, tol=1e-7, memory=memory)
    assert len(res) == count
    evs = [r["stats"]["evals"] for r in res]
    assert len(set(evs)) > 1 or count <= 2                                 # (the solves do end at different iterations)
    q = cfmm.Problem.from_network(net, utility=utils[0])
    for u, r in zip(utils, res):
        assert r["status"] == "optimal" and r["gap"] <= 1e-7 and r["infeas"] <= 1e-7
        assert r["stats"]["batch"] == min(count, p.ctx.batch_capacity())
        o = oracle_lib.Oracle(n_tokens, threads=4); o.add_network(net); o.set_utility(u.c, u.h, u.ctype)
        ro = o.solve(cfmm.start_prices(net, u), tol=1e-7, memory=memory)
        assert ro["status"] == 1
        assert abs(r["value"] - ro["primal_value"]) <= 2e-6 * max(abs(r["value"]), 1.0)
        q.set_utility(u)
        v1 = q.solve(tol=1e-7, memory=memory)
        assert q.status == "optimal" and abs(r["value"] - v1) <= 1e-6 * max(abs(v1), 1.0)
        assert np.abs(r["psi"] - q.psi).max() <= 1e-4 * np.abs(q.psi).max()
    q.close(); p.close()


def test_batched_parametric_sweep_matches_the_primal_model():
    """the batched EVALUATION path (eval_batch_kernel: B price vectors per pool read) on the network of two-asset.py:7-32 without its
    constant-sum pool (cfmm_solve_batch takes no price ties; the UNMODIFIED sweep, all five pools, runs through cfmm_solve_sweep:
    test_two_asset_sweep_in_one_call_all_five_pools) -- 24 values of t in groups
    of 8, each group warm-started from the previous one -- against the primal model (two-asset.py:51-88) solved by SciPy,
    objective 1e-7 and per-pool tenders 1e-6 (two-asset.py:94-98)"""
    from oracle.primal_scipy import solve_primal
    base = I.two_asset(0.0)
    keep = [i for i, k in enumerate(base["kinds"]) if k != "sum"]
    def inst(t):
        d = dict(I.two_asset(t))
        for key in ("local_indices", "reserves", "fees", "kinds", "weights"):
            d[key] = [d[key][i] for i in keep]
        return d
    ts = np.linspace(0.5, 50, 24)
    p = problem_of(inst(0.0))
    res = p.solve_many([cfmm.Swap([t, 0, 0], 2) for t in ts], tol=1e-9, warm_start=True, batch=8)      # (batch given: the batched EVALUATION path; without it a network this small is swept by cfmm_solve_sweep -- test_two_asset_sweep_in_one_call_all_five_pools)
    assert all(r["status"] == "optimal" and r["stats"]["batch"] == 8 for r in res)
    vals = np.array([r["value"] for r in res])
    assert np.all(np.diff(vals) > 0)
    for j in (0, 7, 8, 15, 23):
        r = solve_primal(I.normalise(inst(ts[j])))
        assert abs(vals[j] - r["value"]) <= 1e-7
    w = p._batch_workers[23 % 8]                     # the clone that solved the last point still holds its tenders
    for d, l, y in zip(w.deltas, w.lambdas, r["y"]):
        assert np.abs((np.asarray(l) - np.asarray(d)) - np.asarray(y)).max() <= 1e-6
    p.close()


def test_batched_solve_full_size_c3_properties(oracle_lib):
    """BASELINE config 3 at full size, 8 utilities at once: certificates of every solve, and one of them against the
    oracle's solver"""
    net = synthetic.config("C3", seed=0)
    rng = np.random.default_rng(3)
    n = net["n_tokens"]
    utils = [cfmm.Arbitrage(net["c"] * np.exp(rng.normal(0, 0.01, n))) for _ in range(8)]
    p = cfmm.Problem.from_network(net, utility=utils[0])
    res = p.solve_many(utils, tol=1e-6)
    for r in res:
        assert r["status"] == "optimal" and r["gap"] <= 1e-6 and r["infeas"] <= 1e-6
        assert r["psi"].min() >= -1e-6 * np.abs(r["psi"]).max()
    o = _oracle_for(oracle_lib, net, threads=8); o.set_utility(utils[3].c)
    ro = o.solve(utils[3].c, tol=1e-6)
    assert ro["status"] == 1 and abs(res[3]["value"] - ro["primal_value"]) <= 2e-6 * abs(ro["primal_value"])
    p.close()


def test_batched_solve_error_behaviour():
    net = synthetic.make_network(50, m_cp2=500, m_w2=100, m_gn=60, seed=2)
    u = cfmm.Arbitrage(net["c"])
    a = cfmm.Problem.from_network(net, utility=u); b = cfmm.Problem.from_network(net, utility=u)
    ca, cb = a._ensure_ctx(), b._ensure_ctx()
    for c in (ca, cb):
        c.set_utility(u.c, u.h, u.ctype)
    with pytest.raises(cfmm.CfmmError, match="no start prices"):
        ca.solve_batch([], None)
    with pytest.raises(cfmm.CfmmError, match="does not share"):
        ca.solve_batch([cb], [net["c"], net["c"]])
    k = ca.clone()
    with pytest.raises(cfmm.CfmmError, match="no utility"):
        ca.solve_batch([k], [net["c"], net["c"]])
    k.set_utility(u.c, u.h, u.ctype)
    with pytest.raises(cfmm.CfmmError, match="appears twice"):
        ca.solve_batch([k, k], [net["c"]] * 3)
    sts = ca.solve_batch([k], [net["c"], None], tol=1e-8)         # (None: continue from the prices the context holds)
    assert [s["status"] for s in sts] == [1, 1] and abs(sts[0]["primal_value"] - sts[1]["primal_value"]) <= 1e-9 * abs(sts[0]["primal_value"])
    clones = [ca.clone() for _ in range(ca.batch_capacity())]
    for c in clones:
        c.set_utility(u.c, u.h, u.ctype)
    with pytest.raises(cfmm.CfmmError, match="at most"):
        ca.solve_batch(clones, [net["c"]] * (len(clones) + 1))
    for c in clones + [k]:
        c.close()
    with pytest.raises(ValueError, match="batched path"):
        cfmm.Problem.from_network(synthetic.config("C5", scale=0.01, seed=0), utility=u).solve_many([u], batch=4)
    a.close(); b.close()


@pytest.mark.parametrize("n_tokens,memory", [(700, 8), (1500, 0), (2000, 8), (3000, 0)])
def test_every_update_kernel_instantiation_agrees_with_the_oracle(oracle_lib, n_tokens, memory):
    """the nu update runs as update_reg_kernel<512,8,2> (<= 1024 tokens), <512,4,4> (<= 2048 tokens, memory <= 4)
    or the generic update_kernel (everything else): same iteration, same answer as oracle_step"""
    net = synthetic.make_network(n_tokens, m_cp2=60_000, m_w2=20_000, m_gn=10_000, seed=9)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    v = p.solve(tol=1e-7, memory=memory)
    o = _oracle_for(oracle_lib, net)
    r = o.solve(net["c"], tol=1e-7, memory=memory)
    assert p.status == "optimal" and r["status"] == 1
    assert abs(v - r["primal_value"]) <= 2e-7 * abs(v)
    assert abs(p.stats["evals"] - r["evals"]) <= max(6, r["evals"] // 3)     # same algorithm, fp-noise apart
    p.close()


# ---------------------------------------------------------------------------------------------------------------
# reproducible mode (cfmm_set_deterministic): psi accumulated as exact fixed-point integers
# ---------------------------------------------------------------------------------------------------------------
def _limbs_value(limbs, scale):
    """(limb2 2^64 + limb1 2^32 + limb0) / scale, exactly (Python integers), as the nearest double"""
    l = limbs.astype(np.uint64).view(np.int64)
    return np.array([(int(l[2, j]) * 2 ** 64 + int(l[1, j]) * 2 ** 32 + int(l[0, j])) / scale for j in range(l.shape[1])])


@pytest.mark.parametrize("zipf", [None, 1.1])
def test_reproducible_mode_is_bitwise_run_to_run_and_shard_invariant(oracle_lib, zipf):
    """integer accumulation: psi does not depend on the order in which lanes, waves, workgroups or pool shards arrive --
    10 evaluations and 5 solves give identical bits; the limbs of S = 2, 3, 8 pool shards, added as integers, are the
    unsharded network's limbs bit for bit (what the integer RCCL all-reduce computes); and the values agree with the oracle"""
    net = synthetic.make_network(600, m_cp2=150_000, m_w2=40_000, m_gn=20_000, seed=21, zipf_s=zipf)
    n = net["n_tokens"]
    nu = net["c"] * np.exp(np.random.default_rng(5).normal(0, 0.03, n))
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]), deterministic=True)
    f0, psi0, d0 = p.eval_dual(nu, want_diag=True)
    for _ in range(9):
        f, psi, d = p.eval_dual(nu, want_diag=True)
        assert f == f0 and np.array_equal(psi, psi0) and np.array_equal(d, d0)
    o = _oracle_for(oracle_lib, net)
    fo, psio, do = o.eval(nu, want_diag=True)
    assert abs(f0 - fo) <= 1e-11 * abs(fo) and np.abs(psi0 - psio).max() <= 1e-10 * np.abs(psio).max()
    assert np.abs(d0 - do).max() <= 1e-11 * np.abs(do).max()
    # solves: identical iterates, identical evaluation counts
    runs = []
    for _ in range(5):
        v = p.solve(tol=1e-7)
        runs.append((v, p.stats["evals"], p.nu.copy(), p.psi.copy()))
        assert p.status == "optimal"
    for v, ev, nu_, psi_ in runs[1:]:
        assert v == runs[0][0] and ev == runs[0][1] and np.array_equal(nu_, runs[0][2]) and np.array_equal(psi_, runs[0][3])
    r = o.solve(net["c"], tol=1e-7)
    assert abs(runs[0][0] - r["primal_value"]) <= 2e-7 * abs(r["primal_value"])
    # shard invariance of the integer representation
    mr = max(b[k].max() for b in (net["cp2"], net["w2"]) for k in ("Ra", "Rb"))
    mr = max(mr, max(b["R"].max() for b in net["gn"].values()))
    mf = min(min(net[k]["fee"].min() for k in ("cp2", "w2")), min(b["fee"].min() for b in net["gn"].values()))
    whole = p._ensure_ctx().debug_eval_limbs(nu, mr, mf)
    import math
    scale = 2.0 ** (84 - math.frexp(mr / mf)[1])
    # the device's conversion == exact integer arithmetic: limbs_to_double rounds twice (the low 64 bits to a double, then the sum),
    # always the same two -- bitwise reproducible, and within one unit in the last place of the once-rounded value (round 5: a
    # token whose psi is a cancellation of large contributions hit the double rounding, 7e-15 on 54.8)
    exact = _limbs_value(whole, scale)
    assert np.all(np.abs(exact - psi0) <= np.spacing(np.abs(psi0))) and (exact != psi0).sum() <= 3
    p.close()
    for S in (2, 3, 8):
        tot = np.zeros_like(whole)
        for rk in range(S):
            q = cfmm.Problem.from_network(cfmm.distributed.rank_network(net, rk, S), utility=cfmm.Arbitrage(net["c"]))
            tot = tot + q._ensure_ctx().debug_eval_limbs(nu, mr, mf)      # uint64 addition wraps: exactly the integer all-reduce
            q.close()
        assert np.array_equal(tot, whole), S


def test_default_mode_is_reproducible_to_rounding_only():
    """(the fp64-atomic default, for contrast: repeated evaluations differ in their last bits -- if this ever stops
    being true the reproducible mode has lost its reason to exist)"""
    net = synthetic.config("C3", scale=0.2, seed=2)
    nu = net["c"] * np.exp(np.random.default_rng(5).normal(0, 0.03, net["n_tokens"]))
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    outs = [p.eval_dual(nu)[1] for _ in range(6)]
    p.close()
    gross = np.abs(outs[0]).max()
    assert all(np.abs(x - outs[0]).max() <= 1e-11 * gross for x in outs)


# ---------------------------------------------------------------------------------------------------------------
# one-shot all-reduce (csrc/oneshot.hpp) and the pool-sharded C path with MORE than one rank, on one GPU: the ranks
# are contexts of ONE process on the same device, their mailboxes attached by raw pointer (cfmm_oneshot_attach)
# ---------------------------------------------------------------------------------------------------------------
class _ThreadComm:
    """test double of cfmm.problem.HostComm for ranks that are threads of one process"""
    import threading as _th

    def __init__(self, world):
        self.world = world
        self.bar = self._th.Barrier(world)
        self.box = [None] * world

    def view(self, rank):
        parent = self

        class V:
            world = parent.world

            def __init__(s):
                s.rank = rank

            def _exchange(s, obj):
                parent.box[rank] = obj
                parent.bar.wait()
                out = list(parent.box)
                parent.bar.wait()
                return out

            def broadcast(s, a, src=0):
                return np.array(s._exchange(np.array(a, dtype=np.float64))[src])

            def allreduce_sum(s, a):
                return np.sum(s._exchange(np.array(a, dtype=np.float64)), axis=0)

            def allgather(s, obj):
                return s._exchange(obj)

            def assert_identical(s, a, what):
                parts = s._exchange(np.array(a, dtype=np.float64))
                if not all(np.array_equal(x, parts[0]) for x in parts):
                    raise cfmm.CfmmError(f"pool-sharded solve: {what} differ between ranks")
        return V()


@pytest.mark.parametrize("world,deterministic", [(2, False), (3, False), (2, True)])
def test_pool_sharded_c_path_with_the_one_shot_all_reduce(oracle_lib, world, deterministic, monkeypatch):
    """`world` ranks = `world` contexts on this GPU, each holding one contiguous pool shard, exchanging [psi | sum arb]
    (or the integer limbs) through the one-shot mailboxes: the whole fold -> all-reduce -> in-launch update control
    flow of an N-GPU job runs here with N > 1.  Every rank must see the same bits, and the unsharded optimum."""
    import threading
    net = synthetic.config("C3", scale=0.05, seed=6)
    n = net["n_tokens"]
    nu = net["c"] * np.exp(np.random.default_rng(1).normal(0, 0.02, n))
    whole = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]), deterministic=deterministic)
    f_ref, psi_ref = whole.eval_dual(nu)
    v_ref = whole.solve(tol=1e-7)
    evals_ref = whole.stats["evals"]; nu_ref = whole.nu.copy()
    whole.close()          # (its stream's hardware queue goes back to the pool: see conftest.py on GPU_MAX_HW_QUEUES)
    comm = _ThreadComm(world)
    ranks = []
    monkeypatch.setenv("CFMM_STREAM_POOL", "0")      # fresh streams, created back to back: distinct hardware queues (conftest.py)
    for r in range(world):
        q = cfmm.Problem.from_network(cfmm.distributed.rank_network(net, r, world), utility=cfmm.Arbitrage(net["c"]), deterministic=deterministic)
        q._ensure_ctx()
        ranks.append(q)
    boxes = [q.ctx.oneshot_mailbox() for q in ranks]
    for r, q in enumerate(ranks):
        q.ctx.oneshot_attach(world, r, boxes)
        q._host = comm.view(r)
    out = [None] * world
    err = []

    def run(r):
        try:
            q = ranks[r]
            f, psi = q.eval_dual(nu)
            v = q.solve(tol=1e-7)
            out[r] = dict(f=f, psi=psi, v=v, status=q.status, evals=q.stats["evals"], nu=q.nu.copy(), psi_sol=q.psi.copy(), ranks=q.stats["n_ranks"])
        except Exception as e:       # surfaced below
            err.append(e); comm.bar.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not err, err
    assert all(o is not None for o in out)
    for o in out:
        assert o["status"] == "optimal" and o["ranks"] == world
        assert abs(o["f"] - f_ref) <= 1e-11 * abs(f_ref) and np.abs(o["psi"] - psi_ref).max() <= 1e-10 * np.abs(psi_ref).max()
        assert abs(o["v"] - v_ref) <= 2e-7 * abs(v_ref)
        # rank-order reduction: every rank holds the SAME bits
        assert o["f"] == out[0]["f"] and np.array_equal(o["psi"], out[0]["psi"])
        assert o["evals"] == out[0]["evals"] and np.array_equal(o["nu"], out[0]["nu"]) and np.array_equal(o["psi_sol"], out[0]["psi_sol"])
    if deterministic:                      # integer limbs: the sharded run IS the unsharded run, bit for bit
        assert out[0]["f"] == f_ref and np.array_equal(out[0]["psi"], psi_ref)
        assert out[0]["v"] == v_ref and out[0]["evals"] == evals_ref and np.array_equal(out[0]["nu"], nu_ref)
    for q in ranks:
        q.close()


def test_one_shot_exchange_between_processes_sharing_one_gpu(tmp_path, world=2):
    """the one-shot exchange between REAL processes: two ranks on GPU 0, mailboxes exported / mapped through hipIpc,
    written by the other process's kernels, the host running ahead of the device.  Everything of the multi-GPU path
    except the xGMI hop itself: every rank holds the same bits, they match the unsharded problem to rounding and -- in
    reproducible mode -- bit for bit, the evaluation count included.  (Two processes run side by side on one GPU; with
    three the scheduler time-slices them and the exchange kernels, which WAIT for each other, run into their spin
    bound -- an artefact of sharing a device that one process per GPU does not have.)"""
    import subprocess, sys, json, socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "same_gpu.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(here, "dist_gpu_worker.py"), out, "same_gpu"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(out))
    assert doc["world"] == world
    for mode in ("fp64", "det"):
        ranks, ref = doc["res"][mode]["ranks"], doc["res"][mode]["unsharded"]
        for q in ranks:
            assert q["status"] == "optimal" and q["ranks"] == world
            assert q["f"] == ranks[0]["f"] and q["psi"] == ranks[0]["psi"] and q["nu"] == ranks[0]["nu"] and q["evals"] == ranks[0]["evals"]
        q = ranks[0]
        if mode == "det":
            assert q["f"] == ref["f"] and q["psi"] == ref["psi"] and q["value"] == ref["value"] and q["nu"] == ref["nu"] and q["evals"] == ref["evals"]
        else:
            for f1, f0, p1, p0 in zip(q["f"], ref["f"], q["psi"], ref["psi"]):
                assert abs(f1 - f0) <= 1e-11 * abs(f0) and np.abs(np.array(p1) - np.array(p0)).max() <= 1e-10 * np.abs(p0).max()
            assert abs(q["value"] - ref["value"]) <= 2e-6 * abs(ref["value"])


def test_k_asset_constant_sum_kinks_in_a_pool_sharded_solve(tmp_path, world=2):
    """the K-asset constant-sum kink records of a pool-sharded solve.  Two processes share GPU 0, each holds half of
    1 000 such pools; the optimum has partially drained legs and tied cheapest tokens on BOTH shards.  Every rank must end on the same
    prices, the same fills (records of both owners among them) and the certificates -- and on the unsharded optimum."""
    import subprocess, sys, json, socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "same_gpu_gk.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(here, "dist_gpu_worker.py"), out, "same_gpu_gk"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(out))
    ranks, ref = doc["ranks"], doc["unsharded"]
    assert ref["status"] == "optimal" and ref["ntheta"] > 0
    for q in ranks:
        assert q["status"] == "optimal" and q["gap"] <= 1e-6 and q["infeas"] <= 1e-6, (q["status"], q["gap"], q["infeas"])
        assert q["nu"] == ranks[0]["nu"] and q["theta"] == ranks[0]["theta"] and q["evals"] == ranks[0]["evals"]
        assert len(q["theta"]) > 0 and all(0.0 < th < 1.0 for _, th in q["theta"])
        assert abs(q["value"] - ref["value"]) <= 2e-6 * abs(ref["value"])
    assert ranks[0]["owners"] == list(range(world)), ranks[0]["owners"]       # kinks of pools of EVERY shard were tied and filled


def test_one_shot_all_reduce_against_rccl_on_real_peers(tmp_path):
    """needs >= 2 GPUs (skipped on the one-GPU box): one process per GPU, the same sharded evaluation and solve over RCCL
    and over the one-shot mailboxes mapped through hipIpc.  Every rank holds the same bits either way; the two
    transports agree to rounding (their summation orders differ), and bit for bit in reproducible mode, where the sum
    is an integer sum."""
    import subprocess, sys, json, socket
    import torch
    ngpu = torch.cuda.device_count()
    if ngpu < 2:
        pytest.skip(f"{ngpu} GPU visible: the one-shot exchange over real peers needs two")
    world = min(ngpu, 8)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "oneshot.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(here, "dist_gpu_worker.py"), out], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(out))
    res = doc["res"]
    assert doc["auto"]["how"] == "oneshot" and doc["auto"]["status"] == "optimal", doc["auto"]      # the start-up check passed on real peers
    for k, v in res.items():
        assert v["status"] == "optimal" and v["all_ranks_same_bits"], k
    a, b = res["rccl"], res["oneshot"]
    assert abs(a["f"] - b["f"]) <= 1e-12 * abs(a["f"]) and np.abs(np.array(a["psi"]) - np.array(b["psi"])).max() <= 1e-11 * np.abs(a["psi"]).max()
    assert abs(a["value"] - b["value"]) <= 2e-7 * abs(a["value"])
    a, b = res["rccl_det"], res["oneshot_det"]
    assert a["f"] == b["f"] and a["psi"] == b["psi"] and a["nu"] == b["nu"] and a["evals"] == b["evals"]


def test_bench_line_keeps_the_contract(tmp_path):
    """`python bench.py --full` (N = 1, a short run): ONE JSON line with the contract's keys, BASELINE's metric and unit, the
    roofline and CPU-baseline objects, and the extra figures (batched, PCIe-inclusive) beside -- not instead of -- `value`"""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--cpu-seconds", "1", "--cpu-solves", "1"],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(root, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "pool-subproblems/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    # (throughput floors here are sanity bounds, a tenth of the normal figure: a 2-3 step run on a shared box can hit a multi-ms hiccup --
    #  one run in seventeen did; the measured numbers live in profiles/ and are checked by tests/test_host.py)
    assert d["value"] > 3e9 and abs(d["ms_per_step"] * 1e-3 * d["value"] - d["evals_per_solve"] * d["config"]["pools_total"]) <= 1e-6 * d["evals_per_solve"] * d["config"]["pools_total"]
    rf = d["roofline"]
    assert rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    # frac prices the ALGORITHMIC bytes, hbm_frac the bytes the launch loads as stored: at C3 the latter hold the derived
    # log(R / w) column of the K-asset buckets (+8 B per leg, cfmm_eval_bytes) and no compact mirror -- a few per cent more, never less
    assert rf["frac"] <= rf["hbm_frac"] <= 1.15 * rf["frac"]
    assert abs(rf["hbm_frac"] / rf["frac"] - rf["bytes_as_stored_per_launch"] / rf["algorithmic_bytes_per_launch"]) < 1e-9
    if rf["traffic"]:                       # the PMC traffic of the committed profile reproduces the stored bytes within 10 %
        assert abs(rf["traffic"] / rf["bytes_as_stored_per_launch"] - 1.0) <= 0.12
    # both ceilings are reported and `bound` names the binding one; the vector-issue fraction comes from the
    # newest PMC summary under profiles/ (None when no profile of this kernel is committed)
    assert rf["bound"] in ("hbm", "valu") and (rf["valu_frac"] is None or 0.0 < rf["valu_frac"] < 1.0)
    assert rf["bound"] == ("valu" if (rf["valu_frac"] or 0.0) > rf["hbm_frac"] else "hbm")
    assert rf["evaluation_only"]["bound"] in ("hbm", "valu")
    assert rf["traffic"] is None or rf["traffic"] > 4e7
    assert rf["rocprof_avg_launch_us"] is None or abs(rf["rocprof_avg_launch_us"] - rf["avg_launch_us"]) <= 0.3 * rf["avg_launch_us"]      # live (3 steps) vs committed trace
    # the line explains itself: the timed steps in blocks, the shader clock measured live (a pass of its own behind the
    # timed region) beside the idle clock, and the line's kernel times checked against profiles/budget.json
    assert len(d["ms_per_step_blocks"]) == 3 and abs(sum(d["ms_per_step_blocks"]) / 3 - d["ms_per_step"]) <= 0.05 * d["ms_per_step"]
    assert min(d["ms_per_step_blocks"]) <= d["ms_per_step_median_block"] <= max(d["ms_per_step_blocks"]) and d["extra_warmup_steps"] >= 100
    assert 1.2 < rf["effective_clock_ghz_live"] < 2.6 and 1.2 < rf["clock_ghz_idle"] < 2.6
    assert rf["clock_pass"]["solves"] >= 20 and rf["clock_pass"]["ms_per_step"] > 0.0
    assert 4.0 < rf["clock_probe_fma_chain"]["cycles_per_dependent_v_fma_f64"] < 12.0
    assert isinstance(d["budget_ok"], bool) and d["budget"]["source"] == "profiles/budget.json" and d["budget"]["checked"]
    assert "device_state" in d
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "pool-subproblems/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert cb["numpy_one_thread"]["cores"] == 1 and cb["numpy_one_thread"]["value"] > 1e6      # (baseline B beside A)
    assert d["batched"]["solves_per_batch"] >= 2 and d["batched"]["value"] > 0.7 * d["value"]
    assert d["pcie_inclusive"]["value"] < d["value"]
    # the pool-sharded code path with a one-rank process group (what the driver's --gpus N > 1 runs per rank)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--force-dist", "--no-cpu"],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    d1 = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d1["n_gpus"] == 1 and d1["config"]["rccl_ranks"] == 1 and d1["config"]["allreduce"] == "rccl" and d1["value"] > 2e9
    assert abs(d1["objective"] - d["objective"]) <= 2e-6 * abs(d["objective"])


def _bench_line(tmp_path, *flags):
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *flags], capture_output=True, text=True, timeout=900, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_lines_of_the_other_baseline_configs(tmp_path):
    """every BASELINE.json config has a driver-reproducible line: --config C2 (launch-latency bound), C4 (strong scaling;
    here at a tenth of its size) and C5 (second-order path: the dominant kernel group is the dense factorisation, priced
    against the fp64 vector peak) beside the default C3"""
    base = json_load_baseline()
    d2 = _bench_line(tmp_path, "--full", "--config", "C2", "--steps", "3", "--warmup", "1", "--no-cpu", "--no-batch")
    assert d2["metric"] == base["metric"] and d2["config"]["workload"].startswith("C2:") and d2["config"]["pools_total"] == 10000
    assert d2["value"] > 1e8 and d2["roofline"]["bound"] in ("hbm", "valu") and d2["roofline"]["hbm_frac"] < 0.05
    d4 = _bench_line(tmp_path, "--full", "--config", "C4", "--scale", "0.1", "--steps", "2", "--warmup", "1", "--no-cpu")
    assert d4["scaling"] == "strong" and d4["config"]["workload"].startswith("C4:") and d4["value"] > 2e9
    d5 = _bench_line(tmp_path, "--full", "--config", "C5", "--steps", "1", "--warmup", "1", "--cpu-seconds", "1")
    assert d5["config"]["workload"].startswith("C5:") and d5["config"]["pools_total"] == 550000 and d5["newton_steps_per_solve"] >= 3
    assert d5["gap"] <= 1e-6 and d5["infeas"] <= 1e-6
    rf = d5["roofline"]
    assert rf["bound"] == "valu" and rf["unit"] == "TFLOP/s" and rf["peak"] == 78.6 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert set(rf["newton_step_us"]) == {"smoothed_evaluation_with_hessian", "smoothed_evaluation", "factorisation", "back_substitution"}
    assert 0.0 < rf["smoothed_evaluation"]["hbm_frac"] < 1.0
    assert d5["cpu_baseline"]["kind"] == "port" and d5["cpu_baseline"]["value"] > 0


def test_bench_multi_rank_path_end_to_end_on_one_gpu(tmp_path):
    """`bench.py --gpus 2 --share-gpu`: self-launch -> torch.distributed.run -> two ranks (processes on device 0, gloo + the
    hipIpc one-shot exchange, no RCCL) -> pool shards -> barrier-bracketed timing, max over ranks -> per-iteration split ->
    ONE JSON line from rank 0.  Everything the driver's N > 1 command runs except RCCL and the second device."""
    d = _bench_line(tmp_path, "--full", "--gpus", "2", "--share-gpu", "--steps", "2", "--warmup", "1", "--no-cpu", "--scale", "0.25")
    assert d["n_gpus"] == 2 and d["config"]["rccl_ranks"] == 2 and d["config"]["allreduce"] == "oneshot" and d["scaling"] == "weak"
    assert d["config"]["pools_total"] == 2 * d["config"]["pools_per_gpu"] and "--share-gpu" in d["config"]["workload"]
    assert d["per_iteration_us"]["allreduce"] > 0.0 and d["gap"] <= 1e-6 and d["infeas"] <= 1e-6
    ds = _bench_line(tmp_path, "--full", "--gpus", "2", "--share-gpu", "--config", "C4", "--scale", "0.05", "--steps", "2", "--warmup", "1", "--no-cpu")
    assert ds["n_gpus"] == 2 and ds["scaling"] == "strong" and ds["config"]["pools_total"] == 500000 and ds["config"]["pools_per_gpu"] == 250000
    # four ranks (the one-shot exchange with four mailboxes per rank, rank-ordered sums): what the driver's --gpus 4 runs per rank
    d4 = _bench_line(tmp_path, "--full", "--gpus", "4", "--share-gpu", "--steps", "2", "--warmup", "1", "--no-cpu", "--scale", "0.1")
    assert d4["n_gpus"] == 4 and d4["config"]["rccl_ranks"] == 4 and d4["config"]["allreduce"] == "oneshot"
    assert d4["config"]["pools_total"] == 4 * d4["config"]["pools_per_gpu"] and d4["gap"] <= 1e-6 and d4["infeas"] <= 1e-6


def test_plain_bench_line_and_its_dumped_outputs(tmp_path):
    """`bench.py` without --full: the headline figures alone (nothing that takes a pass of its own), `--steps` timed steps, and
    --dump-outputs: the last timed solve's objective, prices, net trade and trades as float64 arrays, consistent with each other
    and with the line; a second run with the same arguments solves the same instance"""
    lines = [_bench_line(tmp_path, "--config", "C2", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    d = lines[0]
    assert d["metric"] == json_load_baseline()["metric"] and d["unit"] == "pool-subproblems/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 4 and len(d["ms_per_step_blocks"]) == 4 and d["ms_per_step"] > 0.0 and d["gap"] <= 1e-6 and d["infeas"] <= 1e-6
    work = d["evals_per_solve"] * d["config"]["pools_total"]
    assert abs(d["ms_per_step"] * 1e-3 * d["value"] - work) <= 1e-6 * work
    assert not set(d) & {"roofline", "per_iteration_us", "cpu_baseline", "batched", "pcie_inclusive", "budget", "device_state"}, sorted(d)
    names = {"objective", "nu", "psi", "trades_cp2_delta", "trades_cp2_lambda"}
    out = [{f[:-4]: np.load(tmp_path / r / f) for f in os.listdir(tmp_path / r)} for r in ("a", "b")]
    assert set(out[0]) == set(out[1]) == names
    assert all(a.dtype == np.float64 for a in out[0].values()) and sum(a.nbytes for a in out[0].values()) <= 64 << 20
    net = synthetic.config("C2", seed=0)
    n, b = net["n_tokens"], net["cp2"]
    o = out[0]
    assert o["objective"][0] == d["objective"] and o["nu"].shape == o["psi"].shape == (n,)
    assert o["trades_cp2_delta"].shape == o["trades_cp2_lambda"].shape == (2, len(b["Ra"]))
    y = o["trades_cp2_lambda"] - o["trades_cp2_delta"]
    psi = np.bincount(b["ia"], weights=y[0], minlength=n) + np.bincount(b["ib"], weights=y[1], minlength=n)
    assert np.abs(psi - o["psi"]).max() <= 1e-9 * max(1.0, np.abs(psi).max())
    assert abs(net["c"] @ o["psi"] - o["objective"][0]) <= 1e-9 * abs(o["objective"][0])
    assert abs(out[1]["objective"][0] - o["objective"][0]) <= 2e-6 * abs(o["objective"][0])


def json_load_baseline():
    import json
    return json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "BASELINE.json")))


def test_k_asset_tiles_with_and_without_the_log_price_table(oracle_lib):
    """the evaluation that builds the metric keeps a = log(R p / w) per leg; every other evaluation takes it as log(R / w) (a
    column written at upload) + log p (a table per workgroup): the same psi to rounding, both against the oracle, at a mix that
    is mostly K-asset pools of every size -- and the sum of arbitrage profits formed at the flush as nu' psi"""
    net = synthetic.make_network(300, m_cp2=2000, m_w2=1000, m_gn=40_000, seed=11)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    o = _oracle_for(oracle_lib, net)
    rng = np.random.default_rng(3)
    for spread in (0.002, 0.03, 0.3):
        nu = net["c"] * np.exp(rng.normal(0, spread, net["n_tokens"]))
        f1, psi1 = p.eval_dual(nu)                         # log-price table
        f2, psi2, _ = p.eval_dual(nu, want_diag=True)      # per-leg log
        f0, psi0 = o.eval(nu)
        scale = np.abs(psi0).max()
        assert np.abs(psi1 - psi2).max() <= 1e-12 * scale and abs(f1 - f2) <= 1e-11 * max(abs(f0), 1.0)
        assert np.abs(psi1 - psi0).max() <= 1e-10 * scale and abs(f1 - f0) <= 1e-10 * max(abs(f0), 1.0)
        assert abs(f1 - float(nu @ psi1)) <= 1e-10 * max(abs(f0), 1.0)       # sum_i arb_i = nu' psi
    p.close()


def test_compact_mirror_of_ids_and_fees_is_bit_identical(oracle_lib):
    """buckets of >= 1e6 two-asset pools are evaluated from a compact mirror of their token ids (one 32-bit word) and fees (a
    one-byte index into the bucket's distinct fees): kernels.hpp Bucket2::cid; constant-product buckets of >= 8e6 pools in tiles
    of 256 pools per wave (EvalArgs::wide).  Both live in the large-set instantiations of eval_kernel / iter_kernel only
    (cfmm_hip.hip: large_set_mode), with cached or with non-temporal loads.  CFMM_COMPACT=1 CFMM_WIDE=1 (and CFMM_NT=1) force them
    on a small network, in a process of its own (the knobs are read once): the oracle's evaluation, the same certified solve as
    the plain instantiation -- and a bucket with more than 256 distinct fees keeps its columns and its answers; the reproducible
    mode always takes the plain instantiation and stays bit for bit what it was"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, json, numpy as np\n"
        f"sys.path[:0] = [{root!r}, {os.path.join(root, 'cfmm-routing-code_amd')!r}]\n"
        "import cfmm\nfrom cfmm import synthetic\n"
        "out = {}\n"
        "for tag in ('tiers', 'many'):\n"
        "    net = synthetic.config('C3', scale=0.05)\n"
        "    if tag == 'many':\n"
        "        net['cp2']['fee'] = 0.99 + 0.009 * np.random.default_rng(1).random(len(net['cp2']['fee']))\n"
        "    nu = net['c'] * np.exp(np.random.default_rng(0).normal(0, 0.03, net['n_tokens']))\n"
        "    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net['c']))\n"
        "    f, psi, diag = p.eval_dual(nu, want_diag=True)\n"
        "    v = p.solve(tol=1e-6)\n"
        "    q = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net['c']), deterministic=True)\n"
        "    fd, psid = q.eval_dual(nu)\n"
        "    out[tag] = dict(f=f, psi=psi.tolist(), diag=diag.tolist(), v=v, status=p.status, psid=[x.hex() for x in psid.tolist()],\n"
        "                    stored=p.ctx.eval_bytes(), m={k: len(net[k]['Ra']) for k in ('cp2', 'w2')}, gn={int(k): b['R'].shape[1] for k, b in net['gn'].items()})\n"
        "print(json.dumps(out))\n")
    res = {}
    envs = {"1": dict(CFMM_COMPACT="1", CFMM_WIDE="1", CFMM_NT="0"), "nt": dict(CFMM_COMPACT="1", CFMM_WIDE="1", CFMM_NT="1"),
            "mirror": dict(CFMM_COMPACT="1", CFMM_WIDE="0", CFMM_NT="0"), "0": dict(CFMM_COMPACT="0", CFMM_WIDE="0", CFMM_NT="0")}
    for mode, env in envs.items():
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        res[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    for tag, mode in [(t, m) for t in ("tiers", "many") for m in ("1", "nt", "mirror")]:
        a, b = res[mode][tag], res["0"][tag]
        assert a["psid"] == b["psid"]                                            # reproducible mode: bit for bit
        # cfmm_eval_bytes: the columns as stored -- 21 / 29 B per constant-product / weighted pool under a mirror, 32 / 40 without
        # (a bucket with more than 256 distinct fees keeps its columns: "many")
        # K-asset buckets: 20 + 20 k as uploaded + the derived log(R / w) column the iteration's tiles read (8 B per leg)
        kb = sum((20 + 28 * int(k)) * v for k, v in b["gn"].items())
        assert b["stored"] == 32 * b["m"]["cp2"] + 40 * b["m"]["w2"] + kb
        assert a["stored"] == (32 if tag == "many" else 21) * a["m"]["cp2"] + 29 * a["m"]["w2"] + kb
        assert a["status"] == b["status"] == "optimal" and abs(a["v"] - b["v"]) <= 2e-6 * abs(b["v"])
        net = synthetic.config("C3", scale=0.05)
        if tag == "many":
            net["cp2"]["fee"] = 0.99 + 0.009 * np.random.default_rng(1).random(len(net["cp2"]["fee"]))
        o = _oracle_for(oracle_lib, net)
        nu = net["c"] * np.exp(np.random.default_rng(0).normal(0, 0.03, net["n_tokens"]))
        f0, psi0, diag0 = o.eval(nu, True)
        assert np.abs(np.array(a["psi"]) - psi0).max() <= 1e-10 * np.abs(psi0).max() and abs(a["f"] - f0) <= 1e-10 * abs(f0)
        assert np.abs(np.array(a["diag"]) - diag0).max() <= 1e-10 * np.abs(diag0).max()


def test_non_temporal_instantiations_match_the_oracle(oracle_lib, tmp_path):
    """pool sets beyond twice the Infinity Cache stream their columns with non-temporal loads (kernels.hpp: ld_off<NT>; own
    instantiations of eval_kernel / iter_kernel, taken automatically at >= 512 MB).  CFMM_NT=1 forces them on a small network,
    in a process of its own (the knob is read once): same evaluation as the oracle to 1e-10, same certified solve."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, json, numpy as np\n"
        f"sys.path[:0] = [{root!r}, {os.path.join(root, 'cfmm-routing-code_amd')!r}]\n"
        "import cfmm\nfrom cfmm import synthetic\n"
        "net = synthetic.config('C3', scale=0.05)\n"
        "p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net['c']))\n"
        "nu = net['c'] * np.exp(np.random.default_rng(0).normal(0, 0.03, net['n_tokens']))\n"
        "f, psi, diag = p.eval_dual(nu, want_diag=True)\n"
        "v = p.solve(tol=1e-6)\n"
        "print(json.dumps(dict(f=f, psi=psi.tolist(), diag=diag.tolist(), v=v, status=p.status, gap=p.gap, infeas=p.infeas)))\n")
    env = dict(os.environ, CFMM_NT="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    net = synthetic.config("C3", scale=0.05)
    o = _oracle_for(oracle_lib, net)
    nu = net["c"] * np.exp(np.random.default_rng(0).normal(0, 0.03, net["n_tokens"]))
    f0, psi0, diag0 = o.eval(nu, True)
    assert abs(out["f"] - f0) <= 1e-10 * abs(f0) and np.abs(np.array(out["psi"]) - psi0).max() <= 1e-10 * np.abs(psi0).max()
    assert np.abs(np.array(out["diag"]) - diag0).max() <= 1e-10 * np.abs(diag0).max()
    ref = o.solve(net["c"], tol=1e-6)
    assert out["status"] == "optimal" and out["gap"] <= 1e-6 and out["infeas"] <= 1e-6
    assert abs(out["v"] - ref["primal_value"]) <= 2e-6 * abs(out["v"])
