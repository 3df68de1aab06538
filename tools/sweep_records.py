"""The swept solve's records over a fixed list of small networks:
    python tools/sweep_records.py [out.json]                              one run's records
    python tools/sweep_records.py --pin run1.json run2.json ... out.json  several runs made into the pinned file
cfmm_solve_sweep straight through the binding (none of cfmm.Problem's folding or fall-backs behind it), per case and per point: status,
evals, iters, rounds and the method reported, the signs of the tied constant-sum pools (tsgn), their fills (theta, rounded for reading) and, as raw doubles
(float.hex), theta, the library's dual value and psi.  The last case is the shipped arbitrage instance through ctx.solve with the default
method, the library's own one-point sweep (solve_tiny_kinks): its statistics, psi and the partially filled pool's fill read off the tenders.
CFMM_LIB selects the library: tests/golden/sweep_records.json is this tool's output on the build BEFORE cfmm_solve_sweep was divided into
rules (sweep_rules.hpp) and phases, and tests/test_gpu.py holds every later build to it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "cfmm-routing-code_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import cfmm
from cfmm import _lib
from oracle import instances as I
from helpers import problem_of, random_instance, utility_of

INTS = ("status", "evals", "iters", "rounds", "method", "tsgn")
RAW = ("theta", "value", "psi")


def _hex(a):
    return [float(x).hex() for x in np.ravel(a)]            # (float.hex writes nan as 'nan')


def _sweep_points(p, utils, tol):
    """cfmm_solve_sweep over p's pools under `utils`, as Problem._solve_sweep calls it -> one record per point"""
    ctx = p._ensure_ctx()
    C_ = np.stack([u.c for u in utils]); H = np.stack([u.h for u in utils]); CT = np.stack([u.ctype for u in utils]).astype(np.int32)
    NU0 = np.stack([cfmm.start_prices(p.net, u) for u in utils])
    s2 = p.net.get("sum2")
    if s2 is not None and not len(s2["Ra"]):
        s2 = None
    nu, psi, theta, tsgn, _, sts, rounds = ctx.solve_sweep(C_, H, CT, NU0, s2, p._trade_layout()[1], 1e-3, 6, tol=tol, max_evals=2000, memory=0,
                                                           method=_lib.METHODS["lbfgs"])
    out = []
    for b, st in enumerate(sts):
        out.append(dict(status=int(st["status"]), evals=int(st["evals"]), iters=int(st["iters"]), rounds=int(rounds[b]), method=int(st["method"]),
                        tsgn=[int(x) for x in tsgn[b]],
                        theta=[round(float(x), 6) if np.isfinite(x) else None for x in theta[b]],
                        raw=dict(theta=_hex(theta[b]), value=_hex([st["dual_value"]]), psi=_hex(psi[b]))))
    return out


def tiny_network(seed, util):                 # (tests/test_gpu.py: test_swept_solves_match_one_at_a_time_on_random_tiny_networks)
    inst = random_instance(40 + seed, n_tokens=5 + seed % 3, n_pools=10 + 2 * seed, with_sum=True, utility=util)
    rng = np.random.default_rng(seed)
    for i in range(3):
        a, b = rng.choice(inst["n_tokens"], 2, replace=False)
        inst["local_indices"].append([int(a), int(b)]); inst["reserves"].append([float(np.exp(rng.normal(2, 0.5)))] * 2)
        inst["fees"].append(float(rng.choice([0.997, 0.999, 0.99]))); inst["kinds"].append("sum"); inst["weights"].append(None); inst["params"].append(None)
    u0 = utility_of(inst)
    utils = []
    for k in range(12):
        if util == "arbitrage":
            utils.append(cfmm.Arbitrage(u0.c * np.exp(rng.normal(0, 0.02 * (1 + k), inst["n_tokens"]))))
        else:
            h = u0.h * (0.25 + 0.5 * k)
            utils.append(cfmm.Swap(h, inst["utility"]["t"]) if util == "swap" else cfmm.Liquidate(h, inst["utility"]["t"]))
    return inst, utils


def _arbitrage_through_solve():
    """the shipped arbitrage instance through cfmm_solve with the default method: the library's own kink loop ends it (method lbfgs)"""
    inst = I.arbitrage()
    p = problem_of(inst)
    try:
        u = utility_of(inst)
        ctx = p._ensure_ctx(); ctx.set_utility(u.c, u.h, u.ctype)
        st = ctx.solve(cfmm.start_prices(p.net, u), tol=1e-9, method="auto")
        _, psi = ctx.get_solution()
        b = p.net["sum2"]
        d, l = ctx.get_trades2(cfmm.problem.KIND2["sum2"], len(b["Ra"]))
        ya, yb = l[0] - d[0], l[1] - d[1]                   # what the trader receives of the pool's first / second token
        tsgn = np.where(ya < 0, 1, np.where(yb < 0, -1, 0))
        theta = np.where(tsgn > 0, yb / b["Rb"], np.where(tsgn < 0, ya / b["Ra"], np.nan))
        return [dict(status=int(st["status"]), evals=int(st["evals"]), iters=int(st["iters"]), rounds=-1, method=int(st["method"]),
                     tsgn=[int(x) for x in tsgn],
                     theta=[round(float(x), 6) if np.isfinite(x) else None for x in theta],
                     raw=dict(theta=_hex(theta), value=_hex([st["primal_value"]]), psi=_hex(psi)))]
    finally:
        p.close()


def cases():
    """(name, function returning the case's list of point records) -- each builds its problem afresh"""
    def swept(make, tol):
        def run():
            p, utils = make()
            try:
                return _sweep_points(p, utils, tol)
            finally:
                p.close()
        return run
    out = [("two_asset_50", swept(lambda: (problem_of(I.two_asset(0.0)), [cfmm.Swap([t, 0, 0], 2) for t in I.two_asset_sweep()]), 1e-10))]
    for seed, util in ((0, "arbitrage"), (1, "swap"), (2, "liquidate"), (3, "arbitrage"), (4, "swap"), (5, "liquidate")):
        def make(seed=seed, util=util):
            inst, utils = tiny_network(seed, util)
            return problem_of(inst), utils
        out.append((f"tiny{seed}_{util}", swept(make, 1e-9)))

    def no_sum():                              # no constant-sum pool: every point is ONE leg
        inst = random_instance(61, n_tokens=6, n_pools=12, with_sum=False, utility="arbitrage")
        u0, rng = utility_of(inst), np.random.default_rng(61)
        return problem_of(inst), [cfmm.Arbitrage(u0.c * np.exp(rng.normal(0, 0.02 * (1 + k), inst["n_tokens"]))) for k in range(12)]
    out.append(("no_sum_single_leg", swept(no_sum, 1e-9)))
    out.append(("arbitrage_through_solve", _arbitrage_through_solve))      # (rounds -1: cfmm_solve reports none)
    return out


def records():
    return {name: run() for name, run in cases()}


def pin(runs):
    """several runs -> the pinned file: a case whose integers repeat is kept with the first run's records and, per raw quantity, its
    spread (the largest difference between any two runs) and the tolerance a later build is held to.  A case whose runs agree bit for
    bit in every quantity: 0.0, the doubles must be equal.  Otherwise ten times the quantity's spread -- and, for a quantity of such a
    case that happened to repeat, ten times the case's largest spread: it is computed from the ones that moved."""
    kept, dropped = {}, []
    val = lambda h: np.array([float.fromhex(x) for x in h])
    for name in runs[0]:
        per_run = [r[name] for r in runs]
        if any([[pt[k] for k in INTS] for pt in pr] != [[pt[k] for k in INTS] for pt in per_run[0]] for pr in per_run[1:]):
            dropped.append(name)
            continue
        spread = {}
        for q in RAW:
            s = 0.0
            for first, pr in ((x, y) for i, x in enumerate(per_run) for y in per_run[i + 1:]):
                for a, b in zip(first, pr):
                    if a["raw"][q] != b["raw"][q]:
                        va, vb = val(a["raw"][q]), val(b["raw"][q])
                        if not np.array_equal(np.isnan(va), np.isnan(vb)):
                            s = float("inf")
                        else:
                            s = max(s, float(np.nanmax(np.abs(va - vb), initial=0.0)))
            spread[q] = s
        worst = max(spread.values())
        kept[name] = dict(spread=spread, tolerance={q: 10.0 * (s if s > 0.0 else worst) for q, s in spread.items()}, points=per_run[0])
    header = dict(runs=len(runs), recorded_on="the build before cfmm_solve_sweep was divided into sweep_rules.hpp and phases",
                  integers_did_not_repeat=dropped, bitwise=sorted(k for k, c in kept.items() if max(c["spread"].values()) == 0.0),
                  largest_spread={q: max([c["spread"][q] for c in kept.values()] or [0.0]) for q in RAW})
    return dict(header=header, cases=kept)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--pin":
        runs = []
        for path in sys.argv[2:-1]:
            with open(path) as f:
                runs.append(json.load(f))
        text, dest = json.dumps(pin(runs), indent=1, sort_keys=True), sys.argv[-1]
    else:
        text, dest = json.dumps(records(), indent=1, sort_keys=True), sys.argv[1] if len(sys.argv) > 1 else None
    if dest:
        with open(dest, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
