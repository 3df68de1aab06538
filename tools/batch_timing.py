#!/usr/bin/env python
"""B price vectors per pool read (cfmm_solve_batch): cost of a batched outer iteration against B.
For each B: `reps` cold batched solves of the same B utilities (arbitrage under perturbed market values) on one config;
one JSON line per B with wall ms per batch, device us per lock-step iteration, pool-subproblems/s (pools x sum of the
solves' evaluations / wall), and the single-solve path's figures for the same utilities as the reference line.

--mix NAME: a network with stableswap / power-sum / K-asset table pools among the closed-form families, and ONE path per process
(to be interleaved by the caller, one lease, medians):
    c3mixed   C3's mix at scale 0.065 (1000 tokens, 65 000 pools) with 5 % of the pools curve2 and 1 % four-asset table stableswap
              (3 900 stableswap pools: below AUTO_NEWTON_MIN_STABLE, so method="auto" means first order)
    t200      200 tokens, 20 000 cp2 + 4 000 table stableswap (3- and 4-asset) + 20 000 pow2
--mode clone: 8 utilities through solve_many(batch=0, concurrency=2); --mode batch: through solve_many(batch=B), B = --sizes' first
entry.  One JSON line: the median wall ms of --reps calls.  CFMM_BATCH_WARM=0 in the environment makes the table's batched
stableswap search start cold in every evaluation (A/B of the batch's warm-start slab); under rocprofv3 --kernel-trace --stats the
per-launch times of eval_batch_heavy_kernel and table_batch_eval_kernel are the profiler's averages over this process."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cfmm-routing-code_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import cfmm  # noqa: E402
from cfmm import synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="1,2,4,8")
ap.add_argument("--tol", type=float, default=1e-6)
ap.add_argument("--mix", default=None, choices=["c3mixed", "t200"])
ap.add_argument("--mode", default="batch", choices=["batch", "clone"])
ap.add_argument("--method", default="auto")
args = ap.parse_args()


def mixed_network(name):
    if name == "t200":
        return synthetic.make_network(200, m_cp2=20_000, m_gk_stable=4_000, m_pow2=20_000, seed=0)
    total = 65_000
    m_curve, m_table = total * 5 // 100, total // 100
    rest = total - m_curve - m_table
    net = synthetic.make_network(1000, m_cp2=rest * 7 // 10, m_w2=rest * 2 // 10, m_gn=rest // 10, m_curve2=m_curve, seed=0)
    t = synthetic.make_network(1000, m_gk_stable=m_table, gk_sizes=(4, 4), seed=0)
    assert np.array_equal(t["prices"], net["prices"])
    net["gk"] = t["gk"]
    return net


if args.mix:
    net = mixed_network(args.mix)
    n = net["n_tokens"]
    rng = np.random.default_rng(1)
    utils = [cfmm.Arbitrage(net["c"] * np.exp(rng.normal(0, 0.01, n))) for _ in range(8)]
    p = cfmm.Problem.from_network(net, utility=utils[0])
    B = min(int(args.sizes.split(",")[0]), p._ensure_ctx().batch_capacity())
    kw = dict(batch=B) if args.mode == "batch" else dict(batch=0, concurrency=2)
    us = utils[:B] if args.mode == "batch" else utils
    p.solve_many(us, tol=args.tol, method=args.method, **kw)            # warm-up: clones, attributes
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = p.solve_many(us, tol=args.tol, method=args.method, **kw)
        walls.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(mix=args.mix, mode=args.mode, B=B if args.mode == "batch" else 0, solves=len(us), pools=p.m, stableswap_pools=p._stable_count(),
                          method=args.method, tol=args.tol, batch_warm=os.environ.get("CFMM_BATCH_WARM", "1") != "0",
                          wall_ms=sorted(walls)[len(walls) // 2], wall_ms_all=walls, status=[r["status"] for r in res],
                          evals=[r["stats"]["evals"] for r in res], newton_steps=[r["stats"].get("newton_steps", 0) for r in res],
                          values=[r["value"] for r in res])), flush=True)
    p.close()
    sys.exit(0)

net = synthetic.config(args.config, seed=0) if args.config != "C4shard" else synthetic.config("C4", scale=0.125, seed=0)
n = net["n_tokens"]
rng = np.random.default_rng(1)
utils = [cfmm.Arbitrage(net["c"] * np.exp(rng.normal(0, 0.01, n))) for _ in range(8)]
p = cfmm.Problem.from_network(net, utility=utils[0])
m = p.m
# reference: the single-solve path, one utility after the other
p.solve(tol=args.tol)
t0 = time.perf_counter(); ev1 = 0; dev1 = 0.0
for _ in range(args.reps):
    for u in utils:
        p.set_utility(u); p.solve(tol=args.tol)
        assert p.status == "optimal"
        ev1 += p.stats["evals"]; dev1 += p.stats["device_seconds"]
w1 = time.perf_counter() - t0
print(json.dumps(dict(config=args.config, B=0, path="single", solves=8 * args.reps, evals=ev1, wall_ms_per_solve=1e3 * w1 / (8 * args.reps),
                      device_us_per_eval=1e6 * dev1 / ev1, subproblems_per_s=m * ev1 / w1)), flush=True)
for B in [int(x) for x in args.sizes.split(",")]:
    B = min(B, p.ctx.batch_capacity())
    us = utils[:B]
    p.solve_many(us, tol=args.tol, batch=B)         # warm-up: clones, attributes
    t0 = time.perf_counter(); ev = 0; dev = 0.0; iters = 0
    for _ in range(args.reps):
        res = p.solve_many(us, tol=args.tol, batch=B)
        assert all(r["status"] == "optimal" for r in res), [r["status"] for r in res]
        ev += sum(r["stats"]["evals"] for r in res)
        iters += max(r["stats"]["evals"] for r in res)
        dev += res[0]["stats"]["device_seconds"]
    w = time.perf_counter() - t0
    print(json.dumps(dict(config=args.config, B=B, path="batch", solves=B * args.reps, evals=ev, lockstep_iterations=iters,
                          wall_ms_per_batch=1e3 * w / args.reps, device_us_per_iteration=1e6 * dev / iters,
                          device_us_per_solve_iteration=1e6 * dev / ev, subproblems_per_s=m * ev / w,
                          device_subproblems_per_s=m * ev / dev)), flush=True)
p.close()
