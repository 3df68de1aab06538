#!/usr/bin/env python
"""In-place reserve updates (include/cfmm.h: cfmm_update_pools*) against a full re-upload, and a warm re-solve after a block of
swaps against a cold solve of the same network.  One JSON line (profiles/r07_update.json):
  update_ms[count]   host clock around cfmm_update_pools* calls that update `count` pools spread over the buckets in proportion to their
                     size (each call returns synchronised), median of --reps
  reupload_ms        a full upload of the same network into a fresh context (every bucket), median of --reps
  warm / cold        evaluations and milliseconds of solve(warm_start=True) after a 1 % swap-like block (cfmm.synthetic.swap_block),
                     and of a cold solve of the network after the block"""
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
from cfmm import synthetic, _lib  # noqa: E402
from cfmm.problem import KIND2, PARAM2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
net = synthetic.config(args.config, seed=0)
n = net["n_tokens"]


def upload(ctx):
    for key, kind in KIND2.items():
        if key in net:
            b = net[key]
            ctx.upload_pools2(kind, b["Ra"], b["Rb"], b["fee"], b["ia"], b["ib"], b.get(PARAM2[key]) if PARAM2[key] else None)
    for k, b in net.get("gn", {}).items():
        ctx.upload_poolsN(b["idx"], b["R"], b["w"], b["fee"])


p = cfmm.Problem.from_network(synthetic.copy_network(net), utility=cfmm.Arbitrage(net["c"]))
p.solve()                                                         # (runtime initialised, the buckets reordered)
ctx = p.ctx
sizes = {key: len(net[key]["Ra"]) for key in KIND2 if key in net}
sizes.update({k: b["R"].shape[1] for k, b in net.get("gn", {}).items()})
total = sum(sizes.values())
rng = np.random.default_rng(1)
upd = {}
for count in (100, 1000, 10_000, 100_000):
    plan = {}
    for key, m in sizes.items():
        c = max(1, int(round(count * m / total)))
        pos = np.sort(rng.choice(m, c, replace=False)).astype(np.int32)
        if isinstance(key, str):
            plan[key] = (pos, np.ascontiguousarray(net[key]["Ra"][pos]), np.ascontiguousarray(net[key]["Rb"][pos]))
        else:
            plan[key] = (pos, np.ascontiguousarray(net["gn"][key]["R"][:, pos]))
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for key, args_ in plan.items():
            if isinstance(key, str):
                ctx.update_pools2(KIND2[key], *args_)
            else:
                ctx.update_poolsN(*args_)
        ts.append((time.perf_counter() - t0) * 1e3)
    upd[str(count)] = dict(ms=float(np.median(ts)), calls=len(plan), pools=int(sum(len(v[0]) for v in plan.values())),
                           bytes=int(sum(sum(a.nbytes for a in v) for v in plan.values())))
ups = []
for _ in range(args.reps):
    c2 = _lib.Context(n, 0)
    t0 = time.perf_counter()
    upload(c2)
    c2.get_nu()                                                   # (the copies are enqueued asynchronously: wait for them)
    ups.append((time.perf_counter() - t0) * 1e3)
    c2.close()
after, changes = synthetic.swap_block(net, 0.01, seed=7)
t0 = time.perf_counter()
for key, (pos, R) in changes.items():
    p.update_bucket(key, pos, R)
block_ms = (time.perf_counter() - t0) * 1e3
p.solve(warm_start=True)
warm = dict(evals=p.stats["evals"], ms=p.stats["wall_seconds"] * 1e3, status=p.status, value=p.value)
q = cfmm.Problem.from_network(after, utility=cfmm.Arbitrage(after["c"]))
q._ensure_ctx()
q.solve()
cold = dict(evals=q.stats["evals"], ms=q.stats["wall_seconds"] * 1e3, status=q.status, value=q.value)
reup = float(np.median(ups))
print(json.dumps(dict(config=args.config, pools=total, backend=ctx.backend, update=upd, reupload_ms=reup,
                      update_1e4_over_reupload=upd["10000"]["ms"] / reup, block_update_ms=block_ms,
                      block_pools=int(sum(len(v[0]) for v in changes.values())), warm=warm, cold=cold,
                      warm_fewer_evals=warm["evals"] < cold["evals"])))
p.close(); q.close()
