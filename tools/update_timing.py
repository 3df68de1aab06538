#!/usr/bin/env python
"""In-place reserve updates (include/cfmm.h: cfmm_update_pools*) against a full re-upload, and a warm re-solve after a block of
swaps against a cold solve of the same network.  One JSON line (profiles/r07_update.json):
  update_ms[count]   host clock around cfmm_update_pools* calls that update `count` pools spread over the buckets in proportion to their
                     size (each call returns synchronised), median of --reps
  reupload_ms        a full upload of the same network into a fresh context (every bucket), median of --reps
  warm / cold        evaluations and milliseconds of solve(warm_start=True) after a 1 % swap-like block (cfmm.synthetic.swap_block),
                     and of a cold solve of the network after the block
--terms: in-place updates of FEES (include/cfmm.h: cfmm_update_terms*) against the re-upload they replace, written to --out
(profiles/terms_update.json); both sides on the same context in the same run, each with and without the first evaluation behind it
(`ready`: that evaluation carries the token-block ordering after a re-upload, and the rebuild of the compact mirror after either):
  C3    fees of 1e2 / 1e3 / 1e4 pools spread over the eight buckets in proportion to their size (eight calls)
  C4    1e7 constant-product pools (--c4-scale shrinks them), the bucket that carries a compact mirror: fees of 1 % of the pools"""
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
ap.add_argument("--terms", action="store_true")
ap.add_argument("--c4-scale", type=float, default=1.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terms_update.json"))
args = ap.parse_args()


def terms_mode():
    def med(ts):
        return float(np.median(ts))

    def upload_all(ctx, net):
        for key, kind in KIND2.items():
            if key in net:
                b = net[key]
                ctx.upload_pools2(kind, b["Ra"], b["Rb"], b["fee"], b["ia"], b["ib"], b.get(PARAM2[key]) if PARAM2[key] else None)
        for k, b in net.get("gn", {}).items():
            ctx.upload_poolsN(b["idx"], b["R"], b["w"], b["fee"])

    def measure(name, scale, counts):
        net = synthetic.config(name, seed=0, scale=scale)
        nu = net["c"]
        p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
        ctx = p._ensure_ctx()
        for _ in range(3):
            ctx.eval_dual(nu)                                     # (runtime initialised, the buckets reordered, the mirror built)
        sizes = {key: len(net[key]["fee"]) for key in KIND2 if key in net}
        sizes.update({k: len(b["fee"]) for k, b in net.get("gn", {}).items()})
        total = sum(sizes.values())
        rng = np.random.default_rng(1)
        ev = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); ctx.eval_dual(nu); ev.append((time.perf_counter() - t0) * 1e3)
        rec = dict(pools=total, buckets=len(sizes), eval_ms=med(ev), eval_bytes=ctx.eval_bytes(), update={})
        for count in counts:
            plan = {}
            for key, m in sizes.items():
                c = max(1, int(round(count * m / total)))
                pos = np.sort(rng.choice(m, c, replace=False)).astype(np.int32)
                b = net[key] if isinstance(key, str) else net["gn"][key]
                plan[key] = (pos, np.ascontiguousarray(b["fee"][pos]))      # (the fees the pools hold: the network stays what it is)
            ts, ready = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for key, (pos, fee) in plan.items():
                    if isinstance(key, str):
                        ctx.update_terms2(KIND2[key], pos, fee=fee)
                    else:
                        ctx.update_termsN(key, pos, fee=fee)
                ts.append((time.perf_counter() - t0) * 1e3)
                ctx.eval_dual(nu)
                ready.append((time.perf_counter() - t0) * 1e3)
            rec["update"][str(count)] = dict(ms=med(ts), ready_ms=med(ready), calls=len(plan), pools=int(sum(len(v[0]) for v in plan.values())),
                                             eval_bytes_after=ctx.eval_bytes())
        ups, ready = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            upload_all(ctx, net)
            ctx.get_nu()                                          # (the copies are enqueued asynchronously: wait for them)
            ups.append((time.perf_counter() - t0) * 1e3)
            ctx.eval_dual(nu)
            ready.append((time.perf_counter() - t0) * 1e3)
        rec.update(reupload_ms=med(ups), reupload_ready_ms=med(ready), backend=ctx.backend)
        for k, u in rec["update"].items():
            u["over_reupload"] = u["ms"] / rec["reupload_ms"]
            u["ready_over_reupload_ready"] = u["ready_ms"] / rec["reupload_ready_ms"]
        p.close()
        return rec

    doc = dict(C3=measure("C3", 1.0, (100, 1000, 10_000)))
    c4 = measure("C4", args.c4_scale, (int(round(100_000 * args.c4_scale)),))
    c4["scale"] = args.c4_scale
    doc["C4"] = c4
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if args.terms:
    terms_mode()
    sys.exit(0)
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
