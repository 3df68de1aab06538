#!/usr/bin/env python
"""A solve's trades applied to the resident pools on the device (include/cfmm.h: cfmm_apply_trades) against the path a caller had
before it: every bucket's tenders read back (cfmm_get_trades*), R + Delta - Lambda in NumPy, the pools that moved sent back
(cfmm_update_pools*).  After a cold arbitrage solve, --reps repetitions of each on fresh contexts, host clock around synchronised
calls.  One JSON line (profiles/apply_trades.json):
  apply_ms            (a) cfmm_apply_trades, per repetition
  host_leg_ms         (b) read-back + NumPy + updates, per repetition; host_leg_split_ms: its three parts
  pass_us             HIP events around each pass's launches (the pass that checks, the pass that writes), per repetition
  accepted            the slowest (a), with or without the events, is faster than the fastest (b)"""
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
from cfmm.problem import KIND2, post_trade_reserves  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
net = synthetic.config(args.config, seed=0, scale=args.scale)


def solved():
    p = cfmm.Problem.from_network(synthetic.copy_network(net), utility=cfmm.Arbitrage(net["c"]))
    p.solve()
    return p


def bucket_list(p):
    out = [(key, KIND2[key], len(net[key]["Ra"])) for key in KIND2 if key in net]
    out += [(k, None, b["R"].shape[1]) for k, b in net.get("gn", {}).items()]
    return out


def host_leg(p):
    """what a caller did before: tenders back, new reserves in NumPy, the moved pools through the in-place updates"""
    ctx = p.ctx
    t0 = time.perf_counter()
    tr = {}
    for key, kind, m in bucket_list(p):
        tr[key] = ctx.get_trades2(kind, m) if kind is not None else ctx.get_tradesN(key, m)
    t1 = time.perf_counter()
    plan = {}
    for key, kind, m in bucket_list(p):
        d, l = tr[key]
        b = net[key] if kind is not None else net["gn"][key]
        R = np.stack([b["Ra"], b["Rb"]]) if kind is not None else b["R"]
        pos = np.flatnonzero(((d != 0) | (l != 0)).any(axis=0)).astype(np.int32)
        plan[key] = (kind, pos, np.ascontiguousarray(post_trade_reserves(R[:, pos], d[:, pos], l[:, pos], b["fee"][pos], "pool")))
    t2 = time.perf_counter()
    for key, (kind, pos, Rn) in plan.items():
        if kind is not None:
            ctx.update_pools2(kind, pos, Rn[0], Rn[1])
        else:
            ctx.update_poolsN(pos, Rn)
    t3 = time.perf_counter()
    return (t3 - t0) * 1e3, [(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3], int(sum(len(v[1]) for v in plan.values()))


apply_ms, pass_us, host_ms, host_split, moved, host_moved = [], [], [], [], [], []
backend = None
for rep in range(args.reps):
    p = solved()
    backend = p.ctx.backend
    p.ctx.apply_timers(True)
    t0 = time.perf_counter()
    info = p.ctx.apply_trades("pool")
    apply_ms.append((time.perf_counter() - t0) * 1e3)
    pass_us.append([s * 1e6 for s in p.ctx.apply_timers(False)])
    moved.append(int(info["pools_moved"]))
    p.close()
    q = solved()
    ms, split, cnt = host_leg(q)
    host_ms.append(ms); host_split.append(split)
    host_moved.append(cnt)
    q.close()
# the events cost a little of their own: (a) once more without them
plain_ms = []
for rep in range(args.reps):
    p = solved()
    t0 = time.perf_counter()
    p.ctx.apply_trades("pool")
    plain_ms.append((time.perf_counter() - t0) * 1e3)
    p.close()
doc = dict(config=args.config, scale=args.scale, pools=int(sum(m for _, _, m in bucket_list(None))), backend=backend, reps=args.reps,
           pools_moved=moved, host_leg_pools_moved=host_moved, apply_ms=plain_ms, apply_with_events_ms=apply_ms, pass_us=pass_us, host_leg_ms=host_ms, host_leg_split_ms=host_split,
           slowest_apply_ms=max(plain_ms + apply_ms), fastest_host_leg_ms=min(host_ms), accepted=bool(max(plain_ms + apply_ms) < min(host_ms)))
line = json.dumps(doc)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
