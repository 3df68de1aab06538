#!/usr/bin/env python
"""A route audited on the device (include/cfmm.h: cfmm_audit_trades; docs/audit.md) against what a caller did before it: every
bucket's tenders read back (cfmm_get_trades*), then the check in NumPy (cfmm.problem.audit_trades).  After a cold arbitrage solve,
--reps repetitions of each on fresh contexts, host clock around synchronised calls.  One JSON line (profiles/audit.json):
  audit_ms            (a) cfmm_audit_trades, per repetition (the first audit of a context: its scratch is made inside the call);
                      audit_again_ms: a second audit of the same context; audit_with_events_ms: with the HIP events below switched on
  host_leg_ms         (b) read-back + NumPy, per repetition; host_leg_split_ms: its two parts
  launches_us         HIP events around the audit's launches alone, per repetition
  grid_sweep_us       the same for other numbers of workgroups per pass (one context, median of --reps audits each)
  agrees              (a) and (b) report the same limbs, counts and worst pool
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
from cfmm.problem import KIND2, audit_trades, audit_buckets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--grids", default="128,256,512,1024,2048")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
net = synthetic.config(args.config, seed=0, scale=args.scale)
util = cfmm.Arbitrage(net["c"])
buckets = [(b["key"], b["R"].shape[1]) for b in audit_buckets(net)]


def solved():
    p = cfmm.Problem.from_network(synthetic.copy_network(net), utility=util)
    p.solve()
    return p


def host_leg(p):
    ctx = p.ctx
    t0 = time.perf_counter()
    tr = {}
    for key, m in buckets:
        tr[key] = (ctx.get_trades2(KIND2[key], m) if isinstance(key, str) else
                   ctx.get_tradesN(key, m) if isinstance(key, int) else ctx.get_tradesG(_lib.POOLK[key[0]], key[1], m))
    t1 = time.perf_counter()
    rep = audit_trades(net, tr, util)
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, [(t1 - t0) * 1e3, (t2 - t1) * 1e3], rep


audit_ms, again_ms, events_ms, launches_us, host_ms, host_split, agrees = [], [], [], [], [], [], []
backend = None
FIELDS = ("pools", "pools_trading", "pools_violating", "legs_out_of_range", "worst_family", "worst_kind", "worst_k", "worst_pos", "min_tender", "min_leg")
for rep in range(args.reps):
    p = solved()
    backend = p.ctx.backend
    t0 = time.perf_counter()
    a = p.ctx.audit(want_limbs=True)
    audit_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    p.ctx.audit()
    again_ms.append((time.perf_counter() - t0) * 1e3)
    p.ctx.debug_audit_launch(True)
    t0 = time.perf_counter()
    p.ctx.audit()
    events_ms.append((time.perf_counter() - t0) * 1e3)
    launches_us.append(p.ctx.debug_audit_launch(False)[0] * 1e6)
    p.close()
    q = solved()
    ms, split, b = host_leg(q)
    host_ms.append(ms); host_split.append(split)
    # (two solves on fresh contexts end on the same point only to rounding: the comparison is made on ONE context)
    a2 = q.ctx.audit(want_limbs=True)
    agrees.append(bool(np.array_equal(a2["limbs"], b["limbs"]) and all(a2[k] == b[k] for k in FIELDS) and abs(a2["min_slack"] - b["min_slack"]) <= 1e-12))
    q.close()
sweep = {}
p = solved()
p.ctx.audit()
for g in [int(x) for x in args.grids.split(",") if x]:
    p.ctx.debug_audit_launch(True, grid=g)
    us = []
    for _ in range(args.reps):
        p.ctx.audit()
        us.append(p.ctx.debug_audit_launch(True)[0] * 1e6)
    sweep[str(g)] = float(np.median(us))
p.close()
slowest = max(audit_ms + again_ms + events_ms)
doc = dict(config=args.config, scale=args.scale, pools=int(sum(m for _, m in buckets)), tokens=int(net["n_tokens"]), backend=backend, reps=args.reps,
           report={k: a[k] for k in a if k not in ("psi", "limbs")},
           audit_ms=audit_ms, audit_again_ms=again_ms, audit_with_events_ms=events_ms, launches_us=launches_us, grid_sweep_us=sweep,
           host_leg_ms=host_ms, host_leg_split_ms=host_split, agrees=agrees,
           slowest_audit_ms=slowest, fastest_host_leg_ms=min(host_ms), accepted=bool(slowest < min(host_ms)))
line = json.dumps(doc)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
