#!/usr/bin/env python
"""From a solved route to a solved route over the few pools worth executing (docs/subnetwork.md): the device path of this build
against the host path the same build offers without it, on the headline configuration, medians of --reps in ONE run on ONE context.
Writes profiles/subset.json (--out) and prints it as one JSON line:
  solve_ms          the full network's solve (the library's wall clock)
and per entry of --keep (runs):
  keep              pools the threshold keeps (the threshold is the value taken in of the pool just below the keep best ones)
  readback_ms       every tender of the full network read back (cfmm_get_trades*), on its own
  device            (a) select_pools + get_selected* + subnetwork + the sub-network's warm solve + read-back of ITS tenders:
                    total_ms and the steps
  host              (b) every tender read back, v and the threshold in NumPy, the host sub-network built and uploaded as a new Problem,
                    its solve from the same prices, read-back of its tenders: total_ms and the steps
Both paths end on the same pools (checked) and values that agree to the solves' tolerance (checked)."""
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
from cfmm.problem import KIND2, subset_network  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--keep", default="64,20000", help="pools to keep, one measurement each")
ap.add_argument("--tol", type=float, default=1e-6)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset.json"))
args = ap.parse_args()


def buckets(net):
    for key in KIND2:
        if key in net:
            yield key, np.stack([net[key]["ia"], net[key]["ib"]])
    for k, b in net.get("gn", {}).items():
        yield k, b["idx"]
    for key, b in net.get("gk", {}).items():
        yield key, b["idx"]


def values(nu, net, tr):
    out = {}
    for key, idx in buckets(net):
        d = tr[key][0]
        v = nu[idx[0]] * d[0]
        for j in range(1, idx.shape[0]):
            v = v + nu[idx[j]] * d[j]
        out[key] = v
    return out


def clock():
    return time.perf_counter() * 1e3


net = synthetic.config(args.config, seed=0, scale=args.scale)
util = cfmm.Arbitrage(net["c"])
p = cfmm.Problem.from_network(synthetic.copy_network(net), utility=util)
p.solve(tol=args.tol)
p.solve(tol=args.tol)                                             # (runtime initialised, the buckets reordered, launches captured)
ctx = p.ctx
solve_ms = p.stats["wall_seconds"] * 1e3
v0 = values(p.nu, p.net, p._trades())
allv = np.sort(np.concatenate(list(v0.values())))
med = lambda rows: {k: float(np.median([r[k] for r in rows[1:]])) for k in rows[0]}


def measure(keep):
    thr = float(allv[-keep - 1]) if len(allv) > keep else 0.0
    rb, dev, host = [], [], []
    for rep in range(args.reps + 1):                              # (the first round warms both paths and is dropped)
        # the full read-back on its own
        p._trade_cache = None
        t0 = clock(); p._trades(); t1 = clock()
        rb.append(dict(ms=t1 - t0))
        # (a) on the device
        t0 = clock()
        sel = p.select(thr); t1 = clock()
        q = p.subproblem(); t2 = clock()
        q.solve(tol=args.tol, warm_start=True); t3 = clock()
        q._trades(); t4 = clock()
        dev.append(dict(total_ms=t4 - t0, select_and_lists_ms=t1 - t0, subnetwork_ms=t2 - t1, solve_ms=t3 - t2, readback_ms=t4 - t3))
        # (b) through the host
        p._trade_cache = None
        t0 = clock()
        tr = p._trades(); t1 = clock()
        v = values(p.nu, p.net, tr)
        pos = {key: np.flatnonzero(x > thr) for key, x in v.items()}
        sub = subset_network(p.net, {k: x for k, x in pos.items() if len(x)}); t2 = clock()
        h = cfmm.Problem.from_network(sub, utility=util)
        h._ensure_ctx(); h.ctx.get_nu(); t3 = clock()             # (the copies are enqueued asynchronously: wait for them)
        h.solve(tol=args.tol, nu0=p.nu); t4 = clock()
        h._trades(); t5 = clock()
        host.append(dict(total_ms=t5 - t0, readback_ms=t1 - t0, threshold_and_gather_ms=t2 - t1, create_and_upload_ms=t3 - t2, solve_ms=t4 - t3,
                         sub_readback_ms=t5 - t4))
        for key, x in pos.items():
            assert np.array_equal(sel["positions"][key], x), key
        assert q.m == h.m == sel["selected"]
        assert abs(q.value - h.value) <= 10 * args.tol * max(1.0, abs(h.value)), (q.value, h.value)
        rec = dict(keep=q.m, threshold=thr, value_kept=q.value, status_kept=(q.status, h.status), evals_kept=(q.stats["evals"], h.stats["evals"]))
        q.close(); h.close()
    rec.update(readback_ms=med(rb)["ms"], device=med(dev), host=med(host))
    rec["host_over_device"] = rec["host"]["total_ms"] / rec["device"]["total_ms"]
    return rec


doc = dict(config=args.config, scale=args.scale, pools=p.m, tokens=p.n, backend=ctx.backend, reps=args.reps, tol=args.tol, solve_ms=solve_ms,
           value_full=p.value, readback_bytes=int(sum(2 * idx.size * 8 for _, idx in buckets(p.net))),
           runs=[measure(int(k)) for k in args.keep.split(",")])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(doc, fh, indent=1)
    fh.write("\n")
print(json.dumps(doc))
p.close()
