"""Child process of tests/test_gpu_envelope.py: runs the scenarios of the first-order solve's envelope in THIS process's mode (the
switch CFMM_ENVELOPE is read once per process) and writes every record into one .npz.  A record is everything a solve returns that
must not depend on the envelope: evals, iters, status, the four values, the prices and the net trade.

    python tests/envelope_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cfmm-routing-code_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cfmm  # noqa: E402
from cfmm import synthetic  # noqa: E402
from cfmm.problem import KIND2  # noqa: E402

TOL = 1e-6


def mixed_network():
    """1000 tokens, ~2e4 pools: constant product, weighted and one K-asset bucket -- waves without variables in every workgroup, and
    every store role of the iteration launch on a workgroup of its own"""
    return synthetic.make_network(1000, m_cp2=12_000, m_w2=6_000, m_gn=2_000, gn_sizes=(3, 3), seed=3)


def second_utility(net):
    """market values further from the pools' prices than the network's own: another optimum, more evaluations"""
    return cfmm.Arbitrage(net["c"] * np.exp(np.random.default_rng(11).normal(0.0, 0.05, net["n_tokens"])))


def raw_solve(prob, nu0, **kw):
    """one first-order solve on the raw context, and what it left: (stats, nu, psi)"""
    ctx = prob._ensure_ctx()
    prob._send_utility()
    st = ctx.solve(nu0, tol=TOL, method="lbfgs", **kw)
    nu, psi = ctx.get_solution()
    return st, nu, psi


def record(st, nu, psi):
    head = np.array([st["evals"], st["iters"], st["status"]], dtype=np.float64)
    vals = np.array([st["dual_value"], st["primal_value"], st["gap"], st["infeas"]], dtype=np.float64)
    return np.concatenate([head, vals, np.asarray(nu, dtype=np.float64), np.asarray(psi, dtype=np.float64)])


def main(out):
    rec = {}
    # ---- the smallest network of the one-launch-per-iteration path: the cold solve and its edge endings
    net = synthetic.config("C2")
    prob = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    st, nu, psi = raw_solve(prob, net["c"])
    rec["cold"] = record(st, nu, psi)
    full = st["evals"]
    st1, nu1, psi1 = raw_solve(prob, nu)                      # start prices at the optimum: ends at its first update
    rec["at_optimum"] = record(st1, nu1, psi1)
    for k in (1, 2, 4):                                       # cut by the budget, with fewer launches than the host runs ahead
        rec[f"budget_{k}"] = record(*raw_solve(prob, net["c"], max_evals=k))
    rec["budget_exact"] = record(*raw_solve(prob, net["c"], max_evals=full))      # the converging launch is the last one allowed
    prob.close()

    # ---- calls right behind a solve (the mixed network)
    net = mixed_network()
    prob = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = prob._ensure_ctx()
    rec["mixed_cold"] = record(*raw_solve(prob, net["c"]))
    d, l = ctx.get_trades2(KIND2["cp2"], len(net["cp2"]["Ra"]))                   # the read-back, at once
    rec["trades_cp2"] = np.concatenate([d.ravel(), l.ravel()])
    raw_solve(prob, net["c"])
    after, changes = synthetic.swap_block(net, 0.05, seed=5)                      # an in-place update, at once, and the warm re-solve
    for key, (pos, R) in changes.items():
        prob.update_bucket(key, pos, R)
    rec["warm_after_update"] = record(*raw_solve(prob, None))
    prob.set_utility(second_utility(net))                                         # another utility, at once
    rec["other_utility"] = record(*raw_solve(prob, net["c"]))
    raw_solve(prob, net["c"])
    prob.close()                                                                  # ... and the end of the context, at once
    rec["closed"] = np.array([1.0])
    np.savez(out, **rec)


if __name__ == "__main__":
    main(sys.argv[1])
