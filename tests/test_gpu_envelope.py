"""GPU suite (-m gpu): the envelope of the single-GPU first-order solve (csrc/iterate.hpp: EnvRec; docs/solve_envelope.md).

The solve returns once a launch behind the one that stored its result has sealed it: the host synchronises the stream neither at entry
nor at exit, launches that found the solve ended may still be in flight when the call returns, and progress and seal words are told
from an earlier solve's by an epoch.  None of that may show in a result.

What "the same result" can mean.  The envelope changes no arithmetic, so the comparison was meant to be bit for bit -- but two runs
of ONE build are not: outside the reproducible mode (which is not on this path) the workgroups flush their net trade into the
accumulator slices with floating-point atomics, in arrival order.  Measured on an MI355X with this file's worker, twice per build:
the PARENT commit against itself differs in every record (one evaluation: value 3e-16, psi 2e-16 of max |psi|; 22 evaluations: value
4e-14, psi 6e-13; 141 evaluations: value 2e-13, prices 4e-14, psi 4e-12); sealed against synchronised and sealed against the parent
differ by the same amounts (at most value 4e-13, prices 1e-13, psi 1e-11); evals, iters and status agree in all of them.  So:
  * evals, iters and status are compared EXACTLY, between the envelopes and against fresh contexts;
  * what a solve read at the seal (cfmm_get_solution: the pinned mirrors) is compared BIT FOR BIT with what the device holds once the
    stream has drained (cfmm_get_nu / cfmm_get_psi), inside one process: this is the check that the result was complete when it was
    read, and run-to-run noise does not enter it;
  * values, prices and net trade of two RUNS are compared to RTOL = 1e-9: a sum over up to 2e4 pool terms per token in arrival order
    moves by at most 2e4 * 2.2e-16 = 4.4e-12 of its gross size per evaluation, growing at worst linearly over the <= 150 evaluations of
    these solves: 7e-10.  (The suite's existing two-process comparison, test_eager_iteration_path_matches_graph_path, uses the same
    1e-9.)  A record of another iterate or another solve is further off than that: the solves stop at a relative gap of 1e-6."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib

import envelope_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


RTOL = 1e-9


def same(a, b):
    """two runs' records (envelope_worker.record, or a vector of tenders): the integers exactly, the rest to RTOL (module docstring)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    if a.size < 7:                                           # (a marker)
        return a.tobytes() == b.tobytes()
    if a.size % 2 == 0:                                      # tenders: against the largest one
        return bool(np.abs(a - b).max() <= RTOL * np.abs(b).max())
    n = (a.size - 7) // 2
    if a[:3].tobytes() != b[:3].tobytes():                   # evals, iters, status
        return False
    ok = abs(a[3] - b[3]) <= RTOL * abs(b[3]) and abs(a[4] - b[4]) <= RTOL * abs(b[4])       # dual and primal value
    ok = ok and abs(a[5] - b[5]) <= RTOL and abs(a[6] - b[6]) <= RTOL                          # gap and infeasibility: relative figures themselves
    ok = ok and np.abs(a[7:7 + n] - b[7:7 + n]).max() <= RTOL * np.abs(b[7:7 + n]).max()
    return bool(ok and np.abs(a[7 + n:] - b[7 + n:]).max() <= RTOL * np.abs(b[7 + n:]).max())


def sealed_equals_drained(prob):
    """what the last solve left in the pinned mirrors against the device's own buffers behind a drained stream: bit for bit"""
    ctx = prob._ensure_ctx()
    nu, psi = ctx.get_solution()
    nu_d, psi_d = ctx.get_nu(), ctx.get_psi()
    return nu.tobytes() == nu_d.tobytes() and psi.tobytes() == psi_d.tobytes()


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """the worker's records under the sealed envelope and under the synchronised one"""
    d = tmp_path_factory.mktemp("envelope")
    out = {}
    for mode in ("sealed", "classic"):
        env = dict(os.environ)
        env.pop("CFMM_ENVELOPE", None)
        if mode == "classic":
            env["CFMM_ENVELOPE"] = "classic"
        path = str(d / f"{mode}.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "envelope_worker.py"), path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.stdout[-2000:], r.stderr[-2000:])
        with np.load(path) as z:
            out[mode] = {k: z[k] for k in z.files}
    return out


def test_sealed_result_equals_drained_result(both):
    s, c = both["sealed"]["cold"], both["classic"]["cold"]
    assert s[2] == 1.0 and s[0] > 4, s[:7]                   # (converged, over more launches than the host runs ahead)
    assert same(s, c), (s[:7], c[:7])
    net = synthetic.config("C2")                             # ... and in this process: complete when it was read
    prob = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    for kw in ({}, dict(max_evals=1), dict(max_evals=2), dict(max_evals=4), dict(max_evals=int(c[0]))):
        st, _, _ = W.raw_solve(prob, net["c"], **kw)
        assert sealed_equals_drained(prob), (kw, st)
    prob.close()


@pytest.mark.parametrize("case", ["at_optimum", "budget_1", "budget_2", "budget_4", "budget_exact"])
def test_edge_endings(both, case):
    s, c = both["sealed"][case], both["classic"][case]
    full = both["classic"]["cold"][0]
    if case == "at_optimum":
        assert c[2] == 1.0 and c[0] <= 2, c[:7]
    elif case == "budget_exact":
        assert c[2] == 1.0 and c[0] == full, (c[:7], full)  # converged in the last launch the budget allows
    else:
        assert c[2] == 3.0 and c[0] == float(case.split("_")[1]), c[:7]
    assert same(s, c), (case, s[:7], c[:7])


@pytest.mark.parametrize("case", ["mixed_cold", "trades_cp2", "warm_after_update", "other_utility", "closed"])
def test_calls_behind_a_solve_see_a_settled_context(both, case):
    s, c = both["sealed"][case], both["classic"][case]
    assert same(s, c), (case, s[:7], c[:7])


def test_back_to_back_solves_do_not_leak():
    """300 solves on one context, nothing between two solves of a burst but the host-side copy of the result; two utilities (another
    optimum, another evaluation count) and two start points each, every result against the same solve on a fresh context, and the last
    of every burst bit for bit against the drained device"""
    net = W.mixed_network()
    utils = [cfmm.Arbitrage(net["c"]), W.second_utility(net)]
    starts = [net["c"], net["c"] * np.exp(np.random.default_rng(5).normal(0.0, 0.02, net["n_tokens"]))]
    want = {}
    for ui, u in enumerate(utils):
        for si, nu0 in enumerate(starts):
            p = cfmm.Problem.from_network(net, utility=u)
            want[ui, si] = W.record(*W.raw_solve(p, nu0))
            p.close()
    evals = {k: int(v[0]) for k, v in want.items()}
    assert all(v[2] == 1.0 for v in want.values()), evals
    assert len(set(evals.values())) >= 2, evals               # (the solves differ in length: a stale word would be a wrong one)
    assert np.abs(want[0, 0][7:] / want[1, 0][7:] - 1.0).max() > 1e-4           # (... and end elsewhere)
    prob = cfmm.Problem.from_network(net, utility=utils[0])
    rng = np.random.default_rng(0)
    done = 0
    ui = 0
    while done < 300:
        prob.set_utility(utils[ui])
        for _ in range(int(rng.integers(1, 5))):              # a burst: solve upon solve
            si = int(rng.integers(0, 2))
            got = W.record(*W.raw_solve(prob, starts[si]))
            assert same(got, want[ui, si]), (done, ui, si, got[:7], want[ui, si][:7])
            done += 1
        assert sealed_equals_drained(prob), (done, ui)
        ui ^= 1
    prob.close()


def test_device_seconds_is_sane():
    net = synthetic.make_network(1000, m_cp2=400_000, seed=1)      # (the evaluation carries the launch: the bounds are about the kernel)
    prob = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = prob._ensure_ctx()
    W.raw_solve(prob, net["c"])
    per_launch = ctx.time_eval_kernel(_lib.TIME_ALL, 200)
    for _ in range(3):
        st, _, _ = W.raw_solve(prob, net["c"])
        print("evals", st["evals"], "device_seconds", st["device_seconds"], "wall_seconds", st["wall_seconds"], "per launch", per_launch)
        assert st["status"] == 1
        assert 0.0 < st["device_seconds"] < st["wall_seconds"], st
        assert 0.3 * st["evals"] * per_launch <= st["device_seconds"] <= 3.0 * st["evals"] * per_launch, (st, per_launch)
    prob.close()
