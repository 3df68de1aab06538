"""What makes the measured tolerance of tests/step_parity.py a test and not a loophole, on the CPU twin alone: on every scenario the
GPU cases run, the integer records are stable under the perturbation at every budget, every wrong-rule twin leaves the true one by
>= 100 tolerances, and the rule branches (rejection, step cap, active / fixed / free bounds, window wrap) are taken."""
import numpy as np
import pytest

import step_parity as sp

NAMES = sorted(sp.SCENARIOS)
WITH_WRONG_RULES = [(n, w) for n in NAMES for w in sp.wrong_rule_twins(sp.SCENARIOS[n])]


def _listings(net):
    cnt = np.zeros(net["n_tokens"], dtype=np.int64)
    for key in ("cp2", "w2"):
        np.add.at(cnt, net[key]["ia"], 1); np.add.at(cnt, net[key]["ib"], 1)
    for b in net["gn"].values():
        np.add.at(cnt, b["idx"].ravel(), 1)
    return cnt


@pytest.mark.parametrize("name", NAMES)
def test_integer_records_are_stable_under_the_perturbation(oracle_lib, name):
    """(evals, iters, status) of every perturbed twin run equal the unperturbed run's at every budget; the run neither converges nor
    stalls within K (every budget is a distinct state); K >= memory + 6; every token is listed by a pool (an unlisted token's step is
    decided by the SIGN of its psi, which is the noise itself)"""
    sc = sp.SCENARIOS[name]
    ref = sp.reference(sc)
    assert sc.K >= sc.memory + 6 and len(ref.records) == sc.K and len(ref.perturbed) >= 8
    assert _listings(sp.build(sc).net).min() >= 1
    for k in range(sc.K):
        want = sp.integers(ref.records[k])
        assert want[0] == k + 1 and want[2] == 3, (k + 1, want)
        for s, run in enumerate(ref.perturbed):
            assert sp.integers(run[k]) == want, (name, k + 1, s, sp.integers(run[k]), want)
        for q in sp.QUANTITIES:
            assert np.isfinite(ref.tol[k][q]) and ref.tol[k][q] > 0.0
    if sc.rejecting:
        last = ref.records[-1]
        assert last["iters"] < last["evals"] - 1, "the scenario is to reject trial points"


@pytest.mark.parametrize("name,wrong", WITH_WRONG_RULES)
def test_every_wrong_rule_twin_is_separated(oracle_lib, name, wrong):
    """memory - 1, memory + 1 (memory >= 2), armijo = 0.5 (rejecting scenarios), max_step doubled (capped ones): each deviates from
    the true twin by >= 100 tolerances at some budget <= K (or differs in the integer records there)"""
    sc = sp.SCENARIOS[name]
    mult, k, q = sp.separation(sc, sp.wrong_rule_twins(sc)[wrong])
    print(f"{name} {wrong}: {mult:.3g} tolerances at budget {k} ({q})")
    assert mult >= sp.SEPARATION, (name, wrong, mult, k, q)


def test_budget_records_are_budget_runs(oracle_lib):
    """the record twin_records reads off one run at evaluation k IS the end of a run with max_evals = k, bit for bit"""
    for name in ("n70-arbitrage-s2.5-M3", "n64-liquidate-s0.2-M3-ties", "n129-table-s0.2-M8"):
        sc = sp.SCENARIOS[name]
        recs = sp.twin_records(sc)
        for k in range(1, sc.K + 1):
            own = sp.twin_budget_run(sc, k)
            assert sp.integers(own) == sp.integers(recs[k - 1])
            assert np.array_equal(own["nu"], recs[k - 1]["nu"])
            assert all(own[q] == recs[k - 1][q] for q in sp.QUANTITIES[1:])


def _branches(sc):
    """which rule branches the twin takes on a scenario, from its records"""
    ref = sp.reference(sc)
    b = sp.build(sc)
    last = ref.records[-1]
    out = set()
    if last["iters"] < last["evals"] - 1:
        out.add("rejected")
    if sc.capped and sp.separation(sc, dict(max_step=4.0))[0] >= sp.SEPARATION:
        out.add("capped")                       # (with max_step doubled the twin leaves the trajectory: the cap was active)
    if last["iters"] >= 2 * sc.memory + 2:
        out.add("wrapped")
    if b.grp is None:
        lo = b.ctype == sp.GE
        lo &= b.c > 0
        fixed = b.ctype == sp.FREE
        with np.errstate(divide="ignore"):
            logc = np.log(b.c)
        for r in ref.records[2:]:                # accepted iterates behind the (clamped) start
            s = np.log(r["nu"])
            if lo.any() and (s[lo] <= logc[lo] + 1e-14).any() and (s[lo] > logc[lo] + 1e-6).any():
                out.add("bound_active")
            if fixed.any() and np.all(s[fixed] == logc[fixed]):
                out.add("bound_fixed")
            if (b.ctype == sp.EQ).any() or ((b.ctype == sp.GE) & (b.c == 0)).any():
                out.add("bound_free")
    return out


def test_the_scenarios_take_every_rule_branch(oracle_lib):
    seen = {}
    for name in NAMES:
        for br in _branches(sp.SCENARIOS[name]):
            seen.setdefault(br, []).append(name)
    for br in ("rejected", "capped", "wrapped", "bound_active", "bound_fixed", "bound_free"):
        assert seen.get(br), f"no scenario takes the branch {br!r}"
    # ... and on every family of layouts: the one-launch solves (<= 64 tokens), the evaluation-launch and register forms (<= 2048), the
    # generic kernel (2049)
    for br in ("rejected", "capped", "wrapped", "bound_active"):
        ns = {sp.SCENARIOS[nm].n for nm in seen[br]}
        assert any(n <= 64 for n in ns) and any(64 < n <= 1024 for n in ns) and any(1024 < n <= 2048 for n in ns) and any(n > 2048 for n in ns), (br, sorted(ns))
