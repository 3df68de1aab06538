"""GPU suite (-m gpu): a route audited on the device (include/cfmm.h: cfmm_audit_trades; csrc/audit.hpp; docs/audit.md).

In every comparison the reference is the NumPy twin (cfmm.problem.audit_trades) run on cfmm_get_trades* of the same context: the
exact limbs and psi bit for bit, the counts, the smallest tender and leg ratio equal, the smallest slack to 1e-12 (the bound
tests/test_gpu.py:160 puts on the same expression: at most eight logarithms of magnitude <= 50, an ulp each), the worst pool
identical whenever the twin's two smallest slacks are further apart than twice that."""
import ctypes

import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib
from cfmm.problem import KIND2, audit_trades, audit_buckets
from oracle import instances as I
from helpers import golden, problem_of, random_instance, table_instance

pytestmark = pytest.mark.gpu

AUDIT_GRID = 512               # csrc/audit.hpp: AU_GRID workgroups of 256 pools per pass
REORDER_MIN = 16384            # csrc/reorder.hpp: RO_MIN_POOLS -- from here a two-asset bucket over >= 32 tokens is stored reordered
SLACK_TOL = 1e-12
SECOND_ORDER_TOL = 1e-3


# ---------------------------------------------------------------------------------------------------------- helpers
def trades_of(ctx, net):
    out = {}
    for b in audit_buckets(net):
        key, m = b["key"], b["R"].shape[1]
        if isinstance(key, str):
            out[key] = ctx.get_trades2(KIND2[key], m)
        elif isinstance(key, int):
            out[key] = ctx.get_tradesN(key, m)
        else:
            out[key] = ctx.get_tradesG(_lib.POOLK[key[0]], key[1], m)
    return out


def reserves_of(ctx, net):
    out = {}
    for b in audit_buckets(net):
        key, m = b["key"], b["R"].shape[1]
        if isinstance(key, str):
            out[key] = np.stack(ctx.get_reserves2(KIND2[key], m))
        elif isinstance(key, int):
            out[key] = ctx.get_reservesN(key, m)
        else:
            out[key] = ctx.get_reservesG(_lib.POOLK[key[0]], key[1], m)
    return out


def same_report(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f") for k in a)


def assert_matches_twin(rep, tw, what=""):
    """the device's report against the twin's, as the module's docstring says"""
    print(what, {k: rep[k] for k in ("pools", "pools_trading", "pools_violating", "legs_out_of_range", "min_slack", "min_tender", "min_leg")},
          "twin min_slack", tw["min_slack"])
    assert np.array_equal(rep["limbs"], tw["limbs"]), what
    assert np.array_equal(rep["psi"], tw["psi"]), what
    for k in ("fixed_exponent", "pools", "pools_trading", "pools_violating", "legs_out_of_range", "min_tender", "min_leg"):
        assert rep[k] == tw[k], (what, k, rep[k], tw[k])
    assert abs(rep["min_slack"] - tw["min_slack"]) <= SLACK_TOL or rep["min_slack"] == tw["min_slack"], (what, rep["min_slack"], tw["min_slack"])
    s = np.sort(np.concatenate([v for v in tw["slack"].values()]))
    if len(s) < 2 or s[1] - s[0] > 2 * SLACK_TOL:
        for k in ("worst_family", "worst_kind", "worst_k", "worst_pos"):
            assert rep[k] == tw[k], (what, k, rep[k], tw[k])
    if np.isfinite(tw["value"]):
        assert abs(rep["value"] - tw["value"]) <= 1e-12 * max(1.0, abs(tw["value"])) and abs(rep["infeas"] - tw["infeas"]) <= 1e-12, what


def check(ctx, net, util, what="", own=None):
    """audit, audit again (identical bytes), audit on another launch geometry (identical), compare with the twin on the read-back"""
    rep = ctx.audit(own=own, want_limbs=True)
    assert same_report(rep, ctx.audit(own=own, want_limbs=True)), what
    ctx.debug_audit_launch(False, grid=3)
    other = ctx.audit(own=own, want_limbs=True)
    ctx.debug_audit_launch(False, grid=AUDIT_GRID)
    for k in ("limbs", "psi", "pools_trading", "pools_violating", "legs_out_of_range", "min_slack", "min_tender", "min_leg", "worst_pos"):
        assert np.array_equal(rep[k], other[k]), (what, k)
    tr = trades_of(ctx, net)
    if own:
        tr.update(own)
    tw = audit_trades(net, tr, util)
    assert_matches_twin(rep, tw, what)
    return rep, tw


def edge_network(n, sizes, seed):
    """a network over n tokens (peg groups of eight) with the bucket sizes `sizes` ({key: m}; keys as bucket_trades takes them)"""
    rng = np.random.default_rng(seed)
    pi = np.exp(rng.normal(0.0, 0.4, n))
    pi = pi[(np.arange(n) // 8) * 8] * np.exp(rng.normal(0.0, 0.002, n))
    net = dict(n_tokens=n, prices=pi, c=pi * np.exp(rng.normal(0.0, 0.01, n)), seed=seed)
    fees = lambda m: synthetic.FEES[rng.integers(0, len(synthetic.FEES), m)]
    value = lambda m: np.exp(rng.normal(np.log(1e3), 1.0, m))

    def group_mates(ia):
        g0 = (ia // 8) * 8
        gs = np.minimum(8, n - g0)
        return (g0 + (ia - g0 + rng.integers(1, 8, len(ia)) % (gs - 1) + 1) % gs).astype(np.int32)

    def distinct(m, k, within_group):
        if within_group:
            g0 = rng.integers(0, max(1, n // 8), m) * 8
            gs = min(8, n)
            idx = g0[:, None] + np.argsort(rng.random((m, gs)), axis=1)[:, :k]
        else:
            idx = np.argsort(rng.random((m, n)), axis=1)[:, :k]
        return np.ascontiguousarray(idx.T).astype(np.int32)

    for key, m in sizes.items():
        if isinstance(key, str):
            ia = rng.integers(0, n, m).astype(np.int32)
            ib = group_mates(ia) if key == "curve2" else ((ia + rng.integers(1, n, m)) % n).astype(np.int32)
            L = value(m)
            Ra, Rb = L / pi[ia] * np.exp(rng.normal(0.0, 0.02, m)), L / pi[ib]
            b = dict(Ra=Ra, Rb=Rb, fee=fees(m), ia=ia, ib=ib)
            if key == "w2":
                b["wa"] = synthetic.W2_CHOICES[rng.integers(0, len(synthetic.W2_CHOICES), m)]
                b["Ra"], b["Rb"] = 2 * b["wa"] * Ra, 2 * (1 - b["wa"]) * Rb
            elif key == "curve2":
                b["alpha"] = synthetic.curve_alpha_from_A(Ra, Rb, np.array([10.0, 50.0, 200.0])[rng.integers(0, 3, m)])
            elif key == "pow2":
                b["t"] = np.array([0.2, 0.5, 0.8])[rng.integers(0, 3, m)]
                b["Rb"] = L / pi[ia] * (pi[ia] / pi[ib]) ** (1.0 / b["t"])
            net[key] = b
        elif isinstance(key, int):
            idx = distinct(m, key, False)
            w = np.where(rng.integers(0, 2, m).astype(bool)[None, :], np.arange(key, 0, -1.0)[:, None], 1.0)
            w = w / w.sum(axis=0, keepdims=True)
            R = key * w * value(m)[None, :] / pi[idx]
            R[0] *= np.exp(rng.normal(0.0, 0.02, m))
            net.setdefault("gn", {})[key] = dict(R=R, w=w, idx=idx, fee=fees(m))
        else:
            kind, k = key
            idx = distinct(m, k, kind == "stable")
            R = value(m)[None, :] / pi[idx] * np.exp(rng.normal(0.0, 0.02, (k, m)))
            param = np.prod(R, axis=0) * R.mean(axis=0) / (2.0 * np.array([10.0, 50.0, 200.0])[rng.integers(0, 3, m)]) if kind == "stable" else np.zeros(m)
            net.setdefault("gk", {})[key] = dict(idx=idx, R=R, fee=fees(m), param=param)
    return net


# bucket sizes 1, 63, 65, 257, 1000 spread over every family, twice
NET3 = dict(cp2=257, w2=65, sum2=63, curve2=1000, pow2=1)
NET3.update({3: 65, ("stable", 3): 257, ("sum", 3): 1000})
NET200 = dict(cp2=1000, w2=257, sum2=1, curve2=63, pow2=65)
NET200.update({3: 1, 8: 1000, ("stable", 3): 63, ("stable", 8): 65, ("sum", 3): 257})


@pytest.mark.parametrize("n,sizes", [(3, NET3), (200, NET200)], ids=["3tokens", "200tokens"])
def test_every_family_at_edge_shapes_matches_the_twin(n, sizes):
    net = edge_network(n, sizes, seed=11 + n)
    util = cfmm.Arbitrage(net["c"])
    p = cfmm.Problem.from_network(net, utility=util)
    ctx = p._ensure_ctx()
    p._send_utility()
    rng = np.random.default_rng(5)
    for rep_no in range(2):                                   # random prices, no solve: every family trades
        ctx.set_nu(net["c"] * np.exp(rng.normal(0.0, 0.03, n)))
        rep, tw = check(ctx, net, util, f"set_nu {rep_no}")
        assert rep["pools"] == sum(sizes.values()) and rep["pools_trading"] > 0.5 * rep["pools"]
        assert rep["pools_violating"] == 0 and rep["min_slack"] >= -1e-9
    p.solve(tol=1e-6)                                          # ... and at the point a solve ends on
    own = {k: v for k, v in p._trades().items() if k == "sum2" or (isinstance(k, tuple) and k[0] == "sum")} if p._theta else None
    check(ctx, net, util, "after solve", own=own)
    p.close()


def test_chunk_stride_wraps_on_a_reordered_bucket():
    """a constant-product bucket larger than grid x 256 pools (a workgroup walks several chunks) and large enough that the upload stores
    it reordered (positions map through perm)"""
    m = 300_000
    assert m > AUDIT_GRID * 256 and m >= REORDER_MIN
    net = synthetic.make_network(200, m_cp2=m, seed=4)
    util = cfmm.Arbitrage(net["c"])
    p = cfmm.Problem.from_network(net, utility=util)
    ctx = p._ensure_ctx()
    p._send_utility()
    ctx.set_nu(net["c"] * np.exp(np.random.default_rng(2).normal(0.0, 0.03, 200)))
    rep, tw = check(ctx, net, util, "300k set_nu")
    assert rep["pools"] == m and rep["pools_violating"] == 0
    assert ctx.debug_audit_launch()[1] == 1                     # the bucket IS stored reordered: upload positions came through perm
    p.solve(tol=1e-6)
    rep, tw = check(ctx, net, util, "300k solved")
    assert rep["pools_violating"] == 0 and rep["worst_pos"] == tw["worst_pos"]
    p.close()


def test_healthy_first_order_solve_passes_its_audit():
    net = synthetic.config("C3", scale=0.01)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    v = p.solve(tol=1e-6, audit=True)
    rep = p.audit_report
    print({k: rep[k] for k in rep if k != "psi"})
    assert p.status == "optimal" and rep["path"] == "device"
    assert rep["pools_violating"] == 0 and rep["legs_out_of_range"] == 0
    assert rep["min_slack"] >= -1e-12
    assert np.abs(rep["psi"] - p.psi).max() <= 1e-9 * max(1.0, float(np.abs(rep["psi"]).max()))
    assert abs(rep["value"] - p.value) <= 1e-9 * abs(rep["value"]) and v == p.value
    assert rep["psi_mismatch"] <= 1e-9 and rep["gap"] <= 1e-6 * (1 + 1e-6) + 1e-15
    check(p.ctx, net, p.utility, "C3 x 0.01")
    q = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    q.solve(tol=1e-6)                                           # the default: no audit, no report
    assert q.audit_report is None and q.status == "optimal"
    p.close(); q.close()


def test_second_order_solve_gross_smoothed_tenders():
    """Behind a second-order solve the audited tenders are the gross smoothed ones: equal to the twin, none violating, and their exact
    sum agrees with the psi the solve reports.

    The solve is made at tol 1e-3: there every run ends on the barrier path with its certificates (at 1e-6 about two in five end on
    the exact evaluation instead, see below), and psi_mismatch measured 7.7e-11 .. 4.8e-10 over 14 fresh runs (9 more at 1e-4:
    4.6e-11 .. 4.7e-10).  At smaller final barrier weights the two psi agree less well -- up to 2.2e-9 at tol 1e-5 and 1e-6 -- which is
    a property of the smoothed point (docs/audit.md, "Python"), not of the audit, and not what this test is about."""
    net = synthetic.config("C5", scale=0.02)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    # (the default method: second order from 4096 stableswap pools on.  At tol 1e-6 the barrier path stalls at its final weight in
    #  about two runs of five on this instance, and the library then certifies the EXACT evaluation at the prices it ended on --
    #  csrc/cfmm_hip.hip: newton_certify_exact; method 1, barrier weight 0, the pools' own tenders.  At tol 1e-3 the smoothed point
    #  meets its certificates while the barrier weight is three orders above that stall: every run ends smoothed)
    p.solve(tol=SECOND_ORDER_TOL)
    assert p.status == "optimal" and p.stats["method"] == _lib.METHODS["newton"] and p.stats["barrier_mu"] > 0, p.stats
    rep, tw = check(p.ctx, net, p.utility, "C5 x 0.02 newton")
    assert rep["pools_violating"] == 0
    d, l = p.bucket_trades("curve2")
    assert np.any((d > 0) & (l > 0))                           # gross: a leg both receives and pays
    full = p.audit()
    print("MISMATCH", full["psi_mismatch"], "evals", p.stats["evals"], "newton_steps", p.stats["newton_steps"], "mu", p.stats["barrier_mu"])
    assert full["psi_mismatch"] <= 1e-9
    p.close()


def test_the_librarys_kink_loop_tenders_are_audited():
    """the shipped arbitrage instance with the default method through the raw context: cfmm_get_trades2 returns the kink loop's tenders
    (pool 4 filled 38.6 %), and those are what the audit sees"""
    inst = I.arbitrage()
    p = problem_of(inst)
    ctx = p._ensure_ctx()
    p._send_utility()
    st = ctx.solve(nu0=np.asarray(inst["utility"]["c"], dtype=np.float64), tol=1e-9)
    assert st["status"] == 1 and st["method"] == _lib.METHODS["lbfgs"]
    d, l = ctx.get_trades2(_lib.POOL_SUM2, 1)
    assert 0.386 < (d + l).max() / 10.0 < 0.3875
    rep, tw = check(ctx, p.net, p.utility, "arbitrage.py, library kink loop")
    assert rep["pools_violating"] == 0 and rep["pools_trading"] == 5
    nu, psi = ctx.get_solution()
    mismatch = np.abs(rep["psi"] - psi).max() / max(np.abs(rep["psi"]).max(), 1e-12 * 10.0)
    assert mismatch <= 1e-9, mismatch
    assert abs(rep["value"] - golden()["arbitrage"]["kkt"]["value"]) <= 1e-7
    p.close()


# seeds whose Python active-set loop ends with fills held on the host (found by scanning the generators on the device once)
CALLER_KINK_CASES = [("random", 0), ("random", 4), ("table", 0), ("table", 1)]


@pytest.mark.parametrize("gen,seed", CALLER_KINK_CASES)
def test_the_callers_kink_loop_passes_its_fills_as_own(gen, seed):
    inst = random_instance(seed, with_sum=True) if gen == "random" else table_instance(seed)[0]
    p = problem_of(inst)
    p.solve(tol=1e-8, method="lbfgs")
    assert p.status == "optimal" and len(p._theta) > 0, (gen, seed, p.status)
    seen = {}
    real = p.ctx.audit
    p.ctx.audit = lambda own=None, **kw: (seen.update(own=own), real(own=own, **kw))[1]
    rep = p.audit()
    assert rep["path"] == "device" and seen["own"] and all(k == "sum2" or k[0] == "sum" for k in seen["own"])
    own = seen["own"]
    p.ctx.audit = real
    tw = audit_trades(p.net, {b["key"]: p.bucket_trades(b["key"]) for b in audit_buckets(p.net)}, p.utility)
    full = p.ctx.audit(own=own, want_limbs=True)
    assert_matches_twin(full, tw, f"{gen} {seed}")
    assert np.array_equal(rep["psi"], tw["psi"])
    assert rep["pools_violating"] == 0 and rep["psi_mismatch"] <= 1e-8, rep
    # without `own` the flagged pools hand out zeros: the context is served all the same, and the fills are missing from psi
    bare = p.ctx.audit(want_limbs=True)
    assert not np.array_equal(bare["psi"], rep["psi"])
    p.close()


def test_doctored_own_tenders_are_reported_not_refused():
    inst = I.arbitrage()
    p = problem_of(inst)
    ctx = p._ensure_ctx()
    p._send_utility()
    ctx.set_nu(np.asarray(inst["utility"]["c"], dtype=np.float64))
    b = p.net["sum2"]
    R = np.array([b["Ra"][0], b["Rb"][0]]); g = b["fee"][0]
    cases = []
    over = (np.array([[1.5 * R[1] / g], [0.0]]), np.array([[0.0], [1.5 * R[1]]]))           # 1.5 times the full fill of leg b
    cases.append(("overfilled", over, dict(pools_violating=1, legs_out_of_range=0)))
    negative = (np.array([[-1e-3], [0.0]]), np.array([[0.0], [0.0]]))
    cases.append(("negative", negative, dict(pools_violating=1, legs_out_of_range=0)))
    huge = (np.array([[0.0], [0.0]]), np.array([[1e300], [0.0]]))
    cases.append(("1e300", huge, dict(pools_violating=1, legs_out_of_range=1)))
    base = trades_of(ctx, p.net)
    for name, own2, want in cases:
        rc, rep = ctx.audit(own={"sum2": own2}, want_limbs=True, check=False)
        assert rc == 0, name
        tr = dict(base); tr["sum2"] = own2
        tw = audit_trades(p.net, tr, p.utility)
        assert_matches_twin(rep, tw, name)
        assert audit_trades(p.net, base, p.utility)["pools_violating"] == 0
        assert rep["pools_violating"] == want["pools_violating"], (name, rep)
        assert rep["legs_out_of_range"] == want["legs_out_of_range"], name
        assert (rep["worst_family"], rep["worst_kind"], rep["worst_k"], rep["worst_pos"]) == (tw["worst_family"], tw["worst_kind"], tw["worst_k"], tw["worst_pos"])
        if name == "overfilled":
            assert rep["min_leg"] < 0.0
        if name == "negative":
            assert rep["min_tender"] == -1e-3
    # own tenders for a bucket that holds no pool are ignored
    plain = ctx.audit(want_limbs=True)
    ghost = ctx.audit(own={("sum", 5): (np.full((5, 1), 7.0), np.full((5, 1), 7.0))}, want_limbs=True)
    assert same_report(plain, ghost)
    with pytest.raises(_lib.CfmmError) as e:
        ctx.audit(own={"cp2": base["cp2"]})
    assert e.value.code is None
    p.close()


def test_an_audit_moves_nothing():
    """against a twin context that never audited: reserves, cached solution, tenders (a table-stableswap bucket included) and the
    evaluations of a following warm solve are bitwise equal; a clone's cached solution survives the parent's audit"""
    net = synthetic.make_network(200, m_cp2=2000, m_gn=200, m_gk_stable=400, seed=2)
    util = cfmm.Arbitrage(net["c"])
    a = cfmm.Problem.from_network(synthetic.copy_network(net), utility=util, deterministic=True)
    b = cfmm.Problem.from_network(synthetic.copy_network(net), utility=util, deterministic=True)
    for p in (a, b):
        p.solve(tol=1e-6, method="lbfgs", max_evals=300)
    clone = a.clone()
    clone.solve(tol=1e-6, method="lbfgs", max_evals=300)
    clone_sol = clone.ctx.get_solution()
    for _ in range(3):
        rep = a.ctx.audit(want_limbs=True)
    assert rep["pools"] == a.m
    for x, y in zip(a.ctx.get_solution(), b.ctx.get_solution()):
        assert np.array_equal(x, y)
    ra, rb = reserves_of(a.ctx, net), reserves_of(b.ctx, net)
    ta, tb = trades_of(a.ctx, net), trades_of(b.ctx, net)
    assert any(isinstance(k, tuple) and k[0] == "stable" for k in ta)
    for key in ra:
        assert np.array_equal(ra[key], rb[key]), key
        assert np.array_equal(ta[key][0], tb[key][0]) and np.array_equal(ta[key][1], tb[key][1]), key
    for x, y in zip(clone.ctx.get_solution(), clone_sol):
        assert np.array_equal(x, y)
    a.ctx.audit()
    sa, sb = a.ctx.solve(None, tol=1e-7, method=_lib.METHODS["lbfgs"], max_evals=300), b.ctx.solve(None, tol=1e-7, method=_lib.METHODS["lbfgs"], max_evals=300)
    assert sa["evals"] == sb["evals"] and sa["status"] == sb["status"], (sa, sb)
    for x, y in zip(a.ctx.get_solution(), b.ctx.get_solution()):
        assert np.array_equal(x, y)
    clone.close(); a.close(); b.close()


def test_refusals_and_what_is_served():
    net = edge_network(40, dict(cp2=100, sum2=20), seed=3)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    rc, _ = ctx.audit(check=False)
    assert rc == _lib.E_STATE                                   # no prices yet
    ctx.set_nu(net["c"])
    rep = ctx.audit()                                           # no utility yet: value and infeas are NaN
    assert np.isnan(rep["value"]) and np.isnan(rep["infeas"]) and rep["pools"] == 120
    assert ctx.L.cfmm_audit_trades(ctx.h, None, 0.0, None, None, None) == _lib.E_ARG
    assert ctx.L.cfmm_audit_trades(None, None, 0.0, ctypes.byref(_lib.Audit()), None, None) == _lib.E_ARG
    p._send_utility()
    # tie flags set by the caller: served (cfmm_apply_trades refuses these), and the flagged pools hand out zeros
    free, _ = check(ctx, net, p.utility, "no flags")
    flags = np.zeros(20, dtype=np.int32); flags[::2] = 1
    ctx.set_pool_flags(_lib.POOL_SUM2, flags)
    rc, info = ctx.apply_trades(check=False)
    assert rc == _lib.E_UNSUPPORTED
    tied, _ = check(ctx, net, p.utility, "flags")
    d, l = ctx.get_trades2(_lib.POOL_SUM2, 20)
    assert not d[:, ::2].any() and not l[:, ::2].any() and tied["pools_trading"] <= free["pools_trading"]
    ctx.set_pool_flags(_lib.POOL_SUM2, None)
    p.close()
    big = cfmm.Problem.from_network(synthetic.make_network(2600, m_cp2=3000, seed=1), utility=None)
    c2 = big._ensure_ctx()
    c2.set_nu(big.net["c"])
    rc, _ = c2.audit(check=False)
    assert rc == _lib.E_LIMIT and "2560" in c2.L.cfmm_last_error(c2.h).decode()
    big.close()
