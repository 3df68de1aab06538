"""GPU suite (-m gpu): a held route re-quoted on the device (include/cfmm.h: cfmm_hold_route, cfmm_requote_route; csrc/requote.hpp;
docs/requote.md).

Set-up of every test: prices or a solve, hold, the pools moved in place (reserves times exp(u), u uniform in +-0.05; one pool in eight
untouched, one in eight shrunk 100 times, one fee changed), re-quote.  Then
  scales    the device's s against 50-digit roots (tests/requote_ref.py) computed here from the read-back reserves and the held tenders,
            within SCALE_FACTOR times the bound derived from the slack's rounding -- every trading pool
  psi       with the device's scales handed in, the NumPy twin's limbs, psi and counts equal the device's bit for bit; value / infeas to
            1e-12 (the audit suite's bound on the same host expression); min_scale and its pool identical
  slack     the re-quoted tenders (Delta, fl(s Lambda)) audited by the twin at the moved reserves: every slack >= -1e-9 (the audit's
            tol_pool) and at most the slack at the twin's own root plus the derived bound
  geometry  the default grid against grid = 3, and a second call: identical bytes"""
import ctypes

import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib
from cfmm.problem import KIND2, audit_trades, audit_buckets, requote_route
from oracle import instances as I
from helpers import problem_of, mixed_network, table_instance
from test_gpu_audit import trades_of, reserves_of, edge_network, SECOND_ORDER_TOL, REORDER_MIN
import requote_ref as ref

pytestmark = pytest.mark.gpu

REQUOTE_GRID = 2048            # csrc/requote.hpp: RQ_GRID
SCALE_FACTOR = 1.0             # the device's worst |s - s*| / bound measured <= 1 (docs/requote.md): no factor is needed
TOL_POOL = 1e-9


# ---------------------------------------------------------------------------------------------------------- helpers
def per_bucket(net, two, gn, gk):
    out = {}
    for b in audit_buckets(net):
        key, m = b["key"], b["R"].shape[1]
        out[key] = two(KIND2[key], m) if isinstance(key, str) else (gn(key, m) if isinstance(key, int) else gk(_lib.POOLK[key[0]], key[1], m))
    return out


def held_of(ctx, net):
    return per_bucket(net, ctx.held2, ctx.heldN, ctx.heldG)


def scales_of(ctx, net):
    return per_bucket(net, ctx.route_scale2, ctx.route_scaleN, ctx.route_scaleG)


def move_pools(p, seed, through=None):
    """the set-up's move, through Problem.update_bucket / update_bucket_terms of `through` (a clone) or p itself: p.net follows"""
    rng = np.random.default_rng(seed)
    q = through if through is not None else p
    for b in audit_buckets(p.net):
        key, R = b["key"], b["R"]
        m = R.shape[1]
        f = np.exp(rng.uniform(-0.05, 0.05, R.shape))
        f[:, 3::8] *= 0.01
        pos = np.flatnonzero(np.arange(m) % 8 != 0)
        if len(pos):
            q.update_bucket(key, pos, (R * f)[:, pos])
        if m > 1:
            q.update_bucket_terms(key, [1], fee=[0.5 * (float(b["fee"][1]) + 1.0)])


def same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.tobytes() == y.tobytes(), (what, k)


def check(p, what="", every=1, roots=True):
    """the module docstring's checks on the context's held route and the pools as they are now; returns (report, twin with the
    device's scales, the device's worst |s - s*| / bound)"""
    ctx, net, util = p.ctx, p.net, p.utility
    now = reserves_of(ctx, net)
    for b in audit_buckets(net):                               # the host copy follows the in-place updates: the twin reads it
        assert np.array_equal(b["R"], now[b["key"]]), (what, b["key"])
    held = held_of(ctx, net)
    rep = ctx.requote(want_limbs=True)
    sc = scales_of(ctx, net)
    # geometry and repetition
    again, sc_again = ctx.requote(want_limbs=True), scales_of(ctx, net)
    ctx.debug_requote_launch(False, grid=3)
    other, sc_other = ctx.requote(want_limbs=True), scales_of(ctx, net)
    ctx.debug_requote_launch(False, grid=REQUOTE_GRID)
    same_bytes(rep, again, what + " again"); same_bytes(rep, other, what + " grid 3")
    same_bytes(sc, sc_again, what + " scales again"); same_bytes(sc, sc_other, what + " scales grid 3")
    # psi, counts, the report: the twin with the device's scales
    tw = requote_route(net, held, util, scales=sc)
    print(what, {k: rep[k] for k in rep if k not in ("psi", "limbs")})
    assert np.array_equal(rep["limbs"], tw["limbs"]), what
    assert np.array_equal(rep["psi"], tw["psi"]), what
    for k in ("fixed_exponent", "pools", "pools_trading", "pools_short", "pools_long", "pools_capped", "pools_failed", "legs_out_of_range",
              "min_scale", "min_family", "min_kind", "min_k", "min_pos"):
        assert rep[k] == tw[k], (what, k, rep[k], tw[k])
    if util is not None:
        assert abs(rep["value"] - tw["value"]) <= 1e-12 * max(1.0, abs(tw["value"])) and abs(rep["infeas"] - tw["infeas"]) <= 1e-12, what
    else:
        assert np.isnan(rep["value"]) and np.isnan(rep["infeas"])
    for b in audit_buckets(net):
        key = b["key"]
        d, l = held[key]
        idle = ~((d != 0) | (l != 0)).any(axis=0)
        assert np.all(sc[key][idle] == 1.0), (what, key)
    # the pools accept what the call says they pay
    aud = audit_trades(net, {k: (held[k][0], tw["lambdas"][k]) for k in held}, None, tol_pool=TOL_POOL)
    assert aud["pools_violating"] == 0 and aud["min_slack"] >= -TOL_POOL, (what, aud["min_slack"], aud["pools_violating"])
    worst = 0.0
    if roots:
        own = requote_route(net, held, None)                    # the twin's own roots
        aud_own = audit_trades(net, {k: (held[k][0], own["lambdas"][k]) for k in held}, None, tol_pool=TOL_POOL)
        rt = ref.roots(net, held, every=every)
        count = 0
        for b in audit_buckets(net):
            key = b["key"]
            r = rt[key]
            for i in np.flatnonzero(r["trading"] & (np.arange(len(r["s"])) % every == 0)).tolist():
                err = abs(sc[key][i] - r["s"][i])
                if r["tol"][i] > 0:
                    worst = max(worst, err / r["tol"][i])
                assert err <= SCALE_FACTOR * r["tol"][i], (what, key, i, r["kind"][i], sc[key][i], r["s"][i], err, r["tol"][i])
                if r["kind"][i] == "root" and b["cls"] != "sum":
                    # nothing is left on the table
                    assert aud["slack"][key][i] <= aud_own["slack"][key][i] + r["ftol"][i], (what, key, i, aud["slack"][key][i], aud_own["slack"][key][i], r["ftol"][i])
                count += 1
        print(f"{what}: {count} pools against 50-digit roots, the device's worst |s - s*| / bound = {worst:.3f}")
        assert count > 0
    return rep, tw, worst


# ---------------------------------------------------------------------------------------------------------- scales, psi, slack
SMALL = dict(cp2=60, w2=40, sum2=24, curve2=40, pow2=40)
SMALL.update({3: 30, 8: 30, ("stable", 3): 30, ("stable", 8): 20, ("sum", 3): 20})


def test_scales_psi_and_slack_of_every_class():
    net = edge_network(40, SMALL, seed=21)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    p._send_utility()
    ctx.set_nu(net["c"] * np.exp(np.random.default_rng(3).normal(0.0, 0.03, 40)))      # random prices, no solve: every family trades
    before = trades_of(ctx, net)
    info = ctx.hold_route()
    assert info["pools"] == sum(SMALL.values()) and info["pools_trading"] > 0.5 * info["pools"]
    assert info["bytes"] == sum(8 * (2 * b["k"] + 1) * b["R"].shape[1] for b in audit_buckets(net))
    same = ctx.requote()                                       # nothing has moved yet: every pool re-quotes to 1 within rounding
    assert same["pools_short"] == 0 and same["pools_long"] == 0 and same["pools_capped"] == 0 and abs(same["min_scale"] - 1.0) <= 1e-11
    move_pools(p, seed=4)
    rep, tw, worst = check(p, "every class")
    held = held_of(ctx, net)
    for key in before:
        assert np.array_equal(held[key][0], before[key][0]) and np.array_equal(held[key][1], before[key][1]), key
    assert rep["pools_trading"] == info["pools_trading"] and rep["pools_failed"] == 0 and rep["legs_out_of_range"] == 0
    assert rep["pools_short"] > 0 and rep["pools_long"] > 0 and rep["pools_capped"] > 0
    assert rep["pools_short"] + rep["pools_long"] <= rep["pools_trading"]
    # tol_scale: a loose one classifies fewer pools
    loose = ctx.requote(tol_scale=0.03)
    assert loose["pools_short"] < rep["pools_short"] and loose["pools_long"] < rep["pools_long"] and np.array_equal(loose["psi"], rep["psi"])
    p.close()


@pytest.mark.parametrize("sizes", [dict(cp2=255, w2=256, curve2=257), {3: 600, ("stable", 3): 257, "sum2": 255}], ids=["two_asset", "k_asset"])
def test_geometry_at_chunk_edges(sizes):
    net = edge_network(24, sizes, seed=31)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    p._send_utility()
    ctx.set_nu(net["c"] * np.exp(np.random.default_rng(5).normal(0.0, 0.03, 24)))
    ctx.hold_route()
    move_pools(p, seed=6)
    rep, tw, _ = check(p, "chunk edges", roots=False)
    assert rep["pools"] == sum(sizes.values())
    p.close()


def test_a_bucket_stored_reordered():
    """16 384 constant-product pools over 32 tokens: the upload stores the bucket reordered, so held tenders are read and scales are
    written through the permutation"""
    m = REORDER_MIN
    net = synthetic.make_network(32, m_cp2=m, seed=4)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    p._send_utility()
    ctx.set_nu(net["c"] * np.exp(np.random.default_rng(2).normal(0.0, 0.03, 32)))
    before = trades_of(ctx, net)
    ctx.hold_route()
    move_pools(p, seed=7)
    rep, tw, _ = check(p, "reordered", every=64)
    assert ctx.debug_requote_launch()[1] == 1                   # the bucket IS stored reordered
    held = held_of(ctx, net)
    assert np.array_equal(held["cp2"][0], before["cp2"][0]) and np.array_equal(held["cp2"][1], before["cp2"][1])
    assert rep["pools"] == m and rep["pools_trading"] > 0.9 * m
    p.close()


def test_every_bucket_family_in_one_context_after_a_solve():
    net = mixed_network(seed=1, n=60, m=150)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    p._send_utility()
    # through the raw context: no Python kink loop, no tie flags -- the device serves the hold whatever the constant-sum pools do
    st = ctx.solve(nu0=np.asarray(net["c"], dtype=np.float64), tol=1e-6, method=_lib.METHODS["lbfgs"], max_evals=300)
    assert st["status"] in (1, 2, 3)
    info = ctx.hold_route()
    assert info["pools"] == p.m and {b["key"] for b in audit_buckets(net)} >= {"cp2", "w2", "sum2", "curve2"}
    move_pools(p, seed=8)
    rep, tw, _ = check(p, "mixed network", every=4)
    assert rep["pools"] == p.m and rep["pools_trading"] == info["pools_trading"] and rep["pools_failed"] == 0
    p.close()


# helpers.table_instance by seed, and the path Problem.hold_route must take: seeds 2 and 3 end without fills held in Python (the device
# holds the route); seed 0 ends with some (tests/test_gpu_audit.py: CALLER_KINK_CASES), so the route is held here and re-quoted by the twin
TABLE_CASES = [(2, "device"), (3, "device"), (0, "host")]


@pytest.mark.parametrize("seed,want", TABLE_CASES)
def test_table_instances_through_the_problem(seed, want):
    """helpers.table_instance (K-asset stableswap and constant-sum pools among constant-product pools): Problem.hold_route / requote /
    release_route on the path named above -- on the device with every check of the module -- against the twin on the read-back reserves"""
    inst, _ = table_instance(seed)
    p = problem_of(inst)
    v0 = p.solve(tol=1e-8, method="lbfgs")
    tr = {k: (d.copy(), l.copy()) for k, (d, l) in p._trades().items()}
    psi0 = p.psi.copy()
    info = p.hold_route()
    path = p._held_route["path"]
    assert path == want and path == ("host" if p._theta else "device"), (seed, path, len(p._theta))
    move_pools(p, seed=9 + seed)
    out = p.requote()
    assert out["path"] == path
    if path == "device":
        check(p, f"table {seed}")
    tw = requote_route(p.net, tr, p.utility, scales=out["scale"] if path == "device" else None)
    assert np.array_equal(out["psi"], tw["psi"])
    for k in ("pools", "pools_trading", "pools_short", "pools_long", "pools_capped", "pools_failed", "min_scale", "min_pos"):
        assert out[k] == tw[k], (k, out[k], tw[k])
    assert np.array_equal(out["shortfall"], psi0 - out["psi"]) and out["value_held"] == v0
    assert out["pools"] == info["pools"] and set(out["scale"]) == {b["key"] for b in audit_buckets(p.net)}
    lam = [tw["lambdas"][key][:, pos] for key, pos in p.where]
    dlt = [tr[key][0][:, pos] for key, pos in p.where]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out["lambdas"], lam))
    assert all(np.array_equal(a, b) for a, b in zip(out["deltas"], dlt))
    p.release_route()
    with pytest.raises(_lib.CfmmError):
        p.requote()
    p.close()


def test_gross_tenders_of_a_second_order_solve():
    """the audit suite's small C5 case at SECOND_ORDER_TOL: the held tenders are the gross smoothed ones, legs that both receive and pay"""
    net = synthetic.config("C5", scale=0.02)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    p.solve(tol=SECOND_ORDER_TOL)
    assert p.status == "optimal" and p.stats["method"] == _lib.METHODS["newton"] and p.stats["barrier_mu"] > 0, p.stats
    before = trades_of(p.ctx, net)
    p.ctx.hold_route()
    d, l = p.ctx.held2(_lib.POOL_CURVE2, len(net["curve2"]["Ra"]))
    assert np.array_equal(d, before["curve2"][0]) and np.array_equal(l, before["curve2"][1])
    assert np.any((d > 0) & (l > 0))                           # gross: a leg both receives and pays
    move_pools(p, seed=12)
    rep, tw, _ = check(p, "C5 x 0.02 newton", every=16)
    assert rep["pools_failed"] == 0
    p.close()


def test_the_librarys_kink_loop_tenders_are_held():
    """the shipped arbitrage instance through the raw context: the held constant-sum pool is the kink loop's, filled 38.6 %"""
    inst = I.arbitrage()
    p = problem_of(inst)
    ctx = p._ensure_ctx()
    p._send_utility()
    st = ctx.solve(nu0=np.asarray(inst["utility"]["c"], dtype=np.float64), tol=1e-9)
    assert st["status"] == 1 and st["method"] == _lib.METHODS["lbfgs"]
    before = trades_of(ctx, p.net)
    info = ctx.hold_route()
    assert info["pools"] == 5 and info["pools_trading"] == 5
    d, l = ctx.held2(_lib.POOL_SUM2, 1)
    assert np.array_equal(d, before["sum2"][0]) and np.array_equal(l, before["sum2"][1])
    assert 0.386 < (d + l).max() / 10.0 < 0.3875
    same = ctx.requote()
    assert same["pools_trading"] == 5 and same["pools_short"] == 0 and same["pools_long"] == 0
    move_pools(p, seed=13)
    rep, tw, _ = check(p, "arbitrage.py, library kink loop")
    assert rep["pools_trading"] == 5
    p.close()


# ---------------------------------------------------------------------------------------------------------- the hold's contract
def test_the_hold_survives_what_it_must_and_goes_when_it_must():
    net = edge_network(40, dict(cp2=100, curve2=50), seed=3)
    keys = [b["key"] for b in audit_buckets(net)]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    rc, _ = ctx.hold_route(check=False)
    assert rc == _lib.E_STATE                                   # no prices yet
    rc, _ = ctx.requote(check=False)
    assert rc == _lib.E_STATE                                   # no held route
    with pytest.raises(_lib.CfmmError) as e:
        ctx.held2(_lib.POOL_CP2, 100)
    assert e.value.code == _lib.E_STATE
    p._send_utility()
    ctx.set_nu(net["c"] * np.exp(np.random.default_rng(1).normal(0.0, 0.03, 40)))
    # tie flags set by the caller: refused like cfmm_apply_trades
    tnet = edge_network(40, dict(cp2=30, sum2=20), seed=5)
    tied = cfmm.Problem.from_network(tnet, utility=cfmm.Arbitrage(tnet["c"]))
    tctx = tied._ensure_ctx()
    tied._send_utility()
    tctx.set_nu(tied.net["c"])
    flags = np.zeros(20, dtype=np.int32); flags[::2] = 1
    tctx.set_pool_flags(_lib.POOL_SUM2, flags)
    rc, _ = tctx.hold_route(check=False)
    assert rc == _lib.E_UNSUPPORTED
    tctx.set_pool_flags(_lib.POOL_SUM2, None)
    assert tctx.hold_route()["pools"] == 50
    # price ties set by the caller: refused alike, and served again once they are lifted
    grp = np.arange(40, dtype=np.int32); grp[1] = 0; grp[2:] -= 1
    tctx.set_ties(grp, np.zeros(40))
    rc, _ = tctx.hold_route(check=False)
    assert rc == _lib.E_UNSUPPORTED
    tctx.set_ties(None)
    assert tctx.hold_route()["pools"] == 50
    tied.close()
    before = trades_of(ctx, net)
    ctx.hold_route()
    with pytest.raises(_lib.CfmmError) as e:
        ctx.route_scale2(_lib.POOL_CP2, 100)                    # no re-quote yet
    assert e.value.code == _lib.E_STATE
    assert ctx.L.cfmm_requote_route(ctx.h, 0.0, None, None, None) == _lib.E_ARG
    assert ctx.L.cfmm_requote_route(None, 0.0, ctypes.byref(_lib.Requote()), None, None) == _lib.E_ARG

    def still_held(what):
        held = held_of(ctx, net)
        for key in keys:
            assert np.array_equal(held[key][0], before[key][0]) and np.array_equal(held[key][1], before[key][1]), (what, key)

    still_held("at once")
    clone = p.clone()
    rc, _ = clone._ensure_ctx().requote(check=False)
    assert rc == _lib.E_STATE                                   # a clone does not carry the route
    move_pools(p, seed=2, through=clone)                        # an update through a CLONE
    still_held("update through a clone")
    rep1, _, _ = check(p, "after the clone's update", roots=False)
    p.solve(tol=1e-6, method="lbfgs")                           # a re-solve moves the point, not the held route
    still_held("re-solve")
    p.apply_trades()                                            # ... and the pools again
    still_held("apply_trades")
    ctx.set_nu(net["c"])
    p.set_utility(cfmm.Arbitrage(net["c"] * 1.01)); p._send_utility()
    still_held("set_nu, set_utility")
    rep2, _, _ = check(p, "after solve, apply, set_nu", roots=False)
    assert not np.array_equal(rep1["psi"], rep2["psi"])          # the pools moved in between: another quote of the same route
    # a second hold replaces the first
    now = trades_of(ctx, net)
    ctx.hold_route()
    held = held_of(ctx, net)
    assert all(np.array_equal(held[k][0], now[k][0]) and np.array_equal(held[k][1], now[k][1]) for k in keys)
    assert not np.array_equal(held["cp2"][1], before["cp2"][1])
    # a sub-network does not carry it
    sub = ctx.subnetwork({_lib.bucket_slot(_lib.POOL_CP2): np.arange(10, dtype=np.int32)})
    rc, _ = sub.requote(check=False)
    assert rc == _lib.E_STATE
    sub.close()
    # release, and hold again
    ctx.release_route()
    rc, _ = ctx.requote(check=False)
    assert rc == _lib.E_STATE
    ctx.hold_route()
    ctx.requote()
    # an upload into the context's pool store: the positions no longer mean anything
    clone.close()
    b = net["cp2"]
    ctx.upload_pools2(_lib.POOL_CP2, b["Ra"][:50].copy(), b["Rb"][:50].copy(), b["fee"][:50].copy(), b["ia"][:50].copy(), b["ib"][:50].copy())
    rc, _ = ctx.requote(check=False)
    assert rc == _lib.E_STATE
    with pytest.raises(_lib.CfmmError) as e:
        ctx.held2(_lib.POOL_CP2, 50)
    assert e.value.code == _lib.E_STATE
    p.close()
    big = cfmm.Problem.from_network(synthetic.make_network(2600, m_cp2=3000, seed=1), utility=None)
    c2 = big._ensure_ctx()
    c2.set_nu(big.net["c"])
    c2.hold_route()
    rc, _ = c2.requote(check=False)
    assert rc == _lib.E_LIMIT and "2560" in c2.L.cfmm_last_error(c2.h).decode()
    big.close()


def test_hold_and_requote_move_nothing():
    """against a twin context that never held a route: reserves, prices, cached solution, tenders (a table-stableswap bucket included)
    and the evaluations of a following warm solve are bitwise equal"""
    net = synthetic.make_network(200, m_cp2=2000, m_gn=200, m_gk_stable=400, seed=2)
    util = cfmm.Arbitrage(net["c"])
    a = cfmm.Problem.from_network(synthetic.copy_network(net), utility=util, deterministic=True)
    b = cfmm.Problem.from_network(synthetic.copy_network(net), utility=util, deterministic=True)
    for p in (a, b):
        p.solve(tol=1e-6, method="lbfgs", max_evals=300)
    a.ctx.hold_route()
    for _ in range(2):
        rep = a.ctx.requote(want_limbs=True)
    assert rep["pools"] == a.m
    scales_of(a.ctx, net); held_of(a.ctx, net)
    assert np.array_equal(a.ctx.get_nu(), b.ctx.get_nu())
    for x, y in zip(a.ctx.get_solution(), b.ctx.get_solution()):
        assert np.array_equal(x, y)
    ra, rb = reserves_of(a.ctx, net), reserves_of(b.ctx, net)
    ta, tb = trades_of(a.ctx, net), trades_of(b.ctx, net)
    assert any(isinstance(k, tuple) and k[0] == "stable" for k in ta)
    for key in ra:
        assert np.array_equal(ra[key], rb[key]), key
        assert np.array_equal(ta[key][0], tb[key][0]) and np.array_equal(ta[key][1], tb[key][1]), key
    a.ctx.hold_route(); a.ctx.requote()
    sa, sb = a.ctx.solve(None, tol=1e-7, method=_lib.METHODS["lbfgs"], max_evals=300), b.ctx.solve(None, tol=1e-7, method=_lib.METHODS["lbfgs"], max_evals=300)
    assert sa["evals"] == sb["evals"] and sa["status"] == sb["status"], (sa, sb)
    for x, y in zip(a.ctx.get_solution(), b.ctx.get_solution()):
        assert np.array_equal(x, y)
    a.ctx.requote()                                            # the held route outlived the solve
    a.close(); b.close()
