"""GPU suite: the prices the resident pools imply, fitted on the device (cfmm_pool_prices; docs/pool_prices.md), against the exact
50-digit reference of tests/price_ref.py.  The tolerance is derived per instance there; DEVICE_FACTOR is the power of two the device
needed over it when measured against that reference (docs/pool_prices.md records the observed ratios)."""
import numpy as np
import pytest

import cfmm
import price_ref as P
from cfmm import _lib, synthetic
from cfmm.problem import pool_prices
from helpers import random_instance

pytestmark = pytest.mark.gpu

EPS = P.EPS
DEVICE_FACTOR = 1.0


def device_fit(net, anchor=None):
    p = cfmm.Problem.from_network(net)
    try:
        return p.pool_prices(anchor)
    finally:
        p.close()


def check_against(name, ref, prices, info, n, misfit=False):
    tol = DEVICE_FACTOR * ref["tol"]
    err = float(np.abs(info["phi"] - ref["phi"]).max())
    print(f"{name}: |phi - exact| = {err:.3e}, tol {ref['tol']:.3e}, ratio {err / ref['tol'] if ref['tol'] else 0.0:.3f}, iterations {info['iterations']}, "
          f"residual {info['residual']:.2e}, d misfit_max {abs(info['misfit_max'] - ref['misfit_max']):.2e}, d misfit_ss {abs(info['misfit_ss'] - ref['misfit_ss']):.2e}")
    assert info["status"] == 0 and info["iterations"] <= 4 * n + 100 and info["residual"] <= 1e-12
    assert err <= tol
    assert np.array_equal(info["comp"], ref["comp"]) and info["components"] == int(ref["comp"].max()) + 1
    assert info["relations"] == ref["relations"] and info["tokens_unlisted"] == int((ref["deg"] == 0).sum())
    assert np.abs(np.log(prices) - ref["phi"]).max() <= tol + 4 * EPS
    if misfit:
        assert abs(info["misfit_max"] - ref["misfit_max"]) <= 2 * tol
        assert abs(info["misfit_ss"] - ref["misfit_ss"]) <= 4 * tol * ref["misfit_l1"] + ref["relations"] * EPS * ref["misfit_ss"]


# ------------------------------------------------------------------------------------------- 1: every family
@pytest.mark.parametrize("name", ["every_kind", "arbitrage", "liquidation", "two_asset"])
def test_every_family_against_the_exact_reference(name):
    net, ref = P.instance(name), P.reference_of(name)
    prices, info = device_fit(net)
    check_against(name, ref, prices, info, net["n_tokens"], misfit=True)
    if name == "every_kind":
        assert info["relations"] == 17 and info["components"] == 1


# ------------------------------------------------------------------------------------------- 2: chunk and wave edges
EDGES = [(fam, m, n) for fam in ("cp2", "w2", "sum2", "curve2", "pow2") for m in (1, 255, 256, 257, 513) for n in (2, 64, 65)]
EDGES += [("gn8", 257, 64), ("gn8", 257, 65), ("gn3", 513, 65), ("stable3", 257, 65), ("sumk4", 257, 64)]


@pytest.mark.parametrize("family,m,n", EDGES)
def test_chunk_and_wave_edges(family, m, n):
    """single-family buckets at the edges of the 256-pool chunk (a second workgroup, its tail of one pool) over token counts at the
    edges of a wave and of the matrix's 16-byte row words"""
    net = P.single_family(family, m, n)
    ref = P.reference(net)
    prices, info = device_fit(net)
    check_against(f"{family} m={m} n={n}", ref, prices, info, n, misfit=family not in ("sum2", "sumk4"))
    if family in ("sum2", "sumk4"):
        assert info["misfit_max"] == 0.0 and info["misfit_ss"] == 0.0 and np.all(prices == 1.0)


# ------------------------------------------------------------------------------------------- 3: components and anchors
def test_components_and_anchors():
    net, ref = P.instance("three_components"), P.reference_of("three_components")
    anchor = np.zeros(9)
    anchor[0], anchor[2], anchor[8] = 3.7, 11.3, 0.123456789
    prices, info = device_fit(net, anchor)
    tol = DEVICE_FACTOR * ref["tol"]
    assert info["components"] == 4 and info["components_anchored"] == 2 and info["tokens_unlisted"] == 1
    assert list(info["comp"]) == [0, 0, 0, 0, 1, 1, 2, 2, 3]
    assert prices[0] == anchor[0] and prices[2] == anchor[2] and prices[8] == anchor[8]          # bit for bit
    assert np.abs(info["phi"] - ref["phi"]).max() <= tol
    want = P.anchored_prices(ref, anchor)                     # (the offset of component 0 is the mean over its two anchors)
    assert np.abs(np.log(prices) - np.log(want)).max() <= tol + 4 * EPS
    assert np.abs(np.log(prices[4:8]) - ref["phi"][4:8]).max() <= tol + 4 * EPS                  # no anchor: exp(phi)
    free, info0 = device_fit(net)
    assert free[8] == 1.0 and info0["components_anchored"] == 0
    assert np.abs(np.log(free) - ref["phi"]).max() <= tol + 4 * EPS


# ------------------------------------------------------------------------------------------- 4: a hot token, mixed networks, tile edges
@pytest.mark.parametrize("name", ["zipf300", "sparse1000", "sparse2049", "c3_small"])
def test_hot_token_and_mixed_networks(name):
    """zipf300: ~3000 pools of all families, one token with thousands of relations (contended LDS and matrix atomics, the rounding
    term); sparse1000 / sparse2049: ~5000 pools each; 2049 = 2048 + 1 is the implementation's tile edge: one token past a multiple of
    the 1024 threads that own the vectors' entries, of the 64 rows a sweep of the matrix-vector product covers, and of the row word"""
    net, ref = P.instance(name), P.reference_of(name)
    prices, info = device_fit(net)
    check_against(name, ref, prices, info, net["n_tokens"], misfit=True)


# ------------------------------------------------------------------------------------------- 5: worst conditioning
@pytest.mark.parametrize("name", ["chain65", "chain257"])
def test_chains(name):
    net, ref = P.instance(name), P.reference_of(name)
    prices, info = device_fit(net)
    check_against(name, ref, prices, info, net["n_tokens"])
    assert info["components"] == 1 and not info["comp"].any()


# ------------------------------------------------------------------------------------------- 6: follows the device, touches nothing
def net_on_device(p):
    """the Problem's network with the reserves read back from the device"""
    net = synthetic.copy_network(p._net)
    for key, R in p.reserves().items():
        b = net[key] if isinstance(key, str) else (net["gk"][key] if isinstance(key, tuple) else net["gn"][key])
        if isinstance(key, str):
            b["Ra"][:] = R[0]; b["Rb"][:] = R[1]
        else:
            b["R"][:] = R
    return net


def test_follows_updates_and_applied_trades():
    rng = np.random.default_rng(5)
    c = np.exp(rng.normal(0, 0.2, 6))
    p = cfmm.Problem(6, P.IDX, P.RES, P.FEES, P.KINDS, P.WEIGHTS, params=P.PARAMS, utility=cfmm.Arbitrage(c))
    before, _ = p.pool_prices()

    def agrees(what):
        net = net_on_device(p)
        ref = P.reference(net)
        twin_p, twin = pool_prices(net)
        dev_p, dev = p.pool_prices()
        tol = DEVICE_FACTOR * ref["tol"]
        print(f"{what}: |phi_dev - phi_twin| = {np.abs(dev['phi'] - twin['phi']).max():.3e}, tol {ref['tol']:.3e}")
        assert np.abs(dev["phi"] - twin["phi"]).max() <= tol and np.abs(dev["phi"] - ref["phi"]).max() <= tol
        assert np.abs(np.log(dev_p) - np.log(twin_p)).max() <= tol + 4 * EPS
        return dev_p
    p.update_reserves([0, 5, 6, 7, 8], [[13.0, 17.0], [2.0, 2.5, 1.5], [4.5, 5.5, 6.5, 7.5], [8.5, 9.0, 12.0], [11.0, 14.0, 13.0, 12.0]])
    after = agrees("update_reserves")
    assert np.abs(np.log(after) - np.log(before)).max() > 1e-3                  # (the call sees the updated pools)
    p.update_weights([1, 6], [[0.6, 0.4], [4, 3, 2, 1]])
    after2 = agrees("update_weights")
    assert np.abs(np.log(after2) - np.log(after)).max() > 1e-3
    p.close()
    # applied trades (a network without constant-sum pools: the apply then runs on the device), and a call through a clone
    inst = random_instance(7, n_tokens=8, n_pools=40, with_sum=False, with_curve=True, with_power=True)
    p = cfmm.Problem(inst["n_tokens"], inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], inst["weights"],
                     params=inst.get("params"), utility=cfmm.Arbitrage(inst["utility"]["c"]))
    before, _ = p.pool_prices()
    q = p.clone()
    p.solve(tol=1e-8)
    moved = p.apply_trades(sync_host=False)
    assert moved > 0 and p._net.get("_stale")
    via_clone, _ = q.pool_prices()
    assert p._net.get("_stale")                               # (neither call read the reserves back)
    after3 = agrees("apply_trades")
    assert np.abs(np.log(after3) - np.log(before)).max() > 1e-6
    assert np.abs(np.log(via_clone) - np.log(after3)).max() <= 2 * DEVICE_FACTOR * P.reference(net_on_device(p))["tol"] + 4 * EPS
    q.close(); p.close()


def test_nothing_a_later_call_can_see():
    """reproducible mode: solve, pool_prices, solve again from the same start -- bitwise the second solve of a fresh context that never
    made the call; cfmm_get_nu and cfmm_get_trades2 bitwise the same before and after the call"""
    inst = random_instance(11, n_tokens=8, n_pools=40, with_sum=False, with_curve=True, with_power=True)
    u = cfmm.Arbitrage(inst["utility"]["c"])
    start = np.asarray(inst["utility"]["c"], dtype=np.float64) * 1.01

    def run(call):
        p = cfmm.Problem(inst["n_tokens"], inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], inst["weights"],
                         params=inst.get("params"), utility=u, deterministic=True)
        p.solve(tol=1e-8, nu0=start)
        ctx = p.ctx
        m = len(p.net["cp2"]["Ra"])
        nu_b, tr_b = ctx.get_nu(), ctx.get_trades2(_lib.POOL_CP2, m)
        if call:
            prices, info = p.pool_prices()
            assert info["status"] == 0 and np.all(prices > 0)
            nu_a, tr_a = ctx.get_nu(), ctx.get_trades2(_lib.POOL_CP2, m)
            assert np.array_equal(nu_a, nu_b) and np.array_equal(tr_a[0], tr_b[0]) and np.array_equal(tr_a[1], tr_b[1])
        p.solve(tol=1e-8, nu0=start)
        out = (p.nu.copy(), p.psi.copy(), p.stats["evals"], p.status)
        p.close()
        return out
    a, b = run(True), run(False)
    assert a[3] == b[3]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ------------------------------------------------------------------------------------------- 7: refusals
def test_refusals():
    net = P.instance("every_kind")
    p = cfmm.Problem.from_network(net)
    ctx = p._ensure_ctx()
    for bad in (np.nan, -1.0, np.inf):
        a = np.zeros(6); a[3] = bad
        with pytest.raises(cfmm.CfmmError) as e:
            ctx.pool_prices(a)
        assert e.value.code == _lib.E_ARG
    assert ctx.L.cfmm_pool_prices(ctx.h, None, None, None, None, None) == _lib.E_ARG
    prices, info = ctx.pool_prices()                          # (a refusal leaves the context usable)
    assert info["relations"] == 17
    # a context without pools is served: every token its own component
    empty = _lib.Context(5)
    a = np.array([0.0, 2.5, 0.0, 0.0, 7.0])
    pr, inf = empty.pool_prices(a, want_potential=True)
    assert list(pr) == [1.0, 2.5, 1.0, 1.0, 7.0] and inf["components"] == 5 and inf["tokens_unlisted"] == 5 and inf["components_anchored"] == 2
    assert inf["relations"] == 0 and inf["iterations"] == 0 and inf["status"] == 0 and list(inf["comp"]) == [0, 1, 2, 3, 4] and not inf["phi"].any()
    empty.close()
    # pool-sharded: two contexts of this process with attached mailboxes
    ranks = [cfmm.Problem.from_network(cfmm.distributed.rank_network(P.instance("c3_small"), r, 2)) for r in range(2)]
    for q in ranks:
        q._ensure_ctx()
    boxes = [q.ctx.oneshot_mailbox() for q in ranks]
    for r, q in enumerate(ranks):
        q.ctx.oneshot_attach(2, r, boxes)
    with pytest.raises(cfmm.CfmmError) as e:
        ranks[0].ctx.pool_prices()
    assert e.value.code == _lib.E_UNSUPPORTED
    for q in ranks:
        q.close()
    p.close()


# ------------------------------------------------------------------------------------------- 8: the use
def test_liquidation_starts_from_the_pools():
    """a liquidation utility prices one token: solve(nu0="pools") takes its start from the device's fit, ends optimal on the default
    start's value, and after apply_trades(sync_host=False) reads no reserve back (the host network's stale mark survives the solve)"""
    net = synthetic.make_network(50, m_cp2=1200, m_w2=500, m_gn=300, seed=3)
    h = np.zeros(50); h[[3, 7, 20]] = [5.0, 2.0, 1.0]
    u = cfmm.Liquidate(h, 0)
    tol = 1e-6
    a = cfmm.Problem.from_network(synthetic.copy_network(net), utility=u)
    va = a.solve(tol=tol)
    b = cfmm.Problem.from_network(synthetic.copy_network(net), utility=u)
    vb = b.solve(tol=tol, nu0="pools")
    print(f"liquidation: default start {a.stats['evals']} evaluations, nu0='pools' {b.stats['evals']}; values {va:.10g} {vb:.10g}")
    assert a.status == "optimal" and b.status == "optimal"
    assert abs(va - vb) <= 2 * tol * max(1.0, abs(va))
    assert b.apply_trades(sync_host=False) > 0 and b._net.get("_stale")
    vb2 = b.solve(tol=tol, nu0="pools")
    assert b.status == "optimal" and b._net.get("_stale")      # no read-back happened
    a.apply_trades()
    va2 = a.solve(tol=tol)
    print(f"after the apply: default start {a.stats['evals']} evaluations, nu0='pools' {b.stats['evals']}; values {va2:.10g} {vb2:.10g}")
    assert a.status == "optimal" and abs(va2 - vb2) <= 2 * tol * max(1.0, abs(va2))
    with pytest.raises(ValueError):
        b.solve(nu0="pool")
    a.close(); b.close()
