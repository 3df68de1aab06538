"""GPU suite (-m gpu): pools of a solved route selected on the device (include/cfmm.h: cfmm_select_pools, cfmm_get_selected2 / N / G;
csrc/subset.hpp, csrc/subset_rules.hpp; docs/subnetwork.md).

A pool is measured by the value it takes in at the accepted prices, v = sum_j nu_j Delta_j over its legs in slot order with every
product and sum rounded on its own, on exactly the tenders cfmm_get_trades* returns: NumPy on the read-back tenders reproduces v bit
for bit, so the selection at ANY threshold -- a pool's own v included, which the strict comparison leaves out -- is the NumPy one.
The lists come back compacted: ascending upload-order positions, through any permutation of the stored bucket."""
import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib
from cfmm.problem import KIND2, subset_network
from oracle import instances as I

pytestmark = pytest.mark.gpu

copy_net = synthetic.copy_network

# the 11-pool network with one pool of every kind and size (the table of tests/test_terms_host.py)
IDX = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, 1, 2], [1, 2, 3, 4], [2, 3, 4], [0, 2, 4, 5], [1, 5], [0, 5]]
RES = [[10, 20], [30, 40], [5, 6], [7, 8], [9, 11], [1, 2, 3], [4, 5, 6, 7], [8, 9, 10], [11, 12, 13, 14], [3, 4], [6, 7]]
KINDS = ["geomean", "geomean", "sum", "curve", "powersum", "geomean", "geomean", "curve", "sum", "geomean", "geomean"]
WEIGHTS = [None, [0.3, 0.7], None, None, None, None, [1, 2, 3, 4], None, None, None, [0.8, 0.2]]
PARAMS = [None, None, None, 50.0, 0.4, None, None, 20.0, None, None, None]
FEES = [0.997, 0.99, 0.999, 0.9996, 0.995, 0.997, 0.998, 0.9994, 0.9999, 0.9970, 0.98]


# ---------------------------------------------------------------------------------------------------------- helpers
def buckets(net):
    """(key, token ids [k][m]) of every bucket"""
    for key in KIND2:
        if key in net:
            yield key, np.stack([net[key]["ia"], net[key]["ib"]])
    for k, b in net.get("gn", {}).items():
        yield k, b["idx"]
    for key, b in net.get("gk", {}).items():
        yield key, b["idx"]


def slot_of(key):
    if isinstance(key, str):
        return _lib.bucket_slot(KIND2[key])
    return _lib.bucket_slot(("gn", key)) if isinstance(key, int) else _lib.bucket_slot(("table", _lib.POOLK[key[0]], key[1]))


def trades_of(ctx, net):
    out = {}
    for key, idx in buckets(net):
        m = idx.shape[1]
        if isinstance(key, str):
            out[key] = ctx.get_trades2(KIND2[key], m)
        elif isinstance(key, int):
            out[key] = ctx.get_tradesN(key, m)
        else:
            out[key] = ctx.get_tradesG(_lib.POOLK[key[0]], key[1], m)
    return out


def selected_of(ctx, key, cap=None):
    if isinstance(key, str):
        return ctx.get_selected2(KIND2[key], cap)
    return ctx.get_selectedN(key, cap) if isinstance(key, int) else ctx.get_selectedG(_lib.POOLK[key[0]], key[1], cap)


def value_in(nu, idx, delta):
    """v [m] of one bucket: leg by leg in slot order, every product and every sum a rounded float64 operation of its own"""
    v = nu[idx[0]] * delta[0]
    for j in range(1, idx.shape[0]):
        v = v + nu[idx[j]] * delta[j]
    return v


def values_of(ctx, net):
    nu = ctx.get_nu()
    tr = trades_of(ctx, net)
    return {key: value_in(nu, idx, tr[key][0]) for key, idx in buckets(net)}


def check_selection(ctx, net, v, thr, what=""):
    """the device's selection at `thr` against NumPy on v: the lists, the counts per slot and in total, the two sums"""
    info = ctx.select_pools(thr)
    pools = sel = nonfin = 0
    tot = tsel = 0.0
    for key, idx in buckets(net):
        fin = np.isfinite(v[key])
        want = np.flatnonzero(fin & (v[key] > thr)).astype(np.int32)
        got, count = selected_of(ctx, key)
        assert count == len(want), (what, key, thr, count, len(want))
        assert got.dtype == np.int32 and np.array_equal(got, want), (what, key, thr)
        q = slot_of(key)
        assert info["slot_pools"][q] == idx.shape[1] and info["slot_selected"][q] == len(want), (what, key)
        pools += idx.shape[1]; sel += len(want); nonfin += int((~fin).sum())
        tot += float(v[key][fin].sum()); tsel += float(v[key][want].sum())
    assert (info["pools"], info["selected"], info["non_finite"]) == (pools, sel, nonfin), (what, thr, info)
    assert sum(info["slot_pools"]) == pools and sum(info["slot_selected"]) == sel
    print(f"{what} thr={thr!r}: selected {sel} of {pools}; value_in_total {info['value_in_total']!r} (NumPy {tot!r}), "
          f"value_in_selected {info['value_in_selected']!r} (NumPy {tsel!r})")
    assert abs(info["value_in_total"] - tot) <= 1e-12 * abs(tot), (what, thr, info["value_in_total"], tot)
    assert abs(info["value_in_selected"] - tsel) <= 1e-12 * abs(tsel), (what, thr, info["value_in_selected"], tsel)
    return info


def thresholds(v):
    """0, the median of v, one pool's own v exactly (the strict comparison leaves that pool out), above the maximum"""
    allv = np.concatenate([x[np.isfinite(x)] for x in v.values()])
    pos = np.sort(allv[allv > 0])
    own = float(pos[len(pos) // 3]) if len(pos) else 1.0
    return [0.0, float(np.median(allv)), own, float(allv.max()) * 2 + 1.0]


def family_network(fam, m, n, seed):
    if fam == "sum2":
        rng = np.random.default_rng(seed)
        ia = rng.integers(0, n, m).astype(np.int32)
        ib = ((ia + rng.integers(1, n, m)) % n).astype(np.int32)
        Ra = np.exp(rng.normal(3.0, 1.0, m)); Rb = np.exp(rng.normal(3.0, 1.0, m))
        return dict(n_tokens=n, c=np.ones(n), prices=np.ones(n), sum2=dict(Ra=Ra, Rb=Rb, fee=np.full(m, 0.997), ia=ia, ib=ib))
    if isinstance(fam, str):
        return synthetic.make_network(n, seed=seed, **{f"m_{fam}": m})
    kind, k = fam
    if kind == "gn":
        return synthetic.make_network(n, m_gn=m, gn_sizes=(k, k), seed=seed)
    return synthetic.make_network(n, seed=seed, gk_sizes=(k, k), peg=max(4, k), **{f"m_gk_{kind}": m})


def mixed11():
    p = cfmm.Problem(6, IDX, RES, FEES, KINDS, WEIGHTS, PARAMS, utility=cfmm.Arbitrage(np.array([1.0, 1.02, 0.97, 1.05, 0.99, 1.01])))
    return p


# ------------------------------------------------------------------------------------- 1: the selection equals NumPy on the tenders
# every family at the word and workgroup edges of the mask and the scan (m = 1, 63, 64, 65, 257), the two reordered parents of
# tests/test_gpu_apply.py (the lists map through perm), and a bucket of more than one compaction workgroup (20 000 > 16 384 pools)
EDGES = [1, 63, 64, 65, 257]
SHAPES = [(fam, m, 64) for fam in ("cp2", "w2", "sum2", "curve2", "pow2", ("gn", 3), ("gn", 8), ("stable", 3), ("sum", 3)) for m in EDGES]
SHAPES += [("cp2", 20_000, 64), (("gn", 3), 70_000, 1024)]


@pytest.mark.parametrize("fam, m, n", SHAPES, ids=lambda x: str(x))
def test_selection_equals_numpy_on_the_read_back_tenders(fam, m, n):
    rng = np.random.default_rng(23)
    net = family_network(fam, m, n, seed=7)
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    ctx.eval_dual(net["c"])                                   # (uploaded and, where it applies, reordered before the selection)
    ctx.set_nu(net["c"] * np.exp(rng.normal(0.0, 0.1 if "sum" not in str(fam) else 2e-3, n)))
    v = values_of(ctx, net)
    for thr in thresholds(v):
        info = check_selection(ctx, net, v, thr, str((fam, m)))
    assert info["selected"] == 0                              # (above the maximum)
    key = next(iter(v))
    ctx.select_pools(0.0)
    want = np.flatnonzero(v[key] > 0).astype(np.int32)
    got, count = selected_of(ctx, key, cap=min(3, len(want)))       # a short array receives the first positions and the full count
    assert count == len(want) and np.array_equal(got, want[:3])
    p.close()


def test_selection_on_the_mixed_network_with_one_pool_of_every_kind():
    p = mixed11()
    ctx = p._ensure_ctx()
    ctx.set_nu(p.utility.c * np.array([1.03, 0.96, 1.01, 0.99, 1.04, 0.97]))      # (prices off every pool's own: all of them trade)
    v = values_of(ctx, p.net)
    assert set(v) == {"cp2", "w2", "sum2", "curve2", "pow2", 3, 4, ("stable", 3), ("sum", 4)}
    for thr in thresholds(v):
        check_selection(ctx, p.net, v, thr, "mixed11")
    # Problem.select: the same positions, and the selected pools as indices of the lists the Problem was built from
    rep = p.select(0.0)
    want = sorted(i for i, (key, pos) in enumerate(p.where) if v[key][pos] > 0)
    assert rep["pools"].tolist() == want and rep["selected"] == len(want)
    for key in v:
        assert np.array_equal(rep["positions"][key], np.flatnonzero(v[key] > 0))
    # the library's own reading of the selection (lists = NULL): the same pools, kind by kind
    sc = ctx.subnetwork(None)
    assert sc.pool_count() == len(want)
    for key, kind in KIND2.items():
        assert np.array_equal(np.stack(sc.get_reserves2(kind, int((v[key] > 0).sum()))),
                              np.stack(ctx.get_reserves2(kind, len(v[key])))[:, v[key] > 0]), key
    sc.close()
    p.close()


# ------------------------------------------------------------------------------------------- 2: behind a second-order solve
def test_after_a_second_order_solve_every_pool_carries_gross_tenders():
    """the smoothed primal point is interior: every leg of every smoothed pool both receives and pays, so every such pool takes
    something in and threshold 0 selects all of them (K-asset pools enter the second-order solve unsmoothed: they are selected as
    NumPy selects them); the values are those of the gross tenders the read-back hands out, in every family"""
    net = synthetic.make_network(32, seed=3, m_cp2=300, m_w2=65, m_curve2=129, m_gn=65, gn_sizes=(3, 3), m_gk_stable=65, gk_sizes=(3, 3))
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    p.solve(tol=1e-9, method="newton")
    assert p.stats["newton_steps"] > 0
    ctx = p._ensure_ctx()
    v = values_of(ctx, net)
    assert set(v) == {"cp2", "w2", "curve2", 3, ("stable", 3)}       # (the geo-mean and the table bucket: their tenders at the solve's low-order prices and barrier weight)
    info = check_selection(ctx, net, v, 0.0, "newton")
    assert info["pools"] == 300 + 65 + 129 + 65 + 65
    for key, m in (("cp2", 300), ("w2", 65), ("curve2", 129)):        # the smoothed two-asset families: every pool is selected
        assert info["slot_selected"][slot_of(key)] == m, key
    for thr in thresholds(v)[1:]:
        check_selection(ctx, net, v, thr, "newton")
    p.close()


# ------------------------------------------------------------------- 3: the kink loop's tenders (the reference's arbitrage instance)
def test_partly_filled_constant_sum_pool_is_selected_from_the_kink_loops_tenders():
    """arbitrage.py under the default method: the library's own kink loop leaves the constant-sum pool partly filled.  At the solution
    prices the pool sits ON its kink -- its own tenders there are zero or a whole vertex -- so the selection must come from the tenders
    the loop left, which are what cfmm_get_trades2 returns"""
    inst = I.arbitrage()
    p = cfmm.Problem(inst["n_tokens"], inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], inst["weights"],
                     utility=cfmm.Arbitrage(inst["utility"]["c"]))
    p._send_utility()
    ctx = p._ensure_ctx()
    st = ctx.solve(np.asarray(inst["utility"]["c"], dtype=float), tol=1e-9)      # CFMM_METHOD_AUTO: the library's own kink loop
    assert st["status"] == 1 and st["method"] == _lib.METHODS["lbfgs"], st
    rc, _ = ctx.select_pools(0.0, check=False)
    if rc != 0:
        pytest.fail(f"select_pools refused the solved arbitrage instance: {ctx.L.cfmm_last_error(ctx.h).decode()}")
    v = values_of(ctx, p.net)
    d, l = ctx.get_trades2(KIND2["sum2"], len(p.net["sum2"]["Ra"]))
    R = np.stack([p.net["sum2"]["Ra"], p.net["sum2"]["Rb"]])
    part = (l > 1e-9 * R).any(axis=0) & (l < (1 - 1e-9) * R).all(axis=0)
    assert part.any(), "the instance is expected to fill a constant-sum pool partly"
    check_selection(ctx, p.net, v, 0.0, "arbitrage")
    got, _ = selected_of(ctx, "sum2")
    assert set(np.flatnonzero(part)) <= set(got.tolist())
    p.close()


# --------------------------------------------------------------------------------- 4: refusals, and what drops the selection
def test_refusals_and_what_drops_the_selection():
    net = synthetic.make_network(16, seed=11, m_cp2=100)
    net["sum2"] = family_network("sum2", 70, 16, seed=12)["sum2"]
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    ctx.eval_dual(net["c"])
    before = ctx.get_reserves2(KIND2["cp2"], 100)

    def refused(rc_want, call):
        with pytest.raises(_lib.CfmmError) as e:
            call()
        assert e.value.code == rc_want, (e.value.code, str(e.value))

    refused(_lib.E_STATE, lambda: ctx.select_pools(0.0))                     # no prices yet
    refused(_lib.E_STATE, lambda: ctx.get_selected2(KIND2["cp2"]))           # no selection yet
    ctx.set_nu(net["c"] * 1.01)
    refused(_lib.E_ARG, lambda: ctx.select_pools(float("nan")))
    ctx.set_pool_flags(KIND2["sum2"], np.zeros(70, dtype=np.int32))          # caller-held tie flags: the caller holds the fills
    refused(_lib.E_UNSUPPORTED, lambda: ctx.select_pools(0.0))
    ctx.set_pool_flags(KIND2["sum2"], None)
    info = ctx.select_pools(0.0)
    assert info["pools"] == 170
    refused(_lib.E_ARG, lambda: ctx.get_selected2(99))
    refused(_lib.E_ARG, lambda: ctx.get_selectedN(2))
    refused(_lib.E_ARG, lambda: ctx.get_selectedG(0, 9))
    none, count = ctx.get_selectedN(3)                                       # a bucket the network does not have: empty
    assert len(none) == 0 and count == 0
    got, count = ctx.get_selected2(KIND2["cp2"])
    assert count == len(got) > 0
    for a, b in zip(before, ctx.get_reserves2(KIND2["cp2"], 100)):           # nothing of the pools moved
        assert np.array_equal(a, b)
    # every way the tenders go takes the selection with it
    ctx.set_nu(net["c"] * 1.02)
    refused(_lib.E_STATE, lambda: ctx.get_selected2(KIND2["cp2"]))
    ctx.select_pools(0.0)
    ctx.set_utility(net["c"])
    ctx.solve(net["c"], tol=1e-6, method="lbfgs", max_evals=5)               # (a solve moves the point however it ends)
    refused(_lib.E_STATE, lambda: ctx.get_selected2(KIND2["cp2"]))
    ctx.select_pools(0.0)
    ctx.update_pools2(KIND2["cp2"], [0], [before[0][0] * 1.5], [before[1][0]])
    refused(_lib.E_STATE, lambda: ctx.get_selected2(KIND2["cp2"]))
    ctx.set_nu(net["c"])
    ctx.select_pools(0.0)
    c2 = ctx.clone()
    c2.update_pools2(KIND2["cp2"], [1], [before[0][1] * 1.5], [before[1][1]])      # ... through a clone, seen by the generation
    refused(_lib.E_STATE, lambda: ctx.get_selected2(KIND2["cp2"]))
    ctx.set_nu(net["c"])
    assert ctx.select_pools(1e300)["selected"] == 0
    ctx.subnetwork(None).close()                                             # an empty selection is a choice: a context with no pools
    c2.update_pools2(KIND2["cp2"], [1], [before[0][1]], [before[1][1]])
    refused(_lib.E_STATE, lambda: ctx.subnetwork(None))                      # ... but not once it is stale, empty or not
    c2.close()
    p.close()


# =====================================================================================================================================
# the sub-network: cfmm_subnetwork, Problem.subproblem / sparsify
# =====================================================================================================================================
def key_of(fam):
    if isinstance(fam, str):
        return fam
    return fam[1] if fam[0] == "gn" else fam


def bucket_m(net, key):
    return next(idx.shape[1] for k, idx in buckets(net) if k == key)


def reserves_of(ctx, net):
    """{key: (reserves [k][m], parameter column or None)} read back from the device"""
    out = {}
    for key, idx in buckets(net):
        m = idx.shape[1]
        if isinstance(key, str):
            has = key in ("w2", "curve2", "pow2")
            r = ctx.get_reserves2(KIND2[key], m, with_param=has)
            out[key] = (np.stack(r[:2]), r[2] if has else None)
        elif isinstance(key, int):
            out[key] = (ctx.get_reservesN(key, m), None)
        else:
            out[key] = (ctx.get_reservesG(_lib.POOLK[key[0]], key[1], m), None)
    return out


def moved_parent(fam, m, n):
    """a parent whose resident pools have left the host copy behind: reserves and fees updated in place, then (outside the constant-sum
    families, whose pools an apply at these prices would drain) one solve's trades applied"""
    rng = np.random.default_rng(31)
    net = family_network(fam, m, n, seed=9)
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    p._send_utility()
    ctx = p._ensure_ctx()
    ctx.eval_dual(net["c"])                                   # (uploaded and, where it applies, reordered: the parent is permuted)
    key = key_of(fam)
    b = net[key] if isinstance(key, str) else (net["gn"][key] if isinstance(key, int) else net["gk"][key])
    R = np.stack([b["Ra"], b["Rb"]]) if isinstance(key, str) else b["R"]
    pos = np.unique(rng.integers(0, m, max(1, m // 5)))
    p.update_bucket(key, pos, R[:, pos] * np.exp(rng.normal(0.0, 0.05, (R.shape[0], len(pos)))))
    p.update_bucket_terms(key, pos[::2], fee=np.full(len(pos[::2]), 0.9985))
    ctx.set_nu(net["c"] * np.exp(rng.normal(0.0, 0.02 if "sum" not in str(fam) else 1e-4, n)))
    if "sum" not in str(fam):
        p.apply_trades()
    p._refresh_net()                                          # the host copy = get_reserves* of the device (and the terms as updated)
    return p, key


def choices(m):
    """none, all, every third, first and last"""
    return {"none": [], "all": list(range(m)), "third": list(range(0, m, 3)), "ends": sorted({0, m - 1})}


SUB_SHAPES = [(fam, m, 64) for fam in ("cp2", "w2", "sum2", "curve2", "pow2", ("gn", 3), ("stable", 3), ("sum", 3)) for m in EDGES]
SUB_SHAPES += [("cp2", 20_000, 64), (("gn", 3), 70_000, 1024)]


@pytest.mark.parametrize("fam, m, n", SUB_SHAPES, ids=lambda x: str(x))
def test_subnetwork_is_bitwise_a_fresh_upload_of_the_same_pools(fam, m, n):
    """the sub-network of a parent moved on the device against a context uploaded from the parent's read-back reserves and terms of the
    same pools: resident reserves and parameters, tenders at common prices, the reproducible mode's psi and sum arb, and a reproducible
    solve (its evaluations and its prices) are bit for bit the same.
    The choice `all` of the two large shapes is large enough for the token-block ordering, whose stored order is settled by atomics;
    constant-product and geo-mean tenders are functions of the pool alone (pool_math.hpp), so they are bitwise there too.
    The reproducible mode is switched on through the PARENT alone: the sub-network must have carried it over."""
    p, key = moved_parent(fam, m, n)
    c = p.net["c"]
    rng = np.random.default_rng(5)
    nus = [c * np.exp(rng.normal(0.0, 0.05 if "sum" not in str(fam) else 1e-4, n)) for _ in range(2)]
    p.ctx.set_deterministic(True)
    for name, pos in choices(m).items():
        sub = p.subproblem(buckets={key: pos})
        assert sub.ctx.pool_count() == len(pos) == sub.m, (name, sub.ctx.pool_count())
        assert np.array_equal(sub.parent_positions[key], pos)
        if not pos:
            sub.close()
            continue
        fresh = cfmm.Problem.from_network(copy_net(subset_network(p.net, {key: pos})), utility=cfmm.Arbitrage(c))
        a, b = sub._ensure_ctx(), fresh._ensure_ctx()
        ra, rb = reserves_of(a, sub.net), reserves_of(b, fresh.net)
        assert np.array_equal(ra[key][0], rb[key][0]) and np.array_equal(ra[key][0], reserves_of(p.ctx, p.net)[key][0][:, pos]), (name, "reserves")
        assert (ra[key][1] is None) == (rb[key][1] is None) and (ra[key][1] is None or np.array_equal(ra[key][1], rb[key][1])), (name, "param")
        assert np.array_equal(a.get_nu(), p.ctx.get_nu())                      # the accepted prices came along
        b.set_deterministic(True)                                              # (a: carried over from the parent)
        fa, psia = a.eval_dual(nus[0]); fb, psib = b.eval_dual(nus[0])
        assert fa == fb and np.array_equal(psia, psib), (name, "reproducible evaluation", fa, fb)
        a.set_nu(nus[1]); b.set_nu(nus[1])
        ta, tb = trades_of(a, sub.net)[key], trades_of(b, fresh.net)[key]
        for w in (0, 1):
            d = float(np.abs(ta[w] - tb[w]).max())
            print(f"{fam} {m} {name}: tenders[{w}] max |diff| = {d!r}")
            assert np.array_equal(ta[w], tb[w]), (name, "tenders", w, d)
        b.set_utility(c)                                                       # (a carried the parent's)
        sa = a.solve(nus[0], tol=1e-7, method="lbfgs", max_evals=300)
        sb = b.solve(nus[0], tol=1e-7, method="lbfgs", max_evals=300)
        assert sa["evals"] == sb["evals"] and sa["status"] == sb["status"], (name, sa, sb)
        assert np.array_equal(a.get_nu(), b.get_nu()), (name, "solved prices")
        sub.close(); fresh.close()
    p.close()


def test_subnetwork_of_the_mixed_network_keeps_every_kind_in_its_bucket():
    """the 11-pool network, one pool of every kind and size, by pool-list indices: net and where of the subproblem are pack's of the
    sub-list, deltas line up with parent_pools, and a solve of all pools as a sub-network equals the parent's"""
    p = mixed11()
    v_full = p.solve(tol=1e-9, method="newton")
    for pools in ([], list(range(11)), [0, 3, 6, 9], [10, 2, 8, 5]):
        sub = p.subproblem(pools=pools)
        chosen = sorted(pools)
        assert sub.parent_pools.tolist() == chosen and sub.m == len(chosen) == sub.ctx.pool_count()
        want, where = cfmm.problem.pack(6, [IDX[i] for i in chosen], [RES[i] for i in chosen], [FEES[i] for i in chosen],
                                        [KINDS[i] for i in chosen], [WEIGHTS[i] for i in chosen], [PARAMS[i] for i in chosen])
        assert [(k, int(q)) for k, q in sub.where] == [(k, int(q)) for k, q in where]
        got = reserves_of(sub.ctx, sub.net) if chosen else {}
        for key, idx in buckets(want):
            assert np.array_equal(got[key][0], reserves_of(p.ctx, p.net)[key][0][:, sub.parent_positions[key]])
        if len(chosen) == 11:
            v = sub.solve(tol=1e-9, method="newton", warm_start=True)
            assert abs(v - v_full) <= 1e-8 * max(1.0, abs(v_full)), (v, v_full)      # (two solves, each to 1e-9 in gap and infeasibility)
            assert len(sub.deltas) == 11 and all(len(d) == len(IDX[i]) for d, i in zip(sub.deltas, sub.parent_pools))
        sub.close()
    p.close()


# ------------------------------------------------------------------------------------------------------- 5: what it means
def swap_instance(seed=4, n=50, m=2000):
    """2 000 pools over 50 tokens in the reference's vocabulary: constant product, weighted and power-sum pairs, geo-mean pools of 3
    and 4 tokens, reserves worth about the same on both sides of latent prices 3 % off; the utility sells token 0 for token n - 1"""
    rng = np.random.default_rng(seed)
    price = np.exp(rng.normal(0.0, 0.4, n))
    L, R, F, K, W, P = [], [], [], [], [], []
    for i in range(m):
        u = rng.random()
        k = 2 if u < 0.8 else (3 if u < 0.9 else 4)
        toks = rng.choice(n, k, replace=False)
        depth = np.exp(rng.normal(4.0, 1.5))
        L.append(toks.tolist()); R.append((depth / price[toks] * np.exp(rng.normal(0.0, 0.03, k))).tolist())
        F.append(float(rng.choice([0.997, 0.999, 0.9995])))
        if k == 2 and u < 0.1:
            K.append("powersum"); W.append(None); P.append(float(rng.uniform(0.2, 0.8)))
        else:
            K.append("geomean"); P.append(None)
            W.append(None if u < 0.5 else rng.uniform(0.2, 0.8, k).tolist())
    h = np.zeros(n); h[0] = 50.0
    return dict(n=n, L=L, R=R, F=F, K=K, W=W, P=P, utility=cfmm.Swap(h, n - 1))


def value_bound(q, target):
    """|reported value - optimum| of one solve, from its own certificates: see test_sparsify_means_what_it_says"""
    rho = float(q.nu.max() / q.nu[target])
    scale = max(float(np.abs(q.psi).max()), float(np.abs(q.utility.h).max()))
    return q.gap * max(1.0, abs(q.dual_value)) + q.n * rho * q.infeas * scale


def test_sparsify_means_what_it_says():
    """sparsify(0) keeps exactly the pools that trade, so the full optimum is feasible for the sub-network, and the sub-network is a
    restriction of the full one: the two optima are EQUAL, V.  Each solve reports a value v with certificates gap and infeas:
      - weak duality: V <= dual_value, and gap = |dual_value - v| / max(1, |dual_value|), so v >= V - gap max(1, |dual_value|);
      - the reported psi misses psi + h >= 0 by at most infeas x scale per token, scale = max(|psi|, |h|); buying the missing
        amounts of at most n tokens at the solution's prices costs at most n rho infeas scale of the target token, rho = the dearest
        price over the target's: v <= V + n rho infeas scale (to first order in infeas).
    Hence |v - V| <= gap max(1, |dual_value|) + n rho infeas scale =: bound(solve), and |v_sub - v_full| <= bound(sub) + bound(full).
    sparsify(q) with q the 95 % quantile of v keeps about one pool in twenty: a restriction again, so its value is no larger than the
    full one (within the two bounds), and it equals to 1e-9 the value of a Problem built on the host from parent_pools."""
    inst = swap_instance()
    target = inst["n"] - 1
    p = cfmm.Problem(inst["n"], inst["L"], inst["R"], inst["F"], inst["K"], inst["W"], inst["P"], utility=inst["utility"])
    v_full = p.solve(tol=1e-9, max_evals=20000)
    assert p.status == "optimal", (p.status, p.gap, p.infeas)
    v = values_of(p.ctx, p.net)
    vall = np.concatenate(list(v.values()))
    trading = int((vall > 0).sum())
    s0 = p.sparsify(0.0, tol=1e-9, max_evals=20000)
    assert s0.status == "optimal" and s0.m == trading == s0.selection["selected"] and 0 < trading < p.m, (s0.status, s0.m, trading)
    b0 = value_bound(s0, target) + value_bound(p, target)
    print(f"sparsify(0): {s0.m} of {p.m} pools, value {s0.value!r} against {v_full!r}, bound {b0!r}, evals {s0.stats['evals']} (full {p.stats['evals']})")
    assert abs(s0.value - v_full) <= b0, (s0.value, v_full, b0)
    q = float(np.quantile(vall, 0.95))
    s1 = p.sparsify(q, tol=1e-10, max_evals=20000)             # (both sub-solves ten times tighter than the bar they are compared at)
    assert s1.status == "optimal" and s1.m == int((vall > q).sum()) and abs(s1.m - p.m // 20) <= 2, (s1.status, s1.m)
    b1 = value_bound(s1, target) + value_bound(p, target)
    assert s1.value <= v_full + b1, (s1.value, v_full, b1)
    pp = s1.parent_pools.tolist()
    host = cfmm.Problem(inst["n"], [inst["L"][i] for i in pp], [inst["R"][i] for i in pp], [inst["F"][i] for i in pp], [inst["K"][i] for i in pp],
                        [inst["W"][i] for i in pp], [inst["P"][i] for i in pp], utility=inst["utility"])
    v_host = host.solve(tol=1e-10, max_evals=20000)
    print(f"sparsify(q): {s1.m} pools, value {s1.value!r}, host-built {v_host!r}")
    assert host.status == "optimal" and abs(s1.value - v_host) <= 1e-9 * max(1.0, abs(v_host)), (s1.value, v_host)
    for d, i in zip(s1.deltas, pp):
        assert len(d) == len(inst["L"][i])
    for q_ in (s0, s1, host, p):
        q_.close()


# ------------------------------------------------------------------------------- 6: refusals leave everything untouched
def test_subnetwork_refusals_leave_everything_untouched():
    net = synthetic.make_network(16, seed=11, m_cp2=100, m_w2=65)
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    ctx.eval_dual(net["c"])
    before = reserves_of(ctx, net)
    L = ctx.L
    import ctypes as C

    def call(lists):
        """(return code, whether *out stayed NULL) of the raw call"""
        pl, keep = _lib.PoolLists(), []
        for q, pos in lists.items():
            a = np.ascontiguousarray(pos, dtype=np.int32); keep.append(a)
            pl.count[q] = len(a); pl.pos[q] = a.ctypes.data_as(C.POINTER(C.c_int32))
        h = C.c_void_p()
        rc = L.cfmm_subnetwork(ctx.h, C.byref(pl), C.byref(h))
        null = h.value is None
        if not null:
            L.cfmm_destroy(h)
        return rc, null

    cp2, w2 = _lib.bucket_slot(KIND2["cp2"]), _lib.bucket_slot(KIND2["w2"])
    assert call({cp2: [3, 2]}) == (_lib.E_ARG, True)                          # unsorted
    assert call({cp2: [2, 2]}) == (_lib.E_ARG, True)                          # a duplicate
    assert call({cp2: [0, 100]}) == (_lib.E_ARG, True)                        # out of range
    assert call({w2: [-1]}) == (_lib.E_ARG, True)
    assert call({cp2: [1, 2], w2: [5, 4]}) == (_lib.E_ARG, True)              # a good list does not excuse a bad one
    assert call({_lib.bucket_slot(KIND2["curve2"]): [0]}) == (_lib.E_ARG, True)   # a bucket the context does not hold
    h = C.c_void_p()
    assert L.cfmm_subnetwork(ctx.h, None, C.byref(h)) == _lib.E_STATE and h.value is None      # no selection (and no solve)
    with pytest.raises(_lib.CfmmError) as e:
        p.select(0.0)                                                         # no prices yet
    assert e.value.code == _lib.E_STATE
    ctx.set_nu(net["c"] * 1.01)
    ctx.set_ties(np.arange(16) // 2, np.zeros(16))                            # caller-held price ties: no selection is made
    with pytest.raises(_lib.CfmmError) as e:
        ctx.select_pools(0.0)
    assert e.value.code == _lib.E_UNSUPPORTED
    assert L.cfmm_subnetwork(ctx.h, None, C.byref(h)) == _lib.E_STATE and h.value is None
    ctx.set_ties(None)
    # a sharer inside a solve: a clone solves on another thread (the library call releases the interpreter lock) for as long as this
    # thread has not been refused.  A call that falls between two of the clone's solves is served and its context destroyed; the store
    # counts the clone as a reader for the whole of each solve, so the refusal comes within a few calls
    import threading
    clone = ctx.clone()
    clone.set_utility(net["c"])
    stop = threading.Event()

    def sharer():
        while not stop.is_set():
            clone.solve(net["c"] * 1.3, tol=1e-13, method="lbfgs", max_evals=2000)

    t = threading.Thread(target=sharer)
    t.start()
    try:
        seen = []
        for _ in range(5000):
            seen.append(call({cp2: [0, 1], w2: [3]}))
            if seen[-1][0] != 0:
                break
    finally:
        stop.set(); t.join()
    print(f"refused after {len(seen)} calls")
    assert seen[-1] == (_lib.E_STATE, True), seen[-1]
    assert all(x == (0, False) for x in seen[:-1])
    clone.close()
    after = reserves_of(ctx, net)
    for key in before:
        assert np.array_equal(before[key][0], after[key][0])
    p.close()


# ------------------------------------------------------------------------------------------------------------ 7: lifetime
def test_the_subnetwork_outlives_its_parent_and_is_independent_of_it():
    net = synthetic.make_network(32, seed=13, m_cp2=300, m_w2=129, m_gn=65, gn_sizes=(3, 3))
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    p.solve(tol=1e-8, method="lbfgs")
    pos = {"cp2": list(range(0, 300, 2)), "w2": list(range(129)), 3: [0, 64]}
    sub = p.subproblem(buckets=pos)
    twin = p.subproblem(buckets=pos)
    # an update through the parent does not reach the sub-network, nor one through the sub-network the parent
    ra = reserves_of(sub.ctx, sub.net)
    R0 = np.stack([net["cp2"]["Ra"][:1], net["cp2"]["Rb"][:1]])
    p.update_bucket("cp2", [0], R0 * 3.0)
    assert np.array_equal(reserves_of(sub.ctx, sub.net)["cp2"][0], ra["cp2"][0])
    sub.update_bucket("cp2", [1], R0 * 5.0)
    assert np.array_equal(reserves_of(p.ctx, p.net)["cp2"][0][:, 2], np.stack([net["cp2"]["Ra"][2:3], net["cp2"]["Rb"][2:3]])[:, 0])
    assert np.array_equal(reserves_of(twin.ctx, twin.net)["cp2"][0], ra["cp2"][0])
    sub.close()
    # the parent goes; the sub-network is solved, cloned, updated, audited and applied
    p.close()
    v = twin.solve(tol=1e-8, method="lbfgs", warm_start=True)
    assert twin.status == "optimal" and np.isfinite(v)
    c2 = twin.clone()
    assert abs(c2.solve(tol=1e-8, method="lbfgs") - v) <= 1e-7 * max(1.0, abs(v))
    c2.close()
    rep = twin.audit()
    assert rep["pools"] == twin.m == 150 + 129 + 2 and rep["pools_violating"] == 0
    moved = twin.apply_trades()
    assert moved > 0
    twin.update_bucket("w2", [0], np.array([[7.0], [9.0]]))
    assert np.array_equal(reserves_of(twin.ctx, twin.net)["w2"][0][:, 0], [7.0, 9.0])
    v2 = twin.solve(tol=1e-8, method="lbfgs", warm_start=True)
    assert twin.status == "optimal" and np.isfinite(v2)
    twin.close()
