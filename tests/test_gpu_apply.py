"""GPU suite (-m gpu): a solve's trades applied to the resident pools on the device (include/cfmm.h: cfmm_apply_trades,
cfmm_get_reserves2 / N / G; csrc/apply.hpp; docs/apply_trades.md).

The apply commits exactly the tenders cfmm_get_trades* returns at the moment of the call, as (R + g Delta) - Lambda with every
operation rounded on its own: NumPy on the read-back tenders reproduces it.  An applied pool is bitwise the pool a fresh upload of
the new reserves makes; the trading function is preserved (fees aside) or grows (fees to the pool); a refused call -- a drained
constant-sum pool, no prices, caller-held ties, a bad mode -- leaves everything as it was; clones see it; sequential orders see the
pools as the previous order left them."""
import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib
from cfmm.problem import KIND2, post_trade_reserves
from oracle import instances as I

pytestmark = pytest.mark.gpu

MODES = ["pool", "aside"]
copy_net = synthetic.copy_network


# ---------------------------------------------------------------------------------------------------------- helpers
def buckets(net):
    """(key, R [k][m], fee [m]) of every bucket"""
    for key in KIND2:
        if key in net:
            b = net[key]
            yield key, np.stack([b["Ra"], b["Rb"]]), b["fee"]
    for k, b in net.get("gn", {}).items():
        yield k, b["R"], b["fee"]
    for key, b in net.get("gk", {}).items():
        yield key, b["R"], b["fee"]


def min_fee(net):
    return float(min(fee.min() for _, _, fee in buckets(net)))


def trades_of(ctx, net):
    out = {}
    for key, R, _ in buckets(net):
        m = R.shape[1]
        if isinstance(key, str):
            out[key] = ctx.get_trades2(KIND2[key], m)
        elif isinstance(key, int):
            out[key] = ctx.get_tradesN(key, m)
        else:
            out[key] = ctx.get_tradesG(_lib.POOLK[key[0]], key[1], m)
    return out


def reserves_of(ctx, net):
    out = {}
    for key, R, _ in buckets(net):
        m = R.shape[1]
        if isinstance(key, str):
            out[key] = np.stack(ctx.get_reserves2(KIND2[key], m))
        elif isinstance(key, int):
            out[key] = ctx.get_reservesN(key, m)
        else:
            out[key] = ctx.get_reservesG(_lib.POOLK[key[0]], key[1], m)
    return out


def with_reserves(net, res):
    """a copy of the network holding the reserves `res` ({key: [k][m]})"""
    out = copy_net(net)
    for key, R in res.items():
        if isinstance(key, str):
            out[key]["Ra"][:] = R[0]; out[key]["Rb"][:] = R[1]
        else:
            (out["gn"][key] if isinstance(key, int) else out["gk"][key])["R"][:] = R
    return out


def host_expression(net, res, tr, mode):
    return {key: post_trade_reserves(res[key], tr[key][0], tr[key][1], fee, mode) for key, _, fee in buckets(net)}


def assert_matches(got, want, before, what=""):
    """the rule of tests/test_gpu_update.py: bitwise for buckets under 16 384 pools (they keep the caller's order, so the read-back and
    both passes see the same wave neighbours), within 1e-14 R otherwise"""
    for key in want:
        if want[key].shape[1] < 16384:
            assert np.array_equal(got[key], want[key]), (what, key, float(np.abs(got[key] - want[key]).max()))
        else:
            err = np.abs(got[key] - want[key]) / before[key]
            assert np.all(err <= 1e-14), (what, key, float(err.max()))


def sum2_network(n, m, seed):
    rng = np.random.default_rng(seed)
    ia = rng.integers(0, n, m).astype(np.int32)
    ib = ((ia + rng.integers(1, n, m)) % n).astype(np.int32)
    c = np.ones(n)
    Ra = np.exp(rng.normal(3.0, 1.0, m)); Rb = np.exp(rng.normal(3.0, 1.0, m))
    return dict(n_tokens=n, c=c, prices=c, sum2=dict(Ra=Ra, Rb=Rb, fee=np.full(m, 0.997), ia=ia, ib=ib))


def family_network(fam, m, n, seed):
    if fam == "sum2":
        return sum2_network(n, m, seed)
    if isinstance(fam, str):
        return synthetic.make_network(n, seed=seed, **{f"m_{fam}": m})
    kind, k = fam
    if kind == "gn":
        return synthetic.make_network(n, m_gn=m, gn_sizes=(k, k), seed=seed)
    return synthetic.make_network(n, seed=seed, gk_sizes=(k, k), peg=max(4, k), **{f"m_gk_{kind}": m})


def is_constant_sum(fam):
    return fam == "sum2" or (isinstance(fam, tuple) and fam[0] == "sum")


def prices_for(fam, net, rng):
    """c exp(N(0, 0.1)); constant-sum families: inside every pool's fee band (|log nu_a / nu_b| <= 2e-4 < -log 0.9995, the largest fee
    factor the generator draws), so that no pool is traded at its vertex and drained"""
    n = net["n_tokens"]
    if is_constant_sum(fam):
        return np.exp(rng.uniform(-1e-4, 1e-4, n))
    return net["c"] * np.exp(rng.normal(0.0, 0.1, n))


def assert_same_pools(pA, pB, netB, rng, nprices=3):
    """applied context pA against the fresh upload pB (tests/test_gpu_update.py: assert_same_pools): limbs, reproducible-mode psi with
    each context's own exponent, default-mode evaluation, tenders"""
    a, b = pA._ensure_ctx(), pB._ensure_ctx()
    n = netB["n_tokens"]
    ref_r, ref_f = pB._max_reserve(), min_fee(netB)
    nus = [netB["c"] * np.exp(rng.normal(0.0, 0.1, n)) for _ in range(nprices)]
    for nu in nus:
        assert np.array_equal(a.debug_eval_limbs(nu, ref_r, ref_f), b.debug_eval_limbs(nu, ref_r, ref_f))
        fa, psia, da = a.eval_dual(nu, True)
        fb, psib, db = b.eval_dual(nu, True)
        assert abs(fa - fb) <= 1e-12 * max(1.0, abs(fb)), (fa, fb)
        assert np.abs(psia - psib).max() <= 1e-12 * np.abs(psib).max()
        assert np.abs(da - db).max() <= 1e-12 * np.abs(db).max()
    # the reproducible mode with the contexts' OWN exponents: the recorded largest reserve must be a fresh upload's.  Tenders: bitwise
    # where the bucket keeps the caller's order (a permuted bucket holds its pools in an order that differs from upload to upload, and
    # the weighted pools' tender iteration runs to a wave-wide stopping test)
    a.set_deterministic(True); b.set_deterministic(True)
    try:
        assert np.array_equal(a.eval_dual(nus[0])[1], b.eval_dual(nus[0])[1])
        a.set_nu(nus[1]); b.set_nu(nus[1])
        ta, tb = trades_of(a, netB), trades_of(b, netB)
        for key, R, _ in buckets(netB):
            for w in (0, 1):
                if R.shape[1] < 16384:
                    assert np.array_equal(ta[key][w], tb[key][w]), key
                else:
                    assert np.all(np.abs(ta[key][w] - tb[key][w]) <= 1e-14 * R.max(axis=0)), key
    finally:
        a.set_deterministic(False); b.set_deterministic(False)
    a.set_nu(nus[2]); b.set_nu(nus[2])
    ta, tb = trades_of(a, netB), trades_of(b, netB)
    for key, R, _ in buckets(netB):
        for w in (0, 1):
            assert np.all(np.abs(ta[key][w] - tb[key][w]) <= 1e-12 * R.max(axis=0)), key


def apply_ok(ctx, mode):
    rc, info = ctx.apply_trades(mode, check=False)
    assert rc == 0, (rc, info, ctx.L.cfmm_last_error(ctx.h).decode())
    assert info["pools_refused"] == 0 and info["first_pos"] == -1
    return info


# ------------------------------------------------------------------- 1: apply = the host expression on the read-back tenders
# every family below and above its reorder threshold (the shapes of tests/test_gpu_update.py, for its reason), and m = 1, 257 for
# the partial last block
FAMILIES = [
    ("cp2", 1, 64), ("cp2", 257, 64), ("cp2", 2_000, 64), ("cp2", 20_000, 64), ("w2", 2_000, 64), ("w2", 20_000, 64),
    ("sum2", 2_000, 64), ("sum2", 20_000, 64), ("curve2", 2_000, 64), ("curve2", 20_000, 64), ("pow2", 2_000, 64), ("pow2", 20_000, 64),
    (("gn", 3), 2_000, 64), (("gn", 3), 70_000, 1024), (("gn", 4), 2_000, 64), (("gn", 8), 2_000, 64),
    (("stable", 3), 2_000, 64), (("stable", 5), 2_000, 64), (("sum", 3), 2_000, 64),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fam, m, n", FAMILIES, ids=lambda x: str(x))
def test_apply_matches_the_host_expression_on_the_read_back_tenders(fam, m, n, mode, oracle_lib):
    rng = np.random.default_rng(17)
    net = family_network(fam, m, n, seed=5)
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    ctx.eval_dual(net["c"])                                   # (uploaded, reordered and read once before the apply)
    nu = prices_for(fam, net, rng)
    ctx.set_nu(nu)
    before = reserves_of(ctx, net)
    for key, R, _ in buckets(net):                            # the read-back returns the upload, in upload order, through any permutation
        assert np.array_equal(before[key], R), key
    tr = trades_of(ctx, net)
    want = host_expression(net, before, tr, mode)
    info = apply_ok(ctx, mode)
    after = reserves_of(ctx, net)
    assert_matches(after, want, before, (fam, m, mode))
    moved = sum(int(((d != 0) | (l != 0)).any(axis=0).sum()) for d, l in tr.values())
    assert info["pools_moved"] == moved
    assert moved == 0 if is_constant_sum(fam) else (moved > 0 or m == 1)
    assert info["max_reserve"] == max(float(R.max()) for R in after.values())
    # the tenders read back now are those of the NEW reserves at the same prices (the context kept its prices)
    assert np.array_equal(ctx.get_nu(), nu)
    # independent: new reserves formed from the C oracle's tenders at the same prices (tolerance of test_trades_match_oracle_pool_by_pool)
    o = oracle_lib.Oracle(n, threads=4)
    o.add_network(net)
    names = [k for k, _ in o.b2]
    for key, R, fee in buckets(net):
        if isinstance(key, str):
            ya, yb = o.trades2(names.index(key), nu)
            y = np.stack([ya, yb])
            tol = 1e-12 * (R[0] + R[1])
        elif isinstance(key, int):
            y = o.tradesN([k for k, _ in o.bn].index(key), nu)
            tol = 1e-12 * R.max()
        else:
            continue                                          # (the oracle has no K-asset table)
        ref = post_trade_reserves(R, np.maximum(-y, 0.0), np.maximum(y, 0.0), fee, mode)
        err = np.abs(after[key] - ref)
        print(f"oracle {key} m={m} {mode}: max |R' - ref| / tol = {float((err / tol).max()):.3g}")
        assert np.all(err <= tol), (key, float((err / tol).max()))
    p.close()


# ------------------------------------------------------------------------------------------- 2: applied = a fresh upload
MIXED = dict(m_cp2=3000, m_w2=1000, m_curve2=800, m_pow2=600, m_gn=900, gn_sizes=(3, 4), m_gk_stable=400, gk_sizes=(3, 3))


def fresh_upload_case(name):
    if name == "mixed":
        return synthetic.make_network(64, seed=4, **MIXED)
    fam, m, n = name
    return family_network(fam, m, n, seed=5)


@pytest.mark.parametrize("name, mode", [("mixed", "pool"), ("mixed", "aside"), (("cp2", 20_000, 64), "pool"), ((("gn", 3), 70_000, 1024), "aside"),
                                        ((("stable", 5), 2_000, 64), "pool")], ids=lambda x: str(x))
def test_applied_pools_are_a_fresh_upload_bitwise(name, mode):
    rng = np.random.default_rng(23)
    net = fresh_upload_case(name)
    n = net["n_tokens"]
    nu = net["c"] * np.exp(rng.normal(0.0, 0.1, n))
    # the pool holding the network's largest reserve is drawn down: its top leg's token is priced up, so the pool pays it out
    key_top, R_top, _ = max(buckets(net), key=lambda t: t[1].max())
    leg, pos = np.unravel_index(int(np.argmax(R_top)), R_top.shape)
    b = net[key_top] if isinstance(key_top, str) else (net["gn"][key_top] if isinstance(key_top, int) else net["gk"][key_top])
    toks = np.array([b["ia"][pos], b["ib"][pos]]) if isinstance(key_top, str) else b["idx"][:, pos]
    nu[toks] = net["c"][toks]
    nu[toks[leg]] *= 1.5
    pA = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = pA._ensure_ctx()
    ctx.eval_dual(net["c"])
    ctx.set_nu(nu)
    apply_ok(ctx, mode)
    after = reserves_of(ctx, net)
    assert after[key_top][leg, pos] < R_top[leg, pos]                          # (drawn down: the recorded maximum had to be reduced again)
    netB = with_reserves(net, after)
    pB = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(netB["c"]))
    assert_same_pools(pA, pB, netB, rng)
    pA.close(); pB.close()


# ------------------------------------------------------------------------------------------- 3: the trading function
def phi_of(net, key, R):
    if key == "cp2":
        return np.sqrt(R[0] * R[1])
    if key == "w2":
        wa = net["w2"]["wa"]
        return R[0] ** wa * R[1] ** (1.0 - wa)
    if key == "curve2":
        return R[0] + R[1] - net["curve2"]["alpha"] / (R[0] * R[1])
    if key == "pow2":
        t = net["pow2"]["t"]
        return R[0] ** (1.0 - t) + R[1] ** (1.0 - t)
    if isinstance(key, int):
        return np.prod(R ** net["gn"][key]["w"], axis=0)
    assert key[0] == "stable"
    return R.sum(axis=0) - net["gk"][key]["param"] / np.prod(R, axis=0)


@pytest.mark.parametrize("mode", MODES)
def test_trading_function_is_kept_with_fees_aside_and_grows_with_fees_to_the_pool(mode):
    rng = np.random.default_rng(29)
    net = synthetic.make_network(64, seed=8, **MIXED)
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    ctx.set_nu(net["c"] * np.exp(rng.normal(0.0, 0.1, 64)))
    info = apply_ok(ctx, mode)
    assert info["pools_moved"] > 0
    after = reserves_of(ctx, net)
    for key, R, _ in buckets(net):
        rel = phi_of(net, key, after[key]) / phi_of(net, key, R) - 1.0
        print(f"phi {key} {mode}: min {float(rel.min()):.3g} max {float(rel.max()):.3g}")
        if mode == "aside":
            assert np.abs(rel).max() <= 1e-12, (key, float(np.abs(rel).max()))
        else:
            assert rel.min() >= -1e-12, (key, float(rel.min()))
            assert rel.max() > 1e-9, key                        # (the fee stayed in the pool)
    p.close()


# ------------------------------------------------------------------------------------------- 4: sequential orders
def test_sequential_orders_see_the_pools_as_the_previous_order_left_them():
    net = synthetic.make_network(32, m_cp2=1500, m_w2=500, m_gn=300, gn_sizes=(3, 4), seed=6)
    n = net["n_tokens"]
    give = np.zeros(n); give[3] = 50.0 / net["prices"][3] * np.median(net["prices"])
    order = cfmm.Swap(give, 11)
    p = cfmm.Problem.from_network(copy_net(net), utility=order)
    first = p.solve(tol=1e-9)
    assert p.status == "optimal" and first > 0
    assert p.apply_trades() > 0
    second = p.solve(tol=1e-9, warm_start=True)                # the identical order again, warm, over the pools order 1 left
    assert p.status == "optimal"
    netB = with_reserves(net, p.reserves())
    q = cfmm.Problem.from_network(netB, utility=order)
    cold = q.solve(tol=1e-9)
    assert q.status == "optimal"
    assert abs(second - cold) <= 1e-8 * abs(cold), (second, cold)
    assert second < first, (first, second)
    p.close(); q.close()


# ------------------------------------------------------------------------------------------- 5: refusal is atomic
def drained_network():
    """500 constant-product pools over 16 tokens and 300 constant-sum pools: those over tokens 0 .. 7 inside their fee band, pool 137
    alone over tokens (8, 9) with gamma nu_b > nu_a -- traded at its vertex, its leg a paid out whole"""
    n, rng = 16, np.random.default_rng(31)
    net = synthetic.make_network(n, m_cp2=500, seed=12)
    ms = 300
    ia = rng.integers(0, 8, ms).astype(np.int32)
    ib = ((ia + rng.integers(1, 8, ms)) % 8).astype(np.int32)
    ia[137], ib[137] = 8, 9
    net["sum2"] = dict(Ra=np.exp(rng.normal(3.0, 1.0, ms)), Rb=np.exp(rng.normal(3.0, 1.0, ms)), fee=np.full(ms, 0.997), ia=ia, ib=ib)
    nu = net["c"] * np.exp(rng.normal(0.0, 0.05, n))
    nu[:8] = np.exp(rng.uniform(-1e-4, 1e-4, 8))
    nu[9] = 1.2 * nu[8]
    return net, nu


def test_a_drained_pool_refuses_the_whole_call_and_nothing_changes():
    net, nu = drained_network()
    rng = np.random.default_rng(37)
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    pc = p.clone()
    cl = pc._ensure_ctx()
    cl.set_deterministic(True)
    ref = (p._max_reserve(), min_fee(net))
    nus = [net["c"] * np.exp(rng.normal(0.0, 0.1, 16)) for _ in range(3)]
    limbs = [ctx.debug_eval_limbs(x, *ref) for x in nus]
    clone_eval = cl.eval_dual(nus[0])
    ctx.set_nu(nu)
    tr = trades_of(ctx, net)
    assert tr["sum2"][1][0, 137] == net["sum2"]["Ra"][137] or tr["sum2"][1][1, 137] == net["sum2"]["Rb"][137]      # Lambda = R_out
    assert int(((tr["cp2"][0] != 0) | (tr["cp2"][1] != 0)).any(axis=0).sum()) > 0                                  # (the cp2 bucket would have moved)
    before = reserves_of(ctx, net)
    for mode in MODES:
        rc, info = ctx.apply_trades(mode, check=False)
        assert rc == _lib.E_UNSUPPORTED, (rc, info)
        assert info["pools_refused"] == 1
        assert (info["first_family"], info["first_kind"], info["first_k"], info["first_pos"]) == (0, _lib.POOL_SUM2, 2, 137), info
        assert "137" in ctx.L.cfmm_last_error(ctx.h).decode()
    with pytest.raises(cfmm.CfmmError) as e:
        ctx.apply_trades("pool")
    assert e.value.code == _lib.E_UNSUPPORTED
    after = reserves_of(ctx, net)
    for key in before:
        assert np.array_equal(after[key], before[key]), key
    tr2 = trades_of(ctx, net)
    for key in tr:
        assert np.array_equal(tr2[key][0], tr[key][0]) and np.array_equal(tr2[key][1], tr[key][1]), key
    for x, lb in zip(nus, limbs):
        assert np.array_equal(ctx.debug_eval_limbs(x, *ref), lb)
    again = cl.eval_dual(nus[0])
    assert abs(again[0] - clone_eval[0]) <= 1e-12 * abs(clone_eval[0]) and np.array_equal(again[1], clone_eval[1])
    pc.close(); p.close()


def test_a_drained_table_pool_is_named_by_family_kind_size_and_position():
    """the refusal names a bucket beyond the two-asset family: 40 constant-product pools over 16 tokens and 20 three-asset constant-sum
    pools of the K-asset table, those over tokens 0 .. 7 inside their fee band, the one at upload position 7 alone over tokens
    (8, 9, 10) with gamma nu_9 > nu_8 -- its leg in token 9 is paid out whole"""
    n, rng = 16, np.random.default_rng(41)
    net = synthetic.make_network(n, m_cp2=40, seed=12)
    ms, k = 20, 3
    idx = np.stack([rng.choice(8, k, replace=False) for _ in range(ms)]).T.astype(np.int32)
    idx[:, 7] = (8, 9, 10)
    net["gk"] = {("sum", k): dict(idx=np.ascontiguousarray(idx), R=np.exp(rng.normal(3.0, 1.0, (k, ms))), fee=np.full(ms, 0.997), param=np.zeros(ms))}
    nu = net["c"] * np.exp(rng.normal(0.0, 0.05, n))
    nu[:8] = np.exp(rng.uniform(-1e-4, 1e-4, 8))
    nu[9] = 1.2 * nu[8]; nu[10] = 1.0001 * nu[8]
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    ctx.set_nu(nu)
    lam = trades_of(ctx, net)[("sum", k)][1]
    assert lam[1, 7] == net["gk"][("sum", k)]["R"][1, 7], (lam[:, 7], net["gk"][("sum", k)]["R"][:, 7])      # Lambda = R_out
    before = reserves_of(ctx, net)
    for mode in MODES:
        rc, info = ctx.apply_trades(mode, check=False)
        assert rc == _lib.E_UNSUPPORTED, (rc, info)
        assert info["pools_refused"] == 1
        assert (info["first_family"], info["first_kind"], info["first_k"], info["first_pos"]) == (2, _lib.POOLK["sum"], k, 7), info
    after = reserves_of(ctx, net)
    for key in before:
        assert np.array_equal(after[key], before[key]), key
    p.close()


# ------------------------------------------------------------------------------------------- 6: state refusals
def test_state_refusals_leave_the_pools_untouched():
    net, _ = drained_network()
    n = net["n_tokens"]
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    p._send_utility()
    ctx = p._ensure_ctx()
    rc, info = ctx.apply_trades("pool", check=False)                       # no prices yet
    assert rc == _lib.E_STATE and info["pools_moved"] == 0
    before = reserves_of(ctx, net)
    nu = net["c"].copy(); nu[:8] = 1.0; nu[9] = nu[8]                      # every constant-sum pool inside its band
    ctx.set_nu(nu)
    flags = np.zeros(len(net["sum2"]["Ra"]), dtype=np.int32); flags[5] = 1
    ctx.set_pool_flags(_lib.POOL_SUM2, flags)
    assert ctx.apply_trades("pool", check=False)[0] == _lib.E_UNSUPPORTED  # the caller holds a tied pool's fill
    ctx.set_pool_flags(_lib.POOL_SUM2, None)
    ctx.set_ties(np.minimum(np.arange(n), n - 2), np.zeros(n))      # tokens n - 2 and n - 1 tied
    assert ctx.apply_trades("pool", check=False)[0] == _lib.E_UNSUPPORTED
    ctx.set_ties(None, None)
    for bad in (2, -1, 7):
        assert ctx.apply_trades(bad, check=False)[0] == _lib.E_ARG         # no such fee mode
    after = reserves_of(ctx, net)
    for key in before:
        assert np.array_equal(after[key], before[key]), key
    assert apply_ok(ctx, "pool")["pools_moved"] > 0                        # ... and with none of them in the way the call goes through
    p.close()


# ------------------------------------------------------------------------------------------- 7: clones
def test_an_apply_through_a_clone_reaches_every_context():
    """(closed-form and geo-mean families: the K-asset table's stableswap search stops at a residual of 1e-9 of the pool's reserves and
    keeps a warm start that every context of the pool set shares, so two contexts' evaluations of it agree to 1e-12 only on identical
    search histories; what the apply leaves in the table's columns is covered bit for bit by the fresh-upload test above)"""
    rng = np.random.default_rng(9)
    net = synthetic.make_network(64, m_cp2=3000, m_w2=800, m_gn=500, gn_sizes=(3, 4), seed=4)
    pA = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
    nu = net["c"] * np.exp(rng.normal(0.0, 0.1, 64))
    pA.eval_dual(nu)
    cl = pA.clone()
    cl.eval_dual(nu)
    cl._ensure_ctx().set_nu(nu)
    assert apply_ok(cl._ensure_ctx(), "pool")["pools_moved"] > 0
    netB = with_reserves(net, reserves_of(pA._ensure_ctx(), net))
    pB = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(netB["c"]))
    nu2 = net["c"] * np.exp(rng.normal(0.0, 0.1, 64))
    fb, psib = pB.eval_dual(nu2)
    for q in (pA, cl):
        f, psi = q.eval_dual(nu2)
        assert abs(f - fb) <= 1e-12 * max(1.0, abs(fb)) and np.abs(psi - psib).max() <= 1e-12 * np.abs(psib).max()
    cl.close(); pA.close(); pB.close()


# ------------------------------------------------------------------------------------------- 8: after a second-order solve
@pytest.mark.parametrize("mode", MODES)
def test_gross_tenders_of_a_second_order_solve_are_applied(mode):
    net = synthetic.config("C5", scale=0.02)                               # 1 000 constant-product + 10 000 stableswap pools
    n = net["n_tokens"]
    rng = np.random.default_rng(1)                                         # a basket of ten tokens sold for an eleventh
    h = np.zeros(n); idx = rng.choice(n, 10, replace=False)
    h[idx] = np.exp(rng.normal(2, 0.5, 10)) / net["prices"][idx] * 10
    tgt = int(rng.integers(0, n)); h[tgt] = 0
    p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Liquidate(h, tgt))
    p._send_utility()
    ctx = p._ensure_ctx()
    st = ctx.solve(cfmm.start_prices(net, p.utility), method="newton")
    assert st["status"] == 1 and st["method"] == _lib.METHODS["newton"] and st["barrier_mu"] > 0.0, st
    before = reserves_of(ctx, net)
    tr = trades_of(ctx, net)
    d, l = tr["curve2"]
    assert np.any((d > 0) & (l > 0))                                       # gross: a leg both receives and pays
    want = host_expression(net, before, tr, mode)
    assert apply_ok(ctx, mode)["pools_moved"] > 0
    assert_matches(reserves_of(ctx, net), want, before, mode)
    # the barrier weight went with the old reserves: the tenders read back now are the exact ones of the new pools at the same prices
    d2, l2 = ctx.get_trades2(_lib.POOL_CURVE2, d.shape[1])
    assert np.all(d2 * l2 == 0)
    p.close()


# ------------------------------------------------------------------------------------------- 9: the reference's instance, AUTO
def test_reference_arbitrage_instance_with_its_partly_filled_pool():
    inst = I.arbitrage()
    q = cfmm.Problem(inst["n_tokens"], inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], inst["weights"],
                     utility=cfmm.Arbitrage(inst["utility"]["c"]))
    net = q.net
    q._send_utility()
    ctx = q._ensure_ctx()
    st = ctx.solve(np.asarray(inst["utility"]["c"], dtype=float), tol=1e-9)          # CFMM_METHOD_AUTO: the library's own kink loop
    assert st["status"] == 1 and st["method"] == _lib.METHODS["lbfgs"]
    before = reserves_of(ctx, net)
    tr = trades_of(ctx, net)
    d, l = tr["sum2"]
    key, pos = q.where[4]
    assert key == "sum2"
    out = int(np.argmax(l[:, pos]))
    fill = l[out, pos] / before["sum2"][out, pos]
    assert 0.3 < fill < 0.5, fill                                                    # pool 4: filled 38.6 %, not drained
    want = host_expression(net, before, tr, "pool")
    info = apply_ok(ctx, "pool")
    after = reserves_of(ctx, net)
    for k in want:
        assert np.array_equal(after[k], want[k]), k
    assert after["sum2"][out, pos] > 0.0 and after["sum2"][out, pos] == before["sum2"][out, pos] - l[out, pos]
    assert info["pools_moved"] == sum(int(((d != 0) | (l != 0)).any(axis=0).sum()) for d, l in tr.values()) >= 2
    q.close()


# ------------------------------------------------------------------------------------------- 10: Python
def test_problem_apply_trades_on_the_device_path():
    net = synthetic.make_network(32, m_cp2=1500, m_w2=500, m_gn=300, gn_sizes=(3, 4), seed=6)
    for sync_host in (True, False):
        p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
        p.solve(tol=1e-9)
        assert p.status == "optimal" and p._apply_path() == "device"
        tr = {k: (d.copy(), l.copy()) for k, (d, l) in p._trades().items()}
        want = host_expression(net, {k: R for k, R, _ in buckets(net)}, tr, "pool")
        moved = p.apply_trades(sync_host=sync_host)
        assert moved == sum(int(((d != 0) | (l != 0)).any(axis=0).sum()) for d, l in tr.values()) > 0
        assert bool(p._net.get("_stale")) == (not sync_host)
        res = p.reserves()
        for key, R, _ in buckets(p.net):                                           # (p.net: refreshed on first use where it was left stale)
            assert np.array_equal(R, res[key]) and np.array_equal(R, want[key]), key
        assert not p._net.get("_stale")
        # the applied pools hold no arbitrage any more: the next solve is an order, warm from the arbitrage prices, against a fresh Problem
        give = np.zeros(32); give[3] = 50.0 / net["prices"][3] * np.median(net["prices"])
        nxt = cfmm.Swap(give, 11)
        p.set_utility(nxt)
        warm = p.solve(tol=1e-9, warm_start=True)
        q = cfmm.Problem.from_network(with_reserves(net, res), utility=nxt)
        cold = q.solve(tol=1e-9)
        assert p.status == "optimal" and q.status == "optimal" and cold > 0
        assert abs(warm - cold) <= 1e-8 * abs(cold), (warm, cold)
        p.close(); q.close()


def kinked_network(seed=14, depth=1e5, order=1e3):
    """600 constant-product and 60 stableswap pools over 24 tokens in peg groups of four, and one deep constant-sum pool inside each of
    the first three peg groups; the order sells token 0 for token 5.  A constant-sum pool quotes one flat price, so the optimum
    fills it until the routes around it quote the same -- partly (arbitrage.py's pool 4 at size): the Python active-set loop ties
    such a pool's two prices and holds its fill (Problem._theta)"""
    net = synthetic.make_network(24, m_cp2=600, m_curve2=60, seed=seed)
    ia = np.array([0, 4, 8], dtype=np.int32); ib = np.array([1, 5, 9], dtype=np.int32)
    net["sum2"] = dict(Ra=depth / net["prices"][ia], Rb=depth / net["prices"][ib], fee=np.full(3, 0.9995), ia=ia, ib=ib)
    give = np.zeros(24); give[0] = order / net["prices"][0]
    return net, cfmm.Swap(give, 5)


def test_problem_apply_trades_on_the_host_path_with_fills():
    # the reference's own instance: pool 4 ends on its kink, its fill held by the Python loop
    inst = I.arbitrage()
    for fees in MODES:
        p = cfmm.Problem(inst["n_tokens"], inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], inst["weights"],
                         utility=cfmm.Arbitrage(inst["utility"]["c"]))
        p.solve(tol=1e-9, method="lbfgs")
        assert p.status == "optimal" and len(p._theta) == 1 and p._apply_path() == "host"
        d, l = p.deltas, p.lambdas
        want = [post_trade_reserves(np.asarray(inst["reserves"][i], dtype=float), d[i], l[i], inst["fees"][i], fees) for i in range(5)]
        assert 0.0 < l[4].max() < max(inst["reserves"][4])
        assert p.apply_trades(fees=fees) >= 2
        res = p.reserves()
        for i, (key, pos) in enumerate(p.where):
            assert np.array_equal(res[key][:, pos], want[i]), i
            b = p.net[key] if isinstance(key, str) else p.net["gn"][key]
            host = np.array([b["Ra"][pos], b["Rb"][pos]]) if isinstance(key, str) else b["R"][:, pos]
            assert np.array_equal(host, want[i]), i
        p.close()
    # a mid-size network whose kinks the Python loop settles
    net, order = kinked_network()
    p = cfmm.Problem.from_network(copy_net(net), utility=order, deterministic=True)
    p.solve(tol=1e-8, method="lbfgs")
    assert p.status == "optimal" and len(p._theta) > 0 and p._apply_path() == "host", (p.status, len(p._theta))
    tr = {k: (d.copy(), l.copy()) for k, (d, l) in p._trades().items()}
    want = host_expression(net, {k: R for k, R, _ in buckets(net)}, tr, "pool")
    assert np.all(want["sum2"] > 0)
    assert p.apply_trades() > 0
    res = p.reserves()
    for key, R, _ in buckets(p.net):
        assert np.array_equal(res[key], want[key]) and np.array_equal(R, want[key]), key
    p.close()


def test_problem_apply_trades_raises_on_a_drained_pool_and_changes_nothing():
    net, nu = drained_network()
    for host_path in (False, True):
        p = cfmm.Problem.from_network(copy_net(net), utility=cfmm.Arbitrage(net["c"]))
        p._ensure_ctx().set_nu(nu)
        p._dev_ties = host_path                                # (the host path forms the same reserves from the read-back tenders)
        with pytest.raises(ValueError) as e:
            p.apply_trades()
        assert "137" in str(e.value)
        res = p.reserves()
        for key, R, _ in buckets(net):
            assert np.array_equal(res[key], R) and np.array_equal(np.stack([p.net[key]["Ra"], p.net[key]["Rb"]]), R), key
        assert not p._net.get("_stale") and p._net.get("_generation", 0) == 0
        p._dev_ties = False
        p.close()
