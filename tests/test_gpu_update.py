"""GPU suite (-m gpu): in-place updates of resident reserves (include/cfmm.h: cfmm_update_pools2 / N / G; csrc/update.hpp).

An update must leave the pools exactly as a fresh upload of the new reserves would have made them: the reproducible mode's raw
limbs agree bit for bit, the default mode's evaluation (which reads the precomputed log(R / w) column) and the tenders agree to
rounding, and a solve after an update is the fresh solve.  A warm re-solve from the previous block's prices reaches the cold solve's
optimum; clones see an update made through any of them; a refused update leaves nothing half-applied; pool-sharded ranks update
their own slices and stay in step."""
import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib
from cfmm.problem import KIND2, PARAM2
from oracle import instances as I

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- helpers
copy_net = synthetic.copy_network


def buckets(net):
    """(key, R [k][m] view or 2 x m copy, param column or None) of every bucket"""
    for key in KIND2:
        if key in net:
            b = net[key]
            yield key, np.stack([b["Ra"], b["Rb"]]), (b[PARAM2[key]] if PARAM2[key] and key != "w2" else None)
    for k, b in net.get("gn", {}).items():
        yield k, b["R"], None
    for key, b in net.get("gk", {}).items():
        yield key, b["R"], (b["param"] if key[0] == "stable" else None)


def apply(net, key, pos, R, param):
    if isinstance(key, str):
        net[key]["Ra"][pos] = R[0]; net[key]["Rb"][pos] = R[1]
        if param is not None:
            net[key][PARAM2[key]][pos] = param
    else:
        b = net["gn"][key] if isinstance(key, int) else net["gk"][key]
        b["R"][:, pos] = R
        if param is not None:
            b["param"][pos] = param


def perturb(net, frac, rng, params=True):
    """new reserves (and alpha / t) for a random `frac` of every bucket's pools, the pool holding the bucket's largest reserve among
    them and lowered (the path that reduces the bucket again); returns (network B, {key: (pos, R, param)})"""
    netB = copy_net(net)
    changes = {}
    for key, R, prm in buckets(net):
        m = R.shape[1]
        top = int(np.argmax(R.max(axis=0)))
        pos = np.unique(np.concatenate([rng.choice(m, max(1, int(frac * m)), replace=False), [top]]))
        newR = R[:, pos] * np.exp(rng.normal(0.0, 0.3, (R.shape[0], len(pos))))
        newR[:, pos == top] = R[:, [top]] * 0.5
        newp = None
        if params and prm is not None:
            newp = rng.uniform(0.1, 0.9, len(pos)) if key == "pow2" else prm[pos] * np.exp(rng.normal(0.0, 0.2, len(pos)))
        changes[key] = (pos, newR, newp)
        apply(netB, key, pos, newR, newp)
    return netB, changes


def sum2_network(n, m, seed):
    rng = np.random.default_rng(seed)
    ia = rng.integers(0, n, m).astype(np.int32)
    ib = ((ia + rng.integers(1, n, m)) % n).astype(np.int32)
    c = np.exp(rng.normal(0.0, 0.3, n))
    Ra = np.exp(rng.normal(3.0, 1.0, m)); Rb = np.exp(rng.normal(3.0, 1.0, m))
    return dict(n_tokens=n, c=c, prices=c, sum2=dict(Ra=Ra, Rb=Rb, fee=np.full(m, 0.997), ia=ia, ib=ib))


def min_fee(net):
    f = [net[k]["fee"].min() for k in KIND2 if k in net]
    f += [b["fee"].min() for b in list(net.get("gn", {}).values()) + list(net.get("gk", {}).values())]
    return float(min(f))


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


def assert_same_pools(pA, pB, netB, rng, nprices=3):
    """updated context pA against the fresh upload pB: limbs, reproducible-mode psi, default-mode evaluation, tenders"""
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
    # where the bucket keeps the caller's order; a bucket the token-block ordering permuted holds its pools in an order that differs from
    # upload to upload (reorder.hpp: the order inside a key is the reservations'), and the weighted pools' tender iteration runs to a
    # wave-wide stopping test -- the last bits then depend on a pool's wave neighbours, on two fresh uploads as much as here
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


def update_problem(p, changes):
    for key, (pos, R, prm) in changes.items():
        p.update_bucket(key, pos, R, prm)


# ------------------------------------------------------------------------------------------- 1, 2: every bucket family
# (family, size below / above its reorder threshold).  A geo-mean bucket is reordered only where its stray legs leave the
# workgroups' psi tiles sparse (cfmm_hip.hip: pools_ready): above the threshold the network needs enough tokens for that.
FAMILIES = [
    ("cp2", 2_000, 64), ("cp2", 20_000, 64), ("w2", 2_000, 64), ("w2", 20_000, 64),
    ("curve2", 2_000, 64), ("curve2", 20_000, 64), ("pow2", 2_000, 64), ("pow2", 20_000, 64),
    ("sum2", 3_000, 64),
    (("gn", 3), 2_000, 64), (("gn", 3), 70_000, 1024), (("gn", 4), 2_000, 64), (("gn", 4), 70_000, 1600), (("gn", 8), 2_000, 64),
    (("stable", 3), 2_000, 64), (("stable", 5), 2_000, 64), (("sum", 3), 2_000, 64), (("sum", 4), 2_000, 64),
]


def family_network(fam, m, n, seed):
    if fam == "sum2":
        return sum2_network(n, m, seed)
    if isinstance(fam, str):
        return synthetic.make_network(n, seed=seed, **{f"m_{fam}": m})
    kind, k = fam
    if kind == "gn":
        return synthetic.make_network(n, m_gn=m, gn_sizes=(k, k), seed=seed)
    return synthetic.make_network(n, seed=seed, gk_sizes=(k, k), peg=max(4, k), **{f"m_gk_{kind}": m})


@pytest.mark.parametrize("fam, m, n", FAMILIES, ids=lambda x: str(x))
def test_update_is_a_fresh_upload_bitwise(fam, m, n):
    rng = np.random.default_rng(11)
    netA = family_network(fam, m, n, seed=5)
    netB, changes = perturb(netA, 0.05, rng)
    pA = cfmm.Problem.from_network(copy_net(netA), utility=cfmm.Arbitrage(netA["c"]))
    pA.eval_dual(netA["c"])                                       # (uploaded, reordered and read once before the update)
    update_problem(pA, changes)
    pB = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(netB["c"]))
    assert_same_pools(pA, pB, netB, rng)
    pA.close(); pB.close()


# ------------------------------------------------------------------------------------------- 3: a solve after an update
def test_solve_after_update_is_the_fresh_solve():
    rng = np.random.default_rng(3)
    netA = synthetic.config("C3", scale=0.1, seed=2)
    netB, changes = perturb(netA, 0.01, rng, params=False)
    nu0 = netA["c"] * np.exp(rng.normal(0.0, 0.02, netA["n_tokens"]))
    pB = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(netB["c"]), deterministic=True)
    pB.solve(nu0=nu0, method="lbfgs")
    for before in (1, 2):
        pA = cfmm.Problem.from_network(copy_net(netA), utility=cfmm.Arbitrage(netA["c"]), deterministic=True)
        for _ in range(before):
            pA.solve(method="lbfgs")
        update_problem(pA, changes)
        pA.solve(nu0=nu0, method="lbfgs")
        assert np.array_equal(pA.nu, pB.nu), before
        assert pA.stats["evals"] == pB.stats["evals"] and pA.value == pB.value, (before, pA.stats["evals"], pB.stats["evals"])
        pA.close()
    pB.close()


# ------------------------------------------------------------------------------------------- 4: warm re-solve at C3
def test_warm_resolve_after_a_block_at_c3():
    """a block of swaps (cfmm.synthetic.swap_block: 1 % of the pools trade along their own trading functions), then a warm re-solve"""
    netA = synthetic.config("C3", seed=0)
    pA = cfmm.Problem.from_network(copy_net(netA), utility=cfmm.Arbitrage(netA["c"]))
    pA.solve(tol=1e-9)
    assert pA.status == "optimal"
    netB, changes = synthetic.swap_block(netA, 0.01, seed=7)
    for key, (pos, R) in changes.items():
        pA.update_bucket(key, pos, R)
    warm = pA.solve(tol=1e-9, warm_start=True)
    ev_warm = pA.stats["evals"]
    pB = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(netB["c"]))
    cold = pB.solve(tol=1e-9)
    ev_cold = pB.stats["evals"]
    msg = f"warm {ev_warm} evaluations, cold {ev_cold}; values {warm!r} / {cold!r}"
    assert pA.status == "optimal" and pB.status == "optimal", msg
    assert pA.gap <= 1e-6 and pA.infeas <= 1e-6, msg
    assert abs(warm - cold) <= 1e-8 * abs(cold), msg
    # (measured on the MI355X: the warm start does NOT save evaluations here -- 66 against 55 at this seed, 36 against 32 at tol 1e-6;
    #  see docs/reserve_updates.md.  Held to a bound so that a regression of the warm path shows)
    assert ev_warm <= 2 * ev_cold, msg
    pA.close(); pB.close()


# ------------------------------------------------------------------------------------------- 5: second-order path
def test_newton_after_updating_curve_pools():
    rng = np.random.default_rng(5)
    netA = synthetic.config("C5", scale=0.05, seed=1)
    b = netA["curve2"]
    m = len(b["Ra"])
    pos = np.sort(rng.choice(m, max(1, int(0.02 * m)), replace=False))
    R = np.stack([b["Ra"][pos], b["Rb"][pos]]) * np.exp(rng.normal(0.0, 0.05, (2, len(pos))))
    al = b["alpha"][pos] * np.exp(rng.normal(0.0, 0.05, len(pos)))
    netB = copy_net(netA)
    apply(netB, "curve2", pos, R, al)
    pA = cfmm.Problem.from_network(copy_net(netA), utility=cfmm.Arbitrage(netA["c"]))
    pA.solve(method="newton")
    pA.update_bucket("curve2", pos, R, al)
    vA = pA.solve(tol=1e-9, method="newton")          # (solved well inside the 1e-7 the two are compared to)
    pB = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(netB["c"]))
    vB = pB.solve(tol=1e-9, method="newton")
    assert pA.status == "optimal" and pB.status == "optimal"
    assert abs(vA - vB) <= 1e-7 * abs(vB), (vA, vB)
    assert np.abs(pA.psi - pB.psi).max() <= 1e-7 * np.abs(pB.psi).max()
    pA.close(); pB.close()


# ------------------------------------------------------------------------------------------- 6: the reference's instance
def arbitrage_problem(reserves):
    inst = I.arbitrage()
    return cfmm.Problem(inst["n_tokens"], inst["local_indices"], reserves, inst["fees"], inst["kinds"], inst["weights"],
                        utility=cfmm.Arbitrage(inst["utility"]["c"]))


def test_reference_instance_after_updating_two_pools():
    inst = I.arbitrage()
    res0 = [list(map(float, r)) for r in inst["reserves"]]
    new = [list(r) for r in res0]
    new[4] = [res0[4][0] * 0.8, res0[4][1] * 1.3]                 # the constant-sum pool
    new[1] = [res0[1][0] * 1.2, res0[1][1] * 0.9]
    pA = arbitrage_problem(res0)
    pA.solve(tol=1e-9)
    pA.update_reserves([4, 1], [new[4], new[1]])
    vA = pA.solve(tol=1e-9)
    pB = arbitrage_problem(new)
    vB = pB.solve(tol=1e-9)
    assert pA.status == "optimal" and pB.status == "optimal"
    assert abs(vA - vB) <= 1e-10 * abs(vB), (vA, vB)
    assert np.abs(pA.psi - pB.psi).max() <= 1e-10 * np.abs(pB.psi).max()
    for i in range(5):
        tol = 1e-9 * np.asarray(new[i])
        assert np.all(np.abs(pA.deltas[i] - pB.deltas[i]) <= tol) and np.all(np.abs(pA.lambdas[i] - pB.lambdas[i]) <= tol), i
    pA.close(); pB.close()
    # raw C-ABI: an AUTO solve (its kink loop leaves tenders behind), an update, the tenders WITHOUT a re-solve
    qA = arbitrage_problem(res0)
    qA._send_utility()
    ctx = qA._ensure_ctx()
    st = ctx.solve(np.asarray(I.arbitrage()["utility"]["c"], dtype=float), tol=1e-9)     # CFMM_METHOD_AUTO: the library's own kink loop
    assert st["status"] == 1
    ctx.update_pools2(_lib.POOL_SUM2, [0], [new[4][0]], [new[4][1]])
    ctx.update_pools2(_lib.POOL_CP2, [0], [new[1][0]], [new[1][1]])
    nu = ctx.get_nu()
    qB = arbitrage_problem(new)
    fresh = qB._ensure_ctx()
    fresh.set_nu(nu)
    for kind, m in ((_lib.POOL_SUM2, 1), (_lib.POOL_CP2, 3)):
        da, la = ctx.get_trades2(kind, m)
        db, lb = fresh.get_trades2(kind, m)
        assert np.array_equal(da, db) and np.array_equal(la, lb), kind
    qA.close(); qB.close()


# ------------------------------------------------------------------------------------------- 7: clones
def test_an_update_through_a_clone_reaches_every_context():
    rng = np.random.default_rng(9)
    netA = synthetic.make_network(64, m_cp2=3000, m_gn=500, gn_sizes=(3, 4), m_gk_stable=300, seed=4)
    netB, changes = perturb(netA, 0.05, rng)
    pA = cfmm.Problem.from_network(copy_net(netA), utility=cfmm.Arbitrage(netA["c"]))
    nu = netA["c"] * np.exp(rng.normal(0.0, 0.1, 64))
    pA.eval_dual(nu)
    cl = pA.clone()
    cl.eval_dual(nu)
    update_problem(cl, changes)
    pB = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(netB["c"]))
    fb, psib = pB.eval_dual(nu)
    for p in (pA, cl):
        f, psi = p.eval_dual(nu)
        assert abs(f - fb) <= 1e-12 * max(1.0, abs(fb)) and np.abs(psi - psib).max() <= 1e-12 * np.abs(psib).max()
    cl.close(); pA.close(); pB.close()


def test_batched_solves_after_an_update():
    rng = np.random.default_rng(13)
    netA = synthetic.config("C3", scale=0.05, seed=3)
    netB, changes = perturb(netA, 0.01, rng, params=False)
    n = netA["n_tokens"]
    utils = [cfmm.Arbitrage(netA["c"] * np.exp(rng.normal(0.0, 0.01, n))) for _ in range(4)]
    pA = cfmm.Problem.from_network(copy_net(netA), utility=utils[0])
    pA.solve_many(utils, batch=4, tol=1e-9)
    update_problem(pA, changes)
    ra = pA.solve_many(utils, batch=4, tol=1e-9)
    pB = cfmm.Problem.from_network(netB, utility=utils[0])
    rb = pB.solve_many(utils, batch=4, tol=1e-9)
    for x, y in zip(ra, rb):
        assert x["status"] == "optimal" and y["status"] == "optimal"
        assert abs(x["value"] - y["value"]) <= 1e-8 * abs(y["value"]), (x["value"], y["value"])
    pA.close(); pB.close()


# ------------------------------------------------------------------------------------------- 8: refusals
def test_refused_updates_leave_the_pools_as_they_were():
    rng = np.random.default_rng(21)
    net = synthetic.make_network(64, m_cp2=500, m_curve2=300, m_pow2=200, m_gn=200, gn_sizes=(3, 3), m_gk_stable=100, gk_sizes=(3, 3), seed=6)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    nu = net["c"] * np.exp(rng.normal(0.0, 0.1, 64))
    ref = (p._max_reserve(), min_fee(net))
    before = ctx.debug_eval_limbs(nu, *ref)
    m2, mc, mn, mg = len(net["cp2"]["Ra"]), len(net["curve2"]["Ra"]), net["gn"][3]["R"].shape[1], net["gk"][("stable", 3)]["R"].shape[1]
    one, ones3 = np.array([1.0]), np.ones((3, 1))
    cases = [
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CP2, [m2], one, one)),                 # position out of range
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CP2, [-1], one, one)),
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CP2, [3, 3], [1.0, 2.0], [1.0, 2.0])),  # duplicate
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CP2, [1, 2], [1.0, 0.0], [1.0, 1.0])),  # reserve 0 (behind a good entry)
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CP2, [1], [-1.0], one)),
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CP2, [1], one, [np.nan])),
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CURVE2, [0, 1], [1.0, 1.0], [1.0, 1.0], [5.0, -1.0])),   # bad alpha
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_POW2, [0], one, one, [1.5])),          # bad t
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_CP2, [0], one, one, [0.5])),           # no parameter to take
        (_lib.E_ARG, lambda: ctx.update_pools2(_lib.POOL_W2, [0], one, one, [0.5])),            # weights are not updated
        (_lib.E_ARG, lambda: ctx.update_poolsN([0], np.ones((9, 1)))),                          # wrong k
        (_lib.E_STATE, lambda: ctx.update_poolsN([0], np.ones((5, 1)))),                        # empty bucket
        (_lib.E_ARG, lambda: ctx.update_poolsN([mn], ones3)),
        (_lib.E_ARG, lambda: ctx.update_poolsN([0], np.array([[1.0], [np.inf], [1.0]]))),
        (_lib.E_ARG, lambda: ctx.update_poolsG(_lib.POOLK["stable"], [0], ones3, [0.0])),       # bad alpha
        (_lib.E_ARG, lambda: ctx.update_poolsG(_lib.POOLK["stable"], [mg, 0], np.ones((3, 2)))),
        (_lib.E_STATE, lambda: ctx.update_pools2(_lib.POOL_SUM2, [0], one, one)),               # empty bucket
        (_lib.E_STATE, lambda: ctx.update_poolsG(_lib.POOLK["sum"], [0], ones3)),
    ]
    for i, (code, call) in enumerate(cases):
        with pytest.raises(cfmm.CfmmError) as e:
            call()
        assert e.value.code == code and "error" in str(e.value) and len(str(e.value).split(":", 1)[1].strip()) > 0, (i, str(e.value))
        assert np.array_equal(ctx.debug_eval_limbs(nu, *ref), before), i
    ctx.update_pools2(_lib.POOL_CP2, [], np.zeros(0), np.zeros(0))          # count == 0: legal, changes nothing
    assert np.array_equal(ctx.debug_eval_limbs(nu, *ref), before)
    p.close()


# ------------------------------------------------------------------------------------------- 9: pool-sharded
def test_pool_sharded_update_matches_the_unsharded_solve(tmp_path, world=2):
    """two processes share GPU 0 (tests/dist_update_worker.py); rank 0 updates its slices, rank 1 calls with count = 0, and one update
    raises the network's largest reserve on rank 0 only.  The reproducible-mode solve that follows must hold the same bits on both
    ranks and be bit for bit the unsharded fresh solve of the new network: the global maxima were re-reduced in step"""
    import json, os, socket, subprocess, sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "update_sharded.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(here, "dist_update_worker.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(out))
    ranks, ref = doc["ranks"], doc["unsharded"]
    assert doc["world"] == world and ref["status"] == "optimal"
    assert sum(ranks[0]["counts"].values()) > 0 and sum(ranks[1]["counts"].values()) == 0
    for q in ranks:
        assert q["status"] == "optimal"
        assert q["nu"] == ref["nu"] and q["evals"] == ref["evals"] and q["value"] == ref["value"], (q["evals"], ref["evals"])
