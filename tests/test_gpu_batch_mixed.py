"""GPU suite (-m gpu): batched evaluations and solves (cfmm_eval_dual_batch, cfmm_solve_batch, Problem.solve_many) over networks
that hold stableswap / power-sum two-asset pools and buckets of the K-asset table next to the closed-form families: the batched
launches of the heavy tiles (eval_batch_heavy_kernel) and of the table (table_batch_eval_kernel) against the single-vector kernels.

The small network gives every tile family a full wave-tile and a ragged one: heavy tiles hold 64 pools (curve2 130, pow2 70),
table tiles 64 / k pools (k = 2: 70 pools, 3: 50, 4: 40, 5: 30, 8: 20), cp2 tiles 128 (200), w2 tiles 64 (70).

Tolerances.  Evaluation: that of tests/test_gpu_table.py (1e-10 relative; the same root search from different starts).  Values of
solves: each solve brackets the optimum within its own certified gap (tol), so two solves of one utility differ by at most the sum
of the two certificates, 2 tol * max(1, |value|).  Tenders: 1e-10 of the largest reserve, as tests/test_gpu_table.py."""
import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib

pytestmark = pytest.mark.gpu

SEED = 11
TABLE = ((2, 70), (3, 50), (4, 40), (5, 30), (8, 20))


def _small_network(with_sum=False):
    net = synthetic.make_network(24, m_cp2=200, m_w2=70, m_gn=60, m_curve2=130, m_pow2=70, seed=SEED, peg=8)
    gk = {}
    for k, m in TABLE:
        t = synthetic.make_network(24, m_gk_stable=m, gk_sizes=(k, k), seed=SEED, peg=8)
        assert np.array_equal(t["prices"], net["prices"]) and t["gk"][("stable", k)]["R"].shape == (k, m)
        gk[("stable", k)] = t["gk"][("stable", k)]
    if with_sum:
        t = synthetic.make_network(24, m_gk_stable=1, m_gk_sum=30, gk_sizes=(3, 3), seed=SEED, peg=8)
        assert np.array_equal(t["prices"], net["prices"]) and t["gk"][("sum", 3)]["R"].shape == (3, 30)
        gk[("sum", 3)] = t["gk"][("sum", 3)]
    net["gk"] = gk
    return net


@pytest.fixture(scope="module")
def small_net():
    return _small_network()


def _mixed_utilities(net, rng, count):
    """as tests/test_gpu.py: arbitrage under perturbed market values, liquidations and swaps of random baskets"""
    n = net["n_tokens"]
    out = []
    for k in range(count):
        if k % 3 == 0:
            out.append(cfmm.Arbitrage(net["c"] * np.exp(rng.normal(0, 0.003 * (1 + k), n))))
        else:
            h = np.zeros(n); idx = rng.choice(n, 4 + k, replace=False)
            h[idx] = np.exp(rng.normal(2, 0.5, idx.size)) / net["prices"][idx] * 10
            t = int(rng.integers(0, n)); h[t] = 0.0
            out.append(cfmm.Liquidate(h, t) if k % 3 == 1 else cfmm.Swap(h, t))
    return out


def _single_evals(net, nus):
    """eval_dual of every vector on a FRESH context (its stableswap searches start cold)"""
    out = []
    for nu in nus:
        q = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
        out.append(q._ensure_ctx().eval_dual(nu))
        q.close()
    return out


def _assert_evals_agree(arb, psi, ref, what):
    for b, (f1, psi1) in enumerate(ref):
        ef = abs(arb[b] - f1) / abs(f1)
        ep = np.abs(psi[b] - psi1).max() / np.abs(psi1).max()
        print(f"{what} vector {b}: arb_sum rel {ef:.2e}, psi rel {ep:.2e}")
        assert ef <= 1e-10 and ep <= 1e-10, (what, b, ef, ep)


@pytest.mark.parametrize("with_sum", [False, True])
def test_batched_evaluation_matches_single_evaluations(with_sum):
    net = _small_network(with_sum)
    n = net["n_tokens"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    cap = ctx.batch_capacity()
    assert cap == 8
    clones = [ctx.clone() for _ in range(cap - 1)]
    rng = np.random.default_rng(3)
    for nb in (1, 3, cap):
        nus = [net["prices"] * np.exp(rng.normal(0, 0.05, n)) for _ in range(nb)]
        ref = _single_evals(net, nus)
        assert len({round(f, 6) for f, _ in ref}) == nb                 # distinct vectors, distinct answers
        for rep in range(2):               # the second call: accumulators and warm-start slab are re-armed by every call
            arb, psi = ctx.eval_dual_batch(clones[:nb - 1], nus)
            _assert_evals_agree(arb, psi, ref, f"sum={with_sum} nb={nb} call {rep}")
    for c in clones:
        c.close()
    p.close()


def test_one_vector_does_not_leak_into_another(small_net):
    """Vector 0 sits on the peg (every token of a peg group at the group's price: the stableswap pools' no-trade region, where a pool
    writes no warm start), the others 20 % off it: a warm start or a psi tile shared between vectors would show in vector 0, or
    in whichever vector follows it, in one of the two orders."""
    net = small_net
    n = net["n_tokens"]
    peg = net["prices"][(np.arange(n) // 8) * 8]
    rng = np.random.default_rng(4)
    nus = [peg] + [peg * np.exp(0.2 * rng.choice([-1.0, 1.0], n)) for _ in range(3)]
    ref = _single_evals(net, nus)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    ctx = p._ensure_ctx()
    clones = [ctx.clone() for _ in range(3)]
    arb, psi = ctx.eval_dual_batch(clones, nus)
    _assert_evals_agree(arb, psi, ref, "peg first")
    arb, psi = ctx.eval_dual_batch(clones, nus[::-1])
    _assert_evals_agree(arb, psi, ref[::-1], "peg last")
    for c in clones:
        c.close()
    p.close()


@pytest.fixture(scope="module")
def batch_of_five(small_net):
    """5 mixed utilities through ctx.solve_batch (first-order, tol 1e-8), and each alone on a fresh context"""
    net = small_net
    utils = _mixed_utilities(net, np.random.default_rng(5), 5)
    starts = [cfmm.start_prices(net, u) for u in utils]
    singles = []
    for u, nu0 in zip(utils, starts):
        q = cfmm.Problem.from_network(net, utility=u)
        c = q._ensure_ctx()
        c.set_utility(u.c, u.h, u.ctype)
        singles.append(c.solve(nu0, tol=1e-8, max_evals=4000, method="lbfgs"))
        q.close()
    p = cfmm.Problem.from_network(net, utility=utils[0])
    ctx = p._ensure_ctx()
    ctxs = [ctx] + [ctx.clone() for _ in range(4)]
    for c, u in zip(ctxs, utils):
        c.set_utility(u.c, u.h, u.ctype)
    sts = ctx.solve_batch(ctxs[1:], starts, tol=1e-8, max_evals=4000, method="lbfgs")
    yield net, utils, singles, ctxs, sts
    for c in ctxs[1:]:
        c.close()
    p.close()


def test_batched_solves_match_single_solves(batch_of_five):
    net, utils, singles, ctxs, sts = batch_of_five
    for b, (s1, sb) in enumerate(zip(singles, sts)):
        print(f"solve {b}: single status {s1['status']} value {s1['primal_value']:.12g} gap {s1['gap']:.2e} infeas {s1['infeas']:.2e} evals {s1['evals']} | "
              f"batched status {sb['status']} value {sb['primal_value']:.12g} gap {sb['gap']:.2e} infeas {sb['infeas']:.2e} evals {sb['evals']}")
    for b, (s1, sb) in enumerate(zip(singles, sts)):
        assert s1["status"] == 1 and s1["gap"] <= 1e-8 and s1["infeas"] <= 1e-8, (b, s1)
        assert sb["status"] == 1 and sb["gap"] <= 1e-8 and sb["infeas"] <= 1e-8, (b, sb)
        assert abs(sb["primal_value"] - s1["primal_value"]) <= 2e-8 * max(1.0, abs(s1["primal_value"])), (b, sb["primal_value"], s1["primal_value"])
    assert len({sb["evals"] for sb in sts}) > 1                # members end at different iterations: the alive mask is exercised


def test_tenders_read_back_after_a_batch(batch_of_five):
    """a clone of the batch reads back as after cfmm_solve: the tenders of its stableswap buckets at its accepted prices are those of a
    fresh context set to the same prices"""
    net, utils, singles, ctxs, sts = batch_of_five
    c = ctxs[2]
    nu, _ = c.get_solution()
    q = cfmm.Problem.from_network(net, utility=utils[2])
    f = q._ensure_ctx()
    f.set_nu(nu)
    m2 = len(net["curve2"]["Ra"])
    d, l = c.get_trades2(_lib.POOL_CURVE2, m2)
    d0, l0 = f.get_trades2(_lib.POOL_CURVE2, m2)
    e2 = np.abs((l - d) - (l0 - d0)).max()
    assert np.abs(l0 - d0).max() > 0 and e2 <= 1e-10 * max(net["curve2"]["Ra"].max(), net["curve2"]["Rb"].max()), e2
    b = net["gk"][("stable", 4)]
    d, l = c.get_tradesG(_lib.POOLK["stable"], 4, b["R"].shape[1])
    d0, l0 = f.get_tradesG(_lib.POOLK["stable"], 4, b["R"].shape[1])
    eg = np.abs((l - d) - (l0 - d0)).max()
    assert np.abs(l0 - d0).max() > 0 and eg <= 1e-10 * b["R"].max(), eg
    q.close()


def test_solve_many_takes_the_batched_path_end_to_end():
    net = synthetic.make_network(200, m_cp2=20_000, m_gn=2_000, m_gk_stable=3_000, m_pow2=5_000)
    utils = _mixed_utilities(net, np.random.default_rng(6), 6)
    p = cfmm.Problem.from_network(net, utility=utils[0])
    res = p.solve_many(utils, batch=4, method="lbfgs", tol=1e-7)
    assert [r["stats"]["batch"] for r in res] == [4, 4, 4, 4, 2, 2]
    assert all(r["status"] == "optimal" for r in res), [(r["status"], r["gap"], r["infeas"]) for r in res]
    ref = p.solve_many(utils, batch=0, method="lbfgs", tol=1e-7)
    for r, r0 in zip(res, ref):
        assert r0["status"] == "optimal" and "batch" not in r0["stats"]
        assert abs(r["value"] - r0["value"]) <= 2e-7 * max(1.0, abs(r0["value"])), (r["value"], r0["value"])
    p.close()
    c5 = synthetic.config("C5", scale=0.01, seed=0)
    with pytest.raises(ValueError, match="batched path"):         # 5 000 stableswap pools: "auto" means the second-order method there
        cfmm.Problem.from_network(c5, utility=cfmm.Arbitrage(c5["c"])).solve_many([cfmm.Arbitrage(c5["c"])], batch=4)


def test_refusals_are_kept(small_net):
    net = _small_network(with_sum=True)
    u = cfmm.Arbitrage(net["c"])
    p = cfmm.Problem.from_network(net, utility=u)
    ctx = p._ensure_ctx()
    k = ctx.clone()
    for c in (ctx, k):
        c.set_utility(u.c, u.h, u.ctype)
    starts = [net["c"], net["c"]]
    with pytest.raises(cfmm.CfmmError, match="first-order method only"):
        ctx.solve_batch([k], starts, method="newton")
    k.set_pool_flagsG(3, np.ones((3, 30), dtype=np.int32))
    with pytest.raises(cfmm.CfmmError, match="has price ties set"):
        ctx.solve_batch([k], starts, method="lbfgs")
    with pytest.raises(cfmm.CfmmError, match="has price ties set"):
        ctx.eval_dual_batch([k], starts)
    k.close()
    d = cfmm.Problem.from_network(net, utility=u, deterministic=True)
    dc = d._ensure_ctx()
    dk = dc.clone()
    for c in (dc, dk):
        c.set_utility(u.c, u.h, u.ctype)
    with pytest.raises(cfmm.CfmmError, match="reproducible contexts are solved one at a time"):
        dc.solve_batch([dk], starts, method="lbfgs")
    dk.close(); d.close()
    other = cfmm.Problem.from_network(small_net, utility=u)
    with pytest.raises(cfmm.CfmmError, match="does not share"):
        ctx.eval_dual_batch([other._ensure_ctx()], starts)
    other.close(); p.close()
