"""CPU suite: which solves `Problem.solve_many` hands to the batched path (Problem._batch_applies reads the network, the
utilities and the options only -- no device), and the batched evaluation's entry point in the library's symbol list."""
import numpy as np
import pytest

import cfmm
from cfmm import synthetic, _lib
from cfmm.problem import AUTO_NEWTON_MIN_STABLE


def _net(**kw):
    return synthetic.make_network(24, m_cp2=40, seed=1, peg=8, **kw)


NETS = {
    "curve2": dict(m_curve2=30),
    "pow2": dict(m_pow2=30),
    "stable4": dict(m_gk_stable=30, gk_sizes=(4, 4)),
}


def _applies(net, method=None, utilities=None, **pkw):
    u = cfmm.Arbitrage(net["c"])
    p = cfmm.Problem.from_network(net, utility=u, **pkw)
    return p._batch_applies([u] if utilities is None else utilities, {} if method is None else dict(method=method))


@pytest.mark.parametrize("name", sorted(NETS))
def test_search_pool_networks_are_batched_under_lbfgs_and_under_auto_below_the_threshold(name):
    net = _net(**NETS[name])
    assert name == "stable4" and ("stable", 4) in net["gk"] or name in net
    assert _applies(net, "lbfgs") is True
    assert _applies(net, "auto") is True and _applies(net) is True
    assert _applies(net, "newton") is False
    assert _applies(net, "lbfgs", deterministic=True) is False


def test_auto_at_or_above_the_stableswap_threshold_is_not_batched():
    below = synthetic.make_network(40, m_cp2=40, m_curve2=AUTO_NEWTON_MIN_STABLE - 101, m_gk_stable=100, gk_sizes=(4, 4), seed=2)
    at = synthetic.make_network(40, m_cp2=40, m_curve2=AUTO_NEWTON_MIN_STABLE - 100, m_gk_stable=100, gk_sizes=(4, 4), seed=2)
    for net, n_stable in ((below, AUTO_NEWTON_MIN_STABLE - 1), (at, AUTO_NEWTON_MIN_STABLE)):
        p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
        assert p._stable_count() == n_stable            # curve2 plus the table's stableswap pools, as `solve` counts them
    assert _applies(below, "auto") is True
    assert _applies(at, "auto") is False and _applies(at) is False
    assert _applies(at, "lbfgs") is True                # (an explicit first-order method is taken at any count)


def test_constant_sum_pools_utility_table_entries_and_the_other_modes_stay_out():
    sum2 = synthetic.make_network(24, m_cp2=40, seed=1)
    sum2["sum2"] = {k: v[:10].copy() for k, v in sum2["cp2"].items()}
    assert _applies(sum2, "lbfgs") is False and _applies(sum2, "auto") is False
    sum3 = _net(m_gk_stable=10, m_gk_sum=10, gk_sizes=(3, 3))
    assert ("sum", 3) in sum3["gk"]
    assert _applies(sum3, "lbfgs") is False and _applies(sum3, "auto") is False
    plain = _net()
    assert _applies(plain, "lbfgs") is True and _applies(plain, "auto") is True        # (what batches today)
    assert _applies(plain, "newton") is False
    assert _applies(plain, "auto", deterministic=True) is False
    n = plain["n_tokens"]
    ctype = np.zeros(n, dtype=np.int32); ctype[3] = _lib.ULOG
    general = cfmm.Utility(plain["c"], np.zeros(n), ctype)
    assert _applies(plain, "lbfgs", utilities=[cfmm.Arbitrage(plain["c"]), general]) is False


def test_the_batched_evaluation_is_a_public_symbol():
    assert "cfmm_eval_dual_batch" in _lib.SYMBOLS
    assert hasattr(_lib.Context, "eval_dual_batch")
