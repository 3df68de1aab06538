"""GPU suite: the reproducible mode's fixed point on the device against exact integers -- the device's compile of
csrc/fixedpoint.hpp alone (cfmm_debug_scatter_limbs), one evaluation of a network whose read-back repeats what the evaluation
scatters bit for bit, and the psi of a solve.  The only tolerances here are equality and, for psi as a double, the one unit in the
last place that limbs_to_double's double rounding costs (derived in test_gpu.py: test_reproducible_mode_...)."""
import numpy as np
import pytest

import cfmm
from cfmm import _lib
from cfmm.problem import POOL_CP2, POOL_SUM2
from helpers import FIXED_EDGES, fixed_scale_exponent, fixed_random_scaled, exact_floor, limbs_as_integers

pytestmark = pytest.mark.gpu


def _token_sums(n, tok, y, F):
    """per token, the exact sum of floor(Fraction(y_i) 2^F) over its contributions (Python integers)"""
    tot = [0] * n
    for t, v in zip(np.asarray(tok).tolist(), exact_floor(y, F)):
        tot[t] += v
    return tot


@pytest.mark.parametrize("ref", [(1e6, 0.997), (1e12, 1e-3)])
def test_device_split_sums_to_the_exact_floors(ref):
    """Scatter<true>::add on 4096 caller-supplied contributions over 8 tokens: token 0 takes 1024 of mixed sign, token 1 takes 1024
    copies of the value whose low limb is 2^32 - 1 (carry head-room), tokens 6 and 7 one contribution each (2^84 - 2^31 and -0.3
    units: a single split, limbs in isolation), tokens 2..5 share the rest; every token's limbs == the exact sum of the floors"""
    n, count = 8, 4096
    F = fixed_scale_exponent(*ref)
    edges = np.array(FIXED_EDGES)
    mixed = np.concatenate([edges, -edges, fixed_random_scaled(count - 1024 - 2 - 2 * len(edges), 31)])
    assert len(mixed) >= 3000 + 2 * len(edges)
    mixed = mixed[np.random.default_rng(32).permutation(len(mixed))]
    yf = np.concatenate([mixed[:1024], np.full(1024, 2.0 ** 32 - 1), [2.0 ** 84 - 2.0 ** 31, -0.3], mixed[1024:]])
    tok = np.concatenate([np.zeros(1024, int), np.ones(1024, int), [6, 7], 2 + np.arange(len(mixed) - 1024) % 4]).astype(np.int32)
    assert len(yf) == len(tok) == count and (mixed[:1024] < 0).sum() > 300 and (mixed[:1024] > 0).sum() > 300
    order = np.random.default_rng(33).permutation(count)           # (the order of arrival must not matter either)
    yf, tok = yf[order], tok[order]
    y = yf * 2.0 ** -F
    assert np.array_equal(y * 2.0 ** F, yf)
    ctx = _lib.Context(n, 0)
    try:
        limbs = ctx.debug_scatter_limbs(tok, y, *ref)
        again = ctx.debug_scatter_limbs(tok[::-1], y[::-1], *ref)
    finally:
        ctx.close()
    want = _token_sums(n, tok, y, F)
    assert want[7] == -1 and want[6] == 2 ** 84 - 2 ** 31 and want[1] == 1024 * (2 ** 32 - 1)
    assert int(limbs[0, 1]) == 1024 * (2 ** 32 - 1) and limbs[1, 1] == 0 and limbs[2, 1] == 0
    assert [int(limbs[k, 7]) for k in range(3)] == [2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1]          # -1 = (-1) 2^64 + (2^32 - 1) 2^32 + 2^32 - 1
    assert np.all(limbs[:2] < 2 ** 63)                  # (so that reading the low limbs as signed sums gives the same integers)
    assert limbs_as_integers(limbs) == want
    assert np.array_equal(again, limbs)


# ---------------------------------------------------------------------------------------------------------------
# a network whose read-back (trades2_kernel) computes bit for bit what the evaluation scatters: constant-product pools
# (pool_cp2 against pool_cp2_dir: the same operations in the same order) and constant-sum pools (no arithmetic but -R / g)
# ---------------------------------------------------------------------------------------------------------------
N_TOK, M_CP2, M_SUM2 = 16, 300, 130            # 300 = two full 128-pool wave-tiles and a partial one


def _boundary_price(Ra, Rb, g, pa, pb, k):
    """the k-th double pb, counted upwards, at which the pool tenders a:  g (pb Rb) > pa Ra  as the kernels evaluate it"""
    va = pa * Ra
    while g * (pb * Rb) > va:
        pb = np.nextafter(pb, 0.0)
    while not g * (pb * Rb) > va:
        pb = np.nextafter(pb, np.inf)
    for _ in range(k - 1):
        pb = np.nextafter(pb, np.inf)
    return pb


@pytest.fixture(scope="module")
def network():
    rng = np.random.default_rng(2604)
    n = N_TOK
    c = np.exp(rng.normal(0, 0.02, n))                              # the market
    nu = c * np.exp(rng.normal(0, 0.05, n))                         # prices about 5 % off it
    fees = np.array([0.997, 0.999, 0.9995])

    def pairs(m):
        ia = rng.integers(0, n, m)
        return ia.astype(np.int32), ((ia + rng.integers(1, n, m)) % n).astype(np.int32)

    ia, ib = pairs(M_CP2)
    Ra = 10.0 ** rng.uniform(0, 9, M_CP2)                           # log-uniform: nearly half the tenders are below 2^-21 of the largest
    Rb = Ra * c[ia] / c[ib] * np.exp(rng.normal(0, 0.01, M_CP2))
    fee = rng.choice(fees, M_CP2)
    # pools 0..7 sit k = 1..8 doubles inside the region where they tender a: reserves of a few units, so that the tender is a few
    # hundred units of 2^-F at the most.  Pool k - 1 trades tokens (2k - 2, 2k - 1), and the price of the second is made for it.
    for k in range(1, 9):
        i, a, b = k - 1, 2 * k - 2, 2 * k - 1
        ia[i], ib[i] = a, b
        Ra[i] = rng.uniform(1.0, 30.0)
        Rb[i] = nu[a] * Ra[i] / (fee[i] * nu[b])
        nu[b] = _boundary_price(Ra[i], Rb[i], fee[i], nu[a], nu[b], k)
    sa, sb = pairs(M_SUM2)
    sRa, sRb = 10.0 ** rng.uniform(0, 9, M_SUM2), 10.0 ** rng.uniform(0, 9, M_SUM2)
    sfee = rng.choice(fees, M_SUM2)
    # the bang-bang direction of a constant-sum pool is no rounding question
    pa, pb = nu[sa], nu[sb]
    assert np.minimum(np.abs(sfee * pb - pa) / pa, np.abs(sfee * pa - pb) / pb).min() >= 1e-9
    trades = (sfee * pb > pa) | (sfee * pa > pb)
    assert (sfee * pb > pa).sum() >= 20 and (sfee * pa > pb).sum() >= 20 and not trades.all()
    net = dict(n_tokens=n, c=c, cp2=dict(Ra=Ra, Rb=Rb, fee=fee, ia=ia, ib=ib), sum2=dict(Ra=sRa, Rb=sRb, fee=sfee, ia=sa, ib=sb))
    mr = max(Ra.max(), Rb.max(), sRa.max(), sRb.max())
    mf = min(fee.min(), sfee.min())
    return dict(net=net, nu=nu, mr=mr, mf=mf, F=fixed_scale_exponent(mr, mf), tied=int(np.flatnonzero(trades)[0]))


def _read_back_sums(ctx, net, F):
    """per token, the exact sum of floor(y 2^F) over the tenders the device reads back at its accepted prices; y = lambda - delta is exact,
    one of the two being zero.  Also the contributions themselves, in scaled units."""
    tok, y = [], []
    for key, kind in (("cp2", POOL_CP2), ("sum2", POOL_SUM2)):
        b = net[key]
        d, l = ctx.get_trades2(kind, len(b["Ra"]))
        assert np.all((d == 0.0) | (l == 0.0))
        for slot, idx in enumerate((b["ia"], b["ib"])):
            tok.append(idx); y.append(l[slot] - d[slot])
    tok, y = np.concatenate(tok), np.concatenate(y)
    return _token_sums(net["n_tokens"], tok, y, F), y * 2.0 ** F


def test_evaluation_limbs_are_the_exact_sum_of_the_floored_tenders(network):
    """one reproducible-mode evaluation: for every token, debug_eval_limbs == sum over the pools of floor(Fraction(y) 2^F) with y the
    tenders read back at the same prices -- eight constant-product pools a few doubles inside their no-trade boundary (tiny negative
    tenders), reserves over nine decades, and a constant-sum pool with its tie flag set, absent on both sides"""
    net, nu, F = network["net"], network["nu"], network["F"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]), deterministic=True)
    try:
        ctx = p._ensure_ctx()
        flags = np.zeros(M_SUM2, dtype=np.int32); flags[network["tied"]] = 1
        ctx.set_pool_flags(POOL_SUM2, flags)
        ctx.set_nu(nu)
        want, yf = _read_back_sums(ctx, net, F)
        d, l = ctx.get_trades2(POOL_SUM2, M_SUM2)
        assert not d[:, network["tied"]].any() and not l[:, network["tied"]].any()
        assert (d[:, np.arange(M_SUM2) != network["tied"]].sum(axis=0) > 0).sum() >= 19
        # the inputs are what they were built to be: tiny negative tenders from the boundary pools, and most tenders far below the largest
        dcp, _ = ctx.get_trades2(POOL_CP2, M_CP2)
        edge = dcp[0, :8] * 2.0 ** F
        print("boundary pools' tenders in units of 2^-F:", edge.tolist())
        assert ((edge > 0) & (edge < 2.0 ** 10)).sum() >= 4
        neg = yf[yf < 0]
        assert len(neg) >= 150 and (np.abs(neg) < 2.0 ** -21 * np.abs(yf).max()).sum() >= len(neg) // 3
        limbs = ctx.debug_eval_limbs(nu, network["mr"], network["mf"])
        assert limbs_as_integers(limbs) == want
        # ... and with the flag cleared the tied pool's tenders are back on both sides
        ctx.set_pool_flags(POOL_SUM2, None)
        want2, _ = _read_back_sums(ctx, net, F)
        assert want2 != want
        assert limbs_as_integers(ctx.debug_eval_limbs(nu, network["mr"], network["mf"])) == want2
    finally:
        p.close()


def test_psi_of_a_reproducible_solve_is_the_exact_sum_rounded(network):
    """iter_kernel's scatter: after a first-order solve in reproducible mode, the device's psi at the accepted prices lies within one
    unit in the last place of (sum of floor(Fraction(y) 2^F)) / 2^F, y the tenders read back at those prices (limbs_to_double rounds
    twice: one ulp of the once-rounded value, no more); the limbs of an evaluation at those prices are that sum exactly.  psi is the
    device's own: Problem.psi adds the partial fills of tied constant-sum pools, which the host computes, on top."""
    net, F = network["net"], network["F"]
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]), deterministic=True)
    try:
        p.solve(tol=1e-7, method="lbfgs")
        assert p.stats["iters"] >= 1 and p.stats["method"] == _lib.METHODS["lbfgs"]
        ctx = p.ctx
        nu, psi = ctx.get_solution()
        if not p._theta:
            assert np.array_equal(psi, p.psi)
        want, _ = _read_back_sums(ctx, net, F)
        exact = np.array([w / 2 ** F for w in want])                 # (integer / integer: correctly rounded, once)
        print("status", p.status, "evals", p.stats["evals"], "max |psi - exact| in ulps", np.max(np.abs(psi - exact) / np.spacing(np.abs(exact))))
        assert np.any(exact != 0.0)
        assert np.all(np.abs(psi - exact) <= np.spacing(np.abs(exact)))
        assert limbs_as_integers(ctx.debug_eval_limbs(nu, network["mr"], network["mf"])) == want
    finally:
        p.close()
