"""GPU suite (-m gpu): the dense Cholesky (csrc/chol.hpp, csrc/chol2.hpp) against EXACT solutions (dense_ref.py), in all four
modes CFMM_CHOL in {pairs, single} x CFMM_BACKSUB in {default, classic}, at the sizes where a block, a pair of blocks, a
kernel role or a strip loop begins, on ill-conditioned, badly scaled and solver-made (lower-triangular Hessian) systems;
and the contracts the second-order solve leans on: only the lower triangle is read, bitwise determinism, recovery after
a failed factorisation in the same context, a flag for every non-positive or non-finite pivot wherever it sits.

Ceilings (test_dense_ref_host.py proves on the CPU that fp64 LAPACK sits a factor 10 inside each, for every case here):
  forward error   n eps cond_2(A)                 -- and K_FORWARD max(e_LAPACK, eps), measured: docs/cholesky_accuracy.md
  backward error  n eps                           -- CFMM_BACKSUB=classic (triangular back substitution)
                  n eps sqrt(cond_2(A))           -- the default: x = W' y with the explicit inverse factor W = L^-1
Every case prints one `CHOLACC {...}` line with its figures before it asserts (pytest -s shows them)."""
import json

import numpy as np
import pytest

import cfmm
from cfmm import _lib
import dense_ref as D
from helpers import mixed_network, smoothed_hessian_point

pytestmark = pytest.mark.gpu

# forward error of the device against max(LAPACK's on the same system, eps): the next power of two above four times the
# largest ratio measured over every case and mode on an MI355X (docs/cholesky_accuracy.md holds the ratios)
K_FORWARD = 128.0

MODE_IDS = ["%s-%s" % m for m in D.MODES]


def _context(monkeypatch, n, mode):
    """a context created under the mode's knobs (libcfmm_hip.so reads them once per context)"""
    chol, backsub = mode
    monkeypatch.setenv("CFMM_CHOL", chol)
    if backsub == "classic":
        monkeypatch.setenv("CFMM_BACKSUB", "classic")
    else:
        monkeypatch.delenv("CFMM_BACKSUB", raising=False)
    return _lib.Context(n)


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _check_solve(ctx, mode, name, ref, A_dev, b_dev, b2_dev, s=None, k_rule=True):
    """assertions a - d for one system in one mode.  A_dev, b_dev: what the device is handed; s: the diagonal scaling to undo
    (x = s x_dev, exact) so that every figure is taken on ref's own system; k_rule: the K_FORWARD bound beside the ceilings"""
    n, cond, backsub = ref.n, ref.cond, mode[1]
    s = np.ones(n) if s is None else s
    x, info = ctx.debug_cholesky(A_dev, b_dev)
    x = x * s
    finite = bool(np.all(np.isfinite(x)))
    e = D.forward_error(x, ref.xs) if finite else float("inf")
    eta = ref.eta(x) if finite else float("inf")
    rec = dict(case=name, mode="%s-%s" % mode, n=n, cond=cond, info=info, e=e, e_lapack=ref.e_lapack, eta=eta, eta_lapack=ref.eta_lapack)
    x2 = None
    if backsub != "classic":
        x2 = ctx.debug_cholesky_apply(b2_dev) * s
        ok2 = bool(np.all(np.isfinite(x2)))
        rec.update(e2=D.forward_error(x2, ref.xs2) if ok2 else float("inf"), e2_lapack=ref.e2_lapack,
                   eta2=ref.eta2(x2) if ok2 else float("inf"), eta2_lapack=ref.eta2_lapack)      # (eta2: recorded, not asserted)
    print("CHOLACC " + json.dumps(rec))
    assert info == 0                                                                        # a
    assert e <= D.forward_ceiling(n, cond), rec                                             # b: the textbook bound
    assert not k_rule or e <= K_FORWARD * max(ref.e_lapack, D.EPS), rec                     #    and LAPACK's neighbourhood
    assert eta <= D.eta_ceiling(n, cond, backsub), rec                                      # c
    if backsub != "classic":                                                                # d
        assert rec["e2"] <= D.forward_ceiling(n, cond), rec
        assert not k_rule or rec["e2"] <= K_FORWARD * max(ref.e2_lapack, D.EPS), rec
    else:
        # the chord step needs the inverse factor: refused (launch_chord: CFMM_E_STATE), and the context is none the worse
        with pytest.raises(_lib.CfmmError) as err:
            ctx.debug_cholesky_apply(b2_dev)
        assert err.value.code == -3
        xa, info_a = ctx.debug_cholesky(A_dev, b_dev)
        assert info_a == 0 and _same_bits(xa * s, x)


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cid", D.case_ids(), ids=D.case_name)
def test_cholesky_against_exact_solutions(cid, mode, monkeypatch):
    family, n, cond = cid
    ref = D.reference(*cid)
    ctx = _context(monkeypatch, n, mode)
    try:
        if family == "scaled":
            As, bs, b2s, s = D.scaled_system(ref, n)
            _check_solve(ctx, mode, D.case_name(cid), ref, As, bs, b2s, s)
        else:
            _check_solve(ctx, mode, D.case_name(cid), ref, ref.A, ref.b, ref.b2)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
def test_cholesky_of_a_smoothed_hessian_lower_triangle(mode, monkeypatch):
    """the solver's own kind of input -- a lower triangle over an exactly zero upper one, one eigenvalue 1e-9 of the rest --
    on the recorded matrix (dense_ref.hessian_golden), every rule"""
    ref = D.hessian_golden()
    assert 1e8 <= ref.cond <= 1e10 and np.all(np.triu(ref.L, 1) == 0.0)
    ctx = _context(monkeypatch, ref.n, mode)
    try:
        _check_solve(ctx, mode, "hessian-n%d-mu%g" % (ref.n, D.HESSIAN_MU), ref, ref.L, ref.b, ref.b2)
    finally:
        ctx.close()


_LIVE = {}


def _live_hessian_reference():
    """what ctx.eval_smooth returns in THIS run for the recorded matrix's network and prices (its fp64 atomics differ from run to
    run: one evaluation and one exact reference per process)"""
    if "ref" not in _LIVE:
        net = mixed_network(0, D.HESSIAN_TOKENS, D.HESSIAN_POOLS)
        p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
        _, _, _, H = p._ensure_ctx().eval_smooth(smoothed_hessian_point(net), D.HESSIAN_MU, want_hessian=True)
        p.close()
        _LIVE["H"], _LIVE["ref"] = H, D.hessian_reference(H)
    return _LIVE["H"], _LIVE["ref"]


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
def test_cholesky_of_the_devices_own_hessian(mode, monkeypatch):
    """the recorded matrix IS what the device's evaluation produces (to the 1e-8 of test_smoothed_evaluation_matches_numpy_restatement),
    and the run's own matrix, passed as the solver passes it, meets the ceilings.  Not the K_FORWARD multiple of LAPACK's error:
    with one tiny eigenvalue the forward error is a single random scalar for either solver, and between three runs LAPACK's moved
    by a factor 7 and the ratio from 0.9 to 55 (docs/cholesky_accuracy.md) -- a bound on it would be a bound on LAPACK's luck"""
    H, ref = _live_hessian_reference()
    G = np.load(D.HESSIAN_GOLDEN)
    assert np.all(np.triu(H, 1) == 0.0)
    assert np.abs(np.tril(H) - G).max() <= 1e-8 * np.abs(G).max()
    assert ref.delta == D.hessian_golden().delta and 1e8 <= ref.cond <= 1e10
    ctx = _context(monkeypatch, ref.n, mode)
    try:
        _check_solve(ctx, mode, "livehessian-n%d-mu%g" % (ref.n, D.HESSIAN_MU), ref, ref.L, ref.b, ref.b2, k_rule=False)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", D.DIAGONAL_SIZES)
def test_diagonal_systems_to_four_roundings(n, mode, monkeypatch):
    """diag(a) x = b isolates the diagonal block's 1 / sqrt(pivot) (WaveFactor: v_rsq_f64 plus a third-order correction): every
    product beside it has one non-zero term, so x_i = y (y b_i) carries y's error twice and two roundings -- against the
    exact rational b_i / a_i, (1 + u)^4 - 1 with u = 2^-53 (dense_ref.DIAGONAL_BOUND; LAPACK meets it on the CPU).  The
    K_FORWARD rule leaves a factor 4 to 8 of room by construction and cannot see a 1 / sqrt that is a few ulps off; this does"""
    a, b = D.diagonal(n)
    ctx = _context(monkeypatch, n, mode)
    try:
        x, info = ctx.debug_cholesky(np.diag(a), b)
    finally:
        ctx.close()
    err = D.diagonal_error(a, b, x) if np.all(np.isfinite(x)) else float("inf")
    print("CHOLDIAG " + json.dumps(dict(n=n, mode="%s-%s" % mode, info=info, err_over_eps=float(err / D.EPS))))
    assert info == 0
    assert err <= D.DIAGONAL_BOUND, float(err / D.EPS)


# ---------------------------------------------------------------------------------------------------------------
# contracts, every mode, one size inside a pair of blocks and one with every kernel role
# ---------------------------------------------------------------------------------------------------------------
CONTRACT_SIZES = (33, 129)


def _solve_and_apply(ctx, mode, A, b, b2):
    x, info = ctx.debug_cholesky(A, b)
    return x, info, (ctx.debug_cholesky_apply(b2) if mode[1] != "classic" else None)


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", CONTRACT_SIZES)
def test_only_the_lower_triangle_is_read(n, mode, monkeypatch):
    """e: symmetric A, tril(A) over zeros (what the solver passes) and tril(A) under finite garbage: the same bits"""
    ref = D.reference("spectrum", n, 1e8)
    low = np.tril(ref.A)
    junk = low + np.triu(np.random.default_rng(n).normal(0.0, 1e3, (n, n)), 1)
    ctx = _context(monkeypatch, n, mode)
    try:
        out = [_solve_and_apply(ctx, mode, M, ref.b, ref.b2) for M in (ref.A, low, junk)]
    finally:
        ctx.close()
    for x, info, x2 in out:
        assert info == 0
        assert _same_bits(x, out[0][0])
        assert x2 is None or _same_bits(x2, out[0][2])
    assert D.forward_error(out[1][0], ref.xs) <= D.forward_ceiling(n, ref.cond)


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", CONTRACT_SIZES)
def test_factorisation_is_bitwise_deterministic(n, mode, monkeypatch):
    """f: "fixed summation orders throughout" (chol.hpp) -- twice in one context, once in a fresh one"""
    ref = D.reference("spectrum", n, 1e8)
    ctx = _context(monkeypatch, n, mode)
    try:
        first = _solve_and_apply(ctx, mode, ref.A, ref.b, ref.b2)
        second = _solve_and_apply(ctx, mode, ref.A, ref.b, ref.b2)
    finally:
        ctx.close()
    ctx = _context(monkeypatch, n, mode)
    try:
        fresh = _solve_and_apply(ctx, mode, ref.A, ref.b, ref.b2)
    finally:
        ctx.close()
    for x, info, x2 in (second, fresh):
        assert info == 0 and first[1] == 0
        assert _same_bits(x, first[0])
        assert x2 is None or _same_bits(x2, first[2])


def _pivots(n):
    return np.arange(1.0, n + 1) % 4 + 1


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", CONTRACT_SIZES)
def test_recovery_after_a_failed_factorisation(n, mode, monkeypatch):
    """g: the solver's shift-and-retry path -- factor, fail (the inverse blocks and the inverse factor are then full of NaN
    from the failed pivot on), factor again in the same context: the bits of the first time, the chord product included"""
    ref = D.reference("spectrum", n, 1e8)
    d = _pivots(n); d[32] = -1.0
    bad = D.ldl_integer(n, d)
    ctx = _context(monkeypatch, n, mode)
    try:
        first = _solve_and_apply(ctx, mode, ref.A, ref.b, ref.b2)
        _, info_bad = ctx.debug_cholesky(bad, ref.b)
        again = _solve_and_apply(ctx, mode, ref.A, ref.b, ref.b2)
    finally:
        ctx.close()
    assert first[1] == 0 and info_bad != 0 and again[1] == 0
    assert _same_bits(again[0], first[0])
    assert again[2] is None or _same_bits(again[2], first[2])
    assert D.forward_error(again[0], ref.xs) <= D.forward_ceiling(n, ref.cond)


@pytest.mark.parametrize("mode", D.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", CONTRACT_SIZES)
def test_a_bad_pivot_is_flagged_wherever_it_sits(n, mode, monkeypatch):
    """h: info != 0 (non-zero: not positive definite; the value is NOT a position) for a negative pivot at the first and
    last index of a block, of a pair, of the matrix; for an exactly zero pivot; for +inf on the diagonal.  info == 0 for a
    positive definite matrix whose smallest pivot is 1e-300"""
    b = D.reference("spectrum", n, 1e8).b
    ctx = _context(monkeypatch, n, mode)
    try:
        for p in sorted({0, 31, 32, n - 1} | ({64} if n == 129 else set())):
            d = _pivots(n); d[p] = -1.0
            _, info = ctx.debug_cholesky(D.ldl_integer(n, d), b)
            assert info != 0, ("negative pivot", p)
        # the all-ones 2 x 2 block over rows 31, 32 (across the block boundary) inside a diagonal of powers of four:
        # pivot 31 is 1, its square root exact, pivot 32 = 1 - 1 * 1 exactly zero
        Z = np.diag(np.ldexp(1.0, 2 * (np.arange(n) % 3)))
        Z[31:33, 31:33] = 1.0
        _, info = ctx.debug_cholesky(Z, b)
        assert info != 0, "zero pivot"
        Inf = D.ldl_integer(n, _pivots(n))
        Inf[32, 32] = np.inf
        _, info = ctx.debug_cholesky(Inf, b)
        assert info != 0, "+inf on the diagonal"
        d = _pivots(n); d[31] = 1e-300
        x, info = ctx.debug_cholesky(D.ldl_integer(n, d, alone=(31,)), b)
        assert info == 0, "smallest pivot 1e-300"
        assert np.all(np.isfinite(x)) and abs(x[31] - b[31] / 1e-300) <= 1e-12 * abs(b[31] / 1e-300)
    finally:
        ctx.close()
