"""CPU suite: the exact dense reference (dense_ref.py) and the ceilings test_gpu_cholesky.py holds the device's Cholesky to.

For every case of the GPU file: (1) the reference is exact enough to judge fp64 -- its own forward-error bound, from the
EXACT residual of the unrounded iterate, is a thousandth of LAPACK's error against it; (2) fp64 LAPACK sits a factor 10
inside the forward and both backward ceilings, so a device failure cannot be the ceiling's or the reference's doing.

Where LAPACK's answer is the correctly rounded one (n = 1: a single division), its error against x* is 0 and (1) would ask
the impossible: the comparison is floored at eps, the rounding x* itself carries -- the device rule's own floor."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.linalg as sla

import dense_ref as D
from helpers import mixed_network, smoothed_hessian_point


def _check_reference_and_lapack(ref):
    n, cond = ref.n, ref.cond
    # (1) ||x - x^|| <= ||A^-1|| ||r||, r = eta (||A|| ||x^|| + ||b||) <= 2 eta ||A|| ||x^|| (1 + o(1)), and cond_inf <= n cond_2
    for eta_star, e_lap in ((ref.eta_star, ref.e_lapack), (ref.eta_star2, ref.e2_lapack)):
        assert 2 * n * cond * eta_star <= 1e-3 * max(e_lap, D.EPS), (n, cond, eta_star, e_lap)
    # (2) LAPACK under the ceilings with a factor 10 to spare: forward (both right-hand sides), backward -- the tighter of the
    #     two (classic: n eps) and therefore the inverse-factor one (n eps sqrt(cond)) as well
    assert 10 * ref.e_lapack <= D.forward_ceiling(n, cond), (n, cond, ref.e_lapack)
    assert 10 * ref.e2_lapack <= D.forward_ceiling(n, cond), (n, cond, ref.e2_lapack)
    assert 10 * max(ref.eta_lapack, ref.eta2_lapack) <= D.eta_ceiling(n, cond, "classic") <= D.eta_ceiling(n, cond, "default"), (n, cond, ref.eta_lapack, ref.eta2_lapack)
    assert D.lapack_has_room(ref)


@pytest.mark.parametrize("cid", D.case_ids(), ids=D.case_name)
def test_reference_is_exact_and_lapack_has_room_under_the_ceilings(cid):
    family, n, cond = cid
    ref = D.reference(*cid)
    # the condition number the ceilings use is the matrix's own (eigvalsh), and the family delivers what it names
    nominal = cond if n > 1 else 1.0
    assert 0.5 * nominal <= ref.cond <= 2.0 * nominal
    _check_reference_and_lapack(ref)
    # (the family keeps the first draw on which LAPACK has that room: a redraw is the exception, and only where n eps is a few eps)
    assert ref.seed == 0 or (n <= 2 and ref.seed <= 2), ref.seed
    if family == "scaled":
        # the scaling is exact (the device is handed the SAME problem through other exponents), and LAPACK on the scaled
        # system, scaled back, has the same room
        As, bs, b2s, s = D.scaled_system(ref, n)
        assert s.min() >= 2.0 ** -40 and s.max() <= 2.0 ** 40 and np.all(np.log2(s) % 2 == 0)
        assert np.array_equal(As / s[:, None] / s[None, :], ref.A) and np.array_equal(bs / s, ref.b) and np.array_equal(b2s / s, ref.b2)
        x = sla.cho_solve(sla.cho_factor(As, lower=True), bs) * s
        assert 10 * D.forward_error(x, ref.xs) <= D.forward_ceiling(n, ref.cond)
        assert 10 * ref.eta(x) <= D.eta_ceiling(n, ref.cond, "classic")


def test_hessian_family_on_the_recorded_matrix():
    """the `hessian` case as the GPU file runs it (tests/golden/dense_hessian_60.npy), and where the record comes from: the
    NumPy restatement of the device's smoothed evaluation (the GPU file compares the device's own with it)"""
    from oracle import barrier_np
    net = mixed_network(0, D.HESSIAN_TOKENS, D.HESSIAN_POOLS)
    o = barrier_np.smooth_eval(net, smoothed_hessian_point(net), D.HESSIAN_MU, hessian=True)
    G = np.load(D.HESSIAN_GOLDEN)
    assert G.shape == (D.HESSIAN_TOKENS, D.HESSIAN_TOKENS) and np.all(np.triu(G, 1) == 0.0)
    assert np.abs(np.tril(o["H"]) - G).max() <= 1e-10 * np.abs(G).max()
    ref = D.hessian_golden()
    assert 1e8 <= ref.cond <= 1e10 and ref.delta > 0
    assert np.all(np.triu(ref.L, 1) == 0.0) and np.array_equal(np.tril(ref.A), ref.L)
    # H alone is singular along uniform price scaling: the shift is what makes the family solvable
    w = np.linalg.eigvalsh(ref.A - np.diag(ref.delta * np.diag(ref.L) / (1 + ref.delta)))
    assert w[0] <= 1e-10 * w[-1]
    _check_reference_and_lapack(ref)


def test_exact_residual_is_exact():
    """against fractions.Fraction, entry by entry, on a system whose exponents span 160 binades; zero for an exact solution"""
    rng = np.random.default_rng(3)
    n = 7
    s = np.ldexp(1.0, rng.integers(-40, 41, n))
    A = rng.normal(size=(n, n)); A = (A @ A.T + n * np.eye(n)) * s[:, None] * s[None, :]
    x, b = rng.normal(size=n) / s, rng.normal(size=n) * s
    r = [Fraction(b[i]) - sum(Fraction(A[i, j]) * Fraction(x[j]) for j in range(n)) for i in range(n)]
    normA = max(sum(abs(Fraction(A[i, j])) for j in range(n)) for i in range(n))
    eta = max(abs(v) for v in r) / (normA * max(abs(Fraction(v)) for v in x) + max(abs(Fraction(v)) for v in b))
    assert D.exact_residual(A, x, b) == float(eta)
    xi = rng.integers(-9, 10, n).astype(float)
    Ai = np.round(A / s[:, None] / s[None, :] * 8)
    assert D.exact_residual(Ai, xi, Ai @ xi) == 0.0


def test_exact_solve_reaches_a_known_rational_solution():
    """the Hilbert matrix of order 8 (cond 1.5e10) times its fp64 entries' exact inverse image: A x = b with b = A [1 .. 8]
    formed exactly, so x* must come back as the integers, and each refinement step must have shrunk the exact residual"""
    n = 8
    A = np.array([[1.0 / (i + j + 1) for j in range(n)] for i in range(n)])
    xt = np.arange(1.0, n + 1)
    bq = [sum(Fraction(A[i, j]) * int(xt[j]) for j in range(n)) for i in range(n)]
    b = np.array([float(v) for v in bq])                        # rounded: the system solved is A x = fl(b)
    xs, eta = D.exact_solve(A, b)
    assert eta <= 1e-40
    # forward error of the rounded b through cond: x* is within cond eps of the integers, and far closer than LAPACK
    e_lap = D.forward_error(np.linalg.solve(A, b), xs)
    assert D.forward_error(xs, xt) <= D.cond2(A) * D.EPS
    assert D.exact_residual(A, xs, b) <= D.EPS                  # rounding x* to fp64 is all that is left
    assert e_lap > 1e3 * 2 * n * D.cond2(A) * eta


def test_failure_matrices_have_the_pivots_they_name():
    """ldl_integer: the exact Cholesky pivots of the matrices the device's failure-position test uses are the d handed in"""
    n = 33
    d = np.arange(1.0, n + 1) % 4 + 1
    d[31] = -1.0
    A = D.ldl_integer(n, d)
    assert np.array_equal(A, A.T) and np.array_equal(A, np.round(A))
    M = [[Fraction(v) for v in row] for row in A.tolist()]
    piv = []
    for k in range(n):                                          # exact LDL' elimination
        piv.append(M[k][k])
        for i in range(k + 1, n):
            f = M[i][k] / M[k][k]
            for j in range(k, n):
                M[i][j] -= f * M[k][j]
    assert [float(p) for p in piv] == d.tolist()
    d[31] = 1e-300
    A = D.ldl_integer(n, d, alone=(31,))
    assert A[31, 31] == 1e-300 and not A[31, :31].any() and not A[32:, 31].any() and np.all(np.linalg.eigvalsh(np.delete(np.delete(A, 31, 0), 31, 1)) > 0)


@pytest.mark.parametrize("n", D.DIAGONAL_SIZES)
def test_lapack_meets_the_diagonal_bound(n):
    """the four-rounding bound test_gpu_cholesky.py holds the device to on diagonal systems: LAPACK is inside it"""
    a, b = D.diagonal(n)
    x = sla.cho_solve(sla.cho_factor(np.diag(a), lower=True), b)
    assert D.diagonal_error(a, b, x) <= D.DIAGONAL_BOUND
    assert 2 * D.EPS < float(D.DIAGONAL_BOUND) < 2.00001 * D.EPS
