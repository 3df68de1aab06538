"""An exact host reference for dense SPD solves, shared by test_dense_ref_host.py (CPU) and test_gpu_cholesky.py (GPU).

Doubles are dyadic rationals m 2^e, so b - A x is computed EXACTLY in Python integers: A, b and x are held as object
arrays of integers with one common power of two each.  exact_solve() runs iterative refinement around it (the correction
from fp64 LAPACK: scipy's cho_factor / cho_solve; the iterate a sum of doubles, hence dyadic and exact), exact_residual()
measures any candidate solution with the same arithmetic.

The matrix families, the sizes and the ceilings of the device tests live here too, so that the CPU file can prove for
every case the GPU file uses (a) that the reference is far more accurate than what it judges and (b) that fp64 LAPACK
itself sits a factor 10 inside the ceilings -- a device failure is then the device's."""
import functools
import math
import os
from fractions import Fraction

import numpy as np
import scipy.linalg as sla

EPS = 2.0 ** -52

# tokens n -> rows nr = n rounded up to a pair of 32-wide blocks: 1 real row beside 63 of padding; a block (32 / 33) and
# a pair (64 / 65) boundary; no padding at all (64); the first trailing tile and inverse-factor tile (nr = 128); strip
# loops of the back substitution and the inverse-factor product changing shape (nr = 256, 320)
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 257)
CONDS = (1e2, 1e8, 1e12)
N_STRIPS = 577              # nr = 640: all three strip loops of the back substitution, the guarded tail of the eight-wide loads
MODES = tuple((c, s) for c in ("pairs", "single") for s in ("default", "classic"))      # CFMM_CHOL x CFMM_BACKSUB
HESSIAN_TOKENS, HESSIAN_POOLS, HESSIAN_MU = 60, 300, 1e-8
DIAGONAL_SIZES = (33, 257)


# ---------------------------------------------------------------------------------------------------------------
# exact arithmetic
# ---------------------------------------------------------------------------------------------------------------
def _to_int(a):
    """array of doubles -> (object array of Python integers I, exponent e) with a == I 2^e exactly"""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("exact arithmetic needs finite doubles")
    mant, exp = np.frexp(a)
    m = np.ldexp(mant, 53).astype(np.int64)                     # |m| < 2^53: exact
    e = exp.astype(np.int64) - 53
    nz = m != 0
    emin = int(e[nz].min()) if nz.any() else 0
    sh = np.where(nz, e - emin, 0)
    out = np.empty(a.shape, dtype=object)
    out.ravel()[:] = [int(mi) << int(si) for mi, si in zip(m.ravel().tolist(), sh.ravel().tolist())]
    return out, emin


def _to_float(v, e):
    """the integer v times 2^e, correctly rounded to a double"""
    return float(Fraction(v) * (Fraction(2) ** e))


def _absmax(I):
    return max((abs(v) for v in I.ravel().tolist()), default=0)


class ExactSystem:
    """A held as integers once; solve() and residual() for any number of right-hand sides / candidates"""

    def __init__(self, A):
        self.A = np.array(A, dtype=np.float64)
        self.n = self.A.shape[0]
        assert self.A.shape == (self.n, self.n)
        self.Ai, self.eA = _to_int(self.A)
        self.normA = Fraction(max(sum(abs(v) for v in row) for row in self.Ai.tolist())) * Fraction(2) ** self.eA       # ||A||_inf
        self._chol = None

    def _residual_int(self, Xi, ex, Bi, eb):
        """R 2^E = B 2^eb - A X 2^(eA + ex), exactly"""
        AX = self.Ai.dot(Xi)
        E = min(eb, self.eA + ex)
        sb, sa = eb - E, self.eA + ex - E
        R = np.empty(Bi.shape, dtype=object)
        R.ravel()[:] = [(bv << sb) - (av << sa) for bv, av in zip(Bi.ravel().tolist(), AX.ravel().tolist())]
        return R, E

    def _eta(self, R, E, Xi, ex, Bi, eb):
        """||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf) as an exact rational"""
        den = self.normA * _absmax(Xi) * Fraction(2) ** ex + _absmax(Bi) * Fraction(2) ** eb
        return Fraction(_absmax(R)) * Fraction(2) ** E / den if den else Fraction(0)

    def residual(self, x, b):
        """eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), every operation exact, rounded once at the end"""
        Xi, ex = _to_int(x)
        Bi, eb = _to_int(b)
        R, E = self._residual_int(Xi, ex, Bi, eb)
        return float(self._eta(R, E, Xi, ex, Bi, eb))

    def solve(self, b, max_steps=8, eta_stop=1e-45):
        """(x* rounded to fp64, exact eta of the unrounded iterate).  Refinement until the exact residual stops shrinking,
        falls below eta_stop, or max_steps corrections are in (a step shrinks it by about eps cond)"""
        if self._chol is None:
            self._chol = sla.cho_factor(self.A, lower=True)
        b = np.asarray(b, dtype=np.float64)
        Bi, eb = _to_int(b)
        Xi, ex = _to_int(sla.cho_solve(self._chol, b))
        best = None
        for step in range(max_steps + 1):
            R, E = self._residual_int(Xi, ex, Bi, eb)
            eta = self._eta(R, E, Xi, ex, Bi, eb)
            if best is not None and eta >= best[0]:
                break
            best = (eta, Xi, ex)
            if eta <= eta_stop or step == max_steps:
                break
            r = np.array([_to_float(v, E) for v in R.tolist()])
            Di, ed = _to_int(sla.cho_solve(self._chol, r))
            e2 = min(ex, ed)
            Xn = np.empty(Xi.shape, dtype=object)
            Xn[:] = [(xv << (ex - e2)) + (dv << (ed - e2)) for xv, dv in zip(Xi.tolist(), Di.tolist())]
            Xi, ex = Xn, e2
        eta, Xi, ex = best
        return np.array([_to_float(v, ex) for v in Xi.tolist()]), float(eta)


def exact_solve(A, b):
    """x* = A^-1 b rounded to fp64, and the exact relative residual of the unrounded iterate"""
    return (A if isinstance(A, ExactSystem) else ExactSystem(A)).solve(b)


def exact_residual(A, x, b):
    """eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf) in exact arithmetic"""
    return (A if isinstance(A, ExactSystem) else ExactSystem(A)).residual(x, b)


def forward_error(x, xs):
    """relative infinity-norm error of x against the reference xs"""
    return float(np.abs(np.asarray(x) - xs).max() / np.abs(xs).max())


# ---------------------------------------------------------------------------------------------------------------
# matrix families (seeded; every entry is what fp64 holds: the reference solves THAT matrix)
# ---------------------------------------------------------------------------------------------------------------
def spectrum(n, cond, seed=0):
    """Q diag(lambda) Q' symmetrised, lambda log-spaced from 1 down to 1 / cond; with two right-hand sides: b generic (its
    solution lies along the small eigenvalues, ||x|| ~ cond ||b|| / ||A||), b2 = fl(A z) for a generic z (||A|| ||x|| ~ ||b2||:
    the right-hand side on which a product with an explicit inverse shows its rounding)"""
    rng = np.random.default_rng([n, int(round(math.log10(cond))), seed])
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.logspace(0.0, -math.log10(cond), n)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    return A, rng.normal(size=n), A @ rng.normal(size=n)


def scaling(n, seed=0):
    """S = diag(2^k), k even in [-40, 40]: S A S and S b are exact, Cholesky's square roots of 4^k too -- the same problem
    through other exponents"""
    rng = np.random.default_rng([n, 4040, seed])
    return np.ldexp(1.0, 2 * rng.integers(-20, 21, n))


def ldl_integer(n, d, alone=(), seed=0):
    """blockdiag(L_i D_i L_i') with unit lower triangular L_i of small integers (blocks of 16) and the pivots d: in exact
    arithmetic the Cholesky pivots ARE d, and every entry is a small integer (exact in fp64).  The indices in `alone` are
    1 x 1 blocks of their own (A[p][p] = d[p] whatever its size)"""
    rng = np.random.default_rng([n, 77, seed])
    L = np.eye(n)
    for s in range(0, n, 16):
        e = min(s + 16, n)
        L[s:e, s:e] += np.tril(rng.integers(-1, 2, (e - s, e - s)), -1)
    for p in alone:
        L[p, :p] = 0.0
        L[p + 1:, p] = 0.0
    return (L * np.asarray(d, dtype=np.float64)) @ L.T


def diagonal(n, seed=0):
    """(a, b): the system diag(a) x = b with full 53-bit mantissas over [1, 4) and exponents 4^k, k in [-20, 20]"""
    rng = np.random.default_rng([n, 53, seed])
    return rng.uniform(1.0, 4.0, n) * np.ldexp(1.0, 2 * rng.integers(-20, 21, n)), rng.normal(size=n)


# x_i = y (y b_i) with y = fl(1 / sqrt(a_i)) to half an ulp (WaveFactor's third-order correction of v_rsq_f64 leaves 2^-20 of
# an ulp besides the final rounding; LAPACK: a correctly rounded sqrt and two divisions): four relative errors of u = 2^-53
DIAGONAL_BOUND = (1 + Fraction(1, 2 ** 53) * (1 + Fraction(1, 2 ** 20))) ** 4 - 1


def diagonal_error(a, b, x):
    """max_i |x_i - b_i / a_i| / |b_i / a_i|, exact (a rational)"""
    worst = Fraction(0)
    for ai, bi, xi in zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(x).tolist()):
        t = Fraction(bi) / Fraction(ai)
        worst = max(worst, abs(Fraction(xi) - t) / abs(t))
    return worst


def cond2(A):
    w = np.linalg.eigvalsh(A)
    return float(w[-1] / w[0])


def hessian_system(H, want=(1e8, 1e10)):
    """H (lower triangle of a smoothed dual Hessian; singular along uniform price scaling) + delta diag(H), delta the
    largest power of ten that puts cond_2 inside `want`.  Returns (lower triangle with a zero upper one, its symmetric
    completion, delta, cond_2)"""
    Hl = np.tril(np.asarray(H, dtype=np.float64))
    d = np.diag(Hl).copy()
    for k in range(-2, -17, -1):
        delta = 10.0 ** k
        L = Hl + np.diag(delta * d)
        S = L + np.tril(L, -1).T
        c = cond2(S)
        if want[0] <= c <= want[1]:
            return L, S, delta, c
    raise AssertionError("no shift delta diag(H) puts cond_2 inside [%g, %g]" % want)


# ---------------------------------------------------------------------------------------------------------------
# cases, references (cached: computed once per process), ceilings
# ---------------------------------------------------------------------------------------------------------------
def case_ids():
    """(family, n, cond): what test_gpu_cholesky.py runs in every mode"""
    out = [("spectrum", n, c) for c in CONDS for n in SIZES]
    out.append(("spectrum", N_STRIPS, 1e8))
    out += [("scaled", n, 1e8) for n in SIZES]
    return out


def case_name(cid):
    return "%s-n%d-cond1e%d" % (cid[0], cid[1], int(round(math.log10(cid[2]))))


class Reference:
    """A x = b (and b2) with their exact solutions, LAPACK's answers and figures on the same systems"""

    def __init__(self, A, b, b2, cond=None):
        self.A, self.b, self.b2 = A, b, b2
        self.n = len(b)
        self.cond = cond2(A) if cond is None else cond
        self.sys = ExactSystem(A)
        self.xs, self.eta_star = self.sys.solve(b)
        self.xs2, self.eta_star2 = self.sys.solve(b2)
        c = sla.cho_factor(A, lower=True)
        self.x_lapack, self.x2_lapack = sla.cho_solve(c, b), sla.cho_solve(c, b2)
        self.e_lapack, self.e2_lapack = forward_error(self.x_lapack, self.xs), forward_error(self.x2_lapack, self.xs2)
        self.eta_lapack, self.eta2_lapack = self.sys.residual(self.x_lapack, b), self.sys.residual(self.x2_lapack, b2)

    def eta(self, x):
        return self.sys.residual(x, self.b)

    def eta2(self, x2):
        return self.sys.residual(x2, self.b2)


def lapack_has_room(ref, factor=10.0):
    """fp64 LAPACK inside the forward ceiling (both right-hand sides) and the tighter backward ceiling by `factor`"""
    fc, ec = forward_ceiling(ref.n, ref.cond), eta_ceiling(ref.n, ref.cond, "classic")
    return factor * max(ref.e_lapack, ref.e2_lapack) <= fc and factor * max(ref.eta_lapack, ref.eta2_lapack) <= ec


@functools.lru_cache(maxsize=None)
def reference(family, n, cond):
    """The case's system with its exact solutions.  The draw is the first seed 0, 1, 2 .. on which fp64 LAPACK has a factor
    10 of room under the ceilings: at n = 2 the ceilings are 2 eps (cond) and a single unlucky rounding of LAPACK's own
    takes a fifth of that (seed 0 at cond 1e8: room 5.6), which says nothing about a solver.  The rule looks at the host's
    LAPACK only, never at the device.  `scaled` shares `spectrum`'s matrix and reference: the device is handed S A S, S b and
    its answer is scaled back (exactly), so every figure is taken on the unscaled problem"""
    for seed in range(8):
        ref = Reference(*spectrum(n, cond, seed))
        ref.seed = seed
        if lapack_has_room(ref):
            return ref
    raise AssertionError("no draw of spectrum(%d, %g) leaves LAPACK a factor 10 under the ceilings" % (n, cond))


def forward_ceiling(n, cond):
    """the textbook forward bound of a backward stable solve: n eps cond_2(A)"""
    return n * EPS * cond


def eta_ceiling(n, cond, backsub):
    """backward error: n eps for the triangular back substitution; the product with the explicit inverse factor is only
    conditionally backward stable: n eps sqrt(cond_2(A))"""
    return n * EPS * (1.0 if backsub == "classic" else math.sqrt(cond))


def scaled_system(ref, n):
    """what the device is handed for a `scaled` case: (S A S, S b, S b2, S); x = S x_scaled undoes it exactly"""
    s = scaling(n)
    return ref.A * s[:, None] * s[None, :], ref.b * s, ref.b2 * s, s


HESSIAN_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_hessian_60.npy")


@functools.lru_cache(maxsize=None)
def hessian_golden():
    """the `hessian` case on a RECORDED matrix: the lower triangle of the smoothed Hessian of helpers.mixed_network(0, 60, 300)
    at helpers.smoothed_hessian_point, mu = 1e-8, as oracle/barrier_np.py states it.  Recorded, because the device's own
    comes out of fp64 atomics and differs in its last bits from run to run -- and on a matrix with ONE tiny eigenvalue the
    forward error of any solver is one random scalar, so its ratio to LAPACK's swings by a factor 60 between runs (measured:
    docs/cholesky_accuracy.md).  The CPU and GPU files tie the record to the restatement and to the device's evaluation"""
    return hessian_reference(np.load(HESSIAN_GOLDEN))


def hessian_reference(H):
    """the `hessian` case around a smoothed Hessian H (lower triangle): Reference of the symmetric completion of
    H + delta diag(H), with .L the lower-triangular input the solver would pass and .delta the shift"""
    L, S, delta, c = hessian_system(H)
    rng = np.random.default_rng([len(S), 8])
    ref = Reference(S, rng.normal(size=len(S)), S @ rng.normal(size=len(S)), c)
    ref.L, ref.delta = L, delta
    return ref
