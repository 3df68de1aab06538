"""The 50-digit reference of re-quoting a held route (docs/requote.md) and the per-pool bound its tests share.

roots(net, held) finds, for every trading pool of every bucket, the root s* of the pool's slack on x_j(s) = (R_j + gamma Delta_j) - s Lambda_j
in mpmath at 50 digits, from the fp64 inputs as they stand (a bracket on [0, s_cap] kept by sign, Newton steps with the exact
derivative while they stay inside it, to a slack below 1e-42 of its terms), and the tolerance on an fp64 root DERIVED from the slack expression's rounding:

    tol_s = N 2^-52 M / |d slack / d s| (s*)  +  2^-52 s*

M: the sum of the magnitudes of the slack's terms at s*, each with the first-order amplification of the roundings that feed it -- a leg
x_j = up_j - s L_j carries (up_j + s L_j) 2^-52 absolutely, so (up_j + s L_j) / x_j relatively:
    log        sum_j w_j (|log(x_j / R_j)| + (up_j + s L_j) / x_j)
    stable     (sum_j (up_j + s L_j) + c_x sum_j (up_j + s L_j) / x_j + |phi(x)| + sum R + c_R + |phi(R)|) / (sum R + c_R)
    pow        (sum_j x_j^e (1 + e (up_j + s L_j) / x_j) + 2 sum R_j^e) / sum R_j^e
N: the operations on the longest chain from an input to the slack: gamma Delta, R +, s Lambda, up -, the quotient or power, the
function, the weight, K sums, the final difference and quotient: 8 + K.  Everything is evaluated in mpmath.  The second term is the
stopping rule's: the search ends on the double below a sign change, one ulp from it.
The constant-sum kinds are a closed form, s = gamma sum Delta / sum Lambda: 2 (K - 1) additions, a product and a quotient, each within
2^-52: tol_s = (2 K + 1) 2^-52 s*.  A capped pool returns s_cap = min (R_j + gamma Delta_j) / Lambda_j: two roundings in the numerator,
one in the quotient, at most six steps down of an ulp each: tol_s = 10 2^-52 s_cap."""
import mpmath
import numpy as np

from cfmm.problem import audit_buckets

U = 2.0 ** -52


def _mp(x):
    return mpmath.mpf(float(x))


def _slack(cls, R, up, L, w, par, s):
    """(slack, d slack / d s, magnitude M) of one pool at s, all mpmath"""
    k = len(R)
    x = [up[j] - s * L[j] for j in range(k)]
    amp = [(up[j] + s * L[j]) / x[j] for j in range(k)]
    if cls == "log":
        logs = [mpmath.log(x[j] / R[j]) for j in range(k)]
        F = sum(w[j] * logs[j] for j in range(k))
        dF = -sum(w[j] * L[j] / x[j] for j in range(k))
        M = sum(w[j] * (abs(logs[j]) + amp[j]) for j in range(k))
        return F, dF, M
    if cls == "stable":
        Px, PR = mpmath.fprod(x), mpmath.fprod(R)
        cx, cR = par / Px, par / PR
        SR = sum(R)
        phx, phR = sum(x) - cx, SR - cR
        F = (phx - phR) / (SR + cR)
        dF = -(sum(L) + cx * sum(L[j] / x[j] for j in range(k))) / (SR + cR)
        M = (sum(up[j] + s * L[j] for j in range(k)) + cx * sum(amp) + abs(phx) + SR + cR + abs(phR)) / (SR + cR)
        return F, dF, M
    if cls == "pow":
        fx = [x[j] ** par for j in range(k)]
        fR = sum(R[j] ** par for j in range(k))
        F = (sum(fx) - fR) / fR
        dF = -sum(par * fx[j] / x[j] * L[j] for j in range(k)) / fR
        M = (sum(fx[j] * (1 + par * amp[j]) for j in range(k)) + 2 * fR) / fR
        return F, dF, M
    raise ValueError(cls)


def pool_root(cls, R, g, D, L, w=None, par=None):
    """(s*, tol_s, ftol, kind) of one pool from fp64 inputs: kind 'root' | 'capped' | 'one' (sum Lambda = 0) | 'zero' (sum Delta = 0);
    ftol: the bound in units of the slack, N 2^-52 M + 2^-52 s |d slack / d s| (0 where no root is searched)"""
    mpmath.mp.dps = 50
    k = len(R)
    R, D, L = [_mp(v) for v in R], [_mp(v) for v in D], [_mp(v) for v in L]
    g = _mp(g)
    w = [_mp(v) for v in w] if w is not None else None
    par = _mp(par) if par is not None else None
    up = [R[j] + g * D[j] for j in range(k)]
    if sum(L) == 0:
        return 1.0, 0.0, 0.0, "one"
    if sum(D) == 0:
        return 0.0, 0.0, 0.0, "zero"
    cap = min(up[j] / L[j] for j in range(k) if L[j] > 0)
    if cls == "sum":
        s = g * sum(D) / sum(L)
        if s > cap:
            return float(cap), 10 * U * float(cap), 0.0, "capped"
        return float(s), (2 * k + 1) * U * float(s), 0.0, "root"
    lo, hi = mpmath.mpf(0), cap
    # (the slack at the cap itself: -inf for log and stable; the power sum's is finite and may still be >= 0)
    if cls == "pow":
        xs = [up[j] - cap * L[j] for j in range(k)]
        if sum((v if v > 0 else mpmath.mpf(0)) ** par for v in xs) >= sum(R[j] ** par for j in range(k)):
            return float(cap), 10 * U * float(cap), 0.0, "capped"
    # a bracket kept by sign; Newton steps with the exact derivative from the last point while they stay inside it, else its midpoint
    s = (lo + hi) / 2
    for _ in range(400):
        F, dF, M = _slack(cls, R, up, L, w, par, s)
        if abs(F) <= mpmath.mpf(10) ** -42 * max(M, 1):
            break
        if F >= 0:
            lo = s
        else:
            hi = s
        t = s - F / dF
        s = t if lo < t < hi else (lo + hi) / 2
    else:
        raise AssertionError(f"the 50-digit root search did not converge ({cls})")
    ftol = (8 + k) * U * M + U * s * abs(dF)
    tol = (8 + k) * U * M / abs(dF) + U * s
    return float(s), float(tol), float(ftol), "root"


def roots(net, held, every=1):
    """{key: dict(s [m], tol [m], ftol [m] (the bound in units of the slack), kind [m] of str, trading [m] of bool)} for every bucket of
    `net` under the held tenders; every > 1: only the positions 0, every, 2 every, .. are solved (the others stay 'idle')"""
    out = {}
    for b in audit_buckets(net):
        D, L = (np.asarray(a, dtype=np.float64) for a in held[b["key"]])
        m = b["R"].shape[1]
        s, tol, ftol, kind = np.ones(m), np.zeros(m), np.zeros(m), ["idle"] * m
        trading = ((D != 0.0) | (L != 0.0)).any(axis=0)
        for i in np.flatnonzero(trading).tolist():
            if i % every:
                continue
            w = b["w"][:, i] if b["cls"] == "log" else None
            par = b["alpha"][i] if b["cls"] == "stable" else (b["e"][i] if b["cls"] == "pow" else None)
            s[i], tol[i], ftol[i], kind[i] = pool_root(b["cls"], b["R"][:, i], b["fee"][i], D[:, i], L[:, i], w, par)
        out[b["key"]] = dict(s=s, tol=tol, ftol=ftol, kind=kind, trading=trading)
    return out


def moved(net, rng, spread=0.05):
    """a copy of a packed network with every reserve multiplied by exp(u), u uniform in +-spread; per bucket one pool in eight left
    untouched (positions 0, 8, ..), one in eight shrunk 100 times (positions 3, 11, ..), and the first pool's fee changed.  Returns
    (network, {key: untouched positions})"""
    import copy
    out = copy.deepcopy({k: v for k, v in net.items() if not k.startswith("_")})
    still = {}

    def move(R, fee):
        m = R.shape[1]
        f = np.exp(rng.uniform(-spread, spread, R.shape))
        f[:, 0::8] = 1.0
        f[:, 3::8] *= 0.01
        R *= f
        if m > 1:
            fee[1] = 0.5 * (fee[1] + 1.0) if fee[1] < 1.0 else 0.999
        return np.arange(0, m, 8)

    for b in audit_buckets(out):
        key = b["key"]
        if isinstance(key, str):
            bb = out[key]
            R = np.stack([bb["Ra"], bb["Rb"]])
            still[key] = move(R, bb["fee"])
            bb["Ra"][:], bb["Rb"][:] = R[0], R[1]
        elif isinstance(key, tuple):
            still[key] = move(out["gk"][key]["R"], out["gk"][key]["fee"])
        else:
            still[key] = move(out["gn"][key]["R"], out["gn"][key]["fee"])
    return out, still
