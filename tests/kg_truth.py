"""Test infrastructure for the knowledge gradient (gpbo_kg_argbest / suggest_kg; never imported by the product): the fp64 NumPy
restatement of the device's arithmetic (`kg_lines`, `kg_values`: Frazier's sum over the upper envelope), the same quantity in
mpmath at 50 digits from the definition (`kg_lines_truth`, `kg_truth`: per envelope piece the integral of (a + b z) phi(z), the
covariance from an mpmath solve), the candidate x point posterior covariance on matern_family_truth's kernels (`posterior_cov`),
suggest_kg's reference-point rule (`reference_points`) and KgFakeEngine.

    lines (a_0, b_0) = (mu(x), y_std max(v - w, 0) / den),  (a_j, b_j) = (mu_j, y_std cov_j(x) / den),  den = sqrt(v + lambda - w)
    KG(x) = E_Z[max_j (a_j + b_j Z)] - max_j a_j,   v = (sd / y_std)^2
"""
import numpy as np
from scipy import special
from scipy.linalg import cho_solve, cholesky

import matern_family_truth as F
from helpers import FakeEngine
from mes_truth import argbest

BAR = 1e-9                   # the project's bar, on |error| / scale(x), scale(x) = max_j |b_j|
F_ZERO_BELOW = -40.0


def f(z):
    """f(z) = phi(z) + z Phi(z) for z <= 0, as the device forms it (0 below -40)"""
    z = float(z)
    if z < F_ZERO_BELOW:
        return 0.0
    return float(np.exp(-(z * z) / 2.0) / 2.50662827463100050242 + z * special.ndtr(z))


def envelope(a, b):
    """The upper envelope of the lines a + b z as the device builds it: ordered by (slope, intercept), the largest intercept of a
    slope kept, a stack with pops while the new line takes over no later than the top did.  Returns (a, b) of the envelope."""
    order = np.lexsort((a, b))
    a, b = np.asarray(a, dtype=np.float64)[order], np.asarray(b, dtype=np.float64)[order]
    sa, sb = [], []
    n = len(a)
    for i in range(n):
        if i + 1 < n and b[i + 1] == b[i]:
            continue
        while len(sa) >= 2:
            with np.errstate(all="ignore"):
                c_top = (sa[-2] - sa[-1]) / (sb[-1] - sb[-2])
                c_new = (sa[-1] - a[i]) / (b[i] - sb[-1])
            if not c_new <= c_top:
                break
            sa.pop()
            sb.pop()
        sa.append(a[i])
        sb.append(b[i])
    return np.array(sa), np.array(sb)


def kg_lines(a, b):
    """E[max_j (a_j + b_j Z)] - max_j a_j by Frazier's sum; NaN for a set with a NaN or infinite entry"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return float("nan")
    sa, sb = envelope(a, b)
    kg = 0.0
    for k in range(1, len(sa)):
        db = sb[k] - sb[k - 1]
        with np.errstate(all="ignore"):
            c = (sa[k - 1] - sa[k]) / db
        kg = kg + db * f(-abs(c))
    return float(kg)


def lines(mu, sd, cov, mu_points, y_std=1.0, lam=0.0, white=0.0):
    """(a (M, J + 1), b (M, J + 1), den (M,)) of the candidates: mu, sd (M,) raw units, cov (M, J) normalised latent covariance"""
    mu, sd, cov = np.asarray(mu, dtype=np.float64), np.asarray(sd, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    q = sd / y_std
    v = q * q
    with np.errstate(all="ignore"):
        den = np.sqrt((v + lam) - white)
        b0 = (y_std * np.maximum(v - white, 0.0)) / den
        bj = (y_std * cov) / den[:, None]
    a = np.column_stack([mu, np.broadcast_to(np.asarray(mu_points, dtype=np.float64), cov.shape)])
    return a, np.column_stack([b0, bj]), den


def kg_values(mu, sd, cov, mu_points, y_std=1.0, lam=0.0, white=0.0, return_scale=False):
    """KG (M,) with the device's conventions: den == 0 gives 0, a NaN mu / sd or line NaN.  scale (M,) = max_j |b_j|."""
    a, b, den = lines(mu, sd, cov, mu_points, y_std, lam, white)
    out = np.empty(a.shape[0])
    for i in range(a.shape[0]):
        if np.isnan(mu[i]) or np.isnan(sd[i]):
            out[i] = np.nan
        elif den[i] == 0.0:
            out[i] = 0.0
        else:
            out[i] = kg_lines(a[i], b[i])
    if return_scale:
        with np.errstate(all="ignore"):
            return out, np.nanmax(np.abs(np.where(np.isfinite(b), b, np.nan)), axis=1)
    return out


def kg_lines_truth(a, b, digits=50):
    """The same at `digits` digits from the definition: over each envelope piece [c_k, c_k+1] the integral of (a + b z) phi(z) dz
    = a (Phi(c_k+1) - Phi(c_k)) + b (phi(c_k) - phi(c_k+1)), summed, minus max a.  The envelope is found in mpmath too."""
    import mpmath as mp

    with mp.workdps(digits):
        return _mp_lines([mp.mpf(float(v)) for v in a], [mp.mpf(float(v)) for v in b])


def posterior_cov(kind, X, ls, noise, Xc, A):
    """cov (M, J): the latent posterior covariance k(Xc, A) - k(Xc, X) K^-1 k(X, A) of the unit
    model K = k(X, X) + noise I, fp64 (Cholesky solve)"""
    K = F.kernel_matrix(kind, X, None, ls)
    K[np.diag_indices_from(K)] += noise
    L = cholesky(K, lower=True, check_finite=False)
    B = cho_solve((L, True), F.kernel_matrix(kind, X, A, ls), check_finite=False)
    return F.kernel_matrix(kind, Xc, A, ls) - F.kernel_matrix(kind, Xc, X, ls) @ B


def _mp_kernel(kind, r):
    import mpmath as mp

    if kind == F.RBF:
        return mp.exp(-r * r / 2)
    if kind == F.MATERN25:
        s = mp.sqrt(5) * r
        return (1 + s + s * s / 3) * mp.exp(-s)
    if kind == F.MATERN15:
        s = mp.sqrt(3) * r
        return (1 + s) * mp.exp(-s)
    return mp.exp(-r)


def kg_truth(kind, X, yn, ls, noise, Xc, A, y_mean=0.0, y_std=1.0, digits=50):
    """KG of the few candidates Xc over the points A for a UNIT model, everything in mpmath at `digits` digits: the solve, the
    posterior mean / variance / covariances, the envelope and the integral.  (KG (M,), scale (M,))"""
    import mpmath as mp

    with mp.workdps(digits):
        ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))

        def kmat(P, Q):
            return mp.matrix([[_mp_kernel(kind, mp.sqrt(sum(((mp.mpf(float(p[t])) - mp.mpf(float(q[t]))) / mp.mpf(float(ls[t]))) ** 2
                                                             for t in range(len(ls))))) for q in Q] for p in P])

        N = X.shape[0]
        K = kmat(X, X)
        for i in range(N):
            K[i, i] += mp.mpf(float(noise))
        P = np.vstack([Xc, A])
        Ks = kmat(X, P)                                   # (N, M + J)
        sol = mp.inverse(K) * Ks                          # K^-1 k(X, P)
        alpha = mp.lu_solve(K, mp.matrix([mp.mpf(float(v)) for v in yn]))
        M, J = Xc.shape[0], A.shape[0]
        mean = [mp.mpf(float(y_std)) * sum(Ks[i, c] * alpha[i] for i in range(N)) + mp.mpf(float(y_mean)) for c in range(M + J)]
        kpp = kmat(Xc, P)                                 # (M, M + J)
        out, scale = [], []
        for c in range(M):
            cov = [kpp[c, q] - sum(Ks[i, c] * sol[i, q] for i in range(N)) for q in range(M + J)]
            v = cov[c]
            den = mp.sqrt(v + mp.mpf(float(noise)))
            a = [mean[c]] + [mean[M + j] for j in range(J)]
            b = [mp.mpf(float(y_std)) * v / den] + [mp.mpf(float(y_std)) * cov[M + j] / den for j in range(J)]
            out.append(_mp_lines(a, b))
            scale.append(float(max(abs(x) for x in b)))
        return np.array(out), np.array(scale)


def _mp_lines(a, b):
    import mpmath as mp

    best = {}
    for av, bv in zip(a, b):
        best[bv] = av if bv not in best else max(best[bv], av)
    hull = []
    for bv in sorted(best):
        av = best[bv]
        while len(hull) >= 2:
            (b1, a1), (b2, a2) = hull[-1], hull[-2]
            if (a1 - av) / (bv - b1) <= (a2 - a1) / (b1 - b2):
                hull.pop()
            else:
                break
        hull.append((bv, av))
    cuts = [-mp.inf] + [(hull[k - 1][1] - hull[k][1]) / (hull[k][0] - hull[k - 1][0]) for k in range(1, len(hull))] + [mp.inf]
    total = mp.mpf(0)
    for k, (bv, av) in enumerate(hull):
        total += av * (mp.ncdf(cuts[k + 1]) - mp.ncdf(cuts[k])) + bv * (mp.npdf(cuts[k]) - mp.npdf(cuts[k + 1]))
    return float(total - max(a))


def reference_points(mu, n_points):
    """suggest_kg's rule on a mean vector: the ceil(J / 2) highest means (ties to the lowest index) in that order, then the first
    floor(J / 2) indices not among them"""
    mu = np.asarray(mu, dtype=np.float64)
    n_top = (n_points + 1) // 2
    top = list(np.lexsort((np.arange(len(mu)), -mu))[:n_top])
    rest = [i for i in range(len(mu)) if i not in set(top)][:n_points - n_top]
    return np.array(top + rest, dtype=np.int64)


class KgFakeEngine(FakeEngine):
    """tests/helpers.FakeEngine (TEST DOUBLE ONLY) + kg_argbest over `kg_values` on the resident posterior (unit models)."""

    def kg_argbest(self, points, k_seeds=0, index_offset=0, y_mean=0.0, y_std=1.0, return_values=False, return_point_means=False):
        points = np.asarray(points, dtype=np.float64)
        self.calls.append(("kg_argbest", points.shape[0], k_seeds))
        self.points = points.copy()
        if points.ndim != 2 or not (1 <= points.shape[0] <= 64) or not np.isfinite(points).all():
            raise ValueError("kg_argbest: bad points")
        X, kind, ls, noise = self.inputs[0]
        mu, sd = self.post[0]
        cov = posterior_cov(kind, X, ls, noise, self.Xc, points)
        mu_points = y_std * (F.kernel_matrix(kind, points, X, ls) @ self.models[0].alpha) + y_mean
        ys = -kg_values(mu, sd, cov, mu_points, y_std, noise, 0.0)
        bi, bv, si, sv = argbest(ys, k_seeds, index_offset)
        out = (bi, bv, si, sv, (ys if return_values else None))
        return out + (mu_points,) if return_point_means else out
