"""Truth for joint entropy search (gpje_jes_argbest; tests only, never imported by the product): include/gpje.h restated in NumPy.

`r2`: the variance ratio of a normal truncated from above, 1 - b h - h^2 with h = phi(b) / Phi(b), in mpmath at 50 digits from the
definition.  `R2_GRID`: the values r2 is tested over on the device.
`parts`: cov (M, S) as kg_truth.posterior_cov, m_s and p_s of the unit model from one Cholesky written out, so that it runs in
np.longdouble too.  `jes`: a(x) (M,) from the candidates' mu / sd (raw units), cov times c, and the samples' m, c p, fn."""
import mpmath
import numpy as np

import matern_family_truth as F

_EDGES = [-1.0, -2.0, -3.0, -6.0, -10.0]                         # include/gpje.h: every boundary between two of r2's ranges and depths
R2_GRID = np.array([40, 8, 1, 0, -0.5, -28, -1e3, -1e8, -1e150] + _EDGES + [np.nextafter(b, s) for b in _EDGES for s in (-np.inf, np.inf)])


def parts(kind, X, yn, ls, eta, Xc, xs, dtype=np.float64):
    """(cov (M, S), m (S,), p (S,)) of the unit model K' = k(X, X) + eta I, the factorisation and the solves in `dtype`"""
    K = F.kernel_matrix(kind, X, None, ls).astype(dtype)
    K[np.diag_indices_from(K)] += dtype(eta)
    B = np.column_stack([F.kernel_matrix(kind, X, xs, ls), F.kernel_matrix(kind, X, Xc, ls), yn]).astype(dtype)
    L = np.zeros_like(K)
    for j in range(len(K)):                                      # Cholesky, then L^-1 B by forward substitution
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    for i in range(len(K)):
        B[i] = (B[i] - L[i, :i] @ B[:i]) / L[i, i]
    S = len(xs)
    Ws, Wc, wy = B[:, :S], B[:, S:-1], B[:, -1]
    return F.kernel_matrix(kind, Xc, xs, ls).astype(dtype) - Wc.T @ Ws, Ws.T @ wy, 1 - (Ws * Ws).sum(axis=0)


def r2(beta):
    if beta == np.inf:
        return 1.0
    # in the lower tail the three terms cancel like beta^4 and exp(-beta^2 / 2) is as exact as beta^2 is: carry those digits too
    with mpmath.workdps(50 + (int(6 * np.log10(-beta)) + 10 if beta < -1 else 0)):
        b = mpmath.mpf(float(beta))
        h = mpmath.npdf(b) / (mpmath.erfc(-b / mpmath.sqrt(2)) / 2)
        return float(1 - b * h - h * h)


def jes(mu, sd, cov, m, p, fn, c, w, lam, y_mean, y_std, r2_of=r2):
    """a(x) of include/gpje.h; cov, m, p, fn in normalised units, lam = c eta"""
    cov, m, p = (np.asarray(t, dtype=np.float64) for t in (cov, m, p))
    S = cov.shape[1]
    v = (sd / y_std) ** 2
    vl, vo, mn = np.maximum(v - w, 0.0), (v + lam) - w, (mu - y_mean) / y_std
    rho = np.where(p > 0, 1.0 / np.where(p > 0, p, 1.0), 0.0)
    mu_s = mn[:, None] + cov * (rho * (fn - m))
    vl_s = np.maximum(vl[:, None] - cov ** 2 * rho, 0.0)
    acc = np.zeros(len(mu))
    with np.errstate(all="ignore"):
        beta = (fn - mu_s) / np.sqrt(vl_s)
        for s in range(S):
            ratio = np.array([np.nan if (z == 0 or np.isnan(b)) else r2_of(b) for b, z in zip(beta[:, s], vl_s[:, s])])
            acc = acc + np.where(vl_s[:, s] == 0, 0.5 * np.log(lam), 0.5 * np.log(vl_s[:, s] * ratio + lam))
        a = 0.5 * np.log(vo) - acc / S
    return np.where(np.isnan(mu) | np.isnan(sd), np.nan, a)
