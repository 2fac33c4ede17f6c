"""Test infrastructure for the SUR excursion-set acquisition (gpls_sur_argbest / suggest_levelset; never imported by the product): a
plain reference of include/gpls.h's formulas from X, y, theta alone — SciPy's fp64 Cholesky, one step of iterative refinement and all
the GP algebra behind it in `dtype` (np.longdouble, or np.float64 to measure the reference's own spread), and G by 40-node
Gauss-Legendre on [0, asin r2] in the theta form, which shares neither the substitution nor the rule of the device's."""
import numpy as np
from scipy import special
from scipy.linalg import cho_solve, cholesky

import matern_family_truth as F

_X40, _W40 = np.polynomial.legendre.leggauss(40)


def G(h2, r2, dtype=np.longdouble):
    """(1 / 2 pi) int_0^{asin r2} exp(-h2 / (1 + sin theta)) d theta = Phi(h) Phi(-h) - Phi2(h, -h; -r2), broadcast over h2 and r2"""
    h2, r2 = np.asarray(h2, dtype=dtype), np.asarray(r2, dtype=dtype)
    phi = np.arcsin(r2)
    total = np.zeros(np.broadcast(h2, r2).shape, dtype=dtype)
    for x, w in zip(_X40.astype(dtype), _W40.astype(dtype)):
        total = total + w * np.exp(-h2 / (1 + np.sin(phi * (x + 1) / 2)))
    return total * (phi / 2) / (8 * np.arctan(dtype(1)))      # the rule's half-width; 2 pi


def _kernel(kind, P, Q, ls, dtype):
    P, Q = np.asarray(P, dtype=dtype) / ls, np.asarray(Q, dtype=dtype) / ls
    return F.kernel_value(kind, np.sqrt(((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1)))


def sur(kind, X, yn, ls, alpha, Xc, A, omega, level, y_mean, y_std, c=1.0, w=0.0, dtype=np.longdouble):
    """(SUR (M,), p (J,), uncertainty) of the model c k + (w + alpha) I fitted to (X, yn): one noisy observation at each row of Xc,
    integration points A with weights omega, in normalised units as include/gpls.h"""
    ls, eta = np.asarray(ls, dtype=dtype), dtype(w + alpha) / dtype(c)
    K = _kernel(kind, X, X, ls, dtype)
    K[np.diag_indices_from(K)] = 1 + eta
    L = cholesky(K.astype(np.float64), lower=True, check_finite=False)

    def solve(B):
        S = cho_solve((L, True), B.astype(np.float64), check_finite=False).astype(dtype)
        return S + cho_solve((L, True), (B - K @ S).astype(np.float64), check_finite=False).astype(dtype)

    kA, kC = _kernel(kind, X, A, ls, dtype), _kernel(kind, X, Xc, ls, dtype)      # (N, J), (N, M)
    SA = solve(kA)
    m = kA.T @ solve(np.asarray(yn, dtype=dtype)[:, None])[:, 0]
    s2 = c * np.maximum(1 - (kA * SA).sum(0), 0)
    cov = c * (_kernel(kind, Xc, A, ls, dtype) - kC.T @ SA)                        # (M, J)
    den2 = c * np.maximum(1 - (kC * solve(kC)).sum(0), 0) + dtype(alpha) + dtype(w)      # v + lambda - w, v = latent + w
    h = (m - (dtype(level) - dtype(y_mean)) / dtype(y_std)) / np.sqrt(s2)
    p = special.ndtr(h.astype(np.float64))
    omega = np.asarray(omega, dtype=dtype)
    r2 = np.minimum(cov * cov / (den2[:, None] * s2[None, :]), 1)
    return (G(h * h, r2, dtype) @ omega).astype(np.float64), p, float((omega * (p * (1 - p))).sum())
