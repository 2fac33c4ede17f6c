"""Test infrastructure for posterior function draws (gpbo_sample_paths / suggest_thompson; never imported by the product): the
formulas of include/gpbo.h restated three times over tests/matern_family_truth.py's four kernel kinds, and PathsFakeEngine.

With c = the model's amplitude (1 for a unit model), eta = (white + alpha) / c the unit model's noise, xs = x / length_scale,
fs = sqrt(2 c / F):
    phi_j(x) = cos(2 pi (omega_j . xs + phase_j))          omega in turns per unit of the length-scaled input, phase in turns
    g_s(x)   = fs sum_j weights[s, j] phi_j(x)
    u_s      = g_s(X) + eps_s
    v_s      = (K + eta I)^-1 (y_n - u_s)                   K the UNIT kernel matrix
    f_s(x)   = y_std (g_s(x) + k(xs, Xs) . v_s) + y_mean    the latent function: no white part
`paths_cho`   fp64, v by cho_solve;
`paths_winv`  fp64, v = alpha - W^T (W u) through an explicit W = L^-1, the device's route;
`paths_mp`    50-digit mpmath (as tests/acq_truth.py), for tiny cases: the truth the two fp64 routes' own error is measured against.
All return values (S, M).  The fp64 routes reduce the feature argument as the device does (r = t - rint(t): exact in turns)."""
import mpmath as mp
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

import matern_family_truth as F

_ctx = mp.mp.clone()
_ctx.dps = 50


def features(omega, phase, Xs):
    """phi (n, F) at length-scaled points Xs (n, d)"""
    t = np.asarray(Xs, dtype=np.float64) @ np.asarray(omega, dtype=np.float64).T + np.asarray(phase, dtype=np.float64)[None, :]
    return np.cos(2.0 * np.pi * (t - np.rint(t)))


def _parts(kind, X, length_scale, eta, amplitude, omega, phase, weights, eps, Xc):
    ls = np.broadcast_to(np.asarray(length_scale, dtype=np.float64), (np.shape(X)[1],))
    X = np.asarray(X, dtype=np.float64)
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, X.shape[1])
    Fn = np.shape(omega)[0]
    fs = np.sqrt(2.0 * amplitude / Fn)
    w = np.asarray(weights, dtype=np.float64)
    U = fs * (features(omega, phase, X / ls) @ w.T) + np.asarray(eps, dtype=np.float64).T         # (N, S)
    Gc = fs * (features(omega, phase, Xc / ls) @ w.T)                                              # (M, S)
    K = F.kernel_matrix(kind, X, None, ls)
    K[np.diag_indices_from(K)] += eta
    Kt = F.kernel_matrix(kind, Xc, X, ls)
    return U, Gc, K, Kt


def paths_cho(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, Xc, y_mean=0.0, y_std=1.0, amplitude=1.0):
    U, Gc, K, Kt = _parts(kind, X, length_scale, eta, amplitude, omega, phase, weights, eps, Xc)
    L = cholesky(K, lower=True, check_finite=False)
    V = cho_solve((L, True), np.asarray(y_norm, dtype=np.float64)[:, None] - U, check_finite=False)
    return (y_std * (Gc + Kt @ V) + y_mean).T


def path_weights(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, amplitude=1.0):
    """V (N, S) = (K + eta I)^-1 (y_n - u_s), by cho_solve"""
    U, _, K, _ = _parts(kind, X, length_scale, eta, amplitude, omega, phase, weights, eps, np.asarray(X)[:1])
    L = cholesky(K, lower=True, check_finite=False)
    return cho_solve((L, True), np.asarray(y_norm, dtype=np.float64)[:, None] - U, check_finite=False)


def paths_winv(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, Xc, y_mean=0.0, y_std=1.0, amplitude=1.0):
    U, Gc, K, Kt = _parts(kind, X, length_scale, eta, amplitude, omega, phase, weights, eps, Xc)
    L = cholesky(K, lower=True, check_finite=False)
    W = solve_triangular(L, np.eye(L.shape[0]), lower=True, check_finite=False)
    alpha = W.T @ (W @ np.asarray(y_norm, dtype=np.float64))
    V = alpha[:, None] - W.T @ (W @ U)
    return (y_std * (Gc + Kt @ V) + y_mean).T


def posterior_mean(kind, X, y_norm, length_scale, eta, Xc, y_mean=0.0, y_std=1.0):
    """the paths with zero weights and zero noise draws"""
    z = np.zeros((1, 1))
    return paths_cho(kind, X, y_norm, length_scale, eta, np.zeros((1, np.shape(X)[1])), np.zeros(1), z, np.zeros((1, np.shape(X)[0])),
                     Xc, y_mean, y_std)[0]


def _mp_kernel(kind, r2):
    r = _ctx.sqrt(r2)
    if kind == F.RBF:
        return _ctx.exp(-r2 / 2)
    if kind == F.MATERN25:
        s = _ctx.sqrt(5) * r
        return (1 + s + s * s / 3) * _ctx.exp(-s)
    if kind == F.MATERN15:
        s = _ctx.sqrt(3) * r
        return (1 + s) * _ctx.exp(-s)
    if kind == F.MATERN05:
        return _ctx.exp(-r)
    raise ValueError(f"unsupported kernel kind {kind}")


def paths_mp(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, Xc, y_mean=0.0, y_std=1.0, amplitude=1.0):
    """The 50-digit truth, rounded to fp64 at the end.  Every fp64 INPUT is taken as given (the length-scaled coordinate is the
    exact quotient of the two doubles)."""
    m = _ctx.mpf
    X = np.asarray(X, dtype=np.float64)
    N, d = X.shape
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, d)
    M, Fn, S = Xc.shape[0], np.shape(omega)[0], np.shape(weights)[0]
    ls = [m(float(v)) for v in np.broadcast_to(np.asarray(length_scale, dtype=np.float64), (d,))]
    Xs = [[m(float(X[i, t])) / ls[t] for t in range(d)] for i in range(N)]
    Cs = [[m(float(Xc[i, t])) / ls[t] for t in range(d)] for i in range(M)]
    om = [[m(float(omega[j][t])) for t in range(d)] for j in range(Fn)]
    ph = [m(float(phase[j])) for j in range(Fn)]
    w = [[m(float(weights[s][j])) for j in range(Fn)] for s in range(S)]
    fs = _ctx.sqrt(2 * m(float(amplitude)) / Fn)
    two_pi = 2 * _ctx.pi

    def g(points):
        phi = [[_ctx.cos(two_pi * (_ctx.fsum(o[t] * p[t] for t in range(d)) + ph[j])) for j, o in enumerate(om)] for p in points]
        return [[fs * _ctx.fsum(w[s][j] * row[j] for j in range(Fn)) for s in range(S)] for row in phi]

    def k(a, b):
        return _mp_kernel(kind, _ctx.fsum((a[t] - b[t]) ** 2 for t in range(d)))

    K = _ctx.matrix(N, N)
    for i in range(N):
        for j in range(i + 1):
            K[i, j] = K[j, i] = k(Xs[i], Xs[j])
        K[i, i] = 1 + m(float(eta))
    gX, gC = g(Xs), g(Cs)
    L = _ctx.cholesky(K)
    V = _ctx.matrix(N, S)
    for s in range(S):      # (L L^T) v = y_n - u_s: forward, then back substitution
        b = [m(float(y_norm[i])) - gX[i][s] - m(float(eps[s][i])) for i in range(N)]
        for i in range(N):
            b[i] = (b[i] - _ctx.fsum(L[i, j] * b[j] for j in range(i))) / L[i, i]
        for i in reversed(range(N)):
            b[i] = (b[i] - _ctx.fsum(L[j, i] * b[j] for j in range(i + 1, N))) / L[i, i]
        for i in range(N):
            V[i, s] = b[i]
    out = np.empty((S, M))
    ym, ys = m(float(y_mean)), m(float(y_std))
    for c in range(M):
        kt = [k(Cs[c], Xs[i]) for i in range(N)]
        for s in range(S):
            out[s, c] = float(ys * (gC[c][s] + _ctx.fsum(kt[i] * V[i, s] for i in range(N))) + ym)
    return out


def argmax_with_gap(values):
    """(first index of the maximum per path (S,), (best - second best) / (max - min) per path (S,)); one candidate: gap inf"""
    values = np.asarray(values, dtype=np.float64)
    idx = values.argmax(axis=1)
    if values.shape[1] < 2:
        return idx, np.full(values.shape[0], np.inf)
    two = -np.partition(-values, 1, axis=1)[:, :2]
    span = values.max(axis=1) - values.min(axis=1)
    return idx, (two[:, 0] - two[:, 1]) / np.where(span > 0, span, 1.0)


class PathsFakeEngine(F.FamilyFakeEngine):
    """matern_family_truth.FamilyFakeEngine (TEST DOUBLE ONLY) + sample_paths by `paths_cho` for a unit model."""

    def fit(self, X, y_norm, kernel, length_scale, noise, slot=0, precision=0):
        self.targets = getattr(self, "targets", {})
        self.targets[slot] = np.array(y_norm, dtype=np.float64).ravel()
        return super().fit(X, y_norm, kernel, length_scale, noise, slot=slot, precision=precision)

    def fit_append(self, x_new, y_norm, slot=0):
        self.targets[slot] = np.array(y_norm, dtype=np.float64).ravel()
        return super().fit_append(x_new, y_norm, slot=slot)

    def sample_paths(self, omega, phase, weights, eps, slot=0, y_mean=0.0, y_std=1.0, index_offset=0, return_values=False):
        self.calls.append(("sample_paths", slot, np.shape(weights)[0]))
        X, kernel, length_scale, noise = self.inputs[slot]
        yn = self.targets[slot]
        vals = paths_cho(kernel, X, yn, length_scale, noise, omega, phase, weights, eps, self.Xc, y_mean, y_std)
        self.path_values = getattr(self, "path_values", []) + [vals]
        return vals.argmax(axis=1).astype(np.int64) + index_offset, vals.max(axis=1), (vals if return_values else None)
