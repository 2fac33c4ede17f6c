"""Test infrastructure for the opt-in Matern family (never imported by the product): a NumPy restatement of the four kernel kinds'
value and slope (csrc/gpbo_internal.h: gpbo_kernel_value, gpbo_kernel_slope), the posterior and its input gradient over them, and
FamilyFakeEngine — tests/helpers.FakeEngine with the kinds oracle/gp_oracle.py does not know (it has RBF and Matern nu = 2.5 only).

Value, with r the distance of the length-scaled points (sklearn kernels.py, Matern.__call__):
    RBF exp(-r^2 / 2);  nu = 2.5: s = sqrt5 r, (1 + s + s^2 / 3) exp(-s);  nu = 1.5: s = sqrt3 r, (1 + s) exp(-s);  nu = 0.5: exp(-r)
Slope f, with dk / dxs_t = f (xs_t - Xs_t) and dK / dlog l_t = -f (xs_t - Xs_t)^2:
    RBF -k;  nu = 2.5: -(5/3) (1 + s) exp(-s);  nu = 1.5: -3 exp(-sqrt3 r);  nu = 0.5: -exp(-r) / r, and 0 at r = 0 — scikit-learn
    zeroes the non-finite gradient entries of coincident points (kernels.py: K_gradient[~np.isfinite(K_gradient)] = 0).
tests/test_matern_family_host.py pins both against scikit-learn's K and K_gradient."""
import copy

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular
from scipy.spatial.distance import cdist

from helpers import FakeEngine
from oracle import gp_oracle as O

RBF, MATERN25, MATERN15, MATERN05 = 0, 1, 2, 3
FAMILY = (MATERN15, MATERN05)
NU = {MATERN25: 2.5, MATERN15: 1.5, MATERN05: 0.5}


def sk_kernel(kind, length_scale):
    """The scikit-learn kernel of a kind."""
    from sklearn.gaussian_process.kernels import RBF as SkRBF
    from sklearn.gaussian_process.kernels import Matern

    return SkRBF(length_scale=length_scale) if kind == RBF else Matern(nu=NU[kind], length_scale=length_scale)


def data(N, d, seed=0):
    """The suite's data: X uniform on [0, 1]^d, y = sin(3 sum X) + 0.1 noise."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    y = np.sin(3 * X.sum(1)) + 0.1 * rng.randn(N)
    return X, y


def _scaled_distance(Xa, Xb, length_scale):
    ls = np.asarray(length_scale, dtype=np.float64)
    A = np.asarray(Xa, dtype=np.float64) / ls
    B = A if Xb is None else np.asarray(Xb, dtype=np.float64) / ls
    return cdist(A, B, metric="euclidean")


def kernel_value(kind, r):
    if kind == RBF:
        return np.exp(-0.5 * r * r)
    if kind == MATERN25:
        s = np.sqrt(5.0) * r
        return (1.0 + s + s * s / 3.0) * np.exp(-s)
    if kind == MATERN15:
        s = np.sqrt(3.0) * r
        return (1.0 + s) * np.exp(-s)
    if kind == MATERN05:
        return np.exp(-r)
    raise ValueError(f"unsupported kernel kind {kind}")


def kernel_slope(kind, r):
    if kind == RBF:
        return -kernel_value(kind, r)
    if kind == MATERN25:
        s = np.sqrt(5.0) * r
        return -(5.0 / 3.0) * (1.0 + s) * np.exp(-s)
    if kind == MATERN15:
        return -3.0 * np.exp(-np.sqrt(3.0) * r)
    if kind == MATERN05:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, -np.exp(-r) / r, 0.0)
    raise ValueError(f"unsupported kernel kind {kind}")


def kernel_matrix(kind, Xa, Xb, length_scale):
    """k(Xa, Xb), or k(Xa, Xa) with an exact unit diagonal when Xb is None (as oracle.gp_oracle.kernel_matrix)."""
    out = kernel_value(kind, _scaled_distance(Xa, Xb, length_scale))
    if Xb is None:
        np.fill_diagonal(out, 1.0)
    return out


def fit_fixed_theta(kind, X, y, length_scale, noise=1e-6, normalize_y=True):
    X = np.ascontiguousarray(X, dtype=np.float64)
    yn, mean, std = O.normalize_targets(y, normalize_y)
    K = kernel_matrix(kind, X, None, length_scale)
    K[np.diag_indices_from(K)] += noise
    L = cholesky(K, lower=True, check_finite=False)
    alpha = cho_solve((L, True), yn, check_finite=False)
    return O.GPState(kind, np.atleast_1d(np.asarray(length_scale, dtype=np.float64)), float(noise), X, L, alpha, mean, std)


def _normal_variance(gp, Kt):
    V = solve_triangular(gp.L, Kt.T, lower=True, check_finite=False)
    return np.ones(Kt.shape[0]) - np.einsum("ij,ji->i", V.T, V)


def predict(gp, Xc):
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    Kt = kernel_matrix(gp.kind, Xc, gp.X, gp.length_scale)
    var = _normal_variance(gp, Kt)
    var[var < 0] = 0.0
    return gp.y_std * (Kt @ gp.alpha) + gp.y_mean, np.sqrt(var * gp.y_std**2)


def negative_variances(gp, Xc):
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    return int(np.count_nonzero(_normal_variance(gp, kernel_matrix(gp.kind, Xc, gp.X, gp.length_scale)) < 0))


def predict_cov(gp, Xc):
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    Kt = kernel_matrix(gp.kind, Xc, gp.X, gp.length_scale)
    V = solve_triangular(gp.L, Kt.T, lower=True, check_finite=False)
    return gp.y_std * (Kt @ gp.alpha) + gp.y_mean, (kernel_matrix(gp.kind, Xc, None, gp.length_scale) - V.T @ V) * gp.y_std**2


def predict_grad(gp, Xc):
    """(mean, std, d mean / d x, d std / d x): oracle.gp_oracle.predict_grad with the slope of every kind.
    dk/dx_t = f(r) (x_t - X_kt) / l_t^2;  d var_n / d x = -2 (K^-1 k*)^T dk*/dx;  a clipped variance has zero slope."""
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    ls = np.broadcast_to(gp.length_scale, (gp.X.shape[1],))
    mean, std = predict(gp, Xc)
    r = _scaled_distance(Xc, gp.X, ls)
    Kt = kernel_value(gp.kind, r)
    dK = kernel_slope(gp.kind, r)[:, :, None] * ((Xc[:, None, :] - gp.X[None, :, :]) / ls**2)
    dmean = gp.y_std * np.einsum("mnd,n->md", dK, gp.alpha)
    u = cho_solve((gp.L, True), Kt.T, check_finite=False).T
    dvar_n = -2.0 * np.einsum("mnd,mn->md", dK, u)
    sd_n = std / gp.y_std
    with np.errstate(divide="ignore", invalid="ignore"):
        dstd = np.where(sd_n[:, None] > 0, gp.y_std * dvar_n / (2.0 * sd_n[:, None]), 0.0)
    return mean, std, dmean, dstd


def kernel_gradient(kind, X, length_scale):
    """dK / dlog l_t, (N, N, n_ls), as scikit-learn's K_gradient."""
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64))
    Xs = np.asarray(X, dtype=np.float64) / ls
    D = (Xs[:, None, :] - Xs[None, :, :]) ** 2
    g = -kernel_slope(kind, np.sqrt(D.sum(-1)))
    return g[:, :, None] * (D if ls.shape[0] > 1 else D.sum(-1, keepdims=True))


def log_marginal_likelihood(kind, X, y_norm, length_scale, noise=1e-6, eval_gradient=True):
    """As oracle.gp_oracle.log_marginal_likelihood (sklearn _gpr.py:575-652), for every kind."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y_norm, dtype=np.float64)
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64))
    K = kernel_matrix(kind, X, None, ls)
    K[np.diag_indices_from(K)] += noise
    try:
        L = cholesky(K, lower=True, check_finite=False)
    except np.linalg.LinAlgError:
        return (-np.inf, np.zeros(ls.shape[0])) if eval_gradient else -np.inf
    alpha = cho_solve((L, True), y, check_finite=False)
    lml = -0.5 * float(y @ alpha) - np.log(np.diag(L)).sum() - K.shape[0] / 2 * np.log(2 * np.pi)
    if not eval_gradient:
        return lml
    inner = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(K.shape[0]), check_finite=False)
    return lml, 0.5 * np.einsum("ij,ijt->t", inner, kernel_gradient(kind, X, ls))


def neg_acquisition(gp, Xc, acq, param, y_max=0.0):
    mean, std = predict(gp, Xc)
    return -1 * O.base_acq(acq, mean, std, param, y_max)


class FamilyFakeEngine(FakeEngine):
    """helpers.FakeEngine (the GpEngine surface on the CPU; TEST DOUBLE ONLY) over the four kinds, recording the kind every fit,
    LML evaluation and posterior pass ran with: `kinds` = [(call, kind)]."""

    def __init__(self):
        super().__init__()
        self.kinds = []

    def fit(self, X, y_norm, kernel, length_scale, noise, slot=0, precision=0):
        self.calls.append(("fit", slot, X.shape))
        self.kinds.append(("fit", int(kernel)))
        self.models[slot] = fit_fixed_theta(kernel, X, y_norm, length_scale, noise, normalize_y=False)
        self.inputs = getattr(self, "inputs", {})
        self.inputs[slot] = (np.array(X), kernel, length_scale, noise)
        return self._touch(slot)

    def fit_append(self, x_new, y_norm, slot=0):
        self.calls.append(("fit_append", slot, x_new.shape))
        if slot not in self.models:
            raise RuntimeError("gpbo_fit_append: slot has no fitted model (call gpbo_fit first)")
        X0, kernel, length_scale, noise = self.inputs[slot]
        X = np.vstack([X0, x_new]) if x_new.shape[0] else X0
        self.kinds.append(("fit_append", int(kernel)))
        self.models[slot] = fit_fixed_theta(kernel, X, y_norm, length_scale, noise, normalize_y=False)
        self.inputs[slot] = (X, kernel, length_scale, noise)
        return self._touch(slot)

    def lml(self, X, y_norm, kernel, length_scale, noise, eval_gradient=True, slot=0):
        self.calls.append(("lml", slot))
        self.kinds.append(("lml", int(kernel)))
        self._touch(slot)
        self.models.pop(slot, None)
        return log_marginal_likelihood(kernel, X, y_norm, length_scale, noise, eval_gradient)

    def lml_batch(self, X, y_norm, kernel, length_scales, noise, eval_gradient=True, reuse_inputs=False):
        self.calls.append(("lml_batch", len(length_scales)))
        self.kinds.append(("lml_batch", int(kernel)))
        return [log_marginal_likelihood(kernel, X, y_norm, ls, noise, eval_gradient) for ls in np.atleast_2d(length_scales)]

    def posterior(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True):
        self.calls.append(("posterior", slot))
        self.kinds.append(("posterior", int(self.models[slot].kind)))
        mu, sd = predict(self.models[slot], self.Xc)
        mu, sd = y_std * mu + y_mean, sd * y_std
        self.negvar = getattr(self, "negvar", False) or bool(negative_variances(self.models[slot], self.Xc))
        self.post[slot] = (mu, sd)
        return (mu, sd) if fetch else (None, None)

    def predict_cov(self, Xc, slot=0, y_mean=0.0, y_std=1.0):
        self.calls.append(("predict_cov", slot, np.shape(Xc)))
        mu, cov = predict_cov(self.models[slot], np.asarray(Xc, dtype=np.float64))
        return y_std * mu + y_mean, cov * y_std**2

    def predict_grad(self, Xc, slot=0, y_mean=0.0, y_std=1.0):
        self.calls.append(("predict_grad", slot, np.shape(Xc)))
        mu, sd, dmu, dsd = predict_grad(self.models[slot], np.asarray(Xc, dtype=np.float64))
        return y_std * mu + y_mean, sd * y_std, y_std * dmu, y_std * dsd

    def polish_seeds(self, acq, param, y_max, lb, ub, y_means, y_stds, seeds, box, max_iter=0):
        """FakeEngine.polish_seeds for one model without constraint GPs: SciPy's L-BFGS-B over -acquisition with the analytic
        gradient of this module."""
        from scipy.optimize import minimize

        if len(y_means) != 1:
            raise NotImplementedError("FamilyFakeEngine.polish_seeds: one model, no constraint GPs")
        self.calls.append(("polish_seeds", acq, len(seeds)))
        self.kinds.append(("polish_seeds", int(self.models[0].kind)))
        gp = copy.copy(self.models[0])
        gp.y_mean, gp.y_std = float(y_means[0]), float(y_stds[0])
        ym = 0.0 if y_max is None else float(y_max)

        def f_grad(x):
            mu, sd, dmu, dsd = (v[0] for v in predict_grad(gp, x[None]))
            if acq == O.UCB:
                a, ca, cs = mu + param * sd, 1.0, param
            else:
                aa = mu - ym - param
                z = aa / sd
                cdf, pdf = float(O.norm_cdf(z)), float(O.norm_pdf(z))
                a, ca, cs = (aa * cdf + sd * pdf, cdf, pdf) if acq == O.EI else (cdf, pdf / sd, -pdf * z / sd)
            return -a, -(ca * dmu + cs * dsd)

        box = np.asarray(box, dtype=np.float64)
        xs, fs, status = [], [], []
        for s0 in np.asarray(seeds, dtype=np.float64):
            res = minimize(f_grad, s0, jac=True, bounds=box, method="L-BFGS-B")
            xs.append(res.x)
            fs.append(float(np.squeeze(res.fun)))
            status.append(0 if res.success else 2)
        self._resident = False
        return np.array(xs), np.array(fs), np.array(status, dtype=np.int32), 0
