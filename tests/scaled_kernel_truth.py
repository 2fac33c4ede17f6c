"""Test infrastructure for the opt-in scaled kernels  c * k + w  (ConstantKernel * k + WhiteKernel; never imported by the product):
what scikit-learn does not offer — the posterior's input gradient — and ScaledFakeEngine, a NumPy stand-in for the GpEngine surface
with `amplitude` / `white`, for the CPU tests of the host glue.  Everything here works on the FULL model K = c k + (w + a) I, with
none of the device's reduction to a unit model (csrc/scaled_kernel.h): the two meet only in the numbers.
tests/test_scaled_kernel_host.py pins predict / log_marginal_likelihood of this module against scikit-learn.

Data and cases as the issue sets them: X uniform on [0, 1]^d, y = sin(3 sum X) + 0.1 noise, seeded; length scale 0.25 sqrt d, one
value or one per dimension; alpha = 1e-6; (c, w) in CASES."""
import contextlib
import copy

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

import matern_family_truth as F
from oracle import gp_oracle as O

ALPHA = 1e-6
CASES = [(0.3, 0.0), (7.0, 2e-3), (1.0, 5e-2)]
CASE_IDS = ["c0.3_w0", "c7_w2e-3", "c1_w5e-2"]
data = F.data


def length_scale(d, per_dim):
    ls = 0.25 * np.sqrt(d)
    return ls * np.linspace(0.7, 1.4, d) if per_dim else float(ls)


def sk_kernel(c, ls, w, kind=F.MATERN25, white_first=False, constant_last=False):
    """scikit-learn's kernel of a case; w = 0 is the kernel without its WhiteKernel (log 0 is no theta)."""
    from sklearn.gaussian_process.kernels import ConstantKernel, WhiteKernel

    base = F.sk_kernel(kind, ls)
    k = base * ConstantKernel(c) if constant_last else ConstantKernel(c) * base
    if w == 0.0:
        return k
    return WhiteKernel(w) + k if white_first else k + WhiteKernel(w)


class ScaledGP:
    """A fitted model K = c k + (w + a) I: L = chol(K), alpha = K^-1 y_norm."""

    def __init__(self, kind, X, y_norm, ls, c=1.0, w=0.0, a=ALPHA, y_mean=0.0, y_std=1.0):
        self.kind, self.c, self.w, self.a = int(kind), float(c), float(w), float(a)
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.length_scale = np.atleast_1d(np.asarray(ls, dtype=np.float64))
        self.y_mean, self.y_std = float(y_mean), float(y_std)
        K = self.c * F.kernel_matrix(self.kind, self.X, None, self.length_scale)
        K[np.diag_indices_from(K)] += self.w + self.a
        self.K = K
        self.L = cholesky(K, lower=True, check_finite=False)
        self.alpha = cho_solve((self.L, True), np.asarray(y_norm, dtype=np.float64), check_finite=False)


def fit(kind, X, y, ls, c, w, a=ALPHA):
    """The model of GaussianProcessRegressor(kernel=sk_kernel(c, ls, w), alpha=a, normalize_y=True, optimizer=None).fit(X, y)."""
    yn, mean, std = O.normalize_targets(y, True)
    return ScaledGP(kind, X, yn, ls, c, w, a, mean, std)


def _normal_variance(gp, Kt):
    V = solve_triangular(gp.L, Kt.T, lower=True, check_finite=False)
    return np.full(Kt.shape[0], gp.c + gp.w) - np.einsum("ij,ji->i", V.T, V)      # kernel_.diag(X) = c + w (_gpr.py:474-477)


def predict(gp, Xc):
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    Kt = gp.c * F.kernel_matrix(gp.kind, Xc, gp.X, gp.length_scale)
    var = _normal_variance(gp, Kt)
    var[var < 0] = 0.0
    return gp.y_std * (Kt @ gp.alpha) + gp.y_mean, np.sqrt(var * gp.y_std**2)


def negative_variances(gp, Xc):
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    return int(np.count_nonzero(_normal_variance(gp, gp.c * F.kernel_matrix(gp.kind, Xc, gp.X, gp.length_scale)) < 0))


def predict_cov(gp, Xc):
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    Kt = gp.c * F.kernel_matrix(gp.kind, Xc, gp.X, gp.length_scale)
    V = solve_triangular(gp.L, Kt.T, lower=True, check_finite=False)
    prior = gp.c * F.kernel_matrix(gp.kind, Xc, None, gp.length_scale) + gp.w * np.eye(Xc.shape[0])
    return gp.y_std * (Kt @ gp.alpha) + gp.y_mean, (prior - V.T @ V) * gp.y_std**2


def predict_grad(gp, Xc):
    """(mean, std, d mean / d x, d std / d x).  dk*/dx_t = c f(r) (x_t - X_kt) / l_t^2 (f: matern_family_truth.kernel_slope);
    d var_n / d x = -2 (K^-1 k*)^T dk*/dx (the prior variance c + w does not move with x); a clipped variance has zero slope."""
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, gp.X.shape[1])
    ls = np.broadcast_to(gp.length_scale, (gp.X.shape[1],))
    mean, std = predict(gp, Xc)
    r = F._scaled_distance(Xc, gp.X, ls)
    Kt = gp.c * F.kernel_value(gp.kind, r)
    dK = gp.c * F.kernel_slope(gp.kind, r)[:, :, None] * ((Xc[:, None, :] - gp.X[None, :, :]) / ls**2)
    dmean = gp.y_std * np.einsum("mnd,n->md", dK, gp.alpha)
    u = cho_solve((gp.L, True), Kt.T, check_finite=False).T
    dvar_n = -2.0 * np.einsum("mnd,mn->md", dK, u)
    sd_n = std / gp.y_std
    with np.errstate(divide="ignore", invalid="ignore"):
        dstd = np.where(sd_n[:, None] > 0, gp.y_std * dvar_n / (2.0 * sd_n[:, None]), 0.0)
    return mean, std, dmean, dstd


def neg_acquisition(gp, Xc, acq, param, y_max=0.0):
    mean, std = predict(gp, Xc)
    return -1 * O.base_acq(acq, mean, std, param, y_max)


def log_marginal_likelihood(kind, X, y_norm, ls, c, w, a=ALPHA, eval_gradient=True):
    """LML of y_norm under c k + (w + a) I and its gradient in [log c, log l ..., log w] — the order of gpbo_lml_scaled
    (sklearn _gpr.py:575-652 with dK/dlog c = c k, dK/dlog l_t = c dk/dlog l_t, dK/dlog w = w I)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y_norm, dtype=np.float64)
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    k = F.kernel_matrix(kind, X, None, ls)
    K = c * k
    K[np.diag_indices_from(K)] += w + a
    n = K.shape[0]
    try:
        L = cholesky(K, lower=True, check_finite=False)
    except np.linalg.LinAlgError:
        return (-np.inf, np.zeros(ls.shape[0] + 2)) if eval_gradient else -np.inf
    alpha = cho_solve((L, True), y, check_finite=False)
    lml = -0.5 * float(y @ alpha) - np.log(np.diag(L)).sum() - n / 2 * np.log(2 * np.pi)
    if not eval_gradient:
        return lml
    inner = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(n), check_finite=False)
    dK = np.concatenate([(c * k)[:, :, None], c * F.kernel_gradient(kind, X, ls), (w * np.eye(n))[:, :, None]], axis=2)
    return lml, 0.5 * np.einsum("ij,ijt->t", inner, dK)


class ScaledFakeEngine(F.FamilyFakeEngine):
    """matern_family_truth.FamilyFakeEngine (the GpEngine surface on the CPU; TEST DOUBLE ONLY) with GpEngine's `amplitude` / `white`:
    every model is a ScaledGP (1 and 0 where the caller passes none).  `scaled_calls` records (call, amplitude, white) of every call
    that came WITH the two arguments — a unit model's calls must come without."""

    def __init__(self):
        super().__init__()
        self.scaled_calls = []
        self._overlap_depth = 0
        self.overlap_log = []      # (slot, "enqueued" | "synchronous") of every fit made inside overlapped_fits()

    @contextlib.contextmanager
    def overlapped_fits(self):
        """GpEngine.overlapped_fits' rule: inside the block a unit model's fit is enqueued (gpbo_fit_begin), a scaled model's fit
        completes in its call (gpbo_fit_scaled has no gpbo_fit_begin twin).  The stand-in computes both at once and records which."""
        self._overlap_depth += 1
        try:
            yield self
        finally:
            self._overlap_depth -= 1

    def _note(self, call, kw):
        if kw:
            self.scaled_calls.append((call, float(kw.get("amplitude", 1.0)), float(kw.get("white", 0.0))))
        return float(kw.get("amplitude", 1.0)), float(kw.get("white", 0.0))

    def fit(self, X, y_norm, kernel, length_scale, noise, slot=0, precision=0, **kw):
        c, w = self._note("fit", kw)
        if self._overlap_depth > 0:
            self.overlap_log.append((slot, "synchronous" if (c, w) != (1.0, 0.0) else "enqueued"))
        self.calls.append(("fit", slot, X.shape))
        self.kinds.append(("fit", int(kernel)))
        self.models[slot] = ScaledGP(kernel, X, y_norm, length_scale, c, w, noise)
        return self._touch(slot)

    def fit_append(self, x_new, y_norm, slot=0, **kw):
        c, w = self._note("fit_append", kw)
        self.calls.append(("fit_append", slot, x_new.shape))
        if slot not in self.models:
            raise RuntimeError("gpbo_fit_append: slot has no fitted model (call gpbo_fit first)")
        old = self.models[slot]
        if (c, w) != (old.c, old.w):
            raise ValueError("fit_append: amplitude / white differ from the slot's fitted model")
        X = np.vstack([old.X, x_new]) if x_new.shape[0] else old.X
        self.kinds.append(("fit_append", old.kind))
        self.models[slot] = ScaledGP(old.kind, X, y_norm, old.length_scale, c, w, old.a)
        return self._touch(slot)

    def lml(self, X, y_norm, kernel, length_scale, noise, eval_gradient=True, slot=0, scaled=None, **kw):
        c, w = self._note("lml", kw)
        self.calls.append(("lml", slot))
        self.kinds.append(("lml", int(kernel)))
        self._touch(slot)
        self.models.pop(slot, None)
        if not (scaled or (scaled is None and (c != 1.0 or w != 0.0))):
            return F.log_marginal_likelihood(kernel, X, y_norm, length_scale, noise, eval_gradient)
        return log_marginal_likelihood(kernel, X, y_norm, length_scale, c, w, noise, eval_gradient)

    def get_L(self, n, slot=0):
        return self.models[slot].L.copy()

    def get_alpha(self, n, slot=0):
        return self.models[slot].alpha.copy()

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
        """FamilyFakeEngine.polish_seeds over the scaled model: SciPy's L-BFGS-B over -acquisition with this module's gradient."""
        from scipy.optimize import minimize

        if len(y_means) != 1:
            raise NotImplementedError("ScaledFakeEngine.polish_seeds: one model, no constraint GPs")
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
