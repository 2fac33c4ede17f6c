"""Test infrastructure for the ascent of posterior function draws (gpbo_ascend_paths / suggest_thompson(refine=K); never imported by
the product): value AND gradient of a draw, restated over tests/paths_truth.py's formulas, and AscentFakeEngine.

With xs = x / length_scale, t_j = omega_j . xs + phase_j (turns), r_i = |xs - Xs_i|, fs = sqrt(2 c / F), V = paths_truth.path_weights:
    f_s(x)        = y_std (fs sum_j w_sj cos(2 pi t_j) + sum_i V_is k(r_i)) + y_mean
    d f_s / d x_t = y_std (-2 pi fs sum_j w_sj sin(2 pi t_j) omega_jt + sum_i V_is slope(r_i) (xs_t - Xs_it)) / length_scale_t
slope = matern_family_truth.kernel_slope: -k (RBF), -(5/3)(1 + s) exp(-s) (nu 2.5), -3 exp(-s) (nu 1.5), -exp(-r) / r and 0 AT r = 0
(nu 0.5: a point exactly on a training point takes no slope from it — which is also what a central difference gives there).
`path_value_grad`     fp64 NumPy, V by cho_solve (route "cho": matrix products) or through an explicit W = L^-1 (route "winv": the
                      device's route, and the sums as sorted np.sum chains): two summation routes whose spread is the fp64 error bar;
`path_value_grad_mp`  50-digit mpmath, as paths_truth.paths_mp, through `MpPaths` (which also answers at mpf points, unrounded:
                      what the central differences of tests/test_thompson_ascent_host.py are taken of).
Points: Xq (S, K, d), the K points of path s; results f (S, K), g (S, K, d)."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.optimize import minimize

import matern_family_truth as F
import paths_truth as P

_ctx = P._ctx


def _weights_winv(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, amplitude):
    U, _, K, _ = P._parts(kind, X, length_scale, eta, amplitude, omega, phase, weights, eps, np.asarray(X)[:1])
    L = cholesky(K, lower=True, check_finite=False)
    W = solve_triangular(L, np.eye(L.shape[0]), lower=True, check_finite=False)
    alpha = W.T @ (W @ np.asarray(y_norm, dtype=np.float64))
    return alpha[:, None] - W.T @ (W @ U)


def path_value_grad(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, Xq, y_mean=0.0, y_std=1.0, amplitude=1.0,
                    route="cho", V=None, paths=None):
    """(f (S, K), g (S, K, d)) in fp64.  V (N, S): the path weights, when the caller already has them.  paths: the path indices the
    rows of Xq belong to (default: all S, in order)."""
    X = np.asarray(X, dtype=np.float64)
    N, d = X.shape
    ls = np.broadcast_to(np.asarray(length_scale, dtype=np.float64), (d,))
    omega = np.asarray(omega, dtype=np.float64)
    phase = np.asarray(phase, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    S, Fn = w.shape
    paths = list(range(S)) if paths is None else list(paths)
    Xq = np.asarray(Xq, dtype=np.float64).reshape(len(paths), -1, d)
    if V is None:
        V = (P.path_weights if route == "cho" else _weights_winv)(kind, X, y_norm, ls, eta, omega, phase, w, eps, amplitude)
    fs = np.sqrt(2.0 * amplitude / Fn)
    Xs = X / ls
    f = np.empty(Xq.shape[:2])
    g = np.empty(Xq.shape)
    for row, s in enumerate(paths):
        Q = Xq[row] / ls                                            # (K, d)
        t = Q @ omega.T + phase[None, :]
        r = t - np.rint(t)
        cs, sn = np.cos(2.0 * np.pi * r), np.sin(2.0 * np.pi * r)    # (K, F)
        diff = Q[:, None, :] - Xs[None, :, :]                        # (K, N, d)
        dist = np.sqrt((diff * diff).sum(axis=2))
        kv = F.kernel_value(kind, dist)
        sl = F.kernel_slope(kind, dist)
        if route == "cho":
            val = fs * (cs @ w[s]) + kv @ V[:, s]
            grad = (-2.0 * np.pi * fs) * ((sn * w[s][None, :]) @ omega) + np.einsum("kn,knd->kd", sl * V[None, :, s], diff)
        else:      # the same terms as sorted chains
            val = np.sort(np.hstack([fs * cs * w[s][None, :], kv * V[None, :, s]]), axis=1).sum(axis=1)
            terms = np.concatenate([(-2.0 * np.pi * fs) * (sn * w[s][None, :])[:, :, None] * omega[None, :, :],
                                    (sl * V[None, :, s])[:, :, None] * diff], axis=1)
            grad = np.sort(terms, axis=1).sum(axis=1)
        f[row] = y_std * val + y_mean
        g[row] = y_std * grad / ls[None, :]
    return f, g


class MpPaths:
    """The draws of one model at 50 digits: V solved once; value(s, x) / grad(s, x) at a point of mpf (or float) raw coordinates,
    unrounded.  Every fp64 INPUT is taken as given, as paths_truth.paths_mp takes them."""

    def __init__(self, kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, y_mean=0.0, y_std=1.0, amplitude=1.0):
        m = _ctx.mpf
        X = np.asarray(X, dtype=np.float64)
        N, d = X.shape
        Fn, S = np.shape(omega)[0], np.shape(weights)[0]
        self.kind, self.N, self.d, self.F, self.S = kind, N, d, Fn, S
        self.ls = [m(float(v)) for v in np.broadcast_to(np.asarray(length_scale, dtype=np.float64), (d,))]
        self.Xs = [[m(float(X[i, t])) / self.ls[t] for t in range(d)] for i in range(N)]
        self.om = [[m(float(omega[j][t])) for t in range(d)] for j in range(Fn)]
        self.ph = [m(float(phase[j])) for j in range(Fn)]
        self.w = [[m(float(weights[s][j])) for j in range(Fn)] for s in range(S)]
        self.fs = _ctx.sqrt(2 * m(float(amplitude)) / Fn)
        self.ym, self.ys = m(float(y_mean)), m(float(y_std))
        K = _ctx.matrix(N, N)
        for i in range(N):
            for j in range(i + 1):
                K[i, j] = K[j, i] = P._mp_kernel(kind, _ctx.fsum((self.Xs[i][t] - self.Xs[j][t]) ** 2 for t in range(d)))
            K[i, i] = 1 + m(float(eta))
        L = _ctx.cholesky(K)
        gX = [[self._prior(s, p)[0] for s in range(S)] for p in self.Xs]
        self.V = []
        for s in range(S):
            b = [m(float(y_norm[i])) - gX[i][s] - m(float(eps[s][i])) for i in range(N)]
            for i in range(N):
                b[i] = (b[i] - _ctx.fsum(L[i, j] * b[j] for j in range(i))) / L[i, i]
            for i in reversed(range(N)):
                b[i] = (b[i] - _ctx.fsum(L[j, i] * b[j] for j in range(i + 1, N))) / L[i, i]
            self.V.append(b)

    def _prior(self, s, q):
        """(g_s, d g_s / d xs) at the length-scaled point q"""
        two_pi = 2 * _ctx.pi
        arg = [two_pi * (_ctx.fsum(o[t] * q[t] for t in range(self.d)) + self.ph[j]) for j, o in enumerate(self.om)]
        val = self.fs * _ctx.fsum(self.w[s][j] * _ctx.cos(a) for j, a in enumerate(arg))
        grad = [-two_pi * self.fs * _ctx.fsum(self.w[s][j] * _ctx.sin(a) * self.om[j][t] for j, a in enumerate(arg))
                for t in range(self.d)]
        return val, grad

    def _slope(self, r2):
        r = _ctx.sqrt(r2)
        if self.kind == F.RBF:
            return -_ctx.exp(-r2 / 2)
        if self.kind == F.MATERN25:
            s = _ctx.sqrt(5) * r
            return -(_ctx.mpf(5) / 3) * (1 + s) * _ctx.exp(-s)
        if self.kind == F.MATERN15:
            return -3 * _ctx.exp(-_ctx.sqrt(3) * r)
        return -_ctx.exp(-r) / r if r > 0 else _ctx.mpf(0)

    def _scaled(self, x):
        return [_ctx.mpf(v) / self.ls[t] for t, v in enumerate(x)]

    def value(self, s, x):
        q = self._scaled(x)
        kt = [P._mp_kernel(self.kind, _ctx.fsum((q[t] - xi[t]) ** 2 for t in range(self.d))) for xi in self.Xs]
        return self.ys * (self._prior(s, q)[0] + _ctx.fsum(kt[i] * self.V[s][i] for i in range(self.N))) + self.ym

    def grad(self, s, x):
        q = self._scaled(x)
        sl = [self._slope(_ctx.fsum((q[t] - xi[t]) ** 2 for t in range(self.d))) for xi in self.Xs]
        gp = self._prior(s, q)[1]
        return [self.ys * (gp[t] + _ctx.fsum(sl[i] * self.V[s][i] * (q[t] - self.Xs[i][t]) for i in range(self.N))) / self.ls[t]
                for t in range(self.d)]


def path_value_grad_mp(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, Xq, y_mean=0.0, y_std=1.0, amplitude=1.0,
                       model=None):
    """(f (S, K), g (S, K, d)): the 50-digit truth, rounded to fp64 at the end.  model: the MpPaths of these very arguments, when the
    caller already has it."""
    if model is None:
        model = MpPaths(kind, X, y_norm, length_scale, eta, omega, phase, weights, eps, y_mean, y_std, amplitude)
    d = model.d
    Xq = np.asarray(Xq, dtype=np.float64).reshape(model.S, -1, d)
    f = np.empty(Xq.shape[:2])
    g = np.empty(Xq.shape)
    for s in range(model.S):
        for k in range(Xq.shape[1]):
            x = [float(v) for v in Xq[s, k]]
            f[s, k] = float(model.value(s, x))
            g[s, k] = [float(v) for v in model.grad(s, x)]
    return f, g


def projected_gradient_norm(x, grad_f, lo, hi):
    """max_t |P(x + grad f)_t - x_t|, P the projection on the box: the stopping quantity of a box-constrained ASCENT of f (the
    optimiser's own, on -f, is max |P(x - g) - x| with g = -grad f)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(grad_f, dtype=np.float64)
    return np.max(np.abs(np.clip(x + g, lo, hi) - x), axis=-1)


def scipy_ascent(value_grad, starts, lo, hi, method="L-BFGS-B"):
    """SciPy's maximiser of one path from each of its starts (K, d): value_grad(x (d,)) -> (f, g (d,)).  Returns (x (K, d), f (K,))."""
    starts = np.clip(np.asarray(starts, dtype=np.float64), lo, hi)
    xs, fs = [], []
    for x0 in starts:
        def neg(x):
            f, g = value_grad(x)
            return -f, -g

        res = minimize(neg, x0, jac=True, bounds=list(zip(lo, hi)), method=method)
        x = np.clip(res.x, lo, hi)
        xs.append(x)
        fs.append(value_grad(x)[0])
    return np.array(xs), np.array(fs)


class AscentFakeEngine(P.PathsFakeEngine):
    """paths_truth.PathsFakeEngine (TEST DOUBLE ONLY) + ascend_paths: SciPy L-BFGS-B with the analytic gradient over the truth, from
    the truth's own top-K candidates (ties to the lowest index)."""

    def ascend_paths(self, omega, phase, weights, eps, box_lo, box_hi, n_starts=4, starts=None, max_iter=-1, slot=0, y_mean=0.0,
                     y_std=1.0, index_offset=0, return_gradient=False):
        from bayesianoptimization_amd.engine import path_winners

        S = np.shape(weights)[0]
        self.calls.append(("ascend_paths", slot, S))
        X, kernel, length_scale, noise = self.inputs[slot]
        yn = self.targets[slot]
        lo, hi = np.asarray(box_lo, dtype=np.float64), np.asarray(box_hi, dtype=np.float64)
        args = (kernel, X, yn, length_scale, noise, omega, phase, weights, eps)
        V = P.path_weights(*args)
        best_idx = best_val = None
        if starts is None:
            vals = P.paths_cho(*args, self.Xc, y_mean, y_std)
            self.path_values = getattr(self, "path_values", []) + [vals]
            top = np.argsort(-vals, axis=1, kind="stable")[:, :n_starts]
            starts = self.Xc[top]
            start_idx = top.astype(np.int64) + index_offset
            best_idx, best_val = vals.argmax(axis=1).astype(np.int64) + index_offset, vals.max(axis=1)
        else:
            starts = np.asarray(starts, dtype=np.float64)
            start_idx = np.full(starts.shape[:2], -1, dtype=np.int64)
        K, d = starts.shape[1], starts.shape[2]
        x, f = np.empty((S, K, d)), np.empty((S, K))
        for s in range(S):
            def vg(p, s=s):
                fv, gv = path_value_grad(*args, p[None, None, :], y_mean, y_std, V=V, paths=[s])
                return fv[0, 0], gv[0, 0]

            x[s], f[s] = scipy_ascent(vg, starts[s], lo, hi)
        out = {"x": x, "f": f, "status": np.zeros((S, K), dtype=np.int32), "n_eval": np.zeros((S, K), dtype=np.int32),
               "start_idx": start_idx, "best_idx": best_idx, "best_val": best_val}
        if return_gradient:
            out["g"] = path_value_grad(*args, x, y_mean, y_std, V=V)[1]
        out.update(path_winners(x, f))
        return out
