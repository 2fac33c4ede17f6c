"""Truth for gpla_ei2_argbest (tests only): include/gpla.h in NumPy.  `G`: E[(Y - a)^+] from its definition, in mpmath where z <= -1
(the sum cancels there), SciPy elsewhere.  `pieces`: mn, den, bn and the (M, J + 1) tables m_j, g_j, q_j, point 0 the candidate.
`Case`: test_gpu_lookahead.py's inputs (cov, m, p from jes_truth.parts, np.longdouble too) and a host posterior for the CPU checks."""
import mpmath
import numpy as np
from scipy.special import ndtr
import jes_truth as JT
import matern_family_truth as F

NOISE, Y_MEAN, Y_STD, M25, RBF = 1e-6, 3.5, 0.4, F.MATERN25, F.RBF
SCALED = dict(c=2.5, w=0.03, alpha=1e-3)      # gpbo_fit_scaled: lambda = w + alpha, vl and vo leave w out
# N, d, M, kind, J, H; M H (J + 1) stays under ~2e4: the truth's mpmath tail takes 0.1 ms a value
CASES = {"j16": (33, 3, 63, M25, 16, 5), "j17": (33, 3, 63, M25, 17, 5), "j33": (70, 3, 130, M25, 33, 5), "j64": (70, 3, 63, M25, 64, 5),
         "j1h32": (70, 3, 130, M25, 1, 32), "full": (70, 3, 1, M25, 64, 32), "j17h32": (33, 3, 1, M25, 17, 32),
         "h32": (33, 3, 63, M25, 1, 32), "n1": (1, 3, 130, M25, 16, 5), "n1j64": (1, 1, 63, RBF, 64, 1),
         "rbf16h1": (33, 3, 63, RBF, 16, 1), "rbf64": (33, 3, 63, RBF, 64, 5), "rbf1": (70, 3, 1, RBF, 1, 1),
         "rbf33": (70, 3, 130, RBF, 33, 5), "d1": (33, 1, 63, RBF, 17, 5), "d1j33": (70, 1, 130, M25, 33, 1),
         "d1h32": (33, 1, 1, M25, 16, 32), "scaled": (33, 3, 63, M25, 16, 5, SCALED), "scaled33": (70, 3, 63, M25, 33, 5, SCALED),
         "scaledrbf": (33, 1, 130, RBF, 64, 1, SCALED)}


def _tails(zs):      # phi(z) + z Phi(z) at 40 digits; below z = -40 it is under 1e-349: 0
    with mpmath.workdps(40):
        r2 = mpmath.sqrt(2)
        return np.array([0.0 if z < -40 else float(mpmath.npdf(z) + z * mpmath.erfc(-z / r2) / 2) for z in map(mpmath.mpf, zs.tolist())])


def G(mean, sd, a):
    mean, sd, a = (np.array(t, dtype=np.float64) for t in np.broadcast_arrays(mean, sd, a))
    with np.errstate(all="ignore"):
        z = (mean - a) / sd
        out = sd * (np.exp(-z * z / 2) / np.sqrt(2 * np.pi) + z * ndtr(z))
    low = (z <= -1) & (sd != 0)
    out[low] = sd[low] * _tails(z[low])
    out[sd == 0] = np.maximum(mean - a, 0.0)[sd == 0]
    return out


def pieces(mu, sd, cov, m, p, y_best, c, w, lam, y_mean, y_std):      # cov = c cov, p = c p of the unit model, lam = c eta
    cov, m, p = (np.asarray(t, dtype=np.float64) for t in (cov, m, p))
    v = (sd / y_std) ** 2
    vl, vo, mn = np.maximum(v - w, 0.0), (v + lam) - w, (mu - y_mean) / y_std
    with np.errstate(all="ignore"):
        den = np.sqrt(vo)
        covs = np.column_stack([vl, cov])
        g = np.where(den[:, None] == 0, 0.0, covs / den[:, None])
        q = np.sqrt(np.maximum(np.column_stack([vl, np.broadcast_to(np.maximum(p, 0.0), cov.shape)]) - g * g, 0.0))
    return mn, den, (y_best - y_mean) / y_std, np.column_stack([mn, np.broadcast_to(m, cov.shape)]), g, q


def ei2(mu, sd, cov, m, p, nodes, weights, y_best, c, w, lam, y_mean, y_std):
    mn, den, bn, ms, g, q = pieces(mu, sd, cov, m, p, y_best, c, w, lam, y_mean, y_std)
    acc = G(mn, den, bn)
    for z, omega in zip(nodes, weights):
        b = np.maximum(bn, mn + den * z)
        acc = acc + omega * np.max(G(ms + g * z, q, b[:, None]), axis=1)      # np.max keeps a NaN
    return np.where(np.isnan(mu) | np.isnan(sd), np.nan, y_std * acc)


class Case:
    def __init__(self, N, d, M, kind, J, H, scaled={}, alpha=None):
        c, w, a = scaled.get("c", 1.0), scaled.get("w", 0.0), scaled.get("alpha", NOISE)
        alpha = a if alpha is None else alpha
        f = (0.3 if kind == M25 else 0.12) / (1 if d > 1 else 30)      # short enough for K' to stay well conditioned at alpha = 1e-6
        self.N, self.d, self.M, self.kind, self.J, self.H, self.c, self.w, self.alpha = N, d, M, kind, J, H, c, w, alpha
        self.X, y = F.data(N, d, seed=3 * N + d)
        self.yn = (y - y.mean()) / y.std() if N > 1 else np.array([0.5])
        self.y_best = float(Y_STD * self.yn.max() + Y_MEAN)
        self.ls = f * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
        self.Xc = np.random.RandomState(500 + N + d).uniform(size=(1000, d))[:M]
        self.pts = np.random.RandomState(900 + J).uniform(size=(J, d))
        self.nodes, weights = np.polynomial.hermite_e.hermegauss(H)      # the Gauss-Hermite rule of a unit normal
        self.weights = weights / np.sqrt(2 * np.pi)

    def parts(self, Xc=None, pts=None, dtype=np.float64):
        cov, m, p = JT.parts(self.kind, self.X, self.yn, self.ls, (self.w + self.alpha) / self.c, self.Xc if Xc is None else Xc,
                             self.pts if pts is None else pts, dtype)
        return self.c * cov, m, self.c * p

    def host_posterior(self, dtype=np.float64):      # (mu, sd) in raw units as gpbo_posterior leaves them: sd^2 = latent + white
        _cov, m, p = self.parts(self.Xc[:1], self.Xc, dtype)
        m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
        return Y_STD * m + Y_MEAN, Y_STD * np.sqrt(np.maximum(p, 0.0) + self.w)

    def truth(self, mu, sd, parts):
        return ei2(mu, sd, *parts, self.nodes, self.weights, self.y_best, self.c, self.w, self.w + self.alpha, Y_MEAN, Y_STD)
