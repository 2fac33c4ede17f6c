"""CPU: lookahead_truth.pieces against a GP refitted with the fantasised observation appended; the truth's own fp64 noise on the GPU cases"""
import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky

import lookahead_truth as T
import matern_family_truth as F

N, D, J, ETA = 12, 2, 3, 1e-2
X, y = F.data(N, D, seed=5)
YN = (y - y.mean()) / y.std()
LS, XC, PTS = np.array([0.3, 0.4]), np.random.RandomState(1).uniform(size=(4, D)), np.random.RandomState(2).uniform(size=(J, D))


def refit(Xt, yt, at):      # posterior mean and latent sd at `at` of the unit model on (Xt, yt), from its own Cholesky
    K = F.kernel_matrix(F.MATERN25, Xt, None, LS) + ETA * np.eye(len(Xt))
    k = F.kernel_matrix(F.MATERN25, Xt, at, LS)
    sol = cho_solve((cholesky(K, lower=True), True), k)
    return sol.T @ yt, np.sqrt(1.0 - (k * sol).sum(axis=0))


def test_a_node_is_the_refit_with_the_observation_appended():
    cov, m, p = T.JT.parts(F.MATERN25, X, YN, LS, ETA, XC, PTS)
    mn, sl = refit(X, YN, XC)
    bn = float(YN.max()) - 0.3
    mn_, den, bn_, ms, g, q = T.pieces(mn, sl, cov, m, p, bn, 1.0, 0.0, ETA, 0.0, 1.0)
    for i in range(len(XC)):
        for z in (-1.3, 0.0, 0.4, 2.1):
            y_h = mn[i] + den[i] * z                                   # the observation at x_i, noise included
            mean2, sd2 = refit(np.vstack([X, XC[i]]), np.append(YN, y_h), np.vstack([XC[i], PTS]))
            b = max(bn, y_h)                                           # the incumbent after the observation; G is EI's definition
            assert np.abs(T.G(ms[i] + g[i] * z, q[i], b) / T.G(mean2, sd2, b) - 1).max() <= 1e-10


@pytest.mark.parametrize("name", list(T.CASES))
def test_the_truths_own_noise_is_a_tenth_of_the_gpu_bar(name):
    c = T.Case(*T.CASES[name])
    mu, sd = c.host_posterior()
    a64, ald = c.truth(mu, sd, c.parts()), c.truth(mu, sd, c.parts(dtype=np.longdouble))
    D = np.abs(a64 - ald) / (1e-9 * T.Y_STD + 1e-9 * np.abs(ald))
    print(f"{name}: the fp64 truth against the longdouble one, worst {D.max():.2e} of the bar")
    assert D.max() < 0.1
