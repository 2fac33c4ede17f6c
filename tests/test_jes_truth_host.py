"""CPU: the rank-one algebra of include/gpje.h against a GP refitted with the sampled optimum as a noise-free observation, and the
sign of the acquisition."""
import numpy as np
from scipy.linalg import cho_solve, cholesky

import jes_truth as T
import matern_family_truth as F
from kg_truth import posterior_cov

N, D, S, ETA = 12, 2, 3, 1e-2
X, y = F.data(N, D, seed=5)
YN = (y - y.mean()) / y.std()
LS = np.array([0.3, 0.4])
XC, XS = np.random.RandomState(1).uniform(size=(5, D)), np.random.RandomState(2).uniform(size=(S, D))
FN = np.array([1.5, 0.2, 2.5])


def test_the_conditioning_is_the_refit_with_a_noise_free_row_and_a_is_not_negative():
    cov, m, p = T.parts(F.MATERN25, X, YN, LS, ETA, XC, XS)
    assert np.abs(cov - posterior_cov(F.MATERN25, X, LS, ETA, XC, XS)).max() <= 1e-12
    # the candidates' own mean and latent variance
    mn, vl = np.array([[t[0] for t in T.parts(F.MATERN25, X, YN, LS, ETA, XC[:1], XC[i:i + 1])[1:]] for i in range(5)]).T
    for s in range(S):
        X2 = np.vstack([X, XS[s]])
        K2 = F.kernel_matrix(F.MATERN25, X2, None, LS)
        K2[np.arange(N), np.arange(N)] += ETA                         # the new row observes the LATENT value: no noise on it
        L2 = cholesky(K2, lower=True)
        k2 = F.kernel_matrix(F.MATERN25, X2, XC, LS)
        sol = cho_solve((L2, True), k2)
        mean2, var2 = sol.T @ np.append(YN, FN[s]), 1.0 - (k2 * sol).sum(axis=0)
        rho = 1.0 / p[s]
        assert np.abs(mn + cov[:, s] * (rho * (FN[s] - m[s])) - mean2).max() <= 1e-10
        assert np.abs(vl - cov[:, s] ** 2 * rho - var2).max() <= 1e-10
    a = T.jes(mn * 0.4 + 3.5, np.sqrt(vl) * 0.4, cov, m, p, FN, 1.0, 0.0, ETA, 3.5, 0.4)
    assert (a >= -1e-15).all() and (a > 1e-3).any()
