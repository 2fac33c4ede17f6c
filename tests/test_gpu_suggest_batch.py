"""GPU (-m gpu): suggest_batch on the real engine — q = 6 picks from one candidate pass (one gpbo_posterior, five
gpbo_fit_append + gpbo_posterior_refresh + gpbo_acq_argbest) against tests/batch_truth.py: a from-scratch oracle refit of
X u picks per pick at the held theta and the held normalisation, the 50-digit acquisition, first-index argmin.  A pick is compared
only where the truth's own best and second value are further apart than rounding ((second - best) / max |value| >= 1e-6, asserted
on the truth alone; the seeds were picked on the CPU for it).  Also: the first pick is one suggest(n_smart=0) of a twin, and
`predict` after the call equals `predict` before it, bit for bit."""
import numpy as np
import pytest

import batch_truth as B
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_batch

pytestmark = pytest.mark.gpu

D, M, Q = 3, 2000, 6          # M * D >= 4096: the candidates come from the optimizer's RandomState on the device
BOUNDS = np.array([[0.0, 1.0]] * D)
POLICY = {"ucb": lambda: A.UpperConfidenceBound(kappa=2.576), "ei": lambda: A.ExpectedImprovement(xi=0.01)}


def _driver(engine, N, name, **kw):
    X = np.random.RandomState(100 + N).uniform(size=(N, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2          # smooth and noise-free: the theta search ends inside its bounds
    return B.Driver(engine, X, y, BOUNDS, POLICY[name](), seed=7, n_random=M, **kw), X, y


@pytest.mark.parametrize("name", ["ucb", "ei"])
@pytest.mark.parametrize("N", [40, 300])
def test_batch_picks_equal_the_refit_truth(engine, N, name):
    twin, _, _ = _driver(engine, N, name)
    x_twin = twin.suggest_first()
    drv, X, y = _driver(engine, N, name)
    picks = suggest_batch(drv, Q, strategy="min")      # (under the 'max' lie UCB picks one candidate again and again here: rows 1e-6 apart in K)
    assert len(picks) == Q
    assert np.array_equal(np.array(list(picks[0].values())), x_twin)          # pick 1 is that suggest(n_smart=0), bit for bit
    a, b = drv._random_state.get_state(), twin._random_state.get_state()
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    Xc = engine.get_candidate_rows(np.arange(M), D)                           # the one candidate draw is still resident
    gp, fn = drv._gp, drv._acquisition_function
    want, gaps = B.batch_truth(int(gp._kind), np.array(gp._ls), float(gp.alpha), X, y, Xc, fn._acq_kind, [fn._acq_param()] * Q,
                               "min", Q)
    got = B.rows_to_indices(picks, Xc)
    print(f"N={N} {name}: picks {got.tolist()} truth {want.tolist()} gaps {['%.1e' % g for g in gaps]}")
    assert gaps.min() >= B.GAP_FLOOR, f"the truth's own best / second gap {gaps.min():.2e}: pick another seed"
    assert np.array_equal(got, want)
    assert fn.i == Q and gp.X_train_.shape[0] == N


@pytest.mark.parametrize("N", [40, 300])
def test_predict_is_unchanged_by_the_call(engine, N):
    drv, X, y = _driver(engine, N, "ei", n_restarts_optimizer=0)      # no restarts: the two theta searches start and end alike
    drv.suggest_first()
    Xq = np.random.RandomState(9).uniform(size=(64, D))
    mu0, sd0 = drv._gp.predict(Xq, return_std=True)
    suggest_batch(drv, Q, strategy="mean")
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    assert drv._gp.X_train_.shape[0] == N
