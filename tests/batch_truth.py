"""Test infrastructure for suggest_batch (never imported by the product): the truth its picks are held to, and a stand-in for the
slice of bayes_opt.BayesianOptimization that suggest_batch reads, so that the same tests run with and without the reference.

The truth of a batch: constant liar at HELD theta and HELD target normalisation over ONE candidate set, with nothing incremental
in it — for every pick a from-scratch oracle fit of X u picks (the picks' targets = the lie, normalised with the real data's mean
and std), the full posterior over all candidates, the acquisition from tests/acq_truth.py (50-digit EI / POI from the fp64 mu, sd;
UCB is mu + kappa sd in fp64) and the FIRST index of its minimum, as numpy's argmin (bayes_opt/acquisition.py:313).
`gap` per pick = (second smallest - smallest value) / largest |value|: where two candidates are closer than rounding can tell
apart, no implementation's arg-best is "the" answer, so the tests assert a floor on the gap — on this truth alone — before they
compare picks."""
import numpy as np

import acq_truth as T
import matern_family_truth as F
from oracle import gp_oracle as O

GAP_FLOOR = 1e-6


def lie_value(strategy, y):
    if isinstance(strategy, (int, float)):
        return float(strategy)
    return {"min": float(np.min(y)), "mean": float(np.mean(y)), "max": float(np.max(y))}[strategy]


def neg_acquisition(acq, mu, sd, param, y_max):
    """-acq over the candidates from their fp64 posterior: UCB in fp64, EI / POI rounded from the 50-digit truth."""
    if acq == O.UCB:
        return -(mu + param * sd)
    t = T.acq_truth(mu, sd, y_max, param)
    vals = T.to_float(t["ei"] if acq == O.EI else t["poi"])
    if not t["ok"].all():      # sd = 0 (a candidate ON a training point): the NumPy formula's value, as the reference's
        ref = O.base_acq(acq, mu, sd, param, y_max)
        vals = np.where(t["ok"], vals, ref)
    return -vals


def batch_truth(kind, length_scale, noise, X, y, Xc, acq, params, strategy, q, fit=None, predict=None):
    """(indices (q,), gaps (q,)) of the truth's picks.  params: kappa / xi per pick (q,).  `fit(X, y_norm)` / `predict(gp, Xc)`
    default to the four-kind oracle of tests/matern_family_truth.py at (kind, length_scale, noise), un-normalised targets."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    yn, ym, ys = O.normalize_targets(y, True)
    lie = lie_value(strategy, y)
    lie_n = (lie - ym) / ys
    if fit is None:
        def fit(Xa, yna):
            return F.fit_fixed_theta(kind, Xa, yna, length_scale, noise, normalize_y=False)
    if predict is None:
        predict = F.predict
    y_max_real = float(np.max(y))
    idx, gaps, Xa, yna = [], [], X, yn
    for p in range(q):
        gp = fit(Xa, yna)
        mu_n, sd_n = predict(gp, Xc)
        mu, sd = ys * mu_n + ym, ys * sd_n
        y_max = y_max_real if p == 0 else max(y_max_real, lie)
        vals = neg_acquisition(acq, mu, sd, float(params[p]), y_max)
        assert not np.isnan(vals).any()
        best = int(np.argmin(vals))
        two = np.partition(vals, 1)[:2]
        gaps.append(float((two[1] - two[0]) / np.max(np.abs(vals))))
        idx.append(best)
        Xa = np.vstack([Xa, Xc[best][None, :]])
        yna = np.concatenate([yna, [lie_n]])
    return np.array(idx), np.array(gaps)


class Driver:
    """What suggest_batch reads of a BayesianOptimization: `_gp`, `_space`, `_acquisition_function`, `_random_state` — built the
    way accelerate() leaves them (HipGPR in slot 0 sharing the optimizer's RandomState, a fused stock policy, an all-float space)."""

    def __init__(self, engine, X, y, bounds, policy, seed=3, kernel=None, n_restarts_optimizer=2, n_random=None, **gp_kw):
        from sklearn.gaussian_process.kernels import Matern

        from bayesianoptimization_amd.float_space import FloatSpace
        from bayesianoptimization_amd.gpr import HipGPR

        self._random_state = np.random.RandomState(seed)
        self._space = FloatSpace({f"x{j}": tuple(b) for j, b in enumerate(np.asarray(bounds, dtype=np.float64))})
        self._space.register_bulk(X, y)
        self._gp = HipGPR(kernel=Matern(nu=2.5) if kernel is None else kernel, alpha=1e-6, normalize_y=True,
                          n_restarts_optimizer=n_restarts_optimizer, random_state=self._random_state, engine=engine, **gp_kw)
        self._acquisition_function = policy
        if n_random is not None:
            policy.default_n_random = int(n_random)

    def suggest_first(self, n_random=None):
        """one suggest(n_smart=0) of the policy, as BayesianOptimization.suggest() calls it"""
        return self._acquisition_function.suggest(gp=self._gp, target_space=self._space, n_random=n_random, n_smart=0, fit_gp=True,
                                                  random_state=self._random_state)


def rows_to_indices(picks, Xc):
    """index of each pick (a parameter dict or a row) in the candidate matrix, exact match"""
    out = []
    for p in picks:
        row = np.array(list(p.values()), dtype=np.float64) if isinstance(p, dict) else np.asarray(p, dtype=np.float64)
        hit = np.flatnonzero((Xc == row[None, :]).all(axis=1))
        assert hit.size >= 1, "a pick is not one of the candidates"
        out.append(int(hit[0]))
    return np.array(out)
