"""Test infrastructure for suggest_batch (never imported by the product): the truth its picks are held to, and a stand-in for the
slice of bayes_opt.BayesianOptimization that suggest_batch reads, so that the same tests run with and without the reference — with
the data, the driver factory and the RandomState comparison the host tests of suggest_batch / suggest_thompson / suggest_mes share.

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


#: the space of the suggest functions' host tests: d = 3, N = 30 observations
SUGGEST_BOUNDS = np.array([[0.0, 1.0], [-1.0, 2.0], [0.5, 1.5]])
SUGGEST_N = 30


def suggest_data(seed=0):
    lo, hi = SUGGEST_BOUNDS[:, 0], SUGGEST_BOUNDS[:, 1]
    rng = np.random.RandomState(seed)
    X = lo + rng.uniform(size=(SUGGEST_N, lo.shape[0])) * (hi - lo)
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2 + 0.05 * rng.standard_normal(SUGGEST_N)
    return X, y


def suggest_driver(engine_class, policy=None, seed=3, n_random=1500, **kw):
    """(driver, engine, X, y): a Driver over `suggest_data` and a fresh `engine_class()`, a decaying UCB where no policy is given."""
    from bayesianoptimization_amd import fused_acquisition as A

    X, y = suggest_data()
    eng = engine_class()
    policy = A.UpperConfidenceBound(kappa=2.0, exploration_decay=0.9, exploration_decay_delay=0) if policy is None else policy
    return Driver(eng, X, y, SUGGEST_BOUNDS, policy, seed=seed, n_random=n_random, lml_on_device=False, **kw), eng, X, y


def same_state(a, b):
    """Are two RandomStates in the same state?"""
    a, b = a.get_state(), b.get_state()
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def check_shared_refusals(suggest, make, who):
    """`suggest(driver)`, a valid call of the suggest function named `who`, in every state the suggest functions refuse alike — an
    empty space, a constraint, an int parameter, a foreign GP, slot 1, a kernel outside the device path, a device group: the
    exception type, the text that names the function and the reason, and no engine call (no host fallback).  `make(**kw)` ->
    (driver, engine, X, y).  Returns the device-group driver's engine, for the caller's check of the GroupEngine method itself."""
    import pytest
    from sklearn.gaussian_process.kernels import RationalQuadratic

    from bayesianoptimization_amd import fused_acquisition as A
    from bayesianoptimization_amd.constraint_model import HipConstraintModel
    from bayesianoptimization_amd.engine import GroupEngine
    from bayesianoptimization_amd.float_space import FloatSpace, MixedSpace

    empty = {f"x{j}": tuple(b) for j, b in enumerate(SUGGEST_BOUNDS)}

    def no_points(drv, eng, X, y):
        drv._space = FloatSpace(empty)

    def constraint(drv, eng, X, y):
        cm = HipConstraintModel(None, np.array([-np.inf]), np.array([0.5]), engine=eng, random_state=np.random.RandomState(3))
        drv._space = FloatSpace(empty, constraint=cm)
        drv._space.register_bulk(X, y, np.cos(X.sum(1)))

    def int_parameter(drv, eng, X, y):
        drv._gp.transform = MixedSpace({"x0": (0.0, 1.0), "x1": (-1, 2, int), "x2": (0.5, 1.5)}).kernel_transform

    def foreign_gp(drv, eng, X, y):
        drv._gp = object()

    def slot_1(drv, eng, X, y):
        drv._gp.slot = 1

    def device_group(drv, eng, X, y):
        drv._gp.engine = object.__new__(GroupEngine)          # (no devices opened: the type is what is refused)
        drv._gp.engine.__dict__.update(_g=None, _h=None)

    scenarios = [(no_points, {}, A.TargetSpaceEmptyError, "without previous samples"),
                 (constraint, {}, A.ConstraintNotSupportedError, f"but {who} does not support constrained"),
                 (int_parameter, {}, NotImplementedError, f"{who}: the space has an input transform"),
                 (foreign_gp, {}, NotImplementedError, f"{who}: .*accelerate"),
                 (slot_1, {}, NotImplementedError, f"{who}: .*accelerate"),
                 (lambda *a: None, {"kernel": RationalQuadratic()}, NotImplementedError, f"{who}: the model runs on the host"),
                 (device_group, {}, NotImplementedError, f"{who}: a device group")]
    for spoil, kw, error, match in scenarios:
        drv, eng, X, y = make(**kw)
        spoil(drv, eng, X, y)
        with pytest.raises(error, match=match):
            suggest(drv)
        assert not eng.calls, (spoil.__name__, eng.calls)      # refused before anything ran
    return drv._gp.engine


def rows_to_indices(picks, Xc):
    """index of each pick (a parameter dict or a row) in the candidate matrix, exact match"""
    out = []
    for p in picks:
        row = np.array(list(p.values()), dtype=np.float64) if isinstance(p, dict) else np.asarray(p, dtype=np.float64)
        hit = np.flatnonzero((Xc == row[None, :]).all(axis=1))
        assert hit.size >= 1, "a pick is not one of the candidates"
        out.append(int(hit[0]))
    return np.array(out)
