"""CPU: log expected improvement on the host — the formula (tests/log_ei_truth.py's restatement and the policy's base_acq /
base_acq_grad) against the 50-digit truth, its conventions, its agreement with EI where EI is representable and its answer where EI
is a plateau of zeros, and the policy protocol of LogExpectedImprovement over an oracle-backed engine double.

Bar: |value - truth| <= 4 eps W, W = 1 + z^2 + |truth| (gradient: (1 + z^2)(|ca dmu| + |cs dsd|)); log_ei_truth.py has the model.
Measured: value c = 2.13 (at z = -3.03), gradient c = 3.23 (at z = -1.05) — the restatement and the policy give the same bits; the
gradient's worst lies just below the switch at -1, where r = 1 - sqrt(pi) t erfcx(t) = 0.3 is a difference of numbers near 1."""
import types

import numpy as np
import pytest

import acq_truth as T
import batch_truth as B
import log_ei_truth as L
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_batch
from helpers import FakeEngine
from oracle import gp_oracle as O

BAR = 4.0
XI = 0.01
LOG_EI = 3


# ---- the formula -----------------------------------------------------------------------------------------------------------------
def _z_sweep():
    """z in [-1e8, 8] (log-uniform in the far tail, uniform around the switches), the floats either side of each switch point and the
    points themselves, the edge where EI underflows; sd from 1e-12 to 1e3"""
    rng = np.random.RandomState(0)
    special = np.concatenate([np.nextafter(-1.0, [-2.0, 0.0]), [-1.0], np.nextafter(L.SERIES_BELOW, [-30.0, 0.0]), [L.SERIES_BELOW],
                              [-1e8, 8.0, -38.5, -38.6, -40.0, -45.0, -200.0, 0.0]])
    z = np.concatenate([special, -10.0 ** rng.uniform(0, 8, 700), rng.uniform(-40, 8, 860)])
    sd = 10.0 ** rng.uniform(-12, 3, z.size)
    sd[:special.size] = 2.0 ** rng.randint(-40, 10, special.size)       # a power of two: aa / sd gives the special z back exactly
    sd[-4:] = [1e-12, 1e3, 1e-12, 1e3]
    y_max = 0.0                                                         # (with xi = 0: aa = mu, the fp64 value the truth takes as given)
    mu = z * sd
    dmu, dsd = rng.standard_normal((z.size, 2)), rng.standard_normal((z.size, 2))
    return mu, sd, y_max, dmu, dsd


@pytest.fixture(scope="module")
def sweep():
    mu, sd, y_max, dmu, dsd = _z_sweep()
    return mu, sd, y_max, dmu, dsd, L.log_ei_truth(mu, sd, y_max, 0.0, dmu, dsd)


def _policy(y_max=None, xi=XI, **kw):
    p = A.LogExpectedImprovement(xi=xi, **kw)
    p.y_max = y_max
    return p


def test_the_sweep_covers_the_range_and_both_switches(sweep):
    z = sweep[5]["z"]
    assert sweep[5]["ok"].all() and z.min() <= -9e7 and z.max() >= 7.9
    for point in (-1.0, L.SERIES_BELOW):
        assert np.any(z == point) and np.any(z == np.nextafter(point, -np.inf)) and np.any(z == np.nextafter(point, np.inf))
    assert all(np.sum((z >= a) & (z < b)) >= 50 for a, b in ((-1e8, -1e4), (-1e4, -40), (-40, -28), (-28, -8), (-8, -1), (-1, 8)))


@pytest.mark.parametrize("which", ["restatement", "policy"])
def test_values_and_gradients_against_the_truth(sweep, which):
    mu, sd, y_max, dmu, dsd, tr = sweep
    if which == "restatement":
        v, g = L.reference_values(mu, sd, y_max, 0.0, dmu, dsd)
    else:
        p = _policy(y_max, xi=0.0)
        v = p.base_acq(mu, sd)
        v2, dv = p.base_acq_grad(mu, sd, dmu, dsd)
        assert np.array_equal(v, v2)
        g = -dv
    c, cg = T.constants(v, tr["log_ei"], tr["w"], floor=0.0), T.constants(g, tr["g"], tr["w_g"], floor=0.0)
    print(f"{which}: value c {T.worst(c):.3f} at z {tr['z'][np.nanargmax(c)]:.4g}; gradient c {T.worst(cg):.3f} at z "
          f"{tr['z'][np.nanargmax(cg.max(1))]:.4g}")
    assert np.isfinite(v).all() and np.isfinite(g).all()
    assert T.worst(c) <= BAR and T.worst(cg) <= BAR


def test_conventions():
    y_max, xi = 0.5, 0.25                                          # (binary fractions: aa = 0 exactly at mu = 0.75)
    mu = np.array([1.0, 0.2, 0.75, np.nan, 1.0, np.nan])
    sd = np.array([0.0, 0.0, 0.0, 1.0, np.nan, 0.0])
    want = np.array([np.log(0.25), -np.inf, -np.inf, np.nan, np.nan, np.nan])
    d = np.ones((6, 2))
    for v, g in (L.reference_values(mu, sd, y_max, xi, d, d),
                 (_policy(y_max, xi).base_acq(mu, sd), -_policy(y_max, xi).base_acq_grad(mu, sd, d, d)[1])):
        assert np.array_equal(v, want, equal_nan=True)
        assert np.array_equal(g[:3], np.zeros((3, 2)))             # a clipped variance has no slope
    # the selection key -logEI: +inf sorts after every finite value, NaN last, and argmin is the first NaN
    ys = -want
    assert np.array_equal(np.argsort(ys, kind="stable"), [0, 1, 2, 3, 4, 5]) and int(np.argmin(ys)) == 3
    with pytest.raises(ValueError, match="y_max is not set"):
        A.LogExpectedImprovement().base_acq(mu, sd)


# ---- against EI: the same order where EI is representable, an answer where it is not ------------------------------------------------
N_TRAIN, DIM, LS, NOISE = 64, 2, 0.05, 1e-6          # tests/test_gpu_acq_regimes.py's model


def _posterior(M, seed):
    rng = np.random.RandomState(7)
    X = rng.uniform(size=(N_TRAIN, DIM))
    y = np.sin(3 * X.sum(1)) + 0.05 * rng.randn(N_TRAIN)
    gp = O.fit_fixed_theta(O.MATERN25, X, y, LS, NOISE)
    return O.predict(gp, np.random.RandomState(seed).uniform(size=(M, DIM)))


def test_the_order_is_eis_where_ei_is_normal():
    """y_max inside the means' range: every pair of candidates that both truths decide (values further apart than the two bars) is
    ordered the same way by -logEI and by -EI, and as the truth orders it.  With candidate seed 11 the truth alone leaves none of the
    44 850 pairs undecided (two candidates closer than rounding tells apart); 1 % is allowed."""
    mu, sd = _posterior(300, 11)
    y_max = float(np.median(mu))
    tl, te = L.log_ei_truth(mu, sd, y_max, XI), T.acq_truth(mu, sd, y_max, XI)
    assert tl["ok"].all() and te["ok"].all()
    log_ei = _policy(y_max).base_acq(mu, sd)
    ei_policy = A.ExpectedImprovement(xi=XI)
    ei_policy.y_max = y_max
    ei = ei_policy.base_acq(mu, sd)
    bar_l = [BAR * T.EPS * w for w in tl["w"]]
    bar_e = [BAR * T.EPS * w + T.DBL_MIN for w in te["w_ei"]]
    n, undecided, wrong = len(mu), 0, []
    for i in range(n):
        for j in range(i + 1, n):
            gl, ge = tl["log_ei"][i] - tl["log_ei"][j], te["ei"][i] - te["ei"][j]
            if abs(gl) <= bar_l[i] + bar_l[j] or abs(ge) <= bar_e[i] + bar_e[j]:
                undecided += 1
                continue
            assert (gl > 0) == (ge > 0)                    # (the logarithm is monotone: the two truths agree)
            if (log_ei[i] > log_ei[j]) != (gl > 0) or (ei[i] > ei[j]) != (gl > 0):
                wrong.append((i, j))
    pairs = n * (n - 1) // 2
    print(f"undecided pairs {undecided}/{pairs} = {undecided / pairs:.5f}")
    assert undecided <= 0.01 * pairs
    assert not wrong
    if undecided == 0:
        assert np.array_equal(np.argsort(-log_ei, kind="stable"), np.argsort(-ei, kind="stable"))


def test_an_answer_where_every_ei_is_zero():
    mu, sd = _posterior(2048, 8)
    y_max = float(mu.max()) + 60.0 * float(np.median(sd))
    ei_policy = A.ExpectedImprovement(xi=XI)
    ei_policy.y_max = y_max
    ei = ei_policy.base_acq(mu, sd)
    assert np.all(ei == 0.0) and int(np.argmin(-1 * ei)) == 0          # the plateau: candidate 0, whatever it is
    tr = L.log_ei_truth(mu, sd, y_max, XI)
    order = L.argbest([-v for v in tr["log_ei"]])
    gap = tr["log_ei"][order[0]] - tr["log_ei"][order[1]]
    assert gap > BAR * T.EPS * (tr["w"][order[0]] + tr["w"][order[1]]), "the truth does not decide the pick: another seed"
    neg = -1 * _policy(y_max).base_acq(mu, sd)
    assert np.isfinite(neg).all() and int(np.argmin(neg)) == order[0] != 0
    assert T.worst(T.constants(-neg, tr["log_ei"], tr["w"], floor=0.0)) <= BAR


# ---- the policy protocol -----------------------------------------------------------------------------------------------------------
class LogEiFakeEngine(FakeEngine):
    """FakeEngine + acquisition kind 3 (from log_ei_truth's restatement, not from the policy) + posterior_refresh = the full posterior"""

    def acq_argbest(self, acq, param, y_max=0.0, lb=None, ub=None, k_seeds=0, index_offset=0, return_values=False):
        if acq != LOG_EI:
            return super().acq_argbest(acq, param, y_max, lb, ub, k_seeds, index_offset, return_values)
        assert lb is None and ub is None, "kind 3 takes no constraints"
        self.calls.append(("acq_argbest", acq, k_seeds))
        mu, sd = self.post[0]
        ys = -1 * L.reference_values(mu, sd, y_max, param)
        nan = np.isnan(ys)
        order = np.lexsort((np.arange(len(ys)), np.where(nan, np.inf, ys) + 0.0, nan))[:k_seeds]
        bi = int(np.flatnonzero(nan)[0]) if nan.any() else int(ys.argmin())
        return bi + index_offset, float(ys[bi]), order + index_offset, ys[order], (ys if return_values else None)

    def polish_seeds(self, acq, param, y_max, lb, ub, y_means, y_stds, seeds, box, max_iter=0):
        if acq != LOG_EI:
            return super().polish_seeds(acq, param, y_max, lb, ub, y_means, y_stds, seeds, box, max_iter)
        import copy

        from scipy.optimize import minimize

        assert lb is None and ub is None, "kind 3 takes no constraints"
        self.calls.append(("polish_seeds", acq, len(seeds)))
        gp = copy.copy(self.models[0])
        gp.y_mean, gp.y_std = float(y_means[0]), float(y_stds[0])

        def f_grad(x):
            mu, sd, dmu, dsd = O.predict_grad(gp, x[None])
            v, g = L.reference_values(mu, sd, float(y_max), param, dmu, dsd)
            return -float(v[0]), g[0]

        res = [minimize(f_grad, s0, jac=True, bounds=np.asarray(box, dtype=np.float64), method="L-BFGS-B")
               for s0 in np.asarray(seeds, dtype=np.float64)]
        self._resident = False
        return (np.array([r.x for r in res]), np.array([float(r.fun) for r in res]),
                np.array([0 if r.success else 2 for r in res], dtype=np.int32), 0)

    def posterior_refresh(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True, return_route=False):
        self.calls.append(("posterior_refresh", slot))
        mu, sd = O.predict(self.models[slot], self.Xc)
        mu, sd = y_std * mu + y_mean, sd * y_std
        self.post[slot] = (mu, sd)
        out = (mu, sd) if fetch else (None, None)
        return (*out, 1) if return_route else out


D, N, M = 3, 30, 1500
BOUNDS = np.array([[0.0, 1.0], [-1.0, 2.0], [0.5, 1.5]])


def _driver(policy, seed=3):
    rng = np.random.RandomState(0)
    X = BOUNDS[:, 0] + rng.uniform(size=(N, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2 + 0.05 * rng.standard_normal(N)
    eng = LogEiFakeEngine()
    return B.Driver(eng, X, y, BOUNDS, policy, seed=seed, n_random=M, lml_on_device=False), eng, y


def test_the_engine_is_asked_for_kind_three_and_the_pick_is_the_truths():
    assert A.LogExpectedImprovement._acq_kind == LOG_EI == A.E.LOG_EI
    assert A.LogExpectedImprovement not in A._STOCK_POLICIES        # the device differential evolution stays refused
    policy = A.LogExpectedImprovement()
    assert policy.xi == 0.01
    drv, eng, y = _driver(policy)
    x = drv.suggest_first()
    assert ("acq_argbest", LOG_EI, 0) in eng.calls and policy.y_max == float(y.max()) and policy.i == 1
    mu, sd = eng.post[0]
    tr = L.log_ei_truth(mu, sd, policy.y_max, policy.xi)
    order = L.argbest([-v for v in tr["log_ei"]])
    assert tr["log_ei"][order[0]] - tr["log_ei"][order[1]] > BAR * T.EPS * (tr["w"][order[0]] + tr["w"][order[1]])
    assert B.rows_to_indices([x], eng.Xc)[0] == order[0]
    # with local searches: the one-call form on the engine (kind 3 again), then SciPy over the host objective (base_acq)
    f = policy._get_acq(gp=drv._gp)
    f_pick = float(f(x)[0])
    for device_polish in ("auto", False):
        policy.device_polish = device_polish
        x2 = policy.suggest(gp=drv._gp, target_space=drv._space, n_random=M, n_smart=3, fit_gp=False, random_state=np.random.RandomState(5))
        assert np.all(x2 >= BOUNDS[:, 0]) and np.all(x2 <= BOUNDS[:, 1]) and np.isfinite(f(x2)).all()
    assert ("polish_seeds", LOG_EI, 3) in eng.calls and [c[:2] for c in eng.calls].count(("polish_seeds", LOG_EI)) == 1
    assert np.isfinite(f_pick)


def test_warm_up_runs_the_new_kind():
    """dropin.warm_up swallows what a synthetic suggest() raises: look at the engine calls it made instead"""
    from bayesianoptimization_amd.dropin import warm_up

    eng = LogEiFakeEngine()
    took = warm_up(eng, BOUNDS, acquisition=A.LogExpectedImprovement(), n_restarts_optimizer=0, n_random=M, lml_on_device=False, sizes=(12,))
    assert took > 0.0
    assert ("acq_argbest", LOG_EI, 10) in eng.calls and ("polish_seeds", LOG_EI, 10) in eng.calls


def test_a_constrained_space_is_refused():
    space = types.SimpleNamespace(constraint=object())
    with pytest.raises(A.ConstraintNotSupportedError, match="does not support constrained optimization"):
        A.LogExpectedImprovement().suggest(gp=None, target_space=space)


def test_parameters_decay_and_counter():
    with pytest.raises(ValueError):
        A.LogExpectedImprovement(exploration_decay=1.5)
    policy = A.LogExpectedImprovement(xi=0.1, exploration_decay=0.5, exploration_decay_delay=2)
    assert policy.get_acquisition_params() == {"xi": 0.1, "exploration_decay": 0.5, "exploration_decay_delay": 2}
    drv, eng, _ = _driver(policy)
    drv.suggest_first()
    assert policy.i == 1 and policy.xi == 0.1                      # the delay has not passed
    drv.suggest_first()
    assert policy.i == 2 and policy.xi == 0.05
    other = A.LogExpectedImprovement()
    other.set_acquisition_params(policy.get_acquisition_params())
    assert other.get_acquisition_params() == {"xi": 0.05, "exploration_decay": 0.5, "exploration_decay_delay": 2}


def test_the_package_exports_it():
    import bayesianoptimization_amd as pkg

    assert "LogExpectedImprovement" in pkg.__all__ and pkg.LogExpectedImprovement is A.LogExpectedImprovement
    assert issubclass(pkg.LogExpectedImprovement, A._ImprovementBased)


def test_suggest_batch_accepts_it():
    policy = A.LogExpectedImprovement()
    drv, eng, y = _driver(policy)
    picks = suggest_batch(drv, 3)
    idx = B.rows_to_indices(picks, eng.Xc)
    assert len(picks) == 3 and len(set(idx.tolist())) == 3
    assert policy.i == 3 and policy.y_max == float(y.max())         # 'max': the lie is the incumbent
    assert [c[0] for c in eng.calls].count("posterior_refresh") == 2
