"""CPU: constrained Thompson sampling's host side — the NumPy restatement of the rule (tests/scbo_truth.py) on hand-made arrays,
`suggest_constrained_thompson` and `suggest_scbo` over an engine double (the documented RandomState draws replayed on a twin, the
gate, the restart design, the centre), the `ConstrainedTrustRegion` state machine, the header.  The device pass itself is checked in
tests/test_gpu_constrained_paths.py."""
import os
import re
import warnings

import numpy as np
import pytest

import batch_truth as B
import scbo_truth as ST
import turbo_truth as T
from bayesianoptimization_amd import (ConstrainedTrustRegion, TrustRegion, _lib, scbo, sobol_tables, suggest_constrained_thompson,
                                      suggest_scbo)
from bayesianoptimization_amd import _suggest as S
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.constraint_model import HipConstraintModel
from bayesianoptimization_amd.engine import GpEngine, GroupEngine
from bayesianoptimization_amd.float_space import FloatSpace, MixedSpace
from bayesianoptimization_amd.thompson import spectral_draw
from conftest import ROOT

D, N, M = 3, 30, 600
INF = np.inf
PBOUNDS = {f"x{j}": tuple(b) for j, b in enumerate(B.SUGGEST_BOUNDS)}


def constraint_values(X, n_constraints=1):
    c = np.column_stack([np.cos(X.sum(1)), X[:, 0] - X[:, 1]])[:, :n_constraints]
    return c[:, 0] if n_constraints == 1 else c


def constrained_driver(engine_class=ST.ScboFakeEngine, lb=(-INF,), ub=(0.5,), **kw):
    """(driver, engine, X, y, c): batch_truth's driver over a space with len(lb) constraints, constraint j's GP in slot j"""
    drv, eng, X, y = B.suggest_driver(engine_class, n_random=M, **kw)
    cm = HipConstraintModel(None, np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64), engine=eng,
                            random_state=np.random.RandomState(3))
    for g in cm.model:
        g.lml_on_device = False
    c = constraint_values(X, len(lb))
    drv._space = FloatSpace(PBOUNDS, constraint=cm)
    drv._space.register_bulk(X, y, c)
    return drv, eng, X, y, c


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_rule_on_hand_made_arrays():
    nan = np.nan
    f = np.array([[1.0, 5.0, 3.0, 5.0, 2.0],       # feasible: 0, 2, 3, 4 -> the maximum 5.0 at index 3 (index 1 is infeasible)
                  [9.0, 8.0, 7.0, 6.0, 5.0],       # nothing feasible -> the least violation
                  [1.0, 4.0, 4.0, 0.0, 4.0],       # a tie among the feasible -> the lower index
                  [1.0, nan, 3.0, 2.0, 0.0],       # a NaN value wins
                  [1.0, 2.0, 3.0, 2.0, 0.0]])      # a NaN constraint value wins, the first of two
    c1 = np.array([[0.0, 2.0, 0.5, 1.0, -3.0],
                   [3.0, 2.0, 2.0, 4.0, 5.0],
                   [0.0, 0.5, 0.5, 0.5, 0.5],
                   [0.0, 0.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, nan, 0.0, nan]])
    c2 = np.array([[0.0, 0.0, 0.0, 0.0, 0.0],
                   [-2.0, -1.0, -1.0, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0]])
    lb, ub, y_std = np.array([-INF, -0.5]), np.array([1.0, INF]), np.array([7.0, 2.0, 0.5])
    idx, val, bv, feas, viol = ST.rule(np.array([f, c1, c2]), lb, ub, y_std, index_offset=100)
    assert idx.tolist() == [103, 101, 101, 101, 102]
    assert feas.tolist() == [True, False, True, False, False]
    assert val[:3].tolist() == [5.0, 8.0, 4.0] and np.isnan(val[3:]).all()
    assert bv[:3].tolist() == [0.0, 0.5 + 1.0, 0.0] and np.isnan(bv[3:]).all()
    # the violation itself: one-sided bounds (an infinite bound never adds), the division by the slot's y_std, the order of the sum
    assert viol[0].tolist() == [0.0, 0.5, 0.0, 0.0, 0.0]
    assert viol[1].tolist() == [1.0 + 3.0, 0.5 + 1.0, 0.5 + 1.0, 1.5, 2.0]
    assert np.isnan(viol[4, [2, 4]]).all() and (viol[4, [0, 1, 3]] == 0.0).all()
    # both bounds infinite: every candidate is feasible, the pick is the argmax
    i2, v2, b2, f2, _ = ST.rule(np.array([f[:3], c1[:3]]), np.array([-INF]), np.array([INF]), np.array([1.0, 1.0]))
    assert i2.tolist() == [1, 0, 1] and f2.all() and (b2 == 0.0).all() and v2.tolist() == [5.0, 9.0, 4.0]
    # the least violation's tie goes to the lower index
    i3, _, b3, f3, _ = ST.rule(np.array([f[1:2], c1[1:2]]), np.array([-INF]), np.array([1.0]), np.array([1.0, 1.0]))
    assert i3.tolist() == [1] and b3.tolist() == [1.0] and not f3.any()
    # the package's own host restatement (the violation of observed rows) agrees
    got = scbo.violation(np.column_stack([c1[1], c2[1]]), lb, ub, y_std[1:])
    assert got.tolist() == viol[1].tolist()


# ---- suggest_constrained_thompson ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,n_constraints", [(5, 1), (17, 2)])
def test_draws_calls_and_picks(q, n_constraints):
    FEATURES = 48
    lb, ub = ((-INF,), (0.5,)) if n_constraints == 1 else ((-INF, -1.0), (0.5, 1.5))
    drv, eng, X, y, c = constrained_driver(lb=lb, ub=ub)
    twin, teng, _, _, _ = constrained_driver(lb=lb, ub=ub)
    picks = suggest_constrained_thompson(drv, q, n_random=M, n_features=FEATURES)
    assert len(picks) == q and list(picks[0]) == drv._space.keys and drv._acquisition_function.i == 0
    # the replay: the fits (theta searches included), the candidates, then per group and slot the documented draws
    rng = twin._random_state
    gps = [twin._gp, *twin._space.constraint.model]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        twin._gp.fit(twin._space.params, twin._space.target)
        twin._space.constraint.fit(twin._space.params, twin._space._constraint_values)
    teng.generate_candidates_like(M, B.SUGGEST_BOUNDS[:, 0], B.SUGGEST_BOUNDS[:, 1], rng)
    assert np.array_equal(teng.Xc, eng.Xc)
    want, groups = [], [(f, min(16, q - f)) for f in range(0, q, 16)]
    assert len(eng.constrained_args) == len(groups)
    for (first, n), got in zip(groups, eng.constrained_args):
        draws = []
        for g in gps:
            omega, phase = spectral_draw(g._kind, FEATURES, D, rng)
            w = rng.standard_normal((n, FEATURES))
            eps = rng.standard_normal((n, N)) * np.sqrt(float(g.alpha))
            draws.append((omega, phase, w, eps))
        assert len(got["draws"]) == 1 + n_constraints
        for a, b in zip(got["draws"], draws):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        assert np.array_equal(got["lb"], lb) and np.array_equal(got["ub"], ub)
        assert got["y_mean"].tolist() == [float(g._y_train_mean) for g in gps]
        assert got["y_std"].tolist() == [float(g._y_train_std) for g in gps]
        want.extend(teng.sample_paths_constrained(draws, np.array(lb), np.array(ub), got["y_mean"], got["y_std"])[0].tolist())
    assert B.same_state(drv._random_state, rng)
    assert B.rows_to_indices(picks, eng.Xc).tolist() == want
    # the picks are the rule's on the double's own values: a feasible pick is inside the bounds under its draw
    vals = eng.constrained_values[0]
    idx, _, bv, feas, _ = ST.rule(vals, np.array(lb), np.array(ub), eng.constrained_args[0]["y_std"])
    assert idx.tolist() == want[:len(idx)]
    for s in np.flatnonzero(feas):
        assert all(lb[j] <= vals[j + 1, s, idx[s]] <= ub[j] for j in range(n_constraints)) and bv[s] == 0.0
    names = [k[0] for k in eng.calls]
    assert names.count("fit") == 1 + n_constraints and names.count("generate_candidates_like") == 1
    assert names.count("sample_paths_constrained") == len(groups)
    assert not {"posterior", "set_candidates", "sample_paths", "acq_argbest"} & set(names)
    assert max(i for i, k in enumerate(names) if k == "fit") < names.index("generate_candidates_like") < names.index("sample_paths_constrained")
    # afterwards the models answer for the real data as before
    pts = X[:4]
    assert np.array_equal(drv._gp.predict(pts), twin._gp.predict(pts))
    assert np.array_equal(drv._space.constraint.predict(pts), twin._space.constraint.predict(pts))


def _spoil_table(who):
    def no_points(drv, eng):
        drv._space = FloatSpace(PBOUNDS, constraint=drv._space.constraint)

    def unconstrained(drv, eng):
        X, y = B.suggest_data()
        drv._space = FloatSpace(PBOUNDS)
        drv._space.register_bulk(X, y)

    def foreign_constraint(drv, eng):
        cm = drv._space.constraint
        drv._space._constraint = type("Foreign", (), {"lb": cm.lb, "ub": cm.ub, "model": cm.model, "_model": cm._model})()

    def constraint_gp_object(drv, eng):
        drv._space.constraint._model[0] = object()

    def constraint_other_engine(drv, eng):
        drv._space.constraint._model[0].engine = ST.ScboFakeEngine()

    def constraint_other_slot(drv, eng):
        drv._space.constraint._model[0].slot = 2

    def constraint_transform(drv, eng):
        drv._space.constraint._model[0].transform = MixedSpace({"x0": (0.0, 1.0), "x1": (-1, 2, int), "x2": (0.5, 1.5)}).kernel_transform

    def constraint_host_kernel(drv, eng):
        from sklearn.gaussian_process.kernels import RationalQuadratic

        drv._space.constraint._model[0].kernel = RationalQuadratic()

    def int_parameter(drv, eng):
        drv._gp.transform = MixedSpace({"x0": (0.0, 1.0), "x1": (-1, 2, int), "x2": (0.5, 1.5)}).kernel_transform

    def foreign_gp(drv, eng):
        drv._gp = object()

    def slot_1(drv, eng):
        drv._gp.slot = 1

    def device_group(drv, eng):
        drv._gp.engine = object.__new__(GroupEngine)
        drv._gp.engine.__dict__.update(_g=None, _h=None)

    from sklearn.gaussian_process.kernels import RationalQuadratic

    other = "suggest_thompson" if who == "suggest_constrained_thompson" else "suggest_turbo"
    return [(no_points, {}, A.TargetSpaceEmptyError, "without previous samples"),
            (unconstrained, {}, ValueError, f"{who}: the space has no constraint; use {other}"),
            (foreign_constraint, {}, NotImplementedError, f"{who}: .*HipConstraintModel"),
            (constraint_gp_object, {}, NotImplementedError, f"{who}: constraint 1's GP is not on the optimizer's engine in slot 1"),
            (constraint_other_engine, {}, NotImplementedError, f"{who}: constraint 1's GP is not on the optimizer's engine in slot 1"),
            (constraint_other_slot, {}, NotImplementedError, f"{who}: constraint 1's GP is not on the optimizer's engine in slot 1"),
            (constraint_transform, {}, NotImplementedError, f"{who}: constraint 1's GP has an input transform"),
            (constraint_host_kernel, {}, NotImplementedError, f"{who}: constraint 1's model runs on the host"),
            (int_parameter, {}, NotImplementedError, f"{who}: the space has an input transform"),
            (foreign_gp, {}, NotImplementedError, f"{who}: .*accelerate"),
            (slot_1, {}, NotImplementedError, f"{who}: .*accelerate"),
            (lambda *a: None, {"kernel": RationalQuadratic()}, NotImplementedError, f"{who}: the model runs on the host"),
            (device_group, {}, NotImplementedError, f"{who}: a device group")]


@pytest.mark.parametrize("who", ["suggest_constrained_thompson", "suggest_scbo"])
def test_the_gate_refuses_before_anything_runs(who):
    """Everything batch_truth.check_shared_refusals lists except the constraint scenario (a constraint is what these functions are
    for), and what can be wrong with the constraint model itself: the exception, its text, no engine call."""
    def call(drv):
        if who == "suggest_scbo":
            return suggest_scbo(drv, 4, ConstrainedTrustRegion(D, 4))
        return suggest_constrained_thompson(drv, 2)

    for spoil, kw, error, match in _spoil_table(who):
        drv, eng, X, y, c = constrained_driver(**kw)
        before = drv._random_state.get_state()
        spoil(drv, eng)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(error, match=match):
                call(drv)
        assert not eng.calls, (getattr(spoil, "__name__", "host_kernel"), eng.calls)
        after = drv._random_state.get_state()
        assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    with pytest.raises(NotImplementedError, match="device group has no constrained path sampler"):
        GroupEngine.sample_paths_constrained(object.__new__(GroupEngine), [], [], [], [], [])


def test_argument_checks_come_first():
    drv, eng, X, y, c = constrained_driver()
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="q must be"):
            suggest_constrained_thompson(drv, bad)
    with pytest.raises(ValueError, match="n_random"):
        suggest_constrained_thompson(drv, 2, n_random=0)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="n_features"):
            suggest_constrained_thompson(drv, 2, n_features=bad)
    ok = ConstrainedTrustRegion(D, 4)
    for bad in (None, object(), TrustRegion(D, 4), ConstrainedTrustRegion(D + 1, 4), ConstrainedTrustRegion(D, 5)):
        with pytest.raises(ValueError, match="ConstrainedTrustRegion"):
            suggest_scbo(drv, 4, bad)
    for bad in (0, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="n_random"):
            suggest_scbo(drv, 4, ok, n_random=bad)
    for bad in (0, 0.0, -0.5, 1.5, True, "1"):
        with pytest.raises(ValueError, match="perturb"):
            suggest_scbo(drv, 4, ok, perturb=bad)
    with pytest.raises(TypeError):
        suggest_scbo(drv, 4, ok, refine=1)               # out of scope: a climbed draw can leave the feasible set
    with pytest.raises(TypeError):
        suggest_constrained_thompson(drv, 2, refine=1)
    drv._gp = object()
    with pytest.raises(ValueError, match="q must be"):   # the caller's own checks before the gate
        suggest_constrained_thompson(drv, 0)
    assert not eng.calls and ok.seen is None
    # an engine without the call
    import paths_truth as P

    drv, eng, X, y, c = constrained_driver(P.PathsFakeEngine)
    with pytest.raises(NotImplementedError, match="the engine has no sample_paths_constrained"):
        suggest_constrained_thompson(drv, 2)
    assert not eng.calls


def test_the_default_gate_is_unchanged():
    """`constrained` is off by default: a constraint is still ConstraintNotSupportedError, with the old text."""
    drv, eng, X, y, c = constrained_driver()
    with pytest.raises(A.ConstraintNotSupportedError, match="Received constraints, but f does not support constrained optimization."):
        S.gate(drv, "f", "sampled", ("sample_paths",), "g")
    gp, space, got = S.gate(drv, "f", "sampled", ("sample_paths",), "g", constrained=True)
    assert gp is drv._gp and space is drv._space and got is eng and not eng.calls


# ---- ConstrainedTrustRegion -----------------------------------------------------------------------------------------------------------
def test_constrained_trust_region_improvement_rule():
    s = ConstrainedTrustRegion(8, 4)
    assert s.best == -INF and s.best_violation == INF and s.failure_tolerance == 2 and s.success_tolerance == 3
    s.observe([], [])
    assert s.seen is None and s.successes == s.failures == 0
    with pytest.raises(ValueError, match="same length"):
        s.observe([1.0], [0.0, 1.0])
    s.observe([5.0, 1.0], [2.0, 3.0])                       # nothing feasible yet: any finite violation improves on inf
    assert (s.successes, s.failures, s.best, s.best_violation, s.seen) == (1, 0, -INF, 2.0, 2)
    s.observe([9.0], [1.999])                               # within rel_improvement of best_violation: a failure; it still falls
    assert (s.successes, s.failures, s.best_violation) == (0, 1, 1.999)
    s.observe([9.0], [1.0])                                 # clearly lower: a success
    assert (s.successes, s.failures, s.best_violation, s.best) == (1, 0, 1.0, -INF)
    s.observe([100.0, -7.0], [0.5, 0.0])                    # the first feasible point beats -inf, whatever its target
    assert (s.successes, s.failures, s.best, s.best_violation) == (2, 0, -7.0, 0.0)
    s.observe([100.0], [0.5])                               # infeasible after a feasible one: a failure, however small the violation
    assert (s.successes, s.failures, s.best) == (0, 1, -7.0)
    s.observe([-6.999, 50.0], [0.0, 1e-9])                  # feasible but within rel_improvement |best|: the second failure -> halve
    assert (s.successes, s.failures, s.length, s.best) == (0, 0, 0.4, -6.999)
    for k, top in enumerate([-6.0, -5.0]):
        s.observe([top, 1e9], [0.0, 4.0])                   # the infeasible 1e9 does not count
        assert (s.successes, s.failures, s.best) == (k + 1, 0, top)
    s.observe([-4.0], [0.0])                                # the third success in a row: double
    assert (s.successes, s.length, s.best) == (0, 0.8, -4.0)


def test_constrained_trust_region_restart_clears_best_violation():
    s = ConstrainedTrustRegion(2, 1, length=0.5 ** 7, failure_tolerance=1)
    s.observe([1.0], [3.0])
    assert s.best_violation == 3.0 and s.restarts == 0 and s.successes == 1
    s.observe([1.0], [3.0])                                 # a failure at the minimum length: restart
    assert (s.restarts, s.length, s.successes, s.failures, s.best, s.best_violation, s.origin, s.seen, s.design_pending) == \
        (1, 0.5 ** 7, 0, 0, -INF, INF, 2, 2, True)
    s.observe([0.0], [7.0])                                 # after the restart any violation improves again
    assert s.successes == 1 and s.best_violation == 7.0


def test_trust_region_is_as_before():
    s = TrustRegion(8, 4)
    assert not hasattr(s, "best_violation")
    s.observe([1.0, 0.5])
    assert (s.successes, s.failures, s.best, s.seen, s.length) == (1, 0, 1.0, 2, 0.8)
    s.observe([1.0])
    s.observe([1.0005])
    assert (s.successes, s.failures, s.length, s.best) == (0, 0, 0.4, 1.0005)
    with pytest.raises(TypeError):
        s.observe([1.0], [0.0])
    t = TrustRegion(2, 1, length=0.5 ** 7, failure_tolerance=1)
    t.observe([1.0])
    t.observe([1.0])
    assert (t.restarts, t.best, t.origin, t.design_pending) == (1, -INF, 2, True)
    # the box is inherited, not changed
    lo, hi = ConstrainedTrustRegion(3, 2, length=0.4).box([0.5, 0.5, 1.0], [1.0, 2.0, 0.5], B.SUGGEST_BOUNDS)
    lo2, hi2 = TrustRegion(3, 2, length=0.4).box([0.5, 0.5, 1.0], [1.0, 2.0, 0.5], B.SUGGEST_BOUNDS)
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2)


# ---- suggest_scbo ---------------------------------------------------------------------------------------------------------------------
def _replay_seeds(rng):
    return int(rng.randint(0, 2 ** 31 - 1)), int(rng.randint(0, 2 ** 63 - 1, dtype=np.int64))


def test_scbo_step_centre_box_and_draws():
    drv, eng, X, y, c = constrained_driver()
    twin, teng, _, _, _ = constrained_driver()
    state = ConstrainedTrustRegion(D, 5, length=0.4)
    picks = suggest_scbo(drv, 5, state, n_random=M, n_features=32)
    viol = np.maximum(c - 0.5, 0.0) / np.std(c)
    feasible = viol == 0.0
    assert feasible.any() and not feasible.all()
    assert np.array_equal(scbo.observed_violation(drv._space), viol)
    assert (state.seen, state.best, state.best_violation, state.successes, state.failures) == (N, y[feasible].max(), 0.0, 0, 0)
    # the centre is the best FEASIBLE row (here not the best row), the box from the TARGET GP's length scales
    centre = X[int(np.argmax(np.where(feasible, y, -INF)))]
    rng = twin._random_state
    gps, models = scbo._fit_models(twin._gp, twin._space, teng, "twin")
    seed, key = _replay_seeds(rng)
    lo, hi = TrustRegion(D, 5, length=0.4).box(centre, np.atleast_1d(twin._gp.kernel_.length_scale), B.SUGGEST_BOUNDS)
    a = eng.tr_args
    sv, shift = sobol_tables(D, seed)
    assert a["M"] == M and a["bits"] == 30 and a["key"] == key and a["threshold"] == 2 ** 32
    assert np.array_equal(a["centre"], centre) and np.array_equal(a["lo"], lo) and np.array_equal(a["hi"], hi)
    assert np.array_equal(a["sv"], sv) and np.array_equal(a["shift"], shift)
    teng.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, 30, 2 ** 32, key)
    want = scbo.constrained_picks(gps, models, twin._space, teng, rng, 5, 32)
    assert picks == want and B.same_state(drv._random_state, rng)
    names = [k[0] for k in eng.calls]
    assert names.count("fit") == 2 and names.count("generate_candidates_trust_region") == 1
    assert names.count("sample_paths_constrained") == 1 and "generate_candidates_like" not in names and "sample_paths" not in names
    rows = np.array([list(p.values()) for p in picks])
    assert (rows >= lo).all() and (rows <= hi).all()
    B.rows_to_indices(picks, eng.Xc)


def test_scbo_centre_is_the_least_violation_row_when_nothing_is_feasible():
    drv, eng, X, y, c = constrained_driver(lb=(2.0,), ub=(3.0,))              # cos(.) never reaches 2
    state = ConstrainedTrustRegion(D, 2)
    suggest_scbo(drv, 2, state, n_random=64, n_features=16, perturb=0.25)
    viol = (2.0 - c) / np.std(c)
    assert (state.best, state.best_violation) == (-INF, viol.min())
    assert np.array_equal(eng.tr_args["centre"], X[int(np.argmin(viol))]) and eng.tr_args["threshold"] == 2 ** 30
    # the caller registers results; the next call recomputes best_violation with the new stds, then observes the new rows
    drv._space.register(np.array([0.5, 0.5, 1.0]), 0.0, 1.9)                  # lower violation: a success
    drv._space.register(np.array([0.6, 0.5, 1.0]), 9.0, -5.0)
    suggest_scbo(drv, 2, state, n_random=64, n_features=16)
    c2 = np.concatenate([c, [1.9, -5.0]])
    viol2 = (2.0 - c2) / np.std(c2)
    assert (state.seen, state.successes, state.failures, state.best) == (N + 2, 1, 0, -INF)
    assert state.best_violation == viol2.min() == viol2[N] and np.array_equal(eng.tr_args["centre"], [0.5, 0.5, 1.0])
    drv._space.register(np.array([0.7, 0.5, 1.0]), -3.0, 2.5)                 # the first feasible row: a success, and the centre
    drv._space.register(np.array([0.8, 0.5, 1.0]), 50.0, 1.99)
    suggest_scbo(drv, 2, state, n_random=64, n_features=16)
    assert (state.seen, state.successes, state.best, state.best_violation) == (N + 4, 2, -3.0, 0.0)
    assert np.array_equal(eng.tr_args["centre"], [0.7, 0.5, 1.0])
    suggest_scbo(drv, 2, state, n_random=64, n_features=16)                   # nothing new: nothing observed
    assert (state.seen, state.successes, state.failures) == (N + 4, 2, 0)


def test_scbo_design_branch_after_a_restart():
    drv, eng, X, y, c = constrained_driver()
    state = ConstrainedTrustRegion(D, 4)
    suggest_scbo(drv, 4, state, n_random=64, n_features=16)
    state.length, state.failures = state.length_min, state.failure_tolerance - 1
    for k in range(4):
        drv._space.register(np.array([0.1 * (k + 1), 0.0, 1.0]), float(y.min()) - 1.0, 0.0)
    del eng.calls[:]
    before = drv._random_state.get_state()
    picks = suggest_scbo(drv, 4, state, n_random=64, n_features=16)
    assert (state.restarts, state.design_pending, state.origin, state.seen, state.length) == (1, False, N + 4, N + 4, 0.8)
    assert (state.best, state.best_violation) == (-INF, INF)
    assert [k[0] for k in eng.calls] == ["generate_candidates_trust_region"]          # no fit, no sampling
    rng = np.random.RandomState(0)
    rng.set_state(before)
    seed, key = _replay_seeds(rng)
    assert B.same_state(rng, drv._random_state)                                        # the two seeds and nothing else
    a = eng.tr_args
    lo, hi = B.SUGGEST_BOUNDS[:, 0], B.SUGGEST_BOUNDS[:, 1]
    assert a["M"] == 4 and a["threshold"] == 2 ** 32 and a["key"] == key and np.array_equal(a["lo"], lo) and np.array_equal(a["hi"], hi)
    sv, shift = sobol_tables(D, seed)
    rows = np.array([list(p.values()) for p in picks])
    assert np.array_equal(rows, lo + (hi - lo) * T.sobol_unit(4, sv, shift))
    # the design is registered, all of it infeasible; the next call is an ordinary step centred on the least violation SINCE the restart
    for k, x in enumerate(rows):
        drv._space.register(x, 100.0 + k, 0.9 - 0.1 * k)
    suggest_scbo(drv, 4, state, n_random=64, n_features=16)
    assert np.array_equal(eng.tr_args["centre"], rows[3]) and state.best == -INF and state.successes == 1
    assert state.best_violation == scbo.observed_violation(drv._space)[N + 4:].min() > 0.0
    assert "fit" in [k[0] for k in eng.calls]


# ---- the engine method's host checks, header and bindings ---------------------------------------------------------------------------
def test_engine_method_checks_its_shapes_on_the_host():
    eng = object.__new__(GpEngine)                   # (no context: every case is refused before the library is reached)
    eng.__dict__.update(_pending_fits={}, _n_obs={0: (10, 2), 1: (12, 2)}, n_candidates=5)
    om, ph = np.zeros((4, 2)), np.zeros(4)
    good = [(om, ph, np.zeros((3, 4)), np.zeros((3, 10))), (om, ph, np.zeros((3, 4)), np.zeros((3, 12)))]
    one = np.ones(2)
    cases = [(good[:1], [], [], one[:1], one[:1]),                                                       # no constraint
             (good, [0.0, 0.0], [1.0], one, one),                                                        # lb of another length
             (good, [0.0], [1.0], one[:1], one),                                                         # y_mean of another length
             ([good[0], (om, ph, np.zeros((3, 4)), np.zeros((3, 10)))], [0.0], [1.0], one, one),         # eps does not fit slot 1's N
             ([good[0], (np.zeros((4, 3)), ph, np.zeros((3, 4)), np.zeros((3, 12)))], [0.0], [1.0], one, one),   # another d
             ([good[0], (om, ph, np.zeros((2, 4)), np.zeros((2, 12)))], [0.0], [1.0], one, one),         # another S
             ([good[0], (np.zeros((5, 2)), np.zeros(5), np.zeros((3, 5)), np.zeros((3, 12)))], [0.0], [1.0], one, one),   # another F
             ([good[0], good[1][:3]], [0.0], [1.0], one, one)]                                           # not four arrays
    for args in cases:
        with pytest.raises(ValueError, match="sample_paths_constrained"):
            eng.sample_paths_constrained(*args)


def test_exported_and_bound():
    import bayesianoptimization_amd as pkg

    for name in ("suggest_constrained_thompson", "suggest_scbo", "ConstrainedTrustRegion"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(scbo, name)
    assert issubclass(ConstrainedTrustRegion, TrustRegion)
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    m = re.search(r"^int gpbo_sample_paths_constrained\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["gpbo_sample_paths_constrained"][1]) == 19
    bound = [n for n in list(_lib.SIGNATURES) + list(_lib.DEBUG_SIGNATURES) if "constrained" in n]
    assert bound == ["gpbo_sample_paths_constrained"]                          # no group / communicator form
    assert _lib.ABI_VERSION == 4 and "#define GPBO_ABI_VERSION 4" in hdr
