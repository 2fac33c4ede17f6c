"""CPU: the mixed-space differential evolution that gpbo_evolve_mixed runs on the device.

* tests/de_walk.py restates SciPy's DifferentialEvolutionSolver in the configuration bayes_opt uses (acquisition.py:375-396) draw
  for draw on the MT19937 words; here it is held to SciPy itself bit for bit — x, fun, nit, nfev, success, the final population and
  energies and the RandomState afterwards — so the specification the kernel implements fails loudly if SciPy's walk changes.
* the gate of `AcquisitionFunction._evolve_mixed`'s device branch, over a recording test double of the engine."""
import numpy as np
import pytest
import scipy
from scipy.optimize._differentialevolution import DifferentialEvolutionSolver
from sklearn.gaussian_process.kernels import Matern

import de_walk
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.float_space import MixedSpace
from bayesianoptimization_amd.gpr import HipGPR
from helpers import FakeEngine


def _problem(D, S, seed, zero_width=False, bad=False):
    rs = np.random.RandomState(seed)
    b = np.column_stack([-3.0 * rs.rand(D), 2.0 * rs.rand(D) + 0.1])
    if zero_width:
        b[0, 1] = b[0, 0]
    init = b[:, 0] + (b[:, 1] - b[:, 0]) * rs.rand(S, D)
    f0 = de_walk.analytic(rs.rand(D) + 0.1, rs.rand(D) - 0.5, rs.rand(D) < 0.5)

    def f(x):
        if bad and x[0] < b[0, 0] + 0.2 * (b[0, 1] - b[0, 0]):
            return np.nan
        if bad and x[-1] > b[-1, 1] - 0.3 * (b[-1, 1] - b[-1, 0]):
            return np.inf
        return f0(x)

    return b, init, f, rs


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("D,S,maxiter,kw", [
    (1, 15, 1000, {}), (2, 30, 1000, {}), (5, 75, 1000, {}), (16, 240, 25, {}), (64, 960, 2, {}), (5, 5, 1000, {}),
    (3, 45, 1000, {"zero_width": True}), (4, 60, 40, {"bad": True}), (5, 75, 3, {}),
])
def test_the_restated_walk_is_scipys_bit_for_bit(D, S, maxiter, kw):
    b, init, f, rs = _problem(D, S, 10 * D + S, **kw)
    state = rs.get_state(legacy=True)
    mine = de_walk.walk(f, b, init, state[1], state[2], maxiter=maxiter)
    res = DifferentialEvolutionSolver(f, b, polish=False, init=init, rng=rs, maxiter=maxiter).solve()
    after = rs.get_state(legacy=True)
    assert _same(res.x, mine["x"]) and _same(res.fun, mine["fun"])
    assert (res.nit, res.nfev, res.success) == (mine["nit"], mine["nfev"], mine["success"])
    assert _same(res.population, mine["population"]) and _same(res.population_energies, mine["energies"])
    assert np.array_equal(after[1], mine["key"]) and after[2] == mine["pos"]
    if maxiter < 1000 and not kw:
        assert not res.success and res.nit == maxiter          # the runs cut by maxiter


def test_the_matrix_covers_nan_inf_and_the_full_budget():
    b, init, f, rs = _problem(4, 60, 100, bad=True)
    state = rs.get_state(legacy=True)
    mine = de_walk.walk(f, b, init, state[1], state[2], maxiter=40)
    e = mine["energies"]
    assert np.isnan(e).any() or np.isinf(e).any() or mine["nfev"] > 60


def test_pairwise_sum_restatement_is_numpys():
    for n in range(5, 961):
        e = np.random.RandomState(n).randn(n) * 10.0 + 3.0
        m, s = de_walk.mean_std(e)
        assert m == np.mean(e) and s == np.std(e), n


# ---- the gate ------------------------------------------------------------------------------------------------------------------
PB = {"a": (0.0, 2.0), "n": (-3, 7, int), "c": ("x", "y", "z")}


class RecordingEngine(FakeEngine):
    """FakeEngine + evolve_mixed: records its arguments and runs SciPy's solver over the host objective the test hands it."""

    objective = None

    def evolve_mixed(self, acq, param, y_max, y_mean, y_std, groups, bounds, init, random_state, maxiter=1000):
        self.calls.append(("evolve_mixed", [tuple(g[:3]) for g in groups], np.array(bounds), np.array(init),
                           random_state.get_state(legacy=True)))
        res = DifferentialEvolutionSolver(func=self.objective, bounds=bounds, polish=False, init=init, rng=random_state).solve()
        return res.x, float(res.fun), res.nit, res.nfev, res.success


class PlainEngine(FakeEngine):
    """The engine surface as it was before gpbo_evolve_mixed."""


def _suggest(eng, fn_cls=A.UpperConfidenceBound, device=False, n_obs=30, seed=3, rng=None, space=None):
    sp = space if space is not None else MixedSpace(PB)
    r = np.random.RandomState(4)
    X = sp.random_sample(n_obs, r)
    sp.register_bulk(X, np.sin(X[:, 0]) + 0.1 * X[:, 1] + X[:, 2])
    gp = HipGPR(kernel=Matern(nu=2.5, length_scale=1.3), alpha=1e-6, normalize_y=True, optimizer=None, engine=eng,
                transform=sp.kernel_transform)
    fn = fn_cls() if fn_cls in (A.UpperConfidenceBound,) or not issubclass(fn_cls, A._ImprovementBased) else fn_cls(xi=0.01)
    fn.device_evolve = device
    if isinstance(eng, RecordingEngine):
        orig = fn._get_acq

        def get_acq(gp, constraint=None):
            obj = orig(gp, constraint)
            eng.objective = obj
            return obj

        fn._get_acq = get_acq
    rs = rng if rng is not None else np.random.RandomState(seed)
    x = fn.suggest(gp, sp, n_random=200, n_smart=3, random_state=rs)
    return x, rs, fn, gp, sp


def _state_at_solver(monkeypatch, run):
    seen = []
    orig = DifferentialEvolutionSolver.__init__

    def init(self, func, bounds, **kw):
        seen.append((np.array(kw["init"]), kw["rng"].get_state(legacy=True)))
        orig(self, func, bounds, **kw)

    monkeypatch.setattr(DifferentialEvolutionSolver, "__init__", init)
    out = run()
    monkeypatch.setattr(DifferentialEvolutionSolver, "__init__", orig)
    return out, seen


def test_the_default_never_calls_the_device_walk():
    e1, e2 = RecordingEngine(), PlainEngine()
    x1, r1, *_ = _suggest(e1)
    x2, r2, *_ = _suggest(e2)
    assert not [c for c in e1.calls if c[0] == "evolve_mixed"]
    assert [c[0] for c in e1.calls] == [c[0] for c in e2.calls]
    assert np.array_equal(x1, x2) and r1.uniform() == r2.uniform()


@pytest.mark.parametrize("fn_cls", [A.UpperConfidenceBound, A.ExpectedImprovement, A.ProbabilityOfImprovement])
def test_device_evolve_is_one_call_per_suggest_with_what_the_space_implies(monkeypatch, fn_cls):
    host = PlainEngine()
    (x_h, r_h, *_), seen = _state_at_solver(monkeypatch, lambda: _suggest(host, fn_cls))
    eng = RecordingEngine()
    x_d, r_d, fn, gp, sp = _suggest(eng, fn_cls, device=True)
    calls = [c for c in eng.calls if c[0] == "evolve_mixed"]
    assert len(calls) == 1
    _, groups, bounds, init, state = calls[0]
    assert groups == [(0, 0, 1), (1, 1, 1), (2, 2, 3)] and np.array_equal(bounds, sp.bounds)
    assert init.shape == (15 * sp.dim, sp.dim) and np.array_equal(init, seen[0][0])
    assert np.array_equal(state[1], seen[0][1][1]) and state[2] == seen[0][1][2]
    assert np.array_equal(x_d, x_h) and r_d.uniform() == r_h.uniform()


def test_the_gate_excludes_what_the_device_walk_does_not_cover(monkeypatch):
    eng = RecordingEngine()
    _, _, fn, gp, sp = _suggest(eng, device=True)
    rs = np.random.RandomState(0)
    fn._fused = [gp]
    assert fn._device_evolve_groups(sp, rs) is not None
    fn._fused = [gp, gp]                                                    # a constraint GP
    assert fn._device_evolve_groups(sp, rs) is None
    fn._fused = [gp]
    assert fn._device_evolve_groups(sp, np.random.RandomState(np.random.PCG64(1))) is None     # not MT19937
    monkeypatch.setattr(scipy, "__version__", "1.16.0")                     # another SciPy
    assert fn._device_evolve_groups(sp, rs) is None
    monkeypatch.setattr(scipy, "__version__", "1.14.1")
    assert fn._device_evolve_groups(sp, rs) is None
    monkeypatch.undo()
    fn.device_evolve = False
    assert fn._device_evolve_groups(sp, rs) is None
    fn._fused = None

    class MyUCB(A.UpperConfidenceBound):                                    # a custom acquisition
        def base_acq(self, mean, std):
            return mean + 0.5 * std

    for cls, kw in ((MyUCB, {}), (A.UpperConfidenceBound, {"n_obs": 513})):
        e = RecordingEngine()
        _suggest(e, cls, device=True, **kw)
        assert not [c for c in e.calls if c[0] == "evolve_mixed"]          # custom policy; NP > 512

    class Odd(type(sp._params_config["a"])):                               # a custom parameter class
        pass

    sp2 = MixedSpace(PB)
    sp2._params_config["a"] = Odd("a", (0.0, 2.0))
    e = RecordingEngine()
    _suggest(e, device=True, space=sp2)
    assert not [c for c in e.calls if c[0] == "evolve_mixed"]


def test_mixed_search_must_be_reference_or_device():
    from bayesianoptimization_amd import accelerate

    with pytest.raises(ValueError, match="mixed_search"):
        accelerate(object(), mixed_search="gpu")
