"""GPU: gpbo_evolve_mixed — the mixed-space differential evolution with its walk and its evaluations on the device.

1. the walk (gpbo_debug_evolve_walk, over an analytic objective the host evaluates to the same bits) is SciPy's
   DifferentialEvolutionSolver's bit for bit: x, fun, nit, nfev, success and the RandomState afterwards, also across launches;
2. the objective (gpbo_debug_evolve_eval) is the host's reference-shaped objective (_get_acq over _posterior_trusted) to rounding;
3. SciPy's solver driven by that device objective and the device walk leave the same x, nit, nfev and RandomState;
4. suggest() over a MixedSpace with device_evolve gives the host DE's suggestion and RandomState position."""
import numpy as np
import pytest
from scipy.optimize._differentialevolution import DifferentialEvolutionSolver
from scipy.stats import norm
from sklearn.gaussian_process.kernels import RBF, Matern

import de_walk
from bayesianoptimization_amd import engine as E
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.float_space import MixedSpace
from bayesianoptimization_amd.gpr import HipGPR

pytestmark = pytest.mark.gpu

MIXED_PB = {"a": (0.0, 2.0), "n": (-3, 7, int), "b": (1.0, 4.0), "c": ("x", "y", "z"), "e": (5.0, 6.0), "k": (0, 1, int)}


def _analytic_case(D, S, seed, zero_width=False, bad=False):
    rs = np.random.RandomState(seed)
    b = np.column_stack([-3.0 * rs.rand(D), 2.0 * rs.rand(D) + 0.1])
    if zero_width:
        b[0, 1] = b[0, 0]
    init = b[:, 0] + (b[:, 1] - b[:, 0]) * rs.rand(S, D)
    w, a, r = rs.rand(D) + 0.1, rs.rand(D) - 0.5, rs.rand(D) < 0.5
    lo_cut = b[0, 0] + 0.15 * (b[0, 1] - b[0, 0]) if bad else -np.inf
    hi_cut = b[0, 1] - 0.2 * (b[0, 1] - b[0, 0]) if bad else np.inf
    f0 = de_walk.analytic(w, a, r)

    def f(x):
        if x[0] < lo_cut:
            return np.nan
        if x[0] > hi_cut:
            return np.inf
        return f0(x)

    groups = [(1 if r[t] else 0, t, 1) for t in range(D)]
    return b, init, w, a, groups, f, rs, lo_cut, hi_cut


@pytest.mark.parametrize("D,S,maxiter,budget,kw", [
    (1, 15, 1000, 256, {}), (2, 30, 1000, 256, {}), (5, 75, 1000, 256, {}), (16, 240, 25, 256, {}), (64, 960, 2, 256, {}),
    (5, 5, 1000, 256, {}), (3, 45, 1000, 256, {"zero_width": True}), (4, 60, 40, 256, {"bad": True}), (5, 75, 3, 256, {}),
    (5, 75, 1000, 37, {}),
])
def test_device_walk_is_scipys_bit_for_bit(debug_engine, D, S, maxiter, budget, kw):
    b, init, w, a, groups, f, rs, lo_cut, hi_cut = _analytic_case(D, S, 7 * D + S, **kw)
    state = rs.get_state(legacy=True)
    got = debug_engine.debug_evolve_walk(w, a, groups, b, init, state[1], state[2], maxiter=maxiter, budget=budget,
                                         nan_below=lo_cut, inf_above=hi_cut)
    res = DifferentialEvolutionSolver(f, b, polish=False, init=init, rng=rs, maxiter=maxiter).solve()
    after = rs.get_state(legacy=True)
    assert np.array_equal(got["x"], res.x) and np.array_equal(got["fun"], res.fun, equal_nan=True)
    assert (got["nit"], got["nfev"], got["success"]) == (res.nit, res.nfev, res.success)
    assert np.array_equal(got["key"], after[1]) and got["pos"] == after[2]
    if budget < 100:
        assert got["launches"] >= 4          # the run crossed several launch budgets


def _mixed_model(engine, N, seed, kernel="matern"):
    sp = MixedSpace(MIXED_PB)
    rng = np.random.RandomState(seed)
    X = sp.random_sample(N, rng)
    y = np.sin(X[:, 0] + 0.3 * X[:, 1]) + 0.1 * X[:, 2] + X[:, 3] - 0.5 * X[:, 5] + 0.2 * X[:, 7]
    sp.register_bulk(X, y)
    k = Matern(nu=2.5, length_scale=1.3) if kernel == "matern" else RBF(length_scale=1.1)
    gp = HipGPR(kernel=k, alpha=1e-6, normalize_y=True, optimizer=None, engine=engine, transform=sp.kernel_transform).fit(X, y)
    groups = A._mixed_space_groups([gp], sp, np.random.RandomState(0))
    assert groups is not None
    return sp, gp, groups, float(np.max(y))


def _policy(acq):
    return {E.UCB: lambda: A.UpperConfidenceBound(kappa=2.576), E.EI: lambda: A.ExpectedImprovement(xi=0.01),
            E.POI: lambda: A.ProbabilityOfImprovement(xi=0.01)}[acq]()


@pytest.mark.parametrize("N", [40, 120, 130, 300, 512])
@pytest.mark.parametrize("acq", [E.UCB, E.EI, E.POI])
def test_device_objective_is_the_host_objective_to_rounding(debug_engine, N, acq):
    sp, gp, groups, y_max = _mixed_model(debug_engine, N, N + acq, kernel="matern" if N != 130 else "rbf")
    fn = _policy(acq)
    fn.y_max = y_max
    pts = sp.random_sample(40, np.random.RandomState(3))
    pts[:20] += np.random.RandomState(4).uniform(-0.45, 0.45, size=(20, sp.dim))      # off-grid int / one-hot columns
    pts = np.clip(pts, sp.bounds[:, 0], sp.bounds[:, 1])
    got = debug_engine.debug_evolve_eval(fn._acq_kind, fn._acq_param(), y_max, float(gp._y_train_mean), float(gp._y_train_std),
                                         groups, pts)
    obj = fn._get_acq(gp)
    want = np.array([obj(p)[0] for p in pts])
    mu = np.empty(len(pts)); sd = np.empty(len(pts))
    for i, p in enumerate(pts):
        m, s = gp._posterior_trusted(p[None])
        mu[i], sd[i] = m[0], s[0]
    if acq == E.UCB:
        z, scale = np.zeros(len(pts)), np.abs(mu) + 2.576 * sd
    else:
        a = mu - y_max - 0.01
        z = a / sd
        scale = np.abs(a) * norm.cdf(z) + sd * norm.pdf(z) if acq == E.EI else norm.cdf(z)
    assert np.all(np.abs(got - want) <= 1e-11 * (1.0 + z * z) * scale + 1e-300)
    if acq == E.UCB or N not in (40, 300):
        return
    # the same bar over the whole z range: y_max from far below every mean (upper tail) to far above (the late-run regime, where
    # every value is in the lower tail).  gpbo_debug_evolve_eval returns only the objective, so the posterior's own rounding stays
    # in the bar here (tests/test_gpu_acq_regimes.py has the formula alone, on the device's own mu / sd).  Measured on an MI355X: at
    # most 0.012 of the bar (N = 300, |z| < 2), below 0.003 of it in the tails.
    s50, lo, hi = float(np.median(sd)), float(mu.min()), float(mu.max())
    z_seen = []
    for y_sweep in (lo - 12 * s50, lo - 3 * s50, float(np.median(mu)), hi + 3 * s50, hi + 8 * s50, hi + 16 * s50):
        fn.y_max = y_sweep
        got = debug_engine.debug_evolve_eval(fn._acq_kind, fn._acq_param(), y_sweep, float(gp._y_train_mean), float(gp._y_train_std),
                                             groups, pts)
        obj = fn._get_acq(gp)
        want = np.array([obj(p)[0] for p in pts])
        a = mu - y_sweep - 0.01
        z = a / sd
        scale = np.abs(a) * norm.cdf(z) + sd * norm.pdf(z) if acq == E.EI else norm.cdf(z)
        ratio = np.abs(got - want) / (1e-11 * (1.0 + z * z) * scale + 1e-300)
        print(f"evolve eval acq={acq} N={N} y_max={y_sweep:+.3f}: worst |error| / bar {ratio.max():.4f}, z [{z.min():.1f}, {z.max():.1f}]")
        assert np.all(np.abs(got - want) <= 1e-11 * (1.0 + z * z) * scale + 1e-300)
        z_seen.append(z)
    z_seen = np.concatenate(z_seen)
    assert z_seen.min() < -8 and z_seen.max() > 8 and np.sum(np.abs(z_seen) < 1) >= 5


@pytest.mark.parametrize("acq,N", [(E.UCB, 40), (E.EI, 100), (E.POI, 200)])
def test_scipy_over_the_device_objective_walks_as_the_device(debug_engine, acq, N):
    sp, gp, groups, y_max = _mixed_model(debug_engine, N, 11 + N)
    fn = _policy(acq)
    fn.y_max = y_max
    args = (fn._acq_kind, fn._acq_param(), y_max, float(gp._y_train_mean), float(gp._y_train_std), groups)
    init = sp.random_sample(15 * sp.dim, np.random.RandomState(5))
    r_host, r_dev = np.random.RandomState(8), np.random.RandomState(8)
    res = DifferentialEvolutionSolver(lambda x: debug_engine.debug_evolve_eval(*args, x[None])[0], sp.bounds, polish=False,
                                      init=init, rng=r_host).solve()
    gp._ensure_resident()
    x, fun, nit, nfev, ok = debug_engine.evolve_mixed(*args[:5], groups, sp.bounds, init, r_dev)
    assert np.array_equal(x, res.x) and fun == res.fun and (nit, nfev, ok) == (res.nit, res.nfev, res.success)
    s1, s2 = r_host.get_state(legacy=True), r_dev.get_state(legacy=True)
    assert np.array_equal(s1[1], s2[1]) and s1[2] == s2[2]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("policy", ["ucb", "ei", "poi", "hedge"])
def test_suggest_with_device_evolve_is_the_host_de_suggestion(engine, seed, policy):
    out = {}
    for device in (False, True):
        sp = MixedSpace(MIXED_PB)
        rng = np.random.RandomState(seed)
        X = sp.random_sample(25 + 20 * seed, rng)
        sp.register_bulk(X, np.sin(X[:, 0] + 0.3 * X[:, 1]) + 0.1 * X[:, 2] + X[:, 3] - 0.5 * X[:, 5])
        gp = HipGPR(kernel=Matern(nu=2.5, length_scale=1.3), alpha=1e-6, normalize_y=True, optimizer=None, engine=engine,
                    transform=sp.kernel_transform)
        if policy == "hedge":
            bases = [A.UpperConfidenceBound(kappa=2.576), A.ExpectedImprovement(xi=0.01), A.ProbabilityOfImprovement(xi=0.01)]
            fn = A.GPHedge(base_acquisitions=bases)
            for b in bases:
                b.device_evolve = device
        else:
            fn = {"ucb": lambda: A.UpperConfidenceBound(kappa=2.576), "ei": lambda: A.ExpectedImprovement(xi=0.01),
                  "poi": lambda: A.ProbabilityOfImprovement(xi=0.01)}[policy]()
            fn.device_evolve = device
        calls = []
        orig = engine.evolve_mixed
        engine.evolve_mixed = lambda *a, _o=orig, **k: (calls.append(1), _o(*a, **k))[1]
        try:
            rs = np.random.RandomState(100 + seed)
            xs = [fn.suggest(gp, sp, n_random=2000, n_smart=5, random_state=rs) for _ in range(2)]
        finally:
            del engine.evolve_mixed
        st = rs.get_state(legacy=True)
        out[device] = (xs, st, len(calls))
    assert out[False][2] == 0 and out[True][2] >= 2
    assert all(np.array_equal(a, b) for a, b in zip(out[False][0], out[True][0]))
    assert np.array_equal(out[False][1][1], out[True][1][1]) and out[False][1][2] == out[True][1][2]
