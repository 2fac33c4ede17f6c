"""CPU: the host side of suggest_thompson(refine=K) — the truth of tests/paths_ascent_truth.py held to central differences at 50
digits, and `suggest_thompson` over an oracle-backed engine double whose `ascend_paths` is SciPy L-BFGS-B over that truth: the
engine calls, the untouched RandomState, the picks against their draws' candidate maxima, every refusal.
The device's arithmetic is checked in tests/test_gpu_path_ascent.py."""
import functools
import warnings

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_ascent_truth as T
import paths_truth as P
from bayesianoptimization_amd import suggest_thompson
from bayesianoptimization_amd.engine import GroupEngine, path_winners
from bayesianoptimization_amd.thompson import spectral_draw

KINDS = (F.RBF, F.MATERN25, F.MATERN15, F.MATERN05)
KNAME = {F.RBF: "rbf", F.MATERN25: "matern25", F.MATERN15: "matern15", F.MATERN05: "matern05"}


# ---- the truth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=[KNAME[k] for k in KINDS])
def test_mp_gradient_equals_central_differences_at_50_digits(kind):
    """d f_s / d x against (f_s(x + h e_t) - f_s(x - h e_t)) / 2 h of the unrounded 50-digit value, h = 1e-14: the difference's own
    error is h^2 f''' / 6 ~ 1e-28 of the gradient's scale.  nu = 0.5 includes a point exactly ON a training point: the kernel's kink
    there is symmetric, so the central difference takes no slope from that point — the convention of the analytic gradient."""
    N, d, Fn, S = 7, 2, 9, 2
    X, y = F.data(N, d, seed=4)
    yn = (y - y.mean()) / y.std()
    rs = np.random.RandomState(20 + kind)
    omega, phase = spectral_draw(kind, Fn, d, rs)
    w, eps = rs.standard_normal((S, Fn)), rs.standard_normal((S, N)) * 0.03
    ls = np.array([0.4, 0.7])
    args = (kind, X, yn, ls, 1e-3 / 2.5, omega, phase, w, eps)
    model = T.MpPaths(*args, 3.5, 0.4, amplitude=2.5)
    points = [rs.uniform(size=d), rs.uniform(size=d)] + ([X[3].copy()] if kind == F.MATERN05 else [])
    ctx = T._ctx
    h = ctx.mpf(10) ** -14
    worst = ctx.mpf(0)
    for s in range(S):
        for x in points:
            x = [ctx.mpf(float(v)) for v in x]
            g = model.grad(s, x)
            scale = max(abs(v) for v in g)
            for t in range(d):
                up = [v + (h if k == t else 0) for k, v in enumerate(x)]
                dn = [v - (h if k == t else 0) for k, v in enumerate(x)]
                cd = (model.value(s, up) - model.value(s, dn)) / (2 * h)
                worst = max(worst, abs(cd - g[t]) / scale)
    print(f"{KNAME[kind]}: analytic vs central differences, worst relative {float(worst):.2e}")
    assert worst <= ctx.mpf(10) ** -20
    # the rounded value is paths_truth.paths_mp's, and the fp64 restatements agree with the 50-digit one
    Xq = np.array([points[:2]] * S)
    f_mp, g_mp = T.path_value_grad_mp(*args, Xq, 3.5, 0.4, amplitude=2.5)
    assert np.array_equal(f_mp, P.paths_mp(*args, np.array(points[:2]), 3.5, 0.4, amplitude=2.5))
    for route in ("cho", "winv"):
        f64, g64 = T.path_value_grad(*args, Xq, 3.5, 0.4, amplitude=2.5, route=route)
        assert np.max(np.abs(f64 - f_mp)) <= 1e-11 * 0.4 * max(1.0, float(np.max(np.abs(f_mp))))
        assert np.max(np.abs(g64 - g_mp)) <= 1e-10 * max(1.0, float(np.max(np.abs(g_mp))))


def test_on_a_training_point_nu05_takes_no_slope_from_it():
    N, d, Fn = 5, 2, 4
    X, y = F.data(N, d, seed=6)
    yn = (y - y.mean()) / y.std()
    rs = np.random.RandomState(2)
    omega, phase = spectral_draw(F.MATERN05, Fn, d, rs)
    w, eps = rs.standard_normal((1, Fn)), np.zeros((1, N))
    args = (F.MATERN05, X, yn, np.array([0.5]), 1e-4, omega, phase, w, eps)
    _, g = T.path_value_grad(*args, X[2][None, None, :])
    _, g_mp = T.path_value_grad_mp(*args, X[2][None, None, :])
    assert np.isfinite(g).all() and np.max(np.abs(g - g_mp)) <= 1e-10 * max(1.0, float(np.max(np.abs(g_mp))))


def test_projected_gradient_norm_and_winners():
    lo, hi = np.zeros(3), np.ones(3)
    x = np.array([0.0, 0.5, 1.0])
    assert T.projected_gradient_norm(x, np.array([-2.0, 0.0, 3.0]), lo, hi) == 0.0      # pushed outwards on both faces
    assert T.projected_gradient_norm(x, np.array([0.25, -0.125, -2.0]), lo, hi) == 1.0
    f = np.array([[1.0, 3.0, 3.0], [np.nan, -np.inf, np.nan], [np.nan, -2.0, np.inf]])
    xs = np.arange(18.0).reshape(3, 3, 2)
    got = path_winners(xs, f)
    assert got["winner"].tolist() == [1, -1, 1]
    assert np.array_equal(got["x_best"][0], xs[0, 1]) and np.isnan(got["x_best"][1]).all() and got["f_best"][2] == -2.0


# ---- suggest_thompson over the engine double ---------------------------------------------------------------------------------------
D, N, M = 3, 30, 600
BOUNDS = B.SUGGEST_BOUNDS


_driver = functools.partial(B.suggest_driver, T.AscentFakeEngine, n_random=M)
_same_state = B.same_state


def test_refine_zero_is_the_old_call():
    drv, eng, _, _ = _driver()
    twin, teng, _, _ = _driver()
    a = suggest_thompson(drv, 5, n_random=M, n_features=32)
    b = suggest_thompson(twin, 5, n_random=M, n_features=32, refine=0, max_iter=7)
    assert a == b
    assert [c[0] for c in eng.calls] == [c[0] for c in teng.calls] and "ascend_paths" not in [c[0] for c in eng.calls]
    assert _same_state(drv._random_state, twin._random_state)


@pytest.mark.parametrize("q", [1, 16, 17])
def test_refined_picks_calls_and_randomstate(q):
    n_features, K = 32, 2
    drv, eng, X, y = _driver()
    twin, teng, _, _ = _driver()
    fn = drv._acquisition_function
    before = (fn.i, fn.kappa)
    Xq = BOUNDS[:, 0] + np.random.RandomState(9).uniform(size=(20, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    picks = suggest_thompson(drv, q, n_random=M, n_features=n_features, refine=K)
    plain = suggest_thompson(twin, q, n_random=M, n_features=n_features)
    assert len(picks) == q and all(list(p) == drv._space.keys for p in picks)
    # the engine calls: ceil(q / 16) ascend_paths in place of the sample_paths, nothing else new, no rows fetched
    names = [c[0] for c in eng.calls]
    assert names.count("fit") == 1 and names.count("generate_candidates_like") == 1
    assert [c[2] for c in eng.calls if c[0] == "ascend_paths"] == [16] * (q // 16) + ([q % 16] if q % 16 else [])
    assert not {"sample_paths", "posterior", "posterior_refresh", "acq_argbest", "fit_append", "polish_seeds", "predict_grad",
                "get_candidate_rows"} & set(names)
    assert (fn.i, fn.kappa) == before                                        # the policy is not advanced
    assert _same_state(drv._random_state, twin._random_state)                # the refinement draws nothing
    assert np.array_equal(eng.Xc, teng.Xc)
    # inside the bounds, and under its own draw every pick is at least the draw's candidate maximum (the refine=0 twin's pick)
    rows = np.array([list(p.values()) for p in picks])
    assert (rows >= BOUNDS[:, 0]).all() and (rows <= BOUNDS[:, 1]).all()
    gp = drv._gp
    yn = (y - gp._y_train_mean) / gp._y_train_std
    rng = np.random.RandomState(3)
    replay, reng, _, _ = _driver()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        replay._gp.fit(replay._space.params, replay._space.target)
    rng = replay._random_state
    reng.generate_candidates_like(M, BOUNDS[:, 0], BOUNDS[:, 1], rng)
    moved = 0
    for first in range(0, q, 16):
        S = min(16, q - first)
        omega, phase = spectral_draw(gp._kind, n_features, D, rng)
        w = rng.standard_normal((S, n_features))
        eps = rng.standard_normal((S, N)) * np.sqrt(float(gp.alpha))
        args = (gp._kind, X, yn, gp._ls, float(gp.alpha), omega, phase, w, eps)
        cand_max = P.paths_winv(*args, eng.Xc, gp._y_train_mean, gp._y_train_std).max(axis=1)
        f_pick, _ = T.path_value_grad(*args, rows[first:first + S][:, None, :], gp._y_train_mean, gp._y_train_std)
        slack = 1e-9 * gp._y_train_std * max(1.0, float(np.max(np.abs(cand_max))))
        assert (f_pick[:, 0] >= cand_max - slack).all(), (f_pick[:, 0] - cand_max).min()
        moved += int((f_pick[:, 0] > cand_max + slack).sum())
    assert _same_state(rng, drv._random_state)
    assert moved >= 1, "no pick improved on its candidate: the refinement did nothing"
    assert not np.array_equal(rows, np.array([list(p.values()) for p in plain]))
    # gp.predict answers for the real data as before
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    mu0, sd0 = twin._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    assert eng.inputs[0][0].shape[0] == N and drv._gp.X_train_.shape[0] == N


def test_refusals():
    drv, eng, X, y = _driver()
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError, match="refine"):
            suggest_thompson(drv, 2, n_random=M, n_features=16, refine=bad)
    assert not eng.calls
    # every existing refusal still fires with refine=2, before any engine call
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            suggest_thompson(drv, bad, refine=2)
    for kw in ({"n_features": 0}, {"n_features": 4097}, {"n_random": 0}):
        with pytest.raises(ValueError):
            suggest_thompson(drv, 2, refine=2, **kw)
    assert not eng.calls
    group = B.check_shared_refusals(lambda d: suggest_thompson(d, 2, refine=2), _driver, "suggest_thompson")
    assert isinstance(group, GroupEngine)
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.ascend_paths(group, None, None, None, None, None, None)
    # an engine without the ascent: refused, never a silent refine=0
    drv, eng, X, y = _driver()
    drv._gp.engine = P.PathsFakeEngine()
    with pytest.raises(NotImplementedError, match="ascend_paths"):
        suggest_thompson(drv, 2, refine=2)
