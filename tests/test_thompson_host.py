"""CPU: Thompson sampling's host side — `spectral_draw` (shapes, the documented draw order, the feature kernel against the kernel),
the truth of tests/paths_truth.py held to what a posterior draw must satisfy (over the PRODUCT's sampler: its frequencies, its draw
order), and `suggest_thompson` over an oracle-backed engine double: the engine calls, the picks against a twin that replays the
documented RandomState draws through the truth's OTHER route, every refusal, the untouched policy, the state left behind.
The device's arithmetic is checked in tests/test_gpu_sample_paths.py."""
import functools
import warnings

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_truth as P
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_thompson
from bayesianoptimization_amd.thompson import spectral_draw

KINDS = (F.RBF, F.MATERN25, F.MATERN15, F.MATERN05)
KNAME = {F.RBF: "rbf", F.MATERN25: "matern25", F.MATERN15: "matern15", F.MATERN05: "matern05"}


# ---- spectral_draw -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=[KNAME[k] for k in KINDS])
def test_spectral_draw_shapes_order_and_final_state(kind):
    Fn, d = 37, 5
    rs, twin = np.random.RandomState(12), np.random.RandomState(12)
    omega, phase = spectral_draw(kind, Fn, d, rs)
    assert omega.shape == (Fn, d) and phase.shape == (Fn,) and omega.dtype == np.float64 and omega.flags["C_CONTIGUOUS"]
    z = twin.standard_normal((Fn, d))
    if kind != F.RBF:
        nu2 = 2.0 * F.NU[kind]
        z = z / np.sqrt(twin.chisquare(nu2, Fn) / nu2)[:, None]
    ph = twin.uniform(size=Fn)
    assert np.array_equal(omega, z / (2.0 * np.pi)) and np.array_equal(phase, ph)
    assert (phase >= 0).all() and (phase < 1).all()
    a, b = rs.get_state(), twin.get_state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    with pytest.raises(ValueError):
        spectral_draw(7, Fn, d, rs)
    with pytest.raises(ValueError):
        spectral_draw(kind, 0, d, rs)


@pytest.mark.parametrize("kind", KINDS, ids=[KNAME[k] for k in KINDS])
def test_feature_kernel_estimates_the_kernel(kind):
    """2 / F sum_j phi_j(a) phi_j(b) against k(|a - b|) at 50 pairs of length-scaled points, F = 2^16: within 6 standard errors of
    the Monte-Carlo mean, the standard error from the sample itself."""
    Fn, d, pairs = 1 << 16, 3, 50
    rs = np.random.RandomState(100 + kind)
    omega, phase = spectral_draw(kind, Fn, d, rs)
    a = rs.uniform(0.0, 2.0, size=(pairs, d))
    b = a + rs.uniform(-1.0, 1.0, size=(pairs, d)) * rs.uniform(0.05, 1.5, size=(pairs, 1))
    terms = 2.0 * P.features(omega, phase, a) * P.features(omega, phase, b)           # (pairs, F)
    mean = terms.mean(axis=1)
    se = terms.std(axis=1, ddof=1) / np.sqrt(Fn)
    k = F.kernel_value(kind, np.sqrt(((a - b) ** 2).sum(1)))
    z = np.abs(mean - k) / se
    print(f"{KNAME[kind]}: worst |mean - k| / se = {z.max():.2f}")
    assert z.max() <= 6.0


# ---- the truth alone, over the product's sampler ---------------------------------------------------------------------------------
N_T, D_T, NOISE_T, F_T, CALLS, S_T = 40, 3, 1e-4, 1024, 128, 16
LS_T = 0.5 * np.geomspace(0.75, 1.33, D_T)


@functools.lru_cache(maxsize=None)
def _truth_run(kind):
    X, y = F.data(N_T, D_T, seed=1)
    yn = (y - y.mean()) / y.std()
    rs = np.random.RandomState(7 + kind)
    Xc = np.vstack([rs.uniform(size=(96, D_T)), X[:8]])
    gp = F.fit_fixed_theta(kind, X, yn, LS_T, NOISE_T, normalize_y=False)
    mu, sd = F.predict(gp, Xc)
    vals, ident = [], 0.0
    for _ in range(CALLS):
        omega, phase = spectral_draw(kind, F_T, D_T, rs)
        w = rs.standard_normal((S_T, F_T))
        eps = rs.standard_normal((S_T, N_T)) * np.sqrt(NOISE_T)
        f = P.paths_cho(kind, X, yn, LS_T, NOISE_T, omega, phase, w, eps, Xc)
        V = P.path_weights(kind, X, yn, LS_T, NOISE_T, omega, phase, w, eps)
        # (a) f(X_i) + eps_i + eta v_i = y_n,i at the training points among the candidates
        ident = max(ident, float(np.max(np.abs(f[:, 96:] + eps[:, :8] + NOISE_T * V[:8].T - yn[None, :8]))))
        vals.append(f)
    return X, yn, Xc, mu, sd, np.vstack(vals), ident


@pytest.mark.parametrize("kind", KINDS, ids=[KNAME[k] for k in KINDS])
def test_truth_draws_are_posterior_draws(kind):
    X, yn, Xc, mu, sd, vals, ident = _truth_run(kind)
    n = vals.shape[0]
    assert n == CALLS * S_T
    print(f"{KNAME[kind]}: (a) identity {ident:.2e}")
    assert ident <= 1e-10
    # (b) zero weights and zero noise draws: the posterior mean
    zero = P.paths_cho(kind, X, yn, LS_T, NOISE_T, *spectral_draw(kind, F_T, D_T, np.random.RandomState(0)), np.zeros((1, F_T)),
                       np.zeros((1, N_T)), Xc)[0]
    print(f"{KNAME[kind]}: (b) zero draw vs mu {np.max(np.abs(zero - mu)):.2e}")
    assert np.max(np.abs(zero - mu)) <= 1e-10
    assert np.max(np.abs(P.posterior_mean(kind, X, yn, LS_T, NOISE_T, Xc) - mu)) <= 1e-10
    # (c) the mean over the paths against mu, in standard errors of that mean, at every candidate
    se = vals.std(axis=0, ddof=1) / np.sqrt(n)
    zc = np.abs(vals.mean(axis=0) - mu) / se
    print(f"{KNAME[kind]}: (c) worst |mean - mu| / se = {zc.max():.2f}")
    assert zc.max() <= 5.0
    # (d) the sample variance against sigma^2 wherever sigma > 0.05
    wide = sd > 0.05
    assert wide.sum() >= 20
    ratio = vals.var(axis=0, ddof=1)[wide] / sd[wide] ** 2
    print(f"{KNAME[kind]}: (d) variance ratio {ratio.min():.3f} .. {ratio.max():.3f} over {wide.sum()} candidates")
    assert 0.8 <= ratio.min() and ratio.max() <= 1.25


def test_the_two_fp64_routes_and_the_50_digit_truth_agree():
    kind, N, d, M, Fn, S = F.MATERN15, 9, 2, 7, 11, 3
    X, y = F.data(N, d, seed=2)
    yn = (y - y.mean()) / y.std()
    rs = np.random.RandomState(3)
    omega, phase = spectral_draw(kind, Fn, d, rs)
    w, eps = rs.standard_normal((S, Fn)), rs.standard_normal((S, N)) * 0.03
    Xc = rs.uniform(size=(M, d))
    args = (kind, X, yn, np.array([0.4, 0.7]), 1e-3 / 2.5, omega, phase, w, eps, Xc, 3.5, 0.4)
    t = P.paths_mp(*args, amplitude=2.5)
    for route in (P.paths_cho, P.paths_winv):
        assert np.max(np.abs(route(*args, amplitude=2.5) - t)) <= 1e-11 * 0.4 * max(1.0, float(np.max(np.abs(t))))


# ---- suggest_thompson over the engine double ---------------------------------------------------------------------------------------
D, N, M = 3, 30, 1500
BOUNDS = B.SUGGEST_BOUNDS


_driver = functools.partial(B.suggest_driver, P.PathsFakeEngine, n_random=M)
_same_state = B.same_state


def _replay(twin, teng, q, n_features):
    """What suggest_thompson documents, done by hand on a twin: fit, one candidate draw, per call the draws in order — and the
    paths by the truth's W route.  Returns (indices, gaps)."""
    gp, space, rng = twin._gp, twin._space, twin._random_state
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.fit(space.params, space.target)
    teng.generate_candidates_like(M, BOUNDS[:, 0], BOUNDS[:, 1], rng)
    X, y = space.params, space.target
    yn = (y - gp._y_train_mean) / gp._y_train_std
    idx, gaps = [], []
    for first in range(0, q, 16):
        S = min(16, q - first)
        omega, phase = spectral_draw(gp._kind, n_features, D, rng)
        w = rng.standard_normal((S, n_features))
        eps = rng.standard_normal((S, N)) * np.sqrt(float(gp.alpha))
        vals = P.paths_winv(gp._kind, X, yn, gp._ls, float(gp.alpha), omega, phase, w, eps, teng.Xc, gp._y_train_mean, gp._y_train_std)
        i, g = P.argmax_with_gap(vals)
        idx.extend(i.tolist())
        gaps.extend(g.tolist())
    return np.array(idx), np.array(gaps)


@pytest.mark.parametrize("q", [1, 16, 17])
def test_picks_calls_and_randomstate(q):
    n_features = 64
    drv, eng, X, y = _driver()
    twin, teng, _, _ = _driver()
    fn = drv._acquisition_function
    before = (fn.i, fn.kappa)
    picks = suggest_thompson(drv, q, n_random=M, n_features=n_features)
    assert len(picks) == q and all(list(p) == drv._space.keys for p in picks)
    # the engine calls: one fit, one candidate draw, ceil(q / 16) sample_paths, no posterior pass, no acquisition
    names = [c[0] for c in eng.calls]
    assert names.count("fit") == 1 and names.count("generate_candidates_like") == 1 and names.count("set_candidates") == 0
    assert [c[2] for c in eng.calls if c[0] == "sample_paths"] == [16] * (q // 16) + ([q % 16] if q % 16 else [])
    assert not {"posterior", "posterior_refresh", "acq_argbest", "fit_append", "polish_seeds", "predict_grad"} & set(names)
    assert names.index("fit") < names.index("generate_candidates_like") < names.index("sample_paths")
    # the policy is neither consulted nor advanced
    assert (fn.i, fn.kappa) == before
    # the picks: the truth's arg-max under the documented draws
    want, gaps = _replay(twin, teng, q, n_features)
    assert np.array_equal(eng.Xc, teng.Xc)
    assert gaps.min() >= 1e-6, f"the truth's own best / second gap {gaps.min():.2e}: pick another seed"
    assert np.array_equal(B.rows_to_indices(picks, eng.Xc), want)
    assert _same_state(drv._random_state, twin._random_state)
    # the next suggest() sees nothing of the call but the RandomState words it consumed
    assert np.array_equal(drv.suggest_first(), twin.suggest_first())


def test_predict_answers_for_the_real_data_afterwards():
    drv, eng, X, y = _driver(n_restarts_optimizer=0)
    drv.suggest_first()
    Xq = BOUNDS[:, 0] + np.random.RandomState(9).uniform(size=(40, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    mu0, sd0 = drv._gp.predict(Xq, return_std=True)
    suggest_thompson(drv, 5, n_random=M, n_features=32)
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    assert eng.inputs[0][0].shape[0] == N and drv._gp.X_train_.shape[0] == N


def test_refusals():
    drv, eng, X, y = _driver()
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            suggest_thompson(drv, bad)
    for kw in ({"n_features": 0}, {"n_features": 4097}, {"n_random": 0}):
        with pytest.raises(ValueError):
            suggest_thompson(drv, 2, **kw)
    group = B.check_shared_refusals(lambda d: suggest_thompson(d, 2), _driver, "suggest_thompson")
    with pytest.raises(NotImplementedError, match="device group"):
        type(group).sample_paths(group, None, None, None, None)
    # any policy is fine: it is not consulted
    drv, eng, X, y = _driver(A.GPHedge([A.UpperConfidenceBound(kappa=2.0), A.ExpectedImprovement(xi=0.01)]))
    assert len(suggest_thompson(drv, 2, n_random=M, n_features=16)) == 2


def test_exported():
    import bayesianoptimization_amd as pkg
    from bayesianoptimization_amd import thompson

    assert "suggest_thompson" in pkg.__all__ and pkg.suggest_thompson is thompson.suggest_thompson
