"""GPU: gpbo_lml_batch_scaled — the theta-search lanes of scaled models  c * k + w  (per-lane noise and per-lane target scale) — and
the lockstep search built on it (HipGPR(scaled_kernels=True, scaled_lanes=True)).

The contract: lane i is bit for bit gpbo_lml_scaled of the same arguments.  Sizes, the smallest that reach each path:
  N = 40 (NP = 64) the one-launch path, N = 200 the strip path, N = 830 (NP = 832) the blocked path with one lane group (captured into a
  hipGraph on its second sighting, replayed from the third), N = 2000 (NP = 2048) two lane groups on two streams.
Every lane has its own c (0.3 ... 40), w (exactly 0 among them) and length scale(s); alpha = 1e-6; data as tests/scaled_kernel_truth.py.
Bars against scikit-learn: those of tests/test_gpu_scaled_kernel.py for gpbo_lml_scaled (value 1e-10, gradient 1e-7 of its largest
component; posteriors 1e-9)."""
import warnings

import numpy as np
import pytest
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

import scaled_kernel_truth as S
from bayesianoptimization_amd import engine as E
from bayesianoptimization_amd.gpr import HipGPR
from conftest import rel_err

pytestmark = pytest.mark.gpu

A = S.ALPHA
SIZES = [(40, 3), (200, 5), (830, 5), (2000, 4)]
WHITES = np.array([2e-3, 0.0, 5e-2, 1e-4, 0.3, 0.0, 7e-3, 1.5e-2])

_data = {}


def _inputs(N, d):
    """(X, normalised y) of a size, computed once and shared, left unchanged."""
    if (N, d) not in _data:
        X, y = S.data(N, d, 1)
        yn = (y - y.mean()) / y.std()
        X.setflags(write=False)
        yn.setflags(write=False)
        _data[(N, d)] = (X, yn)
    return _data[(N, d)]


def _lanes(n, d, per_dim, shift=0):
    """n different lanes: (length scales (n, n_ls), amplitudes (n,), whites (n,)); `shift` gives other values at the same shape."""
    c = np.geomspace(0.3, 40.0, 8)[(np.arange(n) + shift) % 8]
    w = WHITES[(np.arange(n) + 3 * shift) % 8]
    base = np.atleast_1d(S.length_scale(d, per_dim))
    ls = base[None, :] * (0.6 + 0.15 * ((np.arange(n) + 2 * shift) % 8))[:, None]
    return np.ascontiguousarray(ls), c, w


def _singles(engine, X, yn, kind, ls, c, w, alpha=A):
    """gpbo_lml_scaled lane by lane: values (n,), gradients (n, n_ls + 2)."""
    out = [engine.lml(X, yn, kind, ls[i], alpha, amplitude=c[i], white=w[i], scaled=True) for i in range(len(c))]
    return np.array([v for v, _ in out]), np.array([g for _, g in out])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- every lane is the single evaluation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "per_dim"])
@pytest.mark.parametrize("kind", [E.RBF, E.MATERN25], ids=["rbf", "matern25"])
@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("N,d", SIZES)
def test_every_lane_is_bitwise_gpbo_lml_scaled(engine, N, d, n, kind, per_dim):
    X, yn = _inputs(N, d)
    ls, c, w = _lanes(n, d, per_dim)
    v1, g1 = _singles(engine, X, yn, kind, ls, c, w)
    v, g = engine.lml_batch_scaled_arrays(X, yn, kind, ls, c, w, A)
    assert g.shape == (n, ls.shape[1] + 2) and np.all(np.isfinite(v))
    assert _same_bits(v, v1) and _same_bits(g, g1)
    v0, _ = engine.lml_batch_scaled_arrays(X, yn, kind, ls, c, w, A, eval_gradient=False, reuse_inputs=True)
    assert _same_bits(v0, v1)                                                  # the value-only form


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("N,d", SIZES[:2])
def test_matern05_lanes_are_bitwise_gpbo_lml_scaled(engine, N, d, n):
    X, yn = _inputs(N, d)
    ls, c, w = _lanes(n, d, n == 3)
    v1, g1 = _singles(engine, X, yn, E.MATERN05, ls, c, w)
    v, g = engine.lml_batch_scaled_arrays(X, yn, E.MATERN05, ls, c, w, A)
    assert _same_bits(v, v1) and _same_bits(g, g1)
    v0, _ = engine.lml_batch_scaled_arrays(X, yn, E.MATERN05, ls, c, w, A, eval_gradient=False, reuse_inputs=True)
    assert _same_bits(v0, v1)


# ---- replay: the third and fourth call of a shape run from the captured graph ------------------------------------------------------
@pytest.mark.parametrize("N,d", SIZES[2:])
def test_four_calls_of_one_shape_each_evaluate_their_own_c_w_and_length_scales(engine, N, d):
    """Resident inputs (X = NULL after the first call), other c, w, l every time: a noise or a target scale captured as a launch
    argument would repeat the first call's in calls three and four — the replayed ones as long as the runtime captures the
    sequence; where capture fails the library launches directly and this test cannot tell the difference."""
    X, yn = _inputs(N, d)
    calls = [_lanes(6, d, True, shift=j) for j in range(4)]
    got = []
    for j, (ls, c, w) in enumerate(calls):
        v, g = engine.lml_batch_scaled_arrays(X, yn, E.MATERN25, ls, c, w, A, reuse_inputs=j > 0)
        got.append((v.copy(), g.copy()))
    for (ls, c, w), (v, g) in zip(calls, got):
        v1, g1 = _singles(engine, X, yn, E.MATERN25, ls, c, w)
        assert _same_bits(v, v1) and _same_bits(g, g1)
    assert not _same_bits(got[0][0], got[2][0]) and not _same_bits(got[1][0], got[3][0])


# ---- the two forms share one pool and one slab -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", SIZES[1:3])
def test_nothing_leaks_between_scaled_and_unit_batches_or_into_a_fitted_slot(engine, N, d):
    X, yn = _inputs(N, d)
    Xc = np.random.RandomState(8).uniform(size=(300, d))
    engine.fit(X, yn, E.MATERN25, 0.7, A, slot=3)
    before = engine.predict(Xc, slot=3)
    ls, c, w = _lanes(4, d, True)
    ls2, c2, w2 = _lanes(4, d, True, shift=3)
    s_a = engine.lml_batch_scaled_arrays(X, yn, E.MATERN25, ls, c, w, A)
    s_a = (s_a[0].copy(), s_a[1].copy())
    u = engine.lml_batch_arrays(X, yn, E.MATERN25, ls, A, reuse_inputs=True)
    u = (u[0].copy(), u[1].copy())
    s_b = engine.lml_batch_scaled_arrays(X, yn, E.MATERN25, ls2, c2, w2, A, reuse_inputs=True)
    after = engine.predict(Xc, slot=3)
    assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1])
    for i in range(4):
        v1, g1 = engine.lml(X, yn, E.MATERN25, ls[i], A)
        assert _same_bits(u[0][i], v1) and _same_bits(u[1][i], g1)
    for (v, g), (l_, c_, w_) in ((s_a, (ls, c, w)), (s_b, (ls2, c2, w2))):
        v1, g1 = _singles(engine, X, yn, E.MATERN25, l_, c_, w_)
        assert _same_bits(v, v1) and _same_bits(g, g1)


@pytest.mark.parametrize("N,d", SIZES)
def test_unit_amplitude_and_no_white_lanes_are_gpbo_lml_batch(engine, N, d):
    X, yn = _inputs(N, d)
    ls, _, _ = _lanes(3, d, True)
    v, g = engine.lml_batch_scaled_arrays(X, yn, E.MATERN25, ls, np.ones(3), np.zeros(3), A)
    v, g = v.copy(), g.copy()
    vu, gu = engine.lml_batch_arrays(X, yn, E.MATERN25, ls, A, reuse_inputs=True)
    assert _same_bits(v, vu) and _same_bits(g[:, 1:-1], gu) and np.all(g[:, -1] == 0.0)


# ---- a lane that is not positive definite -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", SIZES[:2])
def test_a_lane_that_is_not_positive_definite_is_a_status_of_that_lane_alone(engine, N, d):
    """Rows 0 and 1 of X identical, alpha = 0: the lane with w = 0 has the exact pivot 1 - 1 * 1 = 0 in its second column — -inf, a
    zero gradient and its info word; its neighbours (w > 0) are their single evaluations."""
    import ctypes as C

    from bayesianoptimization_amd._lib import dptr

    X, yn = _inputs(N, d)
    X = X.copy()
    X[1] = X[0]
    ls, c, _ = _lanes(3, d, False)
    w = np.array([1e-2, 0.0, 3e-2])
    n_ls = ls.shape[1]
    vals, grads, infos = np.zeros(3), np.ones((3, n_ls + 2)), (C.c_int * 3)()
    rc = engine._lib.gpbo_lml_batch_scaled(engine._h, 3, dptr(X), dptr(yn), N, d, E.RBF, dptr(ls), n_ls, dptr(c), dptr(w), 0.0, 1,
                                           dptr(vals), dptr(grads), infos)
    assert rc == 0
    assert vals[1] == -np.inf and np.all(grads[1] == 0.0) and infos[1] != 0 and infos[0] == 0 and infos[2] == 0
    v, g = engine.lml_batch_scaled_arrays(X, yn, E.RBF, ls, c, w, 0.0)             # the Python form: no exception, the same lanes
    assert _same_bits(v, vals) and _same_bits(g, grads)
    for i in (0, 2):
        v1, g1 = engine.lml(X, yn, E.RBF, ls[i], 0.0, amplitude=c[i], white=w[i], scaled=True)
        assert np.isfinite(v1) and _same_bits(vals[i], v1) and _same_bits(grads[i], g1)
    assert engine.lml(X, yn, E.RBF, ls[1], 0.0, amplitude=c[1], white=0.0, scaled=True)[0] == -np.inf


def test_arguments_are_checked_per_lane(engine):
    X, yn = _inputs(40, 3)
    ls, c, w = _lanes(3, 3, False)
    for bad_c, bad_w in ((0.0, 0.0), (-1.0, 0.0), (2.0, -1e-3), (np.inf, 0.0), (2.0, np.nan)):
        c2, w2 = c.copy(), w.copy()
        c2[2], w2[2] = bad_c, bad_w
        with pytest.raises(ValueError, match="amplitude"):
            engine.lml_batch_scaled_arrays(X, yn, E.RBF, ls, c2, w2, A)
    with pytest.raises(ValueError, match="alpha"):
        engine.lml_batch_scaled_arrays(X, yn, E.RBF, ls, c, w, -1.0)
    with pytest.raises(ValueError):
        engine.lml_batch_scaled_arrays(X, yn, E.RBF, np.ones((9, 1)), np.ones(9), np.zeros(9), A)


# ---- against scikit-learn ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", SIZES)
def test_a_lane_against_scikit_learn(engine, N, d):
    X, yn = _inputs(N, d)
    ls, c, w = _lanes(3, d, True)
    lane = 2                                                                   # (c, w) = (1.2, 5e-2)
    assert w[lane] > 0
    sk = GaussianProcessRegressor(kernel=S.sk_kernel(c[lane], ls[lane], w[lane]), alpha=A, optimizer=None).fit(X, yn)
    v_s, g_s = sk.log_marginal_likelihood(sk.kernel_.theta, eval_gradient=True)
    v, g = engine.lml_batch_scaled_arrays(X, yn, E.MATERN25, ls, c, w, A)
    print(N, d, "lml", abs(v[lane] - v_s) / max(1.0, abs(v_s)), "grad", float(np.max(np.abs(g[lane] - g_s)) / np.max(np.abs(g_s))))
    assert g[lane].shape == g_s.shape
    assert abs(v[lane] - v_s) <= 1e-10 * max(1.0, abs(v_s))
    assert np.max(np.abs(g[lane] - g_s)) <= 1e-7 * max(np.max(np.abs(g_s)), 1e-12)


# ---- the search ----------------------------------------------------------------------------------------------------------------------------
def _search(engine, kernel, X, y, lanes, seed=4):
    gp = HipGPR(kernel=kernel, alpha=A, normalize_y=True, n_restarts_optimizer=5, engine=engine, random_state=np.random.RandomState(seed),
                scaled_kernels=True, scaled_lanes=lanes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.fit(X, y)
    assert not gp._host_mode
    return gp


@pytest.mark.parametrize("N,form", [(60, "C*k+W"), (300, "C*k+W"), (60, "k*C_fixed_l")])
def test_the_lockstep_search_is_the_sequential_search(engine, N, form):
    """Every lane returns the bits the sequential run saw and the lockstep driver is iterate for iterate SciPy's: the same theta, the
    same value, the same RandomState afterwards — in fewer rounds than evaluations."""
    d = 3
    X, y = S.data(N, d, 6)
    if form == "C*k+W":
        kernel = ConstantKernel(1.0) * Matern(nu=2.5, length_scale=np.ones(d)) + WhiteKernel(1e-2)
    else:
        kernel = Matern(nu=2.5, length_scale=0.6, length_scale_bounds="fixed") * ConstantKernel(1.0) + WhiteKernel(1e-2)
    lock, seq = _search(engine, kernel, X, y, True), _search(engine, kernel, X, y, False)
    assert _same_bits(lock.kernel_.theta, seq.kernel_.theta)
    assert _same_bits(lock.log_marginal_likelihood_value_, seq.log_marginal_likelihood_value_)
    assert lock.theta_search_rounds_ < lock.theta_search_evals_
    assert not hasattr(seq, "theta_search_rounds_")
    assert lock.random_state.uniform() == seq.random_state.uniform()
    Xq = np.random.RandomState(5).uniform(size=(40, d))
    sk = GaussianProcessRegressor(kernel=lock.kernel_, alpha=A, normalize_y=True, optimizer=None).fit(X, y)
    mu, sd = lock.predict(Xq, return_std=True)
    mu_s, sd_s = sk.predict(Xq, return_std=True)
    assert rel_err(mu, mu_s) < 1e-9 and rel_err(sd, sd_s) < 1e-9


def test_a_constrained_suggest_with_both_models_scaled_and_searched_in_lanes(engine):
    """The fused policy's suggest() (the shape of tests/test_gpu_scaled_kernel.py's constrained test) with the target GP and the
    constraint GP scaled, each with a theta search of three starts in lockstep lanes: a point of the box, both models on the device,
    their posteriors scikit-learn's for the fitted kernels (1e-9)."""
    from bayesianoptimization_amd import fused_acquisition as FA
    from bayesianoptimization_amd.constraint_model import HipConstraintModel
    from bayesianoptimization_amd.float_space import FloatSpace

    N, d = 60, 3
    X, y = S.data(N, d, 4)
    cv = np.cos(2.0 * X.sum(1))
    k_t = S.sk_kernel(7.0, S.length_scale(d, True), 2e-3)
    k_c = S.sk_kernel(0.3, 0.6, 5e-2)
    cm = HipConstraintModel(None, -np.inf, 0.5, engine=engine, random_state=np.random.RandomState(3))
    cm._model[0].set_params(kernel=k_c, n_restarts_optimizer=2, scaled_kernels=True, scaled_lanes=True)
    sp = FloatSpace({f"w{j}": (0.0, 1.0) for j in range(d)}, constraint=cm)
    sp.register_bulk(X, y, cv)
    gp = HipGPR(kernel=k_t, alpha=A, normalize_y=True, n_restarts_optimizer=2, engine=engine, random_state=np.random.RandomState(1),
                scaled_kernels=True, scaled_lanes=True)
    fn = FA.ExpectedImprovement(xi=0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = fn.suggest(gp, sp, n_random=2000, n_smart=2, fit_gp=True, random_state=np.random.RandomState(2))
    assert x.shape == (d,) and np.all(x >= 0.0) and np.all(x <= 1.0)
    assert not gp._host_mode and not cm._model[0]._host_mode
    Xq = np.random.RandomState(5).uniform(size=(50, d))
    for mine, target in ((gp, y), (cm._model[0], cv)):
        assert mine._scale is not None and mine.theta_search_rounds_ < mine.theta_search_evals_
        sk = GaussianProcessRegressor(kernel=mine.kernel_, alpha=A, normalize_y=True, optimizer=None).fit(X, target)
        mu, sd = mine.predict(Xq, return_std=True)
        mu_s, sd_s = sk.predict(Xq, return_std=True)
        assert rel_err(mu, mu_s) < 1e-9 and rel_err(sd, sd_s) < 1e-9
