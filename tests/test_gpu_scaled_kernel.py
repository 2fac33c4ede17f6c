"""GPU (-m gpu): scaled models  c * k + w  (ConstantKernel * k + WhiteKernel, opt-in) on the device — gpbo_fit_scaled /
gpbo_lml_scaled, the slot's amplitude and white in every pass that turns |W k*|^2 into a variance, and HipGPR(scaled_kernels=True) —
against scikit-learn itself (`GaussianProcessRegressor(kernel=C(c) * Matern(nu=2.5) + WhiteKernel(w), alpha=1e-6, normalize_y=True,
optimizer=None)`), at the shapes and bars tests/test_gpu_matern_family.py uses for the same passes:

    K 1e-14, L 1e-10, alpha 1e-8; mu / sigma 1e-9 max-norm and 1e-5 per candidate; LML 1e-10, its gradient 1e-7 of its largest
    component; fp32 mode 1e-4 of the acquisition's range with the arg-best exact.

(c, w) in {(0.3, 0), (7, 2e-3), (1, 5e-2)}, alpha = 1e-6, length scale 0.25 sqrt d (one value or one per dimension); data as elsewhere
in the suite: X uniform on [0, 1]^d, y = sin(3 sum X) + 0.1 noise, seeded.  What scikit-learn does not offer (the input gradient) comes
from tests/scaled_kernel_truth.py, which tests/test_scaled_kernel_host.py pins against scikit-learn."""
import ctypes as C
import os

import numpy as np
import pytest
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

import scaled_kernel_truth as S
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import engine as E
from bayesianoptimization_amd.gpr import HipGPR
from conftest import elementwise_err, load_golden, rel_err
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

KIND = E.MATERN25
A = S.ALPHA
TIERS = [(40, 3), (200, 6), (830, 5)]      # one-workgroup fit (NP = 64), strip path (NP = 256), blocked path (NP = 832)
cases = pytest.mark.parametrize("c,w", S.CASES, ids=S.CASE_IDS)

_fits = {}


def _sk(c, w, N, d, per_dim, seed=0):
    """(X, y, fitted scikit-learn estimator, length scale) of one case, computed once and shared, left unchanged."""
    key = (c, w, N, d, per_dim, seed)
    if key not in _fits:
        X, y = S.data(N, d, seed)
        ls = S.length_scale(d, per_dim)
        sk = GaussianProcessRegressor(kernel=S.sk_kernel(c, ls, w), alpha=A, normalize_y=True, optimizer=None).fit(X, y)
        X.setflags(write=False)
        y.setflags(write=False)
        _fits[key] = (X, y, sk, ls)
    return _fits[key]


def _fit(engine, c, w, X, y, sk, ls, **kw):
    ym, ys = float(sk._y_train_mean), float(sk._y_train_std)
    engine.fit(X, (y - ym) / ys, KIND, ls, A, amplitude=c, white=w, **kw)
    return ym, ys


def _fit_scaled_raw(engine, X, yn, ls, c, w, a, slot=0):
    """gpbo_fit_scaled itself (GpEngine.fit makes the unit model's call at c = 1, w = 0)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    yn = np.ascontiguousarray(yn, dtype=np.float64)
    ls = np.ascontiguousarray(np.atleast_1d(np.asarray(ls, dtype=np.float64)))
    info = C.c_int(0)
    engine._touch(slot)
    rc = engine._lib.gpbo_fit_scaled(engine._h, slot, _lib.dptr(X), _lib.dptr(yn), X.shape[0], X.shape[1], KIND, _lib.dptr(ls), ls.shape[0],
                                     float(c), float(w), float(a), 0, C.byref(info))
    engine._check(rc, info.value)
    engine._touch(slot)


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_invalid_amplitude_or_white_raises(engine):
    X, y = S.data(10, 2)
    for c, w in ((0.0, 0.0), (-1.0, 0.0), (2.0, -1e-3), (np.inf, 0.0), (np.nan, 0.0), (2.0, np.nan), (2.0, np.inf)):
        with pytest.raises(ValueError, match="amplitude"):
            engine.fit(X, y, KIND, 1.0, A, amplitude=c, white=w)
        with pytest.raises(ValueError, match="amplitude"):
            engine.lml(X, y, KIND, 1.0, A, amplitude=c, white=w, scaled=True)
    with pytest.raises(ValueError, match="alpha"):
        engine.fit(X, y, KIND, 1.0, -1.0, amplitude=2.0)
    engine.fit(X, y, KIND, 1.0, A, amplitude=2.0, white=0.1)
    with pytest.raises(ValueError, match="differ"):
        engine.fit_append(X[:1] + 0.3, np.append(y, 0.1))                      # the caller believes it grows a unit model


# ---- fit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "per_dim"])
@pytest.mark.parametrize("N,d", TIERS)
@cases
def test_fit_tiers_against_scikit_learn(engine, c, w, N, d, per_dim):
    X, y, sk, ls = _sk(c, w, N, d, per_dim)
    _fit(engine, c, w, X, y, sk, ls)
    K = sk.kernel_(X)
    K[np.diag_indices_from(K)] += A
    errs = {"K": rel_err(engine.get_K(N), K), "L": rel_err(engine.get_L(N), sk.L_), "alpha": rel_err(engine.get_alpha(N), sk.alpha_),
            "Linv": rel_err(engine.get_Linv(N), np.sqrt(c) * np.linalg.inv(sk.L_))}      # gpbo_get_Linv stays the unit model's W'
    print(c, w, N, d, per_dim, errs)
    assert errs["K"] < 1e-14 and errs["L"] < 1e-10 and errs["alpha"] < 1e-8 and errs["Linv"] < 1e-8
    Kg = engine.get_K(N)
    assert np.array_equal(Kg, Kg.T) and np.all(np.triu(engine.get_L(N), 1) == 0.0)


@pytest.mark.parametrize("N,d", TIERS)
def test_unit_amplitude_and_no_white_are_the_unscaled_bits(engine, N, d):
    """gpbo_fit_scaled and gpbo_lml_scaled at c = 1, w = 0 against gpbo_fit / gpbo_lml at noise = alpha: L, W, alpha, mu, sigma, the
    LML value and the length scales' gradient bit for bit."""
    X, y, sk, ls = _sk(1.0, 0.0, N, d, True)
    ym, ys = float(sk._y_train_mean), float(sk._y_train_std)
    yn = (y - ym) / ys
    Xc = np.random.RandomState(4).uniform(size=(300, d))
    Xc[2] = X[1]
    engine.fit(X, yn, KIND, ls, A)
    ref = [engine.get_K(N), engine.get_L(N), engine.get_Linv(N), engine.get_alpha(N), *engine.predict(Xc, y_mean=ym, y_std=ys),
           *engine.predict(Xc[:5], y_mean=ym, y_std=ys), *engine.predict_grad(Xc[:9], 0, ym, ys)]
    _fit_scaled_raw(engine, X, yn, ls, 1.0, 0.0, A)
    got = [engine.get_K(N), engine.get_L(N), engine.get_Linv(N), engine.get_alpha(N), *engine.predict(Xc, y_mean=ym, y_std=ys),
           *engine.predict(Xc[:5], y_mean=ym, y_std=ys), *engine.predict_grad(Xc[:9], 0, ym, ys)]
    for i, (a, b) in enumerate(zip(ref, got)):
        assert np.array_equal(a, b), i
    v, g = engine.lml(X, yn, KIND, ls, A)
    v1, g1 = engine.lml(X, yn, KIND, ls, A, scaled=True)
    assert v1 == v and g1.shape == (d + 2,) and np.array_equal(g1[1:-1], g) and g1[-1] == 0.0
    assert engine.lml(X, yn, KIND, ls, A, eval_gradient=False, scaled=True) == v


# ---- posterior --------------------------------------------------------------------------------------------------------------------
# path of posterior_plan.h -> (N, d, M), as tests/test_gpu_matern_family.py: NP = 256 (one row chunk), 448 (two), 832 (four, fp64
# slab), 2112 (int8 slab, ragged last chunk)
POST_PATHS = {"small": (200, 6, 5), "fused256": (200, 6, 1000), "fused512": (400, 5, 10000), "slab_f64": (830, 5, 1000),
              "slab_i8": (2050, 16, 300)}


def _assert_posterior(mu, sd, mu_s, sd_s, ys, what):
    errs = (rel_err(mu, mu_s), rel_err(sd, sd_s)) + elementwise_err(sd, sd_s, mu, mu_s, ys)
    print(what, "rel_err mu, sd; elementwise sd, mu:", errs)
    assert errs[0] < 1e-9 and errs[1] < 1e-9 and max(errs[2:]) <= 1e-5, (what, errs)


@pytest.mark.parametrize("path", list(POST_PATHS))
@cases
def test_posterior_paths_against_scikit_learn(engine, c, w, path):
    N, d, M = POST_PATHS[path]
    X, y, sk, ls = _sk(c, w, N, d, path in ("fused512", "slab_i8"))
    Xc = np.random.RandomState(3).uniform(size=(M, d))
    Xc[min(7, M - 1)] = X[3]                     # a training point: the cancellation case, c (1 - q) + w ~ w + alpha
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    ym, ys = _fit(engine, c, w, X, y, sk, ls)
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    assert mu.shape == sd.shape == (M,)
    _assert_posterior(mu, sd, mu_s, sd_s, ys, (c, w, path))


@cases
def test_f32_mode_within_1e4_of_the_range_with_the_exact_arg_best(engine, c, w):
    """precision = F32 at N = 600 (tests/test_gpu_f32.py's bound): -UCB within 1e-4 of its range of scikit-learn's, the arg-best index
    exact (scikit-learn's own top-2 gap stands more than twice the bound clear); mu keeps fp64 accuracy (1e-7).  The variance bound
    of that file, 2e-5 s_y^2, is a bound on the error of q = |W k*|^2 in fp32; the scaled variance is c (1 - q) + w, so it is
    2e-5 c s_y^2 here."""
    N, d, M, kappa = 600, 5, 3000, 2.576
    X, y, sk, ls = _sk(c, w, N, d, False, seed=31)
    Xc = np.random.RandomState(32).uniform(size=(M, d))
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    ref = -(mu_s + kappa * sd_s)
    e = 1e-4 * float(ref.max() - ref.min())
    top = np.sort(ref)[:2]
    assert top[1] - top[0] > 2 * e
    ym, ys = _fit(engine, c, w, X, y, sk, ls, precision=E.F32)
    assert rel_err(engine.get_L(N), sk.L_) < 1e-10             # the factorisation is still fp64
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    bi, bv, _, _, vals = engine.acq_argbest(E.UCB, kappa, return_values=True)
    print(c, w, "f32: max |acq - ref| / bound", float(np.max(np.abs(vals - ref))) / e, "mu", rel_err(mu, mu_s),
          "var / bound", float(np.max(np.abs(sd**2 - sd_s**2))) / (2e-5 * c * ys**2))
    assert np.max(np.abs(vals - ref)) <= e
    assert bi == int(ref.argmin()) and abs(bv - float(ref.min())) <= e
    assert rel_err(mu, mu_s) < 1e-7 and np.max(np.abs(sd**2 - sd_s**2)) < 2e-5 * c * ys**2


# ---- LML --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "per_dim"])
@pytest.mark.parametrize("N,d", TIERS + [(2050, 4)])
@cases
def test_lml_value_and_every_gradient_component_against_scikit_learn(engine, c, w, N, d, per_dim):
    """gpbo_lml_scaled against log_marginal_likelihood(theta, eval_gradient=True): value 1e-10, all n_ls + 2 components
    [log c, log l ..., log w] 1e-7 of the largest; the value-only call returns the same value; the slot is left unfitted.
    (At w = 0 scikit-learn's kernel has no WhiteKernel and no log w entry: the device's is then exactly 0.)"""
    X, y, sk, ls = _sk(c, w, N, d, per_dim)
    yn = (y - sk._y_train_mean) / sk._y_train_std
    v_s, g_s = sk.log_marginal_likelihood(sk.kernel_.theta, eval_gradient=True)
    v, g = engine.lml(X, yn, KIND, ls, A, amplitude=c, white=w, scaled=True)
    n_ls = np.atleast_1d(ls).shape[0]
    assert g.shape == (n_ls + 2,)
    if w == 0.0:
        assert g[-1] == 0.0
        g = g[:-1]
    print(c, w, N, d, per_dim, "lml", abs(v - v_s) / max(1.0, abs(v_s)), "grad", float(np.max(np.abs(g - g_s)) / np.max(np.abs(g_s))))
    assert g.shape == g_s.shape
    assert abs(v - v_s) <= 1e-10 * max(1.0, abs(v_s))
    assert np.max(np.abs(g - g_s)) <= 1e-7 * max(np.max(np.abs(g_s)), 1e-12)
    assert engine.lml(X, yn, KIND, ls, A, eval_gradient=False, amplitude=c, white=w, scaled=True) == v
    with pytest.raises(_lib.GpboError):
        engine.posterior(0)                      # gpbo_lml_scaled leaves the slot unfitted


def test_a_matrix_that_is_not_positive_definite_gives_minus_inf_and_a_zero_gradient(engine):
    """Every row twice and no noise at all (the construction of tests/test_gpu_mid_fit.py): -inf and n_ls + 2 zeros, status OK."""
    X, _ = S.data(150, 3)
    Xd = np.vstack([X, X])
    v, g = engine.lml(Xd, np.zeros(300), E.RBF, [1.0], 0.0, amplitude=3.0, white=0.0, scaled=True)
    assert v == -np.inf and g.shape == (3,) and np.all(g == 0.0)
    assert engine.lml(Xd, np.zeros(300), E.RBF, [1.0], 0.0, eval_gradient=False, amplitude=3.0, scaled=True) == -np.inf


# ---- state ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,M", [(40, 3, 5), (200, 6, 1000), (830, 5, 1000)])
def test_no_amplitude_or_white_leaks_into_a_later_unscaled_fit(engine, N, d, M):
    """One context, in this order: unscaled fit and predict, scaled fit and predict, unscaled fit and predict — the first and the last
    are equal bit for bit; so they are after a gpbo_lml_scaled on the slot, after a scaled fit + gpbo_lml, and in another slot."""
    X, y, sk, ls = _sk(7.0, 2e-3, N, d, False)
    ym, ys = float(sk._y_train_mean), float(sk._y_train_std)
    yn = (y - ym) / ys
    Xc = np.random.RandomState(8).uniform(size=(M, d))

    def unscaled(slot=0):
        engine.fit(X, yn, KIND, ls, A, slot=slot)
        mu, sd = engine.predict(Xc, slot=slot, y_mean=ym, y_std=ys)
        _, cov = engine.predict_cov(Xc[:6], slot=slot, y_mean=ym, y_std=ys)
        return [mu, sd, cov, *engine.predict_grad(Xc[:4], slot, ym, ys), engine.get_K(N, slot), engine.get_L(N, slot), engine.get_alpha(N, slot)]

    first = unscaled()
    engine.fit(X, yn, KIND, ls, A, amplitude=7.0, white=2e-3)
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    assert rel_err(mu, mu_s) < 1e-9 and rel_err(sd, sd_s) < 1e-9 and not np.array_equal(sd, first[1])
    for a, b in zip(first, unscaled()):
        assert np.array_equal(a, b)
    engine.lml(X, yn, KIND, ls, A, amplitude=7.0, white=2e-3, scaled=True)
    for a, b in zip(first, unscaled()):
        assert np.array_equal(a, b)
    engine.fit(X, yn, KIND, ls, A, amplitude=7.0, white=2e-3)
    engine.lml(X, yn, KIND, ls, A)               # gpbo_lml makes the slot a unit model again ...
    engine.fit(X, yn, KIND, ls, A, amplitude=7.0, white=2e-3, slot=1)
    for a, b in zip(first, unscaled()):
        assert np.array_equal(a, b)
    for a, b in zip(first, unscaled(slot=2)):    # ... and a scaled slot 1 says nothing about slot 2
        assert np.array_equal(a, b)
    mu1, sd1 = engine.predict(Xc, slot=1, y_mean=ym, y_std=ys)
    assert rel_err(mu1, mu_s) < 1e-9 and rel_err(sd1, sd_s) < 1e-9


@pytest.mark.parametrize("N,d", [(40, 3), (830, 5)])
def test_scaled_fits_inside_overlapped_fits_are_the_sequential_fits(engine, N, d):
    """Inside overlapped_fits() — where suggest() fits the target GP and the constraint GPs — a unit model's fit is enqueued on its
    slot's stream and a scaled model's fit runs at once on the context's stream (gpbo_fit_begin has no scaled twin): slot 1 unit,
    slots 0 and 2 scaled, slot 0 refitted scaled while slot 1 is still pending.  Every slot's factorisation and posterior are bit for
    bit what the same fits give one after another outside the block."""
    X, y, sk, ls = _sk(7.0, 2e-3, N, d, True)
    ym, ys = float(sk._y_train_mean), float(sk._y_train_std)
    yn = (y - ym) / ys
    Xc = np.random.RandomState(8).uniform(size=(700, d))
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    fits = [(1, {}), (0, {"amplitude": 0.3}), (2, {"amplitude": 1.0, "white": 5e-2}), (0, {"amplitude": 7.0, "white": 2e-3})]

    def read():
        return [[engine.get_L(N, s), engine.get_alpha(N, s), *engine.predict(Xc, slot=s, y_mean=ym, y_std=ys)] for s in (0, 1, 2)]

    for slot, kw in fits:
        engine.fit(X, yn, KIND, ls, A, slot=slot, **kw)
    ref = read()
    for s in (0, 1, 2):
        engine.fit(X[:20], yn[:20], E.RBF, 1.0, 1e-3, slot=s)                  # other models in between
    with engine.overlapped_fits():
        for slot, kw in fits:
            engine.fit(X, yn, KIND, ls, A, slot=slot, **kw)
        assert engine._pending_fits == {1}
    assert not engine._pending_fits
    for a, b in zip(ref, read()):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert rel_err(ref[0][2], mu_s) < 1e-9 and rel_err(ref[0][3], sd_s) < 1e-9 and not np.array_equal(ref[0][3], ref[1][3])


@pytest.mark.parametrize("scale_the_constraint", [False, True], ids=["unit_constraint_gp", "scaled_constraint_gp"])
def test_a_constrained_suggest_fits_scaled_models_and_returns_scikit_learns_posteriors(engine, scale_the_constraint):
    """The fused policy's suggest() with a constraint model — its _fit_gp opens overlapped_fits() around the target GP's and the
    constraint GP's fit — and a scaled kernel on the target GP, and on the constraint GP or not: it returns a point of the box, both
    models are on the device, and their posteriors are scikit-learn's for the same kernels (1e-9)."""
    from bayesianoptimization_amd import fused_acquisition as FA
    from bayesianoptimization_amd.constraint_model import HipConstraintModel
    from bayesianoptimization_amd.float_space import FloatSpace

    N, d = 60, 3
    X, y = S.data(N, d, 4)
    cv = np.cos(2.0 * X.sum(1))
    k_t = S.sk_kernel(7.0, S.length_scale(d, True), 2e-3)
    k_c = S.sk_kernel(0.3, 0.6, 5e-2) if scale_the_constraint else Matern(nu=2.5, length_scale=0.6)
    cm = HipConstraintModel(None, -np.inf, 0.5, engine=engine, random_state=np.random.RandomState(3))
    cm._model[0].set_params(kernel=k_c, optimizer=None, scaled_kernels=True)
    sp = FloatSpace({f"w{j}": (0.0, 1.0) for j in range(d)}, constraint=cm)
    sp.register_bulk(X, y, cv)
    gp = HipGPR(kernel=k_t, alpha=A, normalize_y=True, optimizer=None, engine=engine, scaled_kernels=True)
    fn = FA.ExpectedImprovement(xi=0.01)          # (UCB takes no constraint, as in the reference)
    x = fn.suggest(gp, sp, n_random=2000, n_smart=2, fit_gp=True, random_state=np.random.RandomState(2))
    assert x.shape == (d,) and np.all(x >= 0.0) and np.all(x <= 1.0)
    assert not gp._host_mode and not cm._model[0]._host_mode
    assert gp._scale == (7.0, 2e-3) and (cm._model[0]._scale == (0.3, 5e-2) if scale_the_constraint else cm._model[0]._scale is None)
    Xq = np.random.RandomState(5).uniform(size=(50, d))
    for mine, kernel, target in ((gp, k_t, y), (cm._model[0], k_c, cv)):
        sk = GaussianProcessRegressor(kernel=kernel, alpha=A, normalize_y=True, optimizer=None).fit(X, target)
        mu, sd = mine.predict(Xq, return_std=True)
        mu_s, sd_s = sk.predict(Xq, return_std=True)
        assert rel_err(mu, mu_s) < 1e-9 and rel_err(sd, sd_s) < 1e-9


@pytest.mark.parametrize("n0,n_new", [(100, 3), (126, 3)], ids=["rows_in_the_padding", "rebuild_into_new_padding"])
@cases
def test_fit_append_to_a_scaled_slot_equals_a_full_scaled_fit(engine, c, w, n0, n_new):
    """Appending 3 rows to a scaled slot (inside the 64-row padding: rank-one growth; across it: the rebuild branch, which carries c
    and w over) gives scikit-learn's full fit at the existing append test's bars (tol = 1e-9)."""
    d, tol = 5, 1e-9
    n = n0 + n_new
    X, y, sk, ls = _sk(c, w, n, d, False, seed=61)
    yn0, _, _ = O.normalize_targets(y[:n0])
    engine.fit(X[:n0], yn0, KIND, ls, A, amplitude=c, white=w)
    ym, ys = float(sk._y_train_mean), float(sk._y_train_std)
    yn = (y - ym) / ys
    engine.fit_append(X[n0:], yn, amplitude=c, white=w)
    K = sk.kernel_(X)
    K[np.diag_indices_from(K)] += A
    Xc = np.random.RandomState(62).uniform(size=(300, d))
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    errs = {"K": (rel_err(engine.get_K(n), K), 1e-14), "L": (rel_err(engine.get_L(n), sk.L_), tol),
            "alpha": (rel_err(engine.get_alpha(n), sk.alpha_), 100 * tol), "mu": (rel_err(mu, mu_s), tol), "sd": (rel_err(sd, sd_s), tol)}
    print(c, w, n0, errs)
    for k, (e, bar) in errs.items():
        assert e < bar, f"{k} {e:.2e} over its bar {bar:.0e}"


# ---- covariance, input gradient -----------------------------------------------------------------------------------------------------
@cases
def test_predict_cov_against_return_cov(engine, c, w):
    """HipGPR(scaled_kernels=True).predict(return_cov=True) at N = 50, M = 20 against scikit-learn's, at the bars of
    test_predict_cov_equals_sklearn_return_cov."""
    N, d, M = 50, 4, 20
    X, y, sk, ls = _sk(c, w, N, d, True)
    Xq = np.random.RandomState(6).uniform(size=(M, d))
    mu_s, cov_s = sk.predict(Xq, return_cov=True)
    gp = HipGPR(kernel=S.sk_kernel(c, ls, w), alpha=A, normalize_y=True, optimizer=None, engine=engine, scaled_kernels=True).fit(X, y)
    assert not gp._host_mode and gp._scale == (c, w)
    mu, cov = gp.predict(Xq, return_cov=True)
    assert cov.shape == (M, M)
    assert rel_err(mu, mu_s) < 1e-8
    assert np.max(np.abs(cov - cov_s)) < 1e-8 * np.max(np.abs(cov_s))
    assert np.max(np.abs(cov - cov.T)) < 1e-12 * np.max(np.abs(cov_s))
    _, sd = gp.predict(Xq, return_std=True)
    assert np.max(np.abs(np.sqrt(np.clip(np.diag(cov), 0, None)) - sd)) < 1e-6 * np.max(sd)
    assert rel_err(gp.L_, sk.L_) < 1e-10 and rel_err(gp.alpha_, sk.alpha_) < 1e-8


@pytest.mark.parametrize("N,d,M", [(60, 3, 7), (300, 7, 33)])
@cases
def test_predict_grad_against_the_truth_module(engine, c, w, N, d, M):
    """gpbo_predict_grad against tests/scaled_kernel_truth.predict_grad at the bars of test_predict_grad_equals_the_oracle_gradient
    (d sd / d x gains the factor c; on a training point it stays finite)."""
    X, y, sk, ls = _sk(c, w, N, d, d == 7)
    ym, ys = _fit(engine, c, w, X, y, sk, ls)
    gp = S.fit(KIND, X, y, ls, c, w)
    Xq = np.random.RandomState(5).uniform(size=(M, d))
    mu, sd, dmu, dsd = engine.predict_grad(Xq, 0, ym, ys)
    mu_o, sd_o, dmu_o, dsd_o = S.predict_grad(gp, Xq)
    errs = (rel_err(mu, mu_o), rel_err(sd, sd_o), rel_err(dmu, dmu_o), rel_err(dsd, dsd_o))
    print(c, w, N, d, "mu, sd, dmu, dsd:", errs)
    assert errs[0] < 1e-8 and errs[1] < 1e-7 and errs[2] < 1e-7 and errs[3] < 1e-6
    mu_s, sd_s = sk.predict(Xq, return_std=True)
    assert rel_err(mu, mu_s) < 1e-8 and rel_err(sd, sd_s) < 1e-7
    on = np.vstack([X[:3], X[N - 1:]])
    out = engine.predict_grad(on, 0, ym, ys)
    assert all(np.all(np.isfinite(a)) for a in out)
    assert rel_err(out[2], S.predict_grad(gp, on)[2]) < 1e-7


# ---- the searches -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def any_size():
    old = os.environ.get("GPBO_POLISH_FUSED_MAX_NP")
    os.environ["GPBO_POLISH_FUSED_MAX_NP"] = "512"
    yield
    if old is None:
        os.environ.pop("GPBO_POLISH_FUSED_MAX_NP", None)
    else:
        os.environ["GPBO_POLISH_FUSED_MAX_NP"] = old


# one launch with W in LDS (NP = 64), one launch with W streamed from memory (NP = 448), lockstep rounds (NP = 640: gpbo_predict_grad's kernels)
@pytest.mark.parametrize("N,d", [(50, 3), (400, 5), (600, 4)], ids=["one_launch_lds", "one_launch_memory", "lockstep"])
@cases
def test_polish_seeds_returns_the_scaled_models_acquisition(debug_engine, any_size, c, w, N, d):
    """gpbo_polish_seeds, UCB, kappa = 2.576, on a scaled slot: f_out is the truth's -UCB at x_out within the file's own bars on mu and
    sigma, 1e-7 max(1, max |mu|) + kappa 1e-6 max sigma; no run ends above its (clipped) seed; the points stay in the box."""
    eng, kappa = debug_engine, 2.576
    X, y, sk, ls = _sk(c, w, N, d, False, seed=100 + N)
    ym, ys = _fit(eng, c, w, X, y, sk, ls)
    gp = S.fit(KIND, X, y, ls, c, w)
    cand = np.random.RandomState(9).uniform(size=(3000, d))
    seeds = cand[np.argsort(S.neg_acquisition(gp, cand, O.UCB, kappa))[:10]].copy()
    seeds[0] = np.clip(seeds[0] + 0.7, -0.5, 1.5)
    seeds[1, 0] = 0.0
    box = np.array([[0.0, 1.0]] * d)
    x_out, f_out, status, _ = eng.polish_seeds(O.UCB, kappa, 0.0, None, None, [ym], [ys], seeds, box)
    mu_t, sd_t = S.predict(gp, x_out)
    bar = 1e-7 * max(1.0, float(np.abs(mu_t).max())) + kappa * 1e-6 * float(sd_t.max())
    print(c, w, N, d, "max |f_out + UCB(x_out)| / bar", float(np.max(np.abs(f_out + (mu_t + kappa * sd_t)))) / bar, "status", status)
    assert np.all(np.abs(f_out + (mu_t + kappa * sd_t)) <= bar)
    assert np.all(x_out >= 0.0) and np.all(x_out <= 1.0)
    assert np.all(f_out <= S.neg_acquisition(gp, np.clip(seeds, 0.0, 1.0), O.UCB, kappa) + bar)


@pytest.mark.parametrize("acq", [E.UCB, E.EI, E.POI])
@cases
def test_evolve_mixed_energies_against_the_host(debug_engine, c, w, acq):
    """The energies of the device differential evolution (gpbo_debug_evolve_eval) at N = 100 over a scaled model against the host's
    reference-shaped objective over HipGPR's posterior, at the bar of
    tests/test_gpu_evolve.py::test_device_objective_is_the_host_objective_to_rounding; and that posterior is scikit-learn's."""
    from scipy.stats import norm

    from bayesianoptimization_amd import fused_acquisition as FA
    from bayesianoptimization_amd.float_space import MixedSpace

    N = 100
    sp = MixedSpace({"a": (0.0, 2.0), "n": (-3, 7, int), "b": (1.0, 4.0), "c": ("x", "y", "z"), "e": (5.0, 6.0), "k": (0, 1, int)})
    X = sp.random_sample(N, np.random.RandomState(N + acq))
    y = np.sin(X[:, 0] + 0.3 * X[:, 1]) + 0.1 * X[:, 2] + X[:, 3] - 0.5 * X[:, 5] + 0.2 * X[:, 7]
    sp.register_bulk(X, y)
    kernel = S.sk_kernel(c, 1.3, w)
    gp = HipGPR(kernel=kernel, alpha=A, normalize_y=True, optimizer=None, engine=debug_engine, transform=sp.kernel_transform,
                scaled_kernels=True).fit(X, y)
    assert not gp._host_mode and gp._scale == (c, w)
    groups = FA._mixed_space_groups([gp], sp, np.random.RandomState(0))
    assert groups is not None
    y_max = float(np.max(y))
    fn = {E.UCB: lambda: FA.UpperConfidenceBound(kappa=2.576), E.EI: lambda: FA.ExpectedImprovement(xi=0.01),
          E.POI: lambda: FA.ProbabilityOfImprovement(xi=0.01)}[acq]()
    fn.y_max = y_max
    pts = sp.random_sample(40, np.random.RandomState(3))
    pts[:20] += np.random.RandomState(4).uniform(-0.45, 0.45, size=(20, sp.dim))
    pts = np.clip(pts, sp.bounds[:, 0], sp.bounds[:, 1])
    got = debug_engine.debug_evolve_eval(fn._acq_kind, fn._acq_param(), y_max, float(gp._y_train_mean), float(gp._y_train_std), groups, pts)
    obj = fn._get_acq(gp)
    want = np.array([obj(p)[0] for p in pts])
    mu = np.empty(len(pts))
    sd = np.empty(len(pts))
    for i, p in enumerate(pts):
        m, s = gp._posterior_trusted(p[None])
        mu[i], sd[i] = m[0], s[0]
    sk = GaussianProcessRegressor(kernel=kernel, alpha=A, normalize_y=True, optimizer=None).fit(sp.kernel_transform(X), y)
    mu_s, sd_s = sk.predict(np.vstack([sp.kernel_transform(p[None]) for p in pts]), return_std=True)
    assert rel_err(mu, mu_s) < 1e-9 and rel_err(sd, sd_s) < 1e-9
    if acq == E.UCB:
        z, scale = np.zeros(len(pts)), np.abs(mu) + 2.576 * sd
    else:
        a = mu - y_max - 0.01
        z = a / sd
        scale = np.abs(a) * norm.cdf(z) + sd * norm.pdf(z) if acq == E.EI else norm.cdf(z)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= 1e-11 * (1.0 + z * z) * scale + 1e-300)


# ---- the theta search ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,seed", [(60, 2, 0), (120, 3, 2)])
def test_theta_search_over_c_l_and_w_matches_scikit_learns_optimum(engine, N, d, seed):
    """C(1) * Matern(2.5, ones(d)) + WhiteKernel(1e-2), 3 restarts, against GaussianProcessRegressor with the same RandomState, at
    test_device_theta_search_matches_sklearn_optimum's bars: the next uniform() equal on both, LML within 1e-8 relative, theta to
    1e-4, predictions at 200 points to 1e-5."""
    X, y = S.data(N, d, seed)
    kernel = ConstantKernel(1.0) * Matern(nu=2.5, length_scale=np.ones(d)) + WhiteKernel(1e-2)
    r1, r2 = np.random.RandomState(seed), np.random.RandomState(seed)
    kw = dict(alpha=A, normalize_y=True, n_restarts_optimizer=3)
    sk = GaussianProcessRegressor(kernel=kernel, random_state=r1, **kw).fit(X, y)
    gp = HipGPR(kernel=kernel, random_state=r2, engine=engine, scaled_kernels=True, **kw).fit(X, y)
    assert not gp._host_mode
    assert r1.uniform() == r2.uniform()
    print(N, d, "lml", gp.log_marginal_likelihood_value_, sk.log_marginal_likelihood_value_, "theta", gp.kernel_.theta, sk.kernel_.theta)
    assert gp.log_marginal_likelihood_value_ == pytest.approx(sk.log_marginal_likelihood_value_, rel=1e-8)
    assert np.allclose(gp.kernel_.theta, sk.kernel_.theta, rtol=1e-4, atol=1e-4)
    th = sk.kernel_.theta
    v1, g1 = sk.log_marginal_likelihood(th, eval_gradient=True)
    v2, g2 = gp.log_marginal_likelihood(th, eval_gradient=True)          # on a fitted model: the fit is restored
    assert v2 == pytest.approx(v1, rel=1e-10) and np.max(np.abs(g2 - g1)) <= 1e-7 * max(np.max(np.abs(g1)), 1e-12) + 1e-9
    Xc = np.random.RandomState(5).uniform(size=(200, d))
    m1, s1 = sk.predict(Xc, return_std=True)
    m2, s2 = gp.predict(Xc, return_std=True)
    assert rel_err(m2, m1) < 1e-5 and rel_err(s2, s1) < 1e-5


# ---- the full acquisition pass against the reference's own run (tests/golden/scaled_kernel.npz) ---------------------------------------
def test_full_acquisition_pass_matches_the_reference(engine):
    """d = 3, N = 60, M = 4096 at the theta the reference's own fit found with set_gp_params(kernel=C * Matern(2.5) + WhiteKernel())
    (scripts/gen_scaled_kernel_golden.py): alpha, mu, sigma, -UCB and -EI at tests/test_gpu_golden.py's bars (1e-8 max-norm, 1e-5 per
    candidate), the arg-best index and the top-16 exact."""
    TOL = 1e-8
    g = load_golden("scaled_kernel")
    X, y, Xc = g["X"], g["y"], g["candidates"]
    yn, ym, ys = O.normalize_targets(y)
    assert ym == g["y_mean"] and ys == g["y_std"]
    engine.fit(X, yn, KIND, g["length_scale"], float(g["alpha_estimator"]), amplitude=float(g["constant_value"]), white=float(g["noise_level"]))
    assert rel_err(engine.get_alpha(len(y)), g["alpha"]) < TOL
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    assert rel_err(mu, g["mu"]) < TOL and rel_err(sd, g["sd"]) < TOL
    assert max(elementwise_err(sd, g["sd"], mu, g["mu"], ys)) <= 1e-5
    for name, acq, param in (("ucb", E.UCB, float(g["kappa"])), ("ei", E.EI, float(g["xi"]))):
        ref = g["ys_" + name]
        bi, bv, si, sv, vals = engine.acq_argbest(acq, param, float(g["y_max"]), None, None, k_seeds=16, return_values=True)
        print(name, "max |acq - ref| / max |ref|:", float(np.max(np.abs(vals - ref)) / np.max(np.abs(ref))))
        assert np.max(np.abs(vals - ref)) <= TOL * np.max(np.abs(ref))
        assert bi == int(g["argmin_" + name])
        assert np.array_equal(si, g["topk_idx_" + name])
        assert bv == pytest.approx(float(ref.min()), rel=TOL)
        assert np.allclose(sv, g["topk_val_" + name], rtol=TOL, atol=0)
