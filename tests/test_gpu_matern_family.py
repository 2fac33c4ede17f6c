"""GPU (-m gpu): Matern nu = 1.5 and nu = 0.5 on the device (kinds 2 and 3 of gpbo.h), through every pass that takes the kernel type
as a template argument — the three fit tiers, every posterior path, LML and its gradient, the row append, the covariance, the input
gradient and the one-launch searches — against scikit-learn itself (`GaussianProcessRegressor(kernel=Matern(nu=..), alpha=1e-6,
normalize_y=True, optimizer=None)`), at the bars the suite holds Matern nu = 2.5 to:

    K 1e-14, L 1e-10, L^-1 and alpha 1e-8 (tests/test_gpu_parity.py::test_fit_parity), mu / sigma 1e-9 max-norm and 1e-5 per candidate
    (conftest.elementwise_err), LML 1e-10, its gradient 1e-7 of its largest component, fp32 mode 1e-4 of the acquisition's range with the
    arg-best exact (tests/test_gpu_f32.py).

oracle/gp_oracle.py knows RBF and nu = 2.5 only; where a test needs more than scikit-learn offers (the input gradient, the terms of a
sum) it uses tests/matern_family_truth.py, which tests/test_matern_family_host.py pins against scikit-learn.  Data as elsewhere in the
suite: X uniform on [0, 1]^d, y = sin(3 sum X) + 0.1 noise, seeded."""
import os

import numpy as np
import pytest
from sklearn.gaussian_process import GaussianProcessRegressor

import matern_family_truth as F
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import engine as E
from conftest import elementwise_err, load_golden, rel_err
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

KINDS = [E.MATERN15, E.MATERN05]
NOISE = 1e-6
TIERS = [(40, 3), (200, 6), (830, 5)]      # one-workgroup fit (NP = 64), strip path (NP = 256), blocked path (NP = 832)


def _ls(d, per_dim):
    """The suite's length scale for d dimensions (tests/test_gpu_polish_fused.py: 0.25 sqrt d), one value or one per dimension."""
    ls = 0.25 * np.sqrt(d)
    return ls * np.linspace(0.7, 1.4, d) if per_dim else float(ls)


_fits = {}


def _sk(kind, N, d, per_dim, seed=0, dup=False):
    """(X, y, fitted scikit-learn estimator, length scale) of one case, computed once and shared, left unchanged."""
    key = (kind, N, d, per_dim, seed, dup)
    if key not in _fits:
        X, y = F.data(N, d, seed)
        if dup:
            X[5] = X[2]                         # two identical rows
        ls = _ls(d, per_dim)
        sk = GaussianProcessRegressor(kernel=F.sk_kernel(kind, ls), alpha=NOISE, normalize_y=True, optimizer=None).fit(X, y)
        X.setflags(write=False)
        y.setflags(write=False)
        _fits[key] = (X, y, sk, ls)
    return _fits[key]


def _fit(engine, kind, X, y, sk, ls, **kw):
    ym, ys = float(sk._y_train_mean), float(sk._y_train_std)
    engine.fit(X, (y - ym) / ys, kind, ls, NOISE, **kw)
    return ym, ys


def test_the_new_kinds_are_accepted_and_unknown_ones_are_not(engine):
    X, y = F.data(10, 2)
    for kind in KINDS:
        engine.fit(X, y, kind, 1.0, NOISE)
        assert np.isfinite(engine.lml(X, y, kind, 1.0, NOISE)[0])
    for kind in (4, 7, -1):
        with pytest.raises(NotImplementedError, match="RBF or Matern"):
            engine.fit(X, y, kind, 1.0, NOISE)
        with pytest.raises(NotImplementedError):
            engine.lml(X, y, kind, 1.0, NOISE)


@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "per_dim"])
@pytest.mark.parametrize("N,d", TIERS)
@pytest.mark.parametrize("kind", KINDS)
def test_fit_tiers_against_scikit_learn(engine, kind, N, d, per_dim):
    X, y, sk, ls = _sk(kind, N, d, per_dim)
    _fit(engine, kind, X, y, sk, ls)
    K = sk.kernel_(X)
    K[np.diag_indices_from(K)] += NOISE
    errs = {"K": rel_err(engine.get_K(N), K), "L": rel_err(engine.get_L(N), sk.L_),
            "Linv": rel_err(engine.get_Linv(N), np.linalg.inv(sk.L_)), "alpha": rel_err(engine.get_alpha(N), sk.alpha_)}
    print(kind, N, d, per_dim, errs)
    assert errs["K"] < 1e-14 and errs["L"] < 1e-10 and errs["Linv"] < 1e-8 and errs["alpha"] < 1e-8
    Kg = engine.get_K(N)
    assert np.array_equal(np.diag(Kg), np.full(N, 1.0 + NOISE)) and np.array_equal(Kg, Kg.T)
    assert np.all(np.triu(engine.get_L(N), 1) == 0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_identical_rows_and_a_candidate_on_a_training_point(engine, kind):
    """Two identical rows (r = 0 off the diagonal) at N = 40 and a candidate equal to a training point: K's diagonal is exactly
    1 + noise, the duplicate's entry exactly 1, nothing is non-finite — the factorisation, the posterior, its input gradient, and the
    LML gradient, where nu = 0.5 takes slope 0 at r = 0 as scikit-learn's K_gradient does."""
    N, d = 40, 3
    X, y, sk, ls = _sk(kind, N, d, False, dup=True)
    ym, ys = _fit(engine, kind, X, y, sk, ls)
    Kg = engine.get_K(N)
    K = sk.kernel_(X)
    K[np.diag_indices_from(K)] += NOISE
    assert np.array_equal(np.diag(Kg), np.full(N, 1.0 + NOISE)) and Kg[5, 2] == 1.0 == Kg[2, 5]
    assert rel_err(Kg, K) < 1e-14
    for a in (Kg, engine.get_L(N), engine.get_Linv(N), engine.get_alpha(N)):
        assert np.all(np.isfinite(a))
    Xc = np.random.RandomState(1).uniform(size=(12, d))
    Xc[0], Xc[1] = X[3], X[2]                   # on a training point; on the duplicated one
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(sd))
    # (identical rows at noise 1e-6: cond(K) ~ 2 / noise, measured 1e7 — outside the 1e2 .. 1e5 of every other case here; two correct
    # factorisations differ by ~cond(K) eps there, so the posterior's bar is 100 cond(K) eps ~ 3e-7 instead of 1e-9)
    tol = 100 * float(np.linalg.cond(K)) * np.finfo(np.float64).eps
    assert 1e-9 < tol < 1e-6
    assert rel_err(mu, mu_s) < tol and rel_err(sd, sd_s) < tol
    g = engine.predict_grad(Xc, 0, ym, ys)
    assert all(np.all(np.isfinite(a)) for a in g)
    yn = (y - ym) / ys
    theta = np.log(np.atleast_1d(ls))
    v_s, g_s = sk.log_marginal_likelihood(theta, eval_gradient=True)
    v, gr = engine.lml(X, yn, kind, ls, NOISE)
    assert np.isfinite(v) and np.all(np.isfinite(gr))
    # (y^T K^-1 y ~ 2e5 here, carried by the near-null direction of the identical rows: the value, too, is known to cond(K) eps only)
    assert abs(v - v_s) <= tol * max(1.0, abs(v_s))
    assert np.max(np.abs(gr - g_s)) <= max(1e-7, tol) * max(np.max(np.abs(g_s)), 1e-12)


# The shapes are chosen so that TODAY's rule (csrc/posterior_plan.h: plan_posterior, small_batch_limit) takes the named path; the rule
# itself is pinned on both sides of every edge by tests/test_posterior_plan_host.py — a retune that moves a shape shows there first.
# path of posterior_plan.h -> (N, d, M): NP = 256 (one row chunk), 448 (two), 832 (four, fp64 slab), 2112 (int8 slab, ragged last chunk)
POST_PATHS = {"small": (200, 6, 5), "fused256": (200, 6, 1000), "fused512": (400, 5, 10000), "slab_f64": (830, 5, 1000),
              "slab_i8": (2050, 16, 300)}


def _posterior_case(kind, path):
    N, d, M = POST_PATHS[path]
    X, y, sk, ls = _sk(kind, N, d, path in ("fused512", "slab_i8"))      # per-dimension length scales on two of the paths
    key = ("post", kind, path)
    if key not in _fits:
        Xc = np.random.RandomState(3).uniform(size=(M, d))
        Xc[min(7, M - 1)] = X[3]                 # a training point: variance ~ noise, the cancellation case
        mu_s, sd_s = sk.predict(Xc, return_std=True)
        for a in (Xc, mu_s, sd_s):
            a.setflags(write=False)
        _fits[key] = (Xc, mu_s, sd_s)
    return (X, y, sk, ls) + _fits[key]


def _assert_posterior(mu, sd, mu_s, sd_s, ys, what):
    errs = (rel_err(mu, mu_s), rel_err(sd, sd_s)) + elementwise_err(sd, sd_s, mu, mu_s, ys)
    print(what, "rel_err mu, sd; elementwise sd, mu:", errs)
    assert errs[0] < 1e-9 and errs[1] < 1e-9 and max(errs[2:]) <= 1e-5, (what, errs)


@pytest.mark.parametrize("path", ["small", "fused256", "fused512", "slab_f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_posterior_paths_against_scikit_learn(engine, kind, path):
    X, y, sk, ls, Xc, mu_s, sd_s = _posterior_case(kind, path)
    ym, ys = _fit(engine, kind, X, y, sk, ls)
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    assert mu.shape == sd.shape == (Xc.shape[0],)
    _assert_posterior(mu, sd, mu_s, sd_s, ys, (kind, path))


@pytest.mark.parametrize("kind", KINDS)
def test_int8_slab_path_against_scikit_learn_and_the_fp64_slab(debug_engine, kind):
    """N = 2050, d = 16 (NP = 2112: nine 256-row chunks, the last one ragged): the default is the int8 GEMM; against scikit-learn at
    the posterior's bars and against the fp64 slab GEMM (GPBO_POST_KERNEL=3, debug build) at the agreement bar of
    test_the_three_large_batch_posterior_kernels_agree: 1e-12 on mu, 1e-11 on sigma."""
    X, y, sk, ls, Xc, mu_s, sd_s = _posterior_case(kind, "slab_i8")
    ym, ys = _fit(debug_engine, kind, X, y, sk, ls)
    debug_engine.set_candidates(Xc)
    out = {}
    for path in (None, "8", "3"):
        if path is not None:
            os.environ["GPBO_POST_KERNEL"] = path
        try:
            out[path] = debug_engine.posterior(0, ym, ys)
        finally:
            os.environ.pop("GPBO_POST_KERNEL", None)
    assert np.array_equal(out[None][0], out["8"][0]) and np.array_equal(out[None][1], out["8"][1]), "the default at NP = 2112 is the int8 GEMM"
    _assert_posterior(*out["8"], mu_s, sd_s, ys, (kind, "slab_i8"))
    _assert_posterior(*out["3"], mu_s, sd_s, ys, (kind, "slab_f64 at NP = 2112"))
    agree = (rel_err(out["8"][0], out["3"][0]), rel_err(out["8"][1], out["3"][1]))
    print(kind, "int8 vs fp64 slab: rel_err mu, sd:", agree)
    assert agree[0] <= 1e-12 and agree[1] <= 1e-11


@pytest.mark.parametrize("N", [200, 600])          # 16x16 MFMAs in 256-row chunks; 32x32 MFMAs in 512-row chunks (NP >= 512)
@pytest.mark.parametrize("kind", KINDS)
def test_f32_mode_within_1e4_of_the_range_with_the_exact_arg_best(engine, kind, N):
    """precision = F32 (fp64 factorisation, fp32 k* slab and GEMM): -UCB within 1e-4 of its range of scikit-learn's, the arg-best
    index exact — scikit-learn's own top-2 gap is asserted to stand more than twice that bound clear, so the index is no coin flip;
    mu keeps fp64 accuracy (1e-7) and the variance the bound of tests/test_gpu_f32.py (2e-5 s_y^2)."""
    d, M, kappa = 5, 3000, 2.576
    X, y, sk, ls = _sk(kind, N, d, False, seed=31)
    Xc = np.random.RandomState(32).uniform(size=(M, d))
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    ref = -(mu_s + kappa * sd_s)
    e = 1e-4 * float(ref.max() - ref.min())
    top = np.sort(ref)[:2]
    assert top[1] - top[0] > 2 * e
    ym, ys = _fit(engine, kind, X, y, sk, ls, precision=E.F32)
    assert rel_err(engine.get_L(N), sk.L_) < 1e-10             # the factorisation is still fp64
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    bi, bv, _, _, vals = engine.acq_argbest(E.UCB, kappa, return_values=True)
    print(kind, N, "f32: max |acq - ref| / range", float(np.max(np.abs(vals - ref))) / (e / 1e-4), "mu", rel_err(mu, mu_s),
          "var", float(np.max(np.abs(sd**2 - sd_s**2))) / ys**2)
    assert np.max(np.abs(vals - ref)) <= e
    assert bi == int(ref.argmin()) and abs(bv - float(ref.min())) <= e
    assert rel_err(mu, mu_s) < 1e-7 and np.max(np.abs(sd**2 - sd_s**2)) < 2e-5 * ys**2


@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "per_dim"])
@pytest.mark.parametrize("N,d", TIERS + [(2050, 4)])        # ... and NP >= 2048: the per-lane-stream path of gpbo_lml_batch
@pytest.mark.parametrize("kind", KINDS)
def test_lml_value_and_gradient_against_scikit_learn(engine, kind, N, d, per_dim):
    """gpbo_lml against log_marginal_likelihood(theta, eval_gradient=True): value 1e-10, gradient 1e-7 of its largest component; the
    value alone is the same value; every lane of gpbo_lml_batch is bitwise gpbo_lml."""
    X, y, sk, ls = _sk(kind, N, d, per_dim)
    yn = (y - sk._y_train_mean) / sk._y_train_std
    v_s, g_s = sk.log_marginal_likelihood(np.log(np.atleast_1d(ls)), eval_gradient=True)
    v, g = engine.lml(X, yn, kind, ls, NOISE)
    print(kind, N, d, per_dim, "lml", abs(v - v_s) / max(1.0, abs(v_s)), "grad", float(np.max(np.abs(g - g_s)) / np.max(np.abs(g_s))))
    assert g.shape == g_s.shape
    assert abs(v - v_s) <= 1e-10 * max(1.0, abs(v_s))
    assert np.max(np.abs(g - g_s)) <= 1e-7 * max(np.max(np.abs(g_s)), 1e-12)
    assert engine.lml(X, yn, kind, ls, NOISE, eval_gradient=False) == v
    scales = np.array([np.atleast_1d(ls), 1.3 * np.atleast_1d(ls), 0.8 * np.atleast_1d(ls)])
    lanes = engine.lml_batch(X, yn, kind, scales, NOISE)
    assert lanes[0][0] == v and np.array_equal(lanes[0][1], g)
    for (val, grad), sc in zip(lanes[1:], scales[1:]):
        v1, g1 = engine.lml(X, yn, kind, sc, NOISE)
        assert np.isfinite(val) and val == v1 and np.array_equal(grad, g1)
    with pytest.raises(_lib.GpboError):
        engine.posterior(0)                      # gpbo_lml leaves the slot unfitted


@pytest.mark.parametrize("kind", KINDS)
def test_fit_append_equals_a_full_fit(engine, kind):
    """Growing N = 100 to 101 (rank-one growth inside the 64-row padding) gives the model a from-scratch fit gives — the bars of
    tests/helpers.assert_same_model at the existing append test's tol = 1e-9 — and the appended K row is bitwise the full fit's."""
    d, n0, tol = 5, 100, 1e-9
    X, y, sk, ls = _sk(kind, n0 + 1, d, False, seed=61)
    yn0, _, _ = O.normalize_targets(y[:n0])
    engine.fit(X[:n0], yn0, kind, ls, NOISE)
    ym, ys = float(sk._y_train_mean), float(sk._y_train_std)
    yn = (y - ym) / ys
    engine.fit_append(X[n0:], yn)
    n = n0 + 1
    K = sk.kernel_(X)
    K[np.diag_indices_from(K)] += NOISE
    Xc = np.random.RandomState(62).uniform(size=(300, d))
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    mu_s, sd_s = sk.predict(Xc, return_std=True)
    errs = {"K": (rel_err(engine.get_K(n), K), 1e-14), "L": (rel_err(engine.get_L(n), sk.L_), tol),
            "WL-I": (rel_err(engine.get_Linv(n) @ sk.L_, np.eye(n)), 100 * tol), "alpha": (rel_err(engine.get_alpha(n), sk.alpha_), 100 * tol),
            "mu": (rel_err(mu, mu_s), tol), "sd": (rel_err(sd, sd_s), tol)}
    print(kind, errs)
    for k, (e, bar) in errs.items():
        assert e < bar, f"{k} {e:.2e} over its bar {bar:.0e}"
    K_inc = engine.get_K(n)
    engine.fit(X, yn, kind, ls, NOISE)
    assert np.array_equal(K_inc, engine.get_K(n))


@pytest.mark.parametrize("kind", KINDS)
def test_predict_cov_against_return_cov(engine, kind):
    """HipGPR(matern_family=True).predict(return_cov=True) at N = 50, M = 20 against scikit-learn's, at the bars of
    test_predict_cov_equals_sklearn_return_cov."""
    from bayesianoptimization_amd.gpr import HipGPR

    N, d, M = 50, 4, 20
    X, y, sk, ls = _sk(kind, N, d, True)
    Xq = np.random.RandomState(6).uniform(size=(M, d))
    mu_s, cov_s = sk.predict(Xq, return_cov=True)
    gp = HipGPR(kernel=F.sk_kernel(kind, ls), alpha=NOISE, normalize_y=True, optimizer=None, engine=engine, matern_family=True).fit(X, y)
    assert not gp._host_mode and gp._kind == kind
    mu, cov = gp.predict(Xq, return_cov=True)
    assert cov.shape == (M, M)
    assert rel_err(mu, mu_s) < 1e-8
    assert np.max(np.abs(cov - cov_s)) < 1e-8 * np.max(np.abs(cov_s))
    assert np.max(np.abs(cov - cov.T)) < 1e-12 * np.max(np.abs(cov_s))
    _, sd = gp.predict(Xq, return_std=True)
    assert np.max(np.abs(np.sqrt(np.clip(np.diag(cov), 0, None)) - sd)) < 1e-6 * np.max(sd)


@pytest.mark.parametrize("N,d,M", [(60, 3, 7), (300, 7, 33)])
@pytest.mark.parametrize("kind", KINDS)
def test_predict_grad_against_the_restated_formulas(engine, kind, N, d, M):
    """gpbo_predict_grad against tests/matern_family_truth.predict_grad (gpbo_kernel_slope's formulas in NumPy) at the bars of
    test_predict_grad_equals_the_oracle_gradient; and ON training points, where nu = 0.5 has a kink and the coincident point
    contributes slope 0 on both sides: d mu / d x at the same bar, d sd / d x finite.  (At r = 0 the slope multiplies a zero
    difference, so what this case can detect is a NON-FINITE slope — 0 * inf = NaN — not a wrong finite one; the value of the
    convention itself is checked where it matters, in the LML gradient of identical rows above.)"""
    X, y, sk, ls = _sk(kind, N, d, d == 7)
    ym, ys = _fit(engine, kind, X, y, sk, ls)
    gp = F.fit_fixed_theta(kind, X, y, ls, NOISE)
    Xq = np.random.RandomState(5).uniform(size=(M, d))
    mu, sd, dmu, dsd = engine.predict_grad(Xq, 0, ym, ys)
    mu_o, sd_o, dmu_o, dsd_o = F.predict_grad(gp, Xq)
    errs = (rel_err(mu, mu_o), rel_err(sd, sd_o), rel_err(dmu, dmu_o), rel_err(dsd, dsd_o))
    print(kind, N, d, "mu, sd, dmu, dsd:", errs)
    assert errs[0] < 1e-8 and errs[1] < 1e-7 and errs[2] < 1e-7 and errs[3] < 1e-6
    mu_s, sd_s = sk.predict(Xq, return_std=True)
    assert rel_err(mu, mu_s) < 1e-8 and rel_err(sd, sd_s) < 1e-7
    on = np.vstack([X[:3], X[N - 1:]])          # r = 0 for one training point each
    mu1, sd1, dmu1, dsd1 = engine.predict_grad(on, 0, ym, ys)
    _, _, dmu1_o, _ = F.predict_grad(gp, on)
    assert np.all(np.isfinite(dmu1)) and np.all(np.isfinite(dsd1)) and np.all(np.isfinite(mu1)) and np.all(np.isfinite(sd1))
    assert rel_err(dmu1, dmu1_o) < 1e-7


# ---- the one-launch searches (csrc/polish_fused.hip, csrc/evolve.hip) --------------------------------------------------------------
@pytest.fixture
def any_size():
    old = os.environ.get("GPBO_POLISH_FUSED_MAX_NP")
    os.environ["GPBO_POLISH_FUSED_MAX_NP"] = "512"
    yield
    if old is None:
        os.environ.pop("GPBO_POLISH_FUSED_MAX_NP", None)
    else:
        os.environ["GPBO_POLISH_FUSED_MAX_NP"] = old


def _polish_eval(eng, acq, param, y_max, ym, ys, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n, d = pts.shape
    out = np.empty((n, 4 + 3 * d))
    eng._check(eng._lib.gpbo_debug_polish_eval(eng._h, int(acq), float(param), float(y_max), float(ym), float(ys), _lib.dptr(pts), n, d, 1,
                                               _lib.dptr(out)))
    return {"f": out[:, 0], "mu": out[:, 1], "sd": out[:, 2], "g": out[:, 4:4 + d], "dmu": out[:, 4 + d:4 + 2 * d],
            "dsd": out[:, 4 + 2 * d:4 + 3 * d]}


SEARCH_SHAPES = [(50, 3), (400, 5)]              # W in LDS (NP = 64); W streamed from memory (NP = 448)


@pytest.mark.parametrize("N,d", SEARCH_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_one_evaluation_is_the_six_kernels_to_rounding(debug_engine, any_size, kind, N, d):
    """The bars of tests/test_gpu_polish_fused.py::test_one_evaluation_is_the_six_kernels_to_rounding (512 eps of the sums' terms),
    with a point ON a training point added: both sides take slope 0 from it."""
    eng = debug_engine
    X, y, sk, ls = _sk(kind, N, d, d % 2 == 1, seed=11 + N + d)
    ym, ys = _fit(eng, kind, X, y, sk, ls)
    rng = np.random.RandomState(5)
    pts = np.vstack([rng.uniform(size=(7, d)), X[:2] + 1e-6, np.full((1, d), 0.5), X[4:5]])
    kappa = 2.576
    got = _polish_eval(eng, O.UCB, kappa, 0.0, ym, ys, pts)
    mu, sd, dmu, dsd = eng.predict_grad(pts, slot=0, y_mean=ym, y_std=ys)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    eps = np.finfo(np.float64).eps
    Kst = F.kernel_matrix(kind, pts, X, np.atleast_1d(ls))
    alpha, Wm = eng.get_alpha(N), eng.get_Linv(N)
    term_mu = ys * (np.abs(Kst) @ np.abs(alpha))
    assert np.all(np.abs(got["mu"] - mu) <= 512 * eps * term_mu + 1e-15)
    V, absV = Kst @ Wm.T, np.abs(Kst) @ np.abs(Wm).T
    term_var = ys * ys * 2.0 * np.sum(np.abs(V) * absV, axis=1)
    assert np.all(np.abs(got["sd"] ** 2 - sd ** 2) <= 512 * eps * term_var + 1e-15 * ys * ys)
    amp_mu = max(1.0, float(np.max(term_mu)) / max(float(np.abs(mu).max()), ys))
    amp_w = max(1.0, float(np.max(term_var)) / (ys * ys))
    print(kind, N, d, "dmu", float(np.max(np.abs(got["dmu"] - dmu))) / (2e-13 * amp_mu * float(np.abs(dmu).max())))
    assert np.max(np.abs(got["dmu"] - dmu)) <= 2e-13 * amp_mu * float(np.abs(dmu).max())
    far = sd > 1e-3 * ys
    if far.any():
        assert np.max(np.abs(got["dsd"][far] - dsd[far])) <= 1e-11 * amp_w * amp_w * float(np.abs(dsd[far]).max())
    assert np.max(np.abs(got["f"] + (got["mu"] + kappa * got["sd"]))) <= 1e-15 * max(float(np.abs(mu).max()), ys)
    assert np.allclose(got["g"], -(got["dmu"] + kappa * got["dsd"]), rtol=1e-14, atol=0)
    mu_s, sd_s = sk.predict(pts, return_std=True)
    assert np.allclose(got["mu"], mu_s, rtol=0, atol=1e-7 * max(1.0, float(np.abs(mu_s).max())))
    assert np.allclose(got["sd"], sd_s, rtol=0, atol=1e-6 * float(sd_s.max()))


@pytest.mark.parametrize("N,d", SEARCH_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_whole_ucb_search_against_the_lockstep_path(debug_engine, any_size, kind, N, d):
    """tests/test_gpu_polish_fused.py's rule, the lockstep path (GPBO_POLISH_FUSED=0: six launches per round, the optimiser on the
    host) as the checker: run by run the same value to 1e-8 in at least 8 of 10 runs, the best run always, no run unconverged that
    converged there, the value returned is the objective at the point returned."""
    eng = debug_engine
    X, y, sk, ls = _sk(kind, N, d, False, seed=100 + N)
    ym, ys = _fit(eng, kind, X, y, sk, ls)
    gp = F.fit_fixed_theta(kind, X, y, ls, NOISE)
    cand = np.random.RandomState(9).uniform(size=(3000, d))
    vals = F.neg_acquisition(gp, cand, O.UCB, 2.576)
    seeds = cand[np.argsort(vals)[:10]].copy()
    seeds[0] = np.clip(seeds[0] + 0.7, -0.5, 1.5)
    seeds[1, 0] = 0.0
    box = np.array([[0.0, 1.0]] * d)
    old = os.environ.get("GPBO_POLISH_FUSED")
    try:
        os.environ["GPBO_POLISH_FUSED"] = "0"
        ref = eng.polish_seeds(O.UCB, 2.576, 0.0, None, None, [ym], [ys], seeds, box)
        os.environ.pop("GPBO_POLISH_FUSED")
        got = eng.polish_seeds(O.UCB, 2.576, 0.0, None, None, [ym], [ys], seeds, box)
        nfev = np.array(eng.last_polish["nfev"])
    finally:
        if old is None:
            os.environ.pop("GPBO_POLISH_FUSED", None)
        else:
            os.environ["GPBO_POLISH_FUSED"] = old
    scale = max(abs(float(ref[1].min())), 1e-12)
    close = np.abs(got[1] - ref[1]) <= 1e-8 * scale
    print(kind, N, d, "runs agreeing:", int(close.sum()), "best", float(got[1].min()), float(ref[1].min()), "status", got[2], ref[2])
    assert close.sum() >= min(8, len(ref[1])), (got[1], ref[1])
    assert float(got[1].min()) <= float(ref[1].min()) + 1e-8 * scale
    assert np.all(got[2][ref[2] < 2] < 2)
    f_at = F.neg_acquisition(gp, got[0], O.UCB, 2.576)
    assert np.all(np.abs(got[1] - f_at) <= 1e-6 * np.abs(f_at) + 1e-9)
    assert got[3] == int(np.max(nfev))
    assert np.all(got[0] >= 0.0) and np.all(got[0] <= 1.0)
    assert np.all(got[1] <= F.neg_acquisition(gp, np.clip(seeds, 0.0, 1.0), O.UCB, 2.576) + 1e-9)


@pytest.mark.parametrize("acq", [E.UCB, E.EI, E.POI])
@pytest.mark.parametrize("kind", KINDS)
def test_evolve_mixed_energies_against_the_host(debug_engine, kind, acq):
    """The energies of the device differential evolution (gpbo_debug_evolve_eval: -acquisition at kernel_transform(x)) at N = 100
    against the host's reference-shaped objective over HipGPR's posterior, at the bar of
    tests/test_gpu_evolve.py::test_device_objective_is_the_host_objective_to_rounding."""
    from scipy.stats import norm

    from bayesianoptimization_amd import fused_acquisition as A
    from bayesianoptimization_amd.float_space import MixedSpace
    from bayesianoptimization_amd.gpr import HipGPR

    N = 100
    sp = MixedSpace({"a": (0.0, 2.0), "n": (-3, 7, int), "b": (1.0, 4.0), "c": ("x", "y", "z"), "e": (5.0, 6.0), "k": (0, 1, int)})
    X = sp.random_sample(N, np.random.RandomState(N + acq))
    y = np.sin(X[:, 0] + 0.3 * X[:, 1]) + 0.1 * X[:, 2] + X[:, 3] - 0.5 * X[:, 5] + 0.2 * X[:, 7]
    sp.register_bulk(X, y)
    gp = HipGPR(kernel=F.sk_kernel(kind, 1.3), alpha=NOISE, normalize_y=True, optimizer=None, engine=debug_engine,
                transform=sp.kernel_transform, matern_family=True).fit(X, y)
    assert not gp._host_mode and gp._kind == kind
    groups = A._mixed_space_groups([gp], sp, np.random.RandomState(0))
    assert groups is not None
    y_max = float(np.max(y))
    fn = {E.UCB: lambda: A.UpperConfidenceBound(kappa=2.576), E.EI: lambda: A.ExpectedImprovement(xi=0.01),
          E.POI: lambda: A.ProbabilityOfImprovement(xi=0.01)}[acq]()
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
    # ... and that posterior is scikit-learn's (the mixed space's transform applied on the host, point by point as the objective does)
    sk = GaussianProcessRegressor(kernel=F.sk_kernel(kind, 1.3), alpha=NOISE, normalize_y=True, optimizer=None).fit(sp.kernel_transform(X), y)
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


# ---- the full acquisition pass against the reference's own run (tests/golden/matern_family.npz) ------------------------------------
@pytest.mark.parametrize("nu,kind", [(0.5, E.MATERN05), (1.5, E.MATERN15)])
def test_full_acquisition_pass_matches_the_reference(engine, nu, kind):
    """d = 3, N = 60, M = 4096 at the theta the reference's own fit found (scripts/gen_matern_family_golden.py): alpha, mu, sigma,
    -UCB and -EI at tests/test_gpu_golden.py's bars (1e-8 max-norm, 1e-5 per candidate), the arg-best index and the top-16 exact."""
    TOL = 1e-8
    g = load_golden("matern_family")
    p = f"nu{'05' if nu == 0.5 else '15'}_"
    X, y, Xc = g["X"], g["y"], g["candidates"]
    yn, ym, ys = O.normalize_targets(y)
    assert ym == g[p + "y_mean"] and ys == g[p + "y_std"]
    engine.fit(X, yn, kind, g[p + "length_scale"], float(g["noise"]))
    assert rel_err(engine.get_alpha(len(y)), g[p + "alpha"]) < TOL
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    assert rel_err(mu, g[p + "mu"]) < TOL and rel_err(sd, g[p + "sd"]) < TOL
    assert max(elementwise_err(sd, g[p + "sd"], mu, g[p + "mu"], ys)) <= 1e-5
    for name, acq, param in (("ucb", E.UCB, float(g["kappa"])), ("ei", E.EI, float(g["xi"]))):
        ref = g[p + "ys_" + name]
        bi, bv, si, sv, vals = engine.acq_argbest(acq, param, float(g[p + "y_max"]), None, None, k_seeds=16, return_values=True)
        print(nu, name, "max |acq - ref| / max |ref|:", float(np.max(np.abs(vals - ref)) / np.max(np.abs(ref))))
        assert np.max(np.abs(vals - ref)) <= TOL * np.max(np.abs(ref))
        assert bi == int(g[p + "argmin_" + name])
        assert np.array_equal(si, g[p + "topk_idx_" + name])
        assert bv == pytest.approx(float(ref.min()), rel=TOL)
        assert np.allclose(sv, g[p + "topk_val_" + name], rtol=TOL, atol=0)
