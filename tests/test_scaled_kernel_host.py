"""CPU: the opt-in scaled kernels  c * k + w  (ConstantKernel * k + WhiteKernel) on the host side.

  * csrc/scaled_kernel.h — the reduction to a unit-amplitude model: eta, the target scale, LML(c, l, w) = U - N/2 log c and the chain
    rule — compiled with the system C++ compiler and fed the UNIT model's quantities from NumPy, against scikit-learn's
    log_marginal_likelihood(theta, eval_gradient=True): 1e-10 on the value, 1e-7 of the gradient's largest component;
  * gpr.describe_scaled_kernel: every accepted form in both operand orders, each hyper-parameter free and fixed, the rejected forms;
  * the flag is off by default and nothing changes then;
  * HipGPR(scaled_kernels=True) over a NumPy engine (tests/scaled_kernel_truth.ScaledFakeEngine): theta layout, RandomState
    consumption equal to scikit-learn's, the gradient handed to L-BFGS-B equal to scikit-learn's to 1e-7;
  * tests/scaled_kernel_truth.py and tests/golden/scaled_kernel.npz against scikit-learn."""
import ctypes
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, DotProduct, Matern, WhiteKernel

import matern_family_truth as F
import scaled_kernel_truth as S
from bayesianoptimization_amd import engine as E
from bayesianoptimization_amd.gpr import HipGPR, describe_kernel, describe_scaled_kernel
from conftest import ROOT, load_golden, rel_err
from oracle.refenv import have_reference, import_reference

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")

SHIM = r"""
#include "scaled_kernel.h"
using namespace gpbo;
extern "C" {
int args_ok(double c, double w) { return scaled_args_ok(c, w); }
double eta(double c, double w, double a) { return scaled_eta(c, w, a); }
double target_scale(double c) { return scaled_target_scale(c); }
double lml(double unit, int64_t N, double c) { return scaled_lml(unit, N, c); }
void gradient(double c, double w, double a, int64_t N, double yta, const double* g_ls, int n_ls, double g_eta, double* grad) {
  scaled_lml_gradient(c, w, a, N, yta, g_ls, n_ls, g_eta, grad);
}
double K_entry(double c, double v) { return scaled_K_entry(c, v); }
double L_entry(double c, double v) { return scaled_L_entry(c, v); }
double alpha_entry(double c, double v) { return scaled_alpha_entry(c, v); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    tmp = str(tmp_path_factory.mktemp("scaled_kernel"))
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libscaled.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC, src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    for name, n in (("eta", 3), ("target_scale", 1), ("K_entry", 2), ("L_entry", 2), ("alpha_entry", 2)):
        getattr(L, name).argtypes = [ctypes.c_double] * n
        getattr(L, name).restype = ctypes.c_double
    L.args_ok.argtypes = [ctypes.c_double, ctypes.c_double]
    L.lml.argtypes = [ctypes.c_double, ctypes.c_int64, ctypes.c_double]
    L.lml.restype = ctypes.c_double
    L.gradient.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_double, dp, ctypes.c_int,
                           ctypes.c_double, dp]
    return L


def _unit_evaluation(X, y_scaled, ls, eta):
    """What the device computes: U, (y'')^T alpha'', U's gradient in log l and g_eta, of the unit model k + eta I on targets y''."""
    n = X.shape[0]
    K = F.kernel_matrix(F.MATERN25, X, None, ls)
    K[np.diag_indices_from(K)] += eta
    L = cholesky(K, lower=True, check_finite=False)
    alpha = cho_solve((L, True), y_scaled, check_finite=False)
    Kinv = cho_solve((L, True), np.eye(n), check_finite=False)
    yta = float(y_scaled @ alpha)
    U = -0.5 * yta - np.log(np.diag(L)).sum() - n / 2 * np.log(2 * np.pi)
    g_ls = 0.5 * np.einsum("ij,ijt->t", np.outer(alpha, alpha) - Kinv, F.kernel_gradient(F.MATERN25, X, ls))
    g_eta = 0.5 * (float(alpha @ alpha) - float(np.trace(Kinv)))
    return U, yta, g_ls, g_eta


@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "per_dim"])
@pytest.mark.parametrize("c,w", S.CASES, ids=S.CASE_IDS)
@pytest.mark.parametrize("N,d", [(40, 3), (200, 6)])
def test_the_header_reduction_gives_scikit_learns_lml_and_gradient(shim, N, d, c, w, per_dim):
    X, y = S.data(N, d)
    ls = np.atleast_1d(S.length_scale(d, per_dim))
    sk = GaussianProcessRegressor(kernel=S.sk_kernel(c, ls if per_dim else float(ls[0]), w), alpha=S.ALPHA, normalize_y=True,
                                  optimizer=None).fit(X, y)
    yn = (y - sk._y_train_mean) / sk._y_train_std
    v_s, g_s = sk.log_marginal_likelihood(sk.kernel_.theta, eval_gradient=True)
    eta = shim.eta(c, w, S.ALPHA)
    U, yta, g_ls, g_eta = _unit_evaluation(X, yn * shim.target_scale(c), ls, eta)
    v = shim.lml(U, N, c)
    grad = np.zeros(ls.shape[0] + 2)
    g_ls = np.ascontiguousarray(g_ls)
    dp = ctypes.POINTER(ctypes.c_double)
    shim.gradient(c, w, S.ALPHA, N, yta, g_ls.ctypes.data_as(dp), ls.shape[0], g_eta, grad.ctypes.data_as(dp))
    n_theta = ls.shape[0] + (2 if w else 1)          # (the w = 0 case has no WhiteKernel, so no log w entry in scikit-learn's theta)
    print(N, d, c, w, "lml", abs(v - v_s) / max(1.0, abs(v_s)), "grad", float(np.max(np.abs(grad[:n_theta] - g_s)) / np.max(np.abs(g_s))))
    assert abs(v - v_s) <= 1e-10 * max(1.0, abs(v_s))
    assert np.max(np.abs(grad[:n_theta] - g_s)) <= 1e-7 * np.max(np.abs(g_s))
    if not w:
        assert grad[-1] == 0.0


def test_the_header_at_unit_amplitude_is_the_identity(shim):
    """c = 1, w = 0: eta is alpha itself, the target scale exactly 1, the LML U itself, K / L / alpha entries unchanged — the bits."""
    assert shim.eta(1.0, 0.0, 1e-6) == 1e-6 and shim.target_scale(1.0) == 1.0
    assert shim.lml(-123.456789, 830, 1.0) == -123.456789
    for v in (0.1, -3.7e-5, 12345.678):
        assert shim.K_entry(1.0, v) == v and shim.L_entry(1.0, v) == v and shim.alpha_entry(1.0, v) == v
    assert shim.K_entry(7.0, 0.5) == 3.5 and shim.L_entry(4.0, 0.5) == 1.0 and shim.alpha_entry(4.0, 2.0) == 0.5


@pytest.mark.parametrize("c,w,ok", [(1.0, 0.0, 1), (0.3, 2.0, 1), (0.0, 0.0, 0), (-1.0, 0.0, 0), (1.0, -1e-9, 0), (np.inf, 0.0, 0),
                                    (1.0, np.inf, 0), (np.nan, 0.0, 0), (1.0, np.nan, 0)])
def test_the_header_argument_rule(shim, c, w, ok):
    assert shim.args_ok(c, w) == ok


# ---- describe_scaled_kernel ---------------------------------------------------------------------------------------------------------
def _m(ls=0.7, fixed=False):
    return Matern(nu=2.5, length_scale=ls, length_scale_bounds="fixed" if fixed else (1e-5, 1e5))


def _c(v=2.5, fixed=False):
    return ConstantKernel(v, "fixed" if fixed else (1e-5, 1e5))


def _w(v=3e-2, fixed=False):
    return WhiteKernel(v, "fixed" if fixed else (1e-5, 1e5))


@pytest.mark.parametrize("fixed", [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                                   (True, True, True)], ids=["all_free", "c_fixed", "l_fixed", "w_fixed", "all_fixed"])
@pytest.mark.parametrize("form", ["k", "C*k", "k*C", "k+W", "W+k", "C*k+W", "W+C*k", "k*C+W", "W+k*C"])
@pytest.mark.parametrize("ls", [0.7, np.array([0.5, 0.9, 1.3])], ids=["scalar", "per_dim"])
def test_every_accepted_form(form, fixed, ls):
    fc, fl, fw = fixed
    m, c, w = _m(ls, fl), _c(2.5, fc), _w(3e-2, fw)
    body = {"k": m, "C*k": c * m, "k*C": m * c}[form.replace("+W", "").replace("W+", "")]
    kernel = body if "W" not in form else (w + body if form.startswith("W+") else body + w)
    sk = describe_scaled_kernel(kernel)
    n_ls = np.atleast_1d(ls).shape[0]
    assert sk.kind == E.MATERN25 and np.array_equal(sk.length_scale, np.atleast_1d(ls))
    assert sk.amplitude == (2.5 if "C" in form else 1.0) and sk.white == (3e-2 if "W" in form else 0.0)
    # theta = log(device[theta_index]) with device = [c, l ..., w]: the map reproduces scikit-learn's theta, entry by entry
    device = np.concatenate([[sk.amplitude], sk.length_scale, [sk.white]])
    assert sk.theta_index.shape == (kernel.n_dims,)
    assert np.allclose(np.log(device[sk.theta_index]), kernel.theta, rtol=1e-15, atol=0)
    want = ([0] if "C" in form and not fc else []), ([] if fl else list(range(1, 1 + n_ls))), ([1 + n_ls] if "W" in form and not fw else [])
    assert sorted(sk.theta_index.tolist()) == want[0] + want[1] + want[2]
    # ... and moving theta moves exactly the described parameter
    if kernel.n_dims:
        theta = kernel.theta + np.linspace(0.1, 0.4, kernel.n_dims)
        sk2 = describe_scaled_kernel(kernel.clone_with_theta(theta))
        device2 = np.concatenate([[sk2.amplitude], sk2.length_scale, [sk2.white]])
        assert np.allclose(np.log(device2[sk2.theta_index]), theta, rtol=1e-14, atol=1e-15)


def test_the_family_flag_and_wrapped_unit_kernels_pass_through():
    assert describe_scaled_kernel(_c() * Matern(nu=1.5) + _w(), matern_family=True).kind == E.MATERN15
    with pytest.raises(NotImplementedError, match="only, got nu=1.5"):
        describe_scaled_kernel(_c() * Matern(nu=1.5) + _w())
    assert describe_scaled_kernel(RBF(0.3) * _c(4.0)).kind == E.RBF


@pytest.mark.parametrize("kernel", [_c() * _c(3.0) * _m(), _c() * (_m() + _w()), _m() + _w() + _w(1e-3), _w() + (_m() + _w()),
                                    _m() + _m(), _w() + _w(), DotProduct(), _c() * DotProduct() + _w(), _m() * _m(), _c(),
                                    ConstantKernel(1.0, "fixed") * (_c() * _m())],
                         ids=["two_constants", "C*(k+W)", "nested_sum_left", "nested_sum_right", "k+k", "W+W", "other", "C*other+W",
                              "k*k", "constant_alone", "unit_constant_times_C*k"])
def test_rejected_forms(kernel):
    with pytest.raises(NotImplementedError, match="HIP path supports"):
        describe_scaled_kernel(kernel)


# ---- the flag is off by default ------------------------------------------------------------------------------------------------------
def test_default_off_nothing_changes():
    assert HipGPR().scaled_kernels is False and HipGPR().get_params()["scaled_kernels"] is False
    for kernel in (ConstantKernel(2.0) * Matern(nu=2.5), Matern(nu=2.5) + WhiteKernel(1e-3)):
        with pytest.raises(NotImplementedError):
            describe_kernel(kernel)
        gp = HipGPR(kernel=kernel, engine=S.ScaledFakeEngine())
        assert gp._unsupported_reason(kernel) is not None
        X, y = S.data(20, 2)
        with pytest.warns(UserWarning, match="scikit-learn"):
            gp.fit(X, y)
        assert gp._host_mode and gp.engine.calls == []
    assert describe_kernel(ConstantKernel(1.0, "fixed") * Matern(nu=2.5, length_scale=0.4))[0] == E.MATERN25
    # a unit kernel under the flag makes the calls it makes without it: no amplitude / white argument anywhere
    X, y = S.data(30, 2)
    eng = S.ScaledFakeEngine()
    gp = HipGPR(kernel=Matern(nu=2.5, length_scale=0.5), alpha=S.ALPHA, normalize_y=True, n_restarts_optimizer=1, engine=eng,
                random_state=np.random.RandomState(0), scaled_kernels=True, theta_lockstep=False).fit(X, y)
    gp.predict(X[:3], return_std=True)
    assert eng.scaled_calls == [] and gp._scale is None


# ---- HipGPR(scaled_kernels=True) over the NumPy engine -------------------------------------------------------------------------------
def _search_pair(N, d, seed, kernel, restarts=2):
    X, y = S.data(N, d, seed)
    sk = GaussianProcessRegressor(kernel=kernel, alpha=S.ALPHA, normalize_y=True, n_restarts_optimizer=restarts,
                                  random_state=np.random.RandomState(seed))
    eng = S.ScaledFakeEngine()
    gp = HipGPR(kernel=kernel, alpha=S.ALPHA, normalize_y=True, n_restarts_optimizer=restarts, engine=eng,
                random_state=np.random.RandomState(seed), scaled_kernels=True)
    return X, y, sk, gp, eng


@pytest.mark.parametrize("kernel", [_c(1.0) * _m(np.ones(2)) + _w(1e-2), _w(1e-2) + _m(1.0) * _c(1.0), _c(1.0) * _m(1.0),
                                    _c(2.0, fixed=True) * _m(1.0) + _w(1e-2)], ids=["C*k+W", "W+k*C", "C*k", "fixedC*k+W"])
def test_the_theta_search_over_the_numpy_engine_is_scikit_learns(kernel):
    X, y, sk, gp, eng = _search_pair(40, 2, 3, kernel)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk.fit(X, y)
        gp.fit(X, y)
    assert not gp._host_mode
    assert sk.random_state.uniform() == gp.random_state.uniform()          # the RandomState went through the same draws
    assert all(c[0] != "lml_batch" for c in eng.calls)                      # restarts one after another: no lanes for a scaled model
    assert [c for c in eng.scaled_calls if c[0] == "lml"], "the search ran through the scaled LML"
    assert abs(gp.log_marginal_likelihood_value_ - sk.log_marginal_likelihood_value_) <= 1e-8 * abs(sk.log_marginal_likelihood_value_)
    assert np.allclose(gp.kernel_.theta, sk.kernel_.theta, rtol=0, atol=1e-4)
    fit_call = [c for c in eng.scaled_calls if c[0] == "fit"][-1]
    d = describe_scaled_kernel(gp.kernel_)
    assert fit_call == ("fit", d.amplitude, d.white)
    Xq = np.random.RandomState(1).uniform(size=(50, 2))
    mu, sd = gp.predict(Xq, return_std=True)
    mu_s, sd_s = sk.predict(Xq, return_std=True)
    assert rel_err(mu, mu_s) < 1e-5 and rel_err(sd, sd_s) < 1e-5
    assert rel_err(gp.L_, sk.L_) < 1e-5 and rel_err(gp.alpha_, sk.alpha_) < 1e-4


@pytest.mark.parametrize("kernel", [_c(0.3) * _m(np.array([0.4, 0.6, 0.5])) + _w(2e-3), _w(5e-2) + _m(0.45) * _c(7.0),
                                    _m(0.45, fixed=True) * _c(7.0) + _w(5e-2)], ids=["C*k+W", "W+k*C", "fixed_l"])
def test_the_gradient_handed_to_lbfgsb_is_scikit_learns(kernel):
    """log_marginal_likelihood(theta, eval_gradient=True) of a fitted HipGPR(scaled_kernels=True) at a theta off the fitted one
    against the same call on scikit-learn's estimator: value 1e-10, gradient 1e-7 of its largest component, in theta's own order."""
    X, y = S.data(60, 3, 5)
    sk = GaussianProcessRegressor(kernel=kernel, alpha=S.ALPHA, normalize_y=True, optimizer=None).fit(X, y)
    gp = HipGPR(kernel=kernel, alpha=S.ALPHA, normalize_y=True, optimizer=None, engine=S.ScaledFakeEngine(), scaled_kernels=True).fit(X, y)
    theta = sk.kernel_.theta + np.linspace(-0.3, 0.2, sk.kernel_.n_dims)
    v_s, g_s = sk.log_marginal_likelihood(theta, eval_gradient=True)
    v, g = gp.log_marginal_likelihood(theta, eval_gradient=True)
    assert g.shape == g_s.shape
    assert abs(v - v_s) <= 1e-10 * max(1.0, abs(v_s)) and np.max(np.abs(g - g_s)) <= 1e-7 * np.max(np.abs(g_s))
    assert gp.log_marginal_likelihood(theta) == v
    mu, sd = gp.predict(X[:5] + 0.01, return_std=True)                      # the fit was restored after the evaluation
    mu_s, sd_s = sk.predict(X[:5] + 0.01, return_std=True)
    assert rel_err(mu, mu_s) < 1e-9 and rel_err(sd, sd_s) < 1e-9


def test_appends_keep_the_scale_and_a_changed_scale_refits():
    X, y = S.data(31, 2, 7)
    eng = S.ScaledFakeEngine()
    kernel = _c(2.0) * _m(0.5) + _w(1e-2)
    gp = HipGPR(kernel=kernel, alpha=S.ALPHA, normalize_y=True, optimizer=None, engine=eng, scaled_kernels=True)
    gp.fit(X[:30], y[:30])
    gp.fit(X, y)
    assert [c[0] for c in eng.scaled_calls] == ["fit", "fit_append"] and eng.scaled_calls[1][1:] == (2.0, 1e-2)
    sk = GaussianProcessRegressor(kernel=kernel, alpha=S.ALPHA, normalize_y=True, optimizer=None).fit(X, y)
    assert rel_err(gp.predict(X[:4] + 0.02), sk.predict(X[:4] + 0.02)) < 1e-9
    gp.set_params(kernel=_c(3.0) * _m(0.5) + _w(1e-2))
    gp.fit(X, y)                                                            # another c: the append key differs
    assert eng.scaled_calls[-1] == ("fit", 3.0, 1e-2)


def test_a_device_group_keeps_scaled_kernels_on_the_host():
    class Group(E.GroupEngine):
        def __init__(self):             # (no devices: only the type matters to the rule)
            pass

        def close(self):
            pass

    gp = HipGPR(kernel=_c() * _m() + _w(), engine=Group(), scaled_kernels=True)
    assert "device group" in gp._unsupported_reason(gp.kernel)
    assert gp._unsupported_reason(_m()) is None
    with pytest.raises(NotImplementedError, match="device group"):
        E.GroupEngine.fit(gp.engine, np.zeros((2, 1)), np.zeros(2), 1, 1.0, 1e-6, amplitude=2.0)
    with pytest.raises(NotImplementedError, match="device group"):
        E.GroupEngine.lml(gp.engine, np.zeros((2, 1)), np.zeros(2), 1, 1.0, 1e-6, scaled=True)


@pytest.mark.skipif(not have_reference(), reason="bayes_opt (the reference) is not importable here")
def test_accelerated_optimizer_runs_a_scaled_kernel_on_the_engine():
    """A real bayes_opt optimizer, accelerate(..., scaled_kernels=True) and set_gp_params(kernel=C * Matern(2.5) + WhiteKernel()) —
    what the reference wraps into a dynamic subclass of Sum: maximize() runs with no host warning, the model stays on the engine and
    its fits carry the fitted c and w; the same optimizer without the flag degrades, as before."""
    from sklearn.base import clone

    import_reference()
    from bayes_opt import BayesianOptimization

    from bayesianoptimization_amd import accelerate

    def black_box(x, y):
        return -(x**2) - (y - 1) ** 2 + 1

    pb = {"x": (2, 4), "y": (-3, 3)}
    kernel = ConstantKernel() * Matern(nu=2.5) + WhiteKernel()
    mine = BayesianOptimization(f=black_box, pbounds=pb, random_state=11, verbose=0)
    eng = S.ScaledFakeEngine()
    accelerate(mine, engine=eng, scaled_kernels=True)
    assert mine._gp.scaled_kernels is True and clone(mine._gp).scaled_kernels is True
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        mine.set_gp_params(kernel=kernel, n_restarts_optimizer=2)
        mine.maximize(init_points=3, n_iter=3)
    assert not [w for w in seen if "HIP path" in str(w.message) or "on the host" in str(w.message)], [str(w.message) for w in seen]
    assert not mine._gp._host_mode and len(mine.space) == 6
    sk = describe_scaled_kernel(mine._gp.kernel_)
    assert mine._gp._scale == (sk.amplitude, sk.white)
    assert [c for c in eng.scaled_calls if c[0] == "fit"][-1] == ("fit", sk.amplitude, sk.white)
    assert {"fit", "lml", "posterior"} <= {c for c, _ in eng.kinds} and "lml_batch" not in {c for c, _ in eng.kinds}
    plain = BayesianOptimization(f=black_box, pbounds=pb, random_state=11, verbose=0)
    eng2 = S.ScaledFakeEngine()
    accelerate(plain, engine=eng2)
    with pytest.warns(UserWarning, match="HIP path supports"):
        plain.set_gp_params(kernel=kernel)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain.maximize(init_points=2, n_iter=1)
    assert plain._gp._host_mode and not eng2.kinds


def test_gpengine_runs_a_scaled_fit_synchronously_inside_overlapped_fits():
    """GpEngine.fit's own rule, over a library stand-in that records the entry points called: inside overlapped_fits() a unit
    model's fit is gpbo_fit_begin (waited for when the block ends), a scaled model's is gpbo_fit_scaled, at once, and a pending fit of
    the same slot is waited for first."""
    log = []

    class Lib:
        def __getattr__(self, name):
            def call(*args):
                log.append((name, args[1]) if name.startswith("gpbo_fit") else (name,))
                return 0
            return call

    eng = object.__new__(E.GpEngine)
    eng._lib, eng._h = Lib(), None
    eng._init_state()
    X, y = S.data(8, 2)
    with eng.overlapped_fits():
        eng.fit(X, y, E.MATERN25, 1.0, S.ALPHA, slot=1)
        eng.fit(X, y, E.MATERN25, 1.0, S.ALPHA, slot=0, amplitude=2.0, white=1e-2)
        assert log == [("gpbo_fit_begin", 1), ("gpbo_fit_scaled", 0)] and eng._pending_fits == {1} and eng._scaled == {0: (2.0, 1e-2)}
        eng.fit(X, y, E.MATERN25, 1.0, S.ALPHA, slot=1, amplitude=3.0)          # the slot's pending unit fit is settled first
        assert log[2:] == [("gpbo_fit_wait", 1), ("gpbo_fit_scaled", 1)] and not eng._pending_fits
        eng.fit(X, y, E.MATERN25, 1.0, S.ALPHA, slot=0)                          # a unit model again: enqueued, no longer scaled
        assert 0 not in eng._scaled
    assert log[4:] == [("gpbo_fit_begin", 0), ("gpbo_fit_wait", 0)]
    eng._lib = None                                                              # (nothing to close)


@pytest.mark.skipif(not have_reference(), reason="bayes_opt (the reference) is not importable here")
def test_constrained_accelerated_optimizer_fits_scaled_models_inside_the_overlap_block():
    """With a constraint, suggest() fits the target GP and the constraint GP inside engine.overlapped_fits(): a scaled kernel on
    either must fit there (synchronously) and not raise — the target scaled and the constraint GP a unit model, then both scaled."""
    import_reference()
    from bayes_opt import BayesianOptimization
    from scipy.optimize import NonlinearConstraint

    from bayesianoptimization_amd import accelerate

    cons = NonlinearConstraint(lambda x, y: np.cos(x) * np.cos(y) - np.sin(x) * np.sin(y), -np.inf, 0.5)
    scaled = ConstantKernel(2.0, "fixed") * Matern(nu=2.5, length_scale=1.0) + WhiteKernel(1e-2, "fixed")
    for scale_the_constraint in (False, True):
        mine = BayesianOptimization(f=lambda x, y: -(x**2) - (y - 1) ** 2 + 1, pbounds={"x": (2, 4), "y": (-3, 3)}, random_state=7,
                                    verbose=0, constraint=cons)
        mine.set_gp_params(kernel=scaled)
        if scale_the_constraint:
            for m in mine._space.constraint._model:
                m.set_params(kernel=ConstantKernel(0.5) * Matern(nu=2.5) + WhiteKernel(1e-3))
        eng = S.ScaledFakeEngine()
        with warnings.catch_warnings():
            warnings.simplefilter("error")              # accelerate() notes no unsupported kernel
            accelerate(mine, engine=eng, scaled_kernels=True)
        cm = mine._space.constraint._model
        assert cm[0].scaled_kernels is True and cm[0].slot == 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mine.maximize(init_points=4, n_iter=0)
            mine._acquisition_function.suggest(mine._gp, mine._space, n_random=1500, n_smart=0, random_state=mine._random_state)
        assert not mine._gp._host_mode and not cm[0]._host_mode
        assert mine._gp._scale == (2.0, 1e-2) and (cm[0]._scale is not None) == scale_the_constraint
        assert (0, "synchronous") in eng.overlap_log, eng.overlap_log
        assert (1, "synchronous" if scale_the_constraint else "enqueued") in eng.overlap_log, eng.overlap_log
        assert ("posterior", 0) in eng.calls and ("posterior", 1) in eng.calls


# ---- the truth module and the golden against scikit-learn -----------------------------------------------------------------------------
@pytest.mark.parametrize("c,w", S.CASES, ids=S.CASE_IDS)
def test_the_truth_module_is_scikit_learn(c, w):
    N, d = 60, 3
    X, y = S.data(N, d)
    ls = S.length_scale(d, True)
    sk = GaussianProcessRegressor(kernel=S.sk_kernel(c, ls, w), alpha=S.ALPHA, normalize_y=True, optimizer=None).fit(X, y)
    gp = S.fit(F.MATERN25, X, y, ls, c, w)
    assert rel_err(gp.L, sk.L_) < 1e-12 and rel_err(gp.alpha, sk.alpha_) < 1e-10
    Xq = np.random.RandomState(2).uniform(size=(25, d))
    Xq[3] = X[4]
    mu_s, sd_s = sk.predict(Xq, return_std=True)
    mu, sd = S.predict(gp, Xq)
    assert rel_err(mu, mu_s) < 1e-10 and rel_err(sd, sd_s) < 1e-9
    _, cov_s = sk.predict(Xq, return_cov=True)
    assert rel_err(S.predict_cov(gp, Xq)[1], cov_s) < 1e-9
    yn = (y - sk._y_train_mean) / sk._y_train_std
    v_s, g_s = sk.log_marginal_likelihood(sk.kernel_.theta, eval_gradient=True)
    v, g = S.log_marginal_likelihood(F.MATERN25, X, yn, ls, c, w)
    assert abs(v - v_s) <= 1e-10 * abs(v_s) and np.max(np.abs(g[:g_s.shape[0]] - g_s)) <= 1e-9 * np.max(np.abs(g_s))
    # the input gradient against central differences of the truth's own posterior (step 1e-6: error ~1e-12 / 1e-6 + 1e-12)
    _, _, dmu, dsd = S.predict_grad(gp, Xq[:3])
    for t in range(d):
        e = np.zeros(d)
        e[t] = 1e-6
        mp, sp = S.predict(gp, Xq[:3] + e)
        mm, sm = S.predict(gp, Xq[:3] - e)
        assert np.allclose((mp - mm) / 2e-6, dmu[:, t], rtol=1e-5, atol=1e-6) and np.allclose((sp - sm) / 2e-6, dsd[:, t], rtol=1e-5, atol=1e-6)


def test_the_golden_is_scikit_learns_model_at_the_stored_theta():
    g = load_golden("scaled_kernel")
    X, y, Xc = g["X"], g["y"], g["candidates"]
    c, w, ls, a = float(g["constant_value"]), float(g["noise_level"]), g["length_scale"], float(g["alpha_estimator"])
    assert X.shape == (60, 3) and Xc.shape == (4096, 3) and c > 0 and w > 0 and a == 1e-6
    kernel = ConstantKernel(c) * Matern(nu=2.5, length_scale=ls) + WhiteKernel(w)
    assert np.allclose(kernel.theta, g["theta"], rtol=1e-14, atol=0)
    sk = GaussianProcessRegressor(kernel=kernel, alpha=a, normalize_y=True, optimizer=None).fit(X, y)
    assert sk._y_train_mean == g["y_mean"] and sk._y_train_std == g["y_std"]
    mu, sd = sk.predict(Xc, return_std=True)
    assert rel_err(sk.alpha_, g["alpha"]) < 1e-9 and rel_err(mu, g["mu"]) < 1e-10 and rel_err(sd, g["sd"]) < 1e-10
    ucb = -(mu + float(g["kappa"]) * sd)
    assert rel_err(ucb, g["ys_ucb"]) < 1e-10 and int(ucb.argmin()) == int(g["argmin_ucb"])
    assert np.array_equal(np.argsort(g["ys_ucb"])[:16], g["topk_idx_ucb"]) and np.array_equal(np.argsort(g["ys_ei"])[:16], g["topk_idx_ei"])
    # the top-2 gaps stand clear of the device test's tolerance (1e-8 of the largest value), so its exact arg-best is no coin flip
    for name in ("ucb", "ei"):
        v = g["topk_val_" + name]
        assert np.min(np.diff(v)) > 1e-6 * np.max(np.abs(g["ys_" + name]))
