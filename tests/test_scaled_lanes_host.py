"""CPU: the opt-in lockstep theta search of scaled models (`scaled_lanes=True` on top of `scaled_kernels=True`) on the host side.

  * HipGPR over a NumPy engine with a batched scaled call (LaneFakeEngine below, on tests/scaled_kernel_truth.ScaledFakeEngine): the
    search of C*k + W, k*C and C*k goes through the batched call and never the single one, the RandomState ends where
    scikit-learn's does, theta and the LML value EQUAL the sequential path's over the same engine and lie within the existing scaled
    host test's bars of scikit-learn's;
  * `scaled_lanes=False` makes the calls it makes today;
  * the theta row -> (c, l, w) map and the gradient pick for every accepted form, each hyper-parameter free and fixed;
  * accelerate(scaled_lanes=True) without scaled_kernels raises; clone / get_params / from_sklearn carry the flag; GroupEngine refuses."""
import warnings

import numpy as np
import pytest
from sklearn.base import clone
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

import scaled_kernel_truth as S
from bayesianoptimization_amd import engine as E
from bayesianoptimization_amd.gpr import HipGPR, describe_scaled_kernel
from oracle.refenv import have_reference, import_reference


class LaneFakeEngine(S.ScaledFakeEngine):
    """ScaledFakeEngine + GpEngine.lml_batch_scaled_arrays: every row is the single scaled evaluation of the same arguments (the same
    function, so the same bits).  `batches` records (n_rows, reuse_inputs) per call, `rows` the parameters of every row."""

    def __init__(self):
        super().__init__()
        self.batches, self.rows = [], []

    def lml_batch_scaled_arrays(self, X, y_norm, kernel, length_scales, amplitudes, whites, noise, eval_gradient=True, reuse_inputs=False):
        ls = np.atleast_2d(np.asarray(length_scales, dtype=np.float64))
        n, n_ls = ls.shape
        assert 1 <= n <= 8 and len(amplitudes) == n and len(whites) == n
        self.batches.append((n, bool(reuse_inputs)))
        self.calls.append(("lml_batch_scaled", n))
        self.kinds.append(("lml_batch_scaled", int(kernel)))
        vals, grads = np.zeros(n), np.zeros((n, n_ls + 2))
        for i in range(n):
            self.rows.append((float(amplitudes[i]), ls[i].copy(), float(whites[i])))
            vals[i], grads[i] = S.log_marginal_likelihood(kernel, X, y_norm, ls[i], float(amplitudes[i]), float(whites[i]), noise, True)
        return vals, grads


def _m(ls=0.7, fixed=False):
    return Matern(nu=2.5, length_scale=ls, length_scale_bounds="fixed" if fixed else (1e-5, 1e5))


def _c(v=2.5, fixed=False):
    return ConstantKernel(v, "fixed" if fixed else (1e-5, 1e5))


def _w(v=3e-2, fixed=False):
    return WhiteKernel(v, "fixed" if fixed else (1e-5, 1e5))


def _gp(kernel, eng, seed, lanes, restarts=2):
    return HipGPR(kernel=kernel, alpha=S.ALPHA, normalize_y=True, n_restarts_optimizer=restarts, engine=eng,
                  random_state=np.random.RandomState(seed), scaled_kernels=True, scaled_lanes=lanes)


SEARCH_KERNELS = [_c(1.0) * _m(np.ones(2)) + _w(1e-2), _w(1e-2) + _m(1.0) * _c(1.0), _c(1.0) * _m(1.0), _m(np.ones(2)) * _c(1.0),
                  _c(2.0, fixed=True) * _m(1.0) + _w(1e-2), _c(2.0, fixed=True) * _m(np.ones(2)) + _w(1e-2)]
SEARCH_IDS = ["C*k+W_per_dim", "W+k*C", "C*k", "k*C_per_dim", "fixedC*k+W", "fixedC*k+W_per_dim"]


@pytest.mark.parametrize("kernel", SEARCH_KERNELS, ids=SEARCH_IDS)
def test_the_search_runs_through_the_batched_scaled_call(kernel):
    X, y = S.data(40, 2, 3)
    sk = GaussianProcessRegressor(kernel=kernel, alpha=S.ALPHA, normalize_y=True, n_restarts_optimizer=2, random_state=np.random.RandomState(3))
    eng, eng_seq = LaneFakeEngine(), LaneFakeEngine()
    gp, seq = _gp(kernel, eng, 3, True), _gp(kernel, eng_seq, 3, False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk.fit(X, y)
        gp.fit(X, y)
        seq.fit(X, y)
    assert not gp._host_mode
    # the batched call and never the single one; inputs uploaded by the first round only
    assert eng.batches and not [c for c in eng.calls if c[0] == "lml"]
    assert eng.batches[0] == (3, False) and all(reuse for _, reuse in eng.batches[1:])
    assert gp.theta_search_rounds_ == len(eng.batches) < gp.theta_search_evals_ == sum(n for n, _ in eng.batches)
    # ... scaled_lanes=False: today's calls
    assert not eng_seq.batches and [c for c in eng_seq.scaled_calls if c[0] == "lml"]
    assert all(c[0] not in ("lml_batch", "lml_batch_scaled") for c in eng_seq.calls)
    # the RandomState went through the same draws
    u = sk.random_state.uniform()
    assert gp.random_state.uniform() == u and seq.random_state.uniform() == u
    # the sequential path's theta and value, exactly: every lane returns the single evaluation's bits, the driver is SciPy's
    assert np.array_equal(gp.kernel_.theta, seq.kernel_.theta)
    assert gp.log_marginal_likelihood_value_ == seq.log_marginal_likelihood_value_
    assert gp.theta_search_evals_ == len([c for c in eng_seq.scaled_calls if c[0] == "lml"])
    # scikit-learn's, at the bars of tests/test_scaled_kernel_host.py
    assert abs(gp.log_marginal_likelihood_value_ - sk.log_marginal_likelihood_value_) <= 1e-8 * abs(sk.log_marginal_likelihood_value_)
    assert np.allclose(gp.kernel_.theta, sk.kernel_.theta, rtol=0, atol=1e-4)
    d = describe_scaled_kernel(gp.kernel_)
    assert [c for c in eng.scaled_calls if c[0] == "fit"][-1] == ("fit", d.amplitude, d.white)


def test_a_single_start_and_a_custom_optimizer_keep_the_sequential_path():
    X, y = S.data(30, 2, 5)
    kernel = _c(1.0) * _m(1.0) + _w(1e-2)
    eng = LaneFakeEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _gp(kernel, eng, 5, True, restarts=0).fit(X, y)
    assert not eng.batches and [c for c in eng.scaled_calls if c[0] == "lml"]

    def custom(obj_func, initial_theta, bounds):
        return initial_theta, obj_func(initial_theta, eval_gradient=False)

    eng = LaneFakeEngine()
    gp = _gp(kernel, eng, 5, True)
    gp.optimizer = custom
    gp.fit(X, y)
    assert not eng.batches and len([c for c in eng.scaled_calls if c[0] == "lml"]) == 3


FORMS = {"C*k": lambda c, k, w: c * k, "k*C": lambda c, k, w: k * c, "C*k+W": lambda c, k, w: c * k + w, "W+C*k": lambda c, k, w: w + c * k,
         "k*C+W": lambda c, k, w: k * c + w, "W+k*C": lambda c, k, w: w + k * c, "k+W": lambda c, k, w: k + w, "W+k": lambda c, k, w: w + k}


@pytest.mark.parametrize("fixed", [(False, False, False), (True, False, False), (False, True, False), (False, False, True)],
                         ids=["free", "fixed_c", "fixed_l", "fixed_w"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("ls", [0.45, np.array([0.4, 0.6, 0.5])], ids=["scalar", "per_dim"])
def test_the_theta_row_map_and_the_gradient_pick(form, fixed, ls):
    """A lockstep round's rows at thetas off the kernel's own: the engine receives scikit-learn's reading of each theta (fixed
    hyper-parameters from the kernel), and the rows handed to L-BFGS-B are scikit-learn's value (1e-10) and gradient (1e-7 of its
    largest component) in theta's own order."""
    kernel = FORMS[form](_c(0.8, fixed[0]), _m(ls, fixed[1]), _w(2e-2, fixed[2]))
    X, y = S.data(30, 3, 9)
    sk = GaussianProcessRegressor(kernel=kernel, alpha=S.ALPHA, normalize_y=True, optimizer=None).fit(X, y)
    eng = LaneFakeEngine()
    gp = HipGPR(kernel=kernel, alpha=S.ALPHA, normalize_y=True, optimizer=None, engine=eng, scaled_kernels=True, scaled_lanes=True).fit(X, y)
    desc = describe_scaled_kernel(gp.kernel_)
    evaluate = gp._scaled_lane_rounds(eng, desc, gp._tx(gp.X_train_), gp.y_train_, S.ALPHA, [gp.kernel_.theta])
    thetas = [gp.kernel_.theta + s * np.linspace(-0.3, 0.2, kernel.n_dims) for s in (1.0, -0.7, 0.4)]
    rows = evaluate(thetas)
    assert rows.shape == (3, 1 + kernel.n_dims) and eng.batches == [(3, False)]
    for theta, row, (c, l, w) in zip(thetas, rows, eng.rows):
        want = describe_scaled_kernel(kernel.clone_with_theta(theta))
        assert np.allclose([c, w], [want.amplitude, want.white], rtol=1e-14, atol=0) and np.allclose(l, want.length_scale, rtol=1e-14, atol=0)
        if fixed[0] or "C" not in form:
            assert c == desc.amplitude
        if fixed[1]:
            assert np.array_equal(l, desc.length_scale)
        if fixed[2] or "W" not in form:
            assert w == desc.white
        v_s, g_s = sk.log_marginal_likelihood(theta, eval_gradient=True)
        assert abs(row[0] - v_s) <= 1e-10 * max(1.0, abs(v_s)) and np.max(np.abs(row[1:] - g_s)) <= 1e-7 * np.max(np.abs(g_s))


def test_the_flag_is_a_real_parameter():
    assert HipGPR().scaled_lanes is False and HipGPR().get_params()["scaled_lanes"] is False
    gp = HipGPR(kernel=_c() * _m() + _w(), scaled_kernels=True, scaled_lanes=True, engine=LaneFakeEngine())
    assert gp.get_params()["scaled_lanes"] is True and clone(gp).scaled_lanes is True and clone(gp).scaled_kernels is True
    sk = GaussianProcessRegressor(kernel=_c() * _m())
    assert HipGPR.from_sklearn(sk, engine=gp.engine, scaled_kernels=True, scaled_lanes=True).scaled_lanes is True
    assert HipGPR.from_sklearn(sk, engine=gp.engine, scaled_kernels=True).scaled_lanes is False


def test_scaled_lanes_alone_does_not_admit_a_scaled_model():
    X, y = S.data(20, 2)
    gp = HipGPR(kernel=_c() * _m() + _w(), engine=LaneFakeEngine(), scaled_lanes=True, n_restarts_optimizer=1)
    with pytest.warns(UserWarning, match="scikit-learn"):
        gp.fit(X, y)
    assert gp._host_mode and gp.engine.calls == []


def test_a_device_group_refuses_the_batched_scaled_call():
    class Group(E.GroupEngine):
        def __init__(self):             # (no devices: only the type matters to the rule)
            pass

        def close(self):
            pass

    g = Group()
    with pytest.raises(NotImplementedError, match="device group"):
        g.lml_batch_scaled_arrays(np.zeros((2, 1)), np.zeros(2), 1, np.ones((1, 1)), np.ones(1), np.zeros(1), 1e-6)
    with pytest.raises(NotImplementedError, match="device group"):
        g.lml_search_rounds_scaled(np.zeros((2, 1)), np.zeros(2), 1, 1, 1e-6)
    gp = HipGPR(kernel=_c() * _m() + _w(), engine=g, scaled_kernels=True, scaled_lanes=True)
    assert "device group" in gp._unsupported_reason(gp.kernel)      # the model stays on the host, as without the flag


class _Optimizer:
    """What accelerate() reads before it swaps anything."""
    _space = None


def test_accelerate_refuses_scaled_lanes_without_scaled_kernels():
    from bayesianoptimization_amd import accelerate

    with pytest.raises(ValueError, match="scaled_kernels"):
        accelerate(_Optimizer(), engine=LaneFakeEngine(), scaled_lanes=True)


@pytest.mark.skipif(not have_reference(), reason="bayes_opt (the reference) is not importable here")
def test_accelerate_hands_the_flag_to_the_target_and_every_constraint_model():
    import_reference()
    from bayes_opt import BayesianOptimization
    from scipy.optimize import NonlinearConstraint

    from bayesianoptimization_amd import accelerate

    def black_box(x, y):
        return -(x**2) - (y - 1) ** 2 + 1

    pb = {"x": (2, 4), "y": (-3, 3)}
    kernel = ConstantKernel() * Matern(nu=2.5) + WhiteKernel()
    con = NonlinearConstraint(lambda x, y: x + y, -np.inf, 4.0)
    mine = BayesianOptimization(f=black_box, pbounds=pb, constraint=con, random_state=11, verbose=0)
    eng = LaneFakeEngine()
    accelerate(mine, engine=eng, scaled_kernels=True, scaled_lanes=True)
    models = [mine._gp, *mine._space._constraint._model]
    assert len(models) == 2 and all(m.scaled_kernels is True and m.scaled_lanes is True for m in models)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        mine.set_gp_params(kernel=kernel, n_restarts_optimizer=2)
        for m in models[1:]:
            m.set_params(kernel=ConstantKernel(0.5) * Matern(nu=2.5) + WhiteKernel(1e-3), n_restarts_optimizer=2)
        mine.maximize(init_points=6, n_iter=0)
        mine._acquisition_function.suggest(mine._gp, mine._space, n_random=1500, n_smart=0, random_state=mine._random_state)
    assert not [w for w in seen if "HIP path" in str(w.message) or "on the host" in str(w.message)], [str(w.message) for w in seen]
    assert not any(m._host_mode for m in models) and all(m.theta_search_rounds_ < m.theta_search_evals_ for m in models)
    assert len(eng.batches) == sum(m.theta_search_rounds_ for m in models) and not [c for c in eng.calls if c[0] == "lml"]
    plain = BayesianOptimization(f=black_box, pbounds=pb, random_state=11, verbose=0)
    accelerate(plain, engine=LaneFakeEngine(), scaled_kernels=True)
    assert plain._gp.scaled_lanes is False
