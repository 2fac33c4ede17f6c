"""GPU (-m gpu): the posterior GEMM on int8 matrix cores (posterior_i8.hip), the default for fp64 models on the k* slab
route from NP = 2048 on, against the fp64 slab GEMM it replaces (GPBO_POST_KERNEL=3, debug build) and the oracle:

  * C3 size (N = 4096, d = 16, M = 2^20): mu bitwise equal (k* . alpha is the same fp64 code), sigma within 1e-12 of s_y,
    UCB and EI arg-best and top-16 identical, acquisition values within 1e-12 of their range;
  * ill-conditioned RBF, d = 2, N = 4000, candidates within 1e-4 of training points (sigma -> sqrt(noise), the cancellation
    1 - sum v^2): elementwise 1e-5 against the oracle, as tests/test_gpu_conditioning.py asserts;
  * the int8 route depends on no batch size: 3 000 candidates give the bits of the same candidates in a 2^18 batch."""
import os

import numpy as np
import pytest

from bayesianoptimization_amd import workloads as W
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


def _posterior(engine, path, ym, ys):
    if path is None:
        os.environ.pop("GPBO_POST_KERNEL", None)
    else:
        os.environ["GPBO_POST_KERNEL"] = path
    try:
        return engine.posterior(0, ym, ys)
    finally:
        os.environ.pop("GPBO_POST_KERNEL", None)


def _acq(engine, acq, param, y_max, path, ym, ys):
    _posterior(engine, path, ym, ys)
    bi, bv, si, sv, vals = engine.acq_argbest(acq, param, y_max, k_seeds=16, return_values=True)
    return bi, np.asarray(si), np.asarray(vals)


def test_c3_int8_gemm_matches_the_fp64_gemm(debug_engine):
    w = W.C3
    X, y, _ = W.make_observations(w)
    Xc = W.make_candidates(w.bounds_array(), w.M, 7)
    yn, ym, ys = O.normalize_targets(y)
    debug_engine.fit(X, yn, w.kernel, w.length_scale, w.noise)
    debug_engine.set_candidates(Xc)
    mu8, sd8 = _posterior(debug_engine, "8", ym, ys)
    mu0, sd0 = _posterior(debug_engine, None, ym, ys)
    mu3, sd3 = _posterior(debug_engine, "3", ym, ys)
    assert np.array_equal(mu0, mu8) and np.array_equal(sd0, sd8), "the default at NP = 4096 is the int8 GEMM"
    assert np.array_equal(mu8, mu3), "mu does not go through the GEMM: bitwise the fp64 path's"
    d_sd = float(np.max(np.abs(sd8 - sd3)) / ys)
    assert d_sd <= 1e-12, d_sd
    y_max = float(y.max())
    for acq, param, name in ((O.UCB, 2.576, "ucb"), (O.EI, 0.01, "ei")):
        b8, s8, v8 = _acq(debug_engine, acq, param, y_max, None, ym, ys)
        b3, s3, v3 = _acq(debug_engine, acq, param, y_max, "3", ym, ys)
        rng = float(np.max(v3) - np.min(v3))
        assert b8 == b3 and np.array_equal(s8, s3), name
        assert np.max(np.abs(v8 - v3)) <= 1e-12 * rng, name


def test_ill_conditioned_rbf_n4000_elementwise(engine):
    rng = np.random.RandomState(41)
    N, M, n_near, ls = 4000, 4001, 200, 0.5
    X = rng.uniform(size=(N, 2))
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    Xc = rng.uniform(size=(M, 2))
    Xc[:n_near] = np.clip(X[:n_near] + 1e-4 * rng.standard_normal((n_near, 2)), 0.0, 1.0)
    gp = O.fit_fixed_theta(O.RBF, X, y, ls, 1e-6)
    mu_o, sd_o = O.predict(gp, Xc)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, O.RBF, ls, 1e-6)
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    pos = sd_o > 0
    e_sd = float(np.max(np.abs(sd - sd_o)[pos] / sd_o[pos]))
    e_mu = float(np.max(np.abs(mu - mu_o) / np.maximum(np.abs(mu_o), ys)))
    assert e_sd <= 1e-5 and e_mu <= 1e-5, (e_sd, e_mu)


def test_int8_route_does_not_depend_on_the_batch(engine):
    w = W.C3
    X, y, _ = W.make_observations(w)
    Xc = W.make_candidates(w.bounds_array(), 1 << 18, 8)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, w.kernel, w.length_scale, w.noise)
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    sub = np.random.RandomState(3).permutation(Xc.shape[0])[:3000]
    engine.set_candidates(Xc[sub])
    mu_s, sd_s = engine.posterior(0, ym, ys)
    assert np.array_equal(mu_s, mu[sub]) and np.array_equal(sd_s, sd[sub])
    mu2, sd2 = engine.posterior(0, ym, ys)
    assert np.array_equal(mu2, mu_s) and np.array_equal(sd2, sd_s)

