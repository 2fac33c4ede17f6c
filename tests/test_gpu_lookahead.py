"""GPU (-m gpu): gpla_ei2_argbest against lookahead_truth on the device's own mu / sd; suggest_lookahead.  The bar is the project's
fp64 bar in target units, 1e-9 y_std + 1e-9 |truth|; test_lookahead_truth_host.py holds the truth's own noise under a tenth of it.
Measured on an MI355X: worst 1.9e-11 against a bar of 2.3e-9 (d1j33, the worst conditioned K'), at most 5.5e-14 in every other case."""
import numpy as np
import pytest

import batch_truth as B
import lookahead_truth as T
from bayesianoptimization_amd import _lib, _suggest as S, fused_acquisition as A, suggest_lookahead
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import EI, GpEngine, GroupEngine
from mes_truth import argbest

pytestmark = pytest.mark.gpu

Y_MEAN, Y_STD, KW = T.Y_MEAN, T.Y_STD, dict(y_mean=T.Y_MEAN, y_std=T.Y_STD)


def posterior(eng, c, Xc=None):
    scaled = {} if (c.c, c.w) == (1.0, 0.0) else dict(amplitude=c.c, white=c.w)
    eng.fit(c.X, c.yn, c.kind, c.ls, c.alpha, **scaled)
    eng.set_candidates(c.Xc if Xc is None else Xc)
    return eng.posterior(0, Y_MEAN, Y_STD)


def ei2(eng, c, pts=None, **kw):
    return eng.ei2_argbest(c.pts if pts is None else pts, c.nodes, c.weights, c.y_best, **{**KW, **kw})


def check_values(what, ys, want, rows=slice(None)):
    assert np.array_equal(np.isnan(ys), np.isnan(want))
    err, bar = np.abs(-ys - want)[rows], (1e-9 * Y_STD + 1e-9 * np.abs(want))[rows]
    print(f"{what}: worst |error| = {np.nanmax(err):.2e} (bar {np.nanmin(bar):.1e}), worst error / bar = {np.nanmax(err / bar):.2e}")
    assert np.nanmax(want) >= 1e-6 * Y_STD, "the truth is within a thousand bars of zero everywhere: this fixture checks nothing"
    assert not (err > bar).any(), f"{what}: over the bar"


@pytest.mark.parametrize("name", list(T.CASES))
def test_values_and_selection(engine, name):
    c = T.Case(*T.CASES[name])
    mu, sd = posterior(engine, c)
    parts = c.parts()
    k = min(8, c.M)
    bi, bv, si, sv, ys, mu_pts, var_pts = ei2(engine, c, k_seeds=k, return_values=True, return_point_moments=True)
    check_values(name, ys, c.truth(mu, sd, parts))
    assert np.abs(mu_pts - (Y_STD * parts[1] + Y_MEAN)).max() <= 1e-9 * Y_STD
    assert np.abs(var_pts - Y_STD ** 2 * np.maximum(parts[2], 0.0)).max() <= 1e-9 * Y_STD ** 2
    wi, wv, wsi, wsv = argbest(ys, k)
    assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv)
    assert ei2(engine, c, index_offset=10_000_000_000)[:2] == (bi + 10_000_000_000, bv)


def test_one_node_and_a_far_point_is_one_step_ei_twice(engine):      # a = e1 + max(G(mn, q_0, b), G(0, 1, b)): no truth module
    c = T.Case(*T.CASES["j16"])
    mu, sd = posterior(engine, c)
    ys = engine.ei2_argbest(np.full((1, c.d), 50.0), [0.0], [1.0], c.y_best, return_values=True, **KW)[4]
    mn, v, bn = (mu - Y_MEAN) / Y_STD, (sd / Y_STD) ** 2, (c.y_best - Y_MEAN) / Y_STD
    b = np.maximum(bn, mn)
    q0 = np.sqrt(v - v * v / (v + c.alpha))
    want = Y_STD * (T.G(mn, np.sqrt(v + c.alpha), bn) + np.maximum(T.G(mn, q0, b), T.G(0.0, 1.0, b)))
    check_values("anchor", ys, want)


def test_conventions(engine):
    """A row with 0 < sd <= 1e-3 y_std at alpha = 0 has g = cov / den, a rounding error over the root of one: |g z| <= 1e-15 / 1e-8 * 3
    moves a mean by under 1e-6, and G is 1-Lipschitz in the mean, so those rows are held to 1e-6 y_std and the others to the bar."""
    c = T.Case(*T.CASES["j16"])
    Xn = np.random.RandomState(3).uniform(size=(150, c.d))
    pts = np.vstack([Xn[7:8], c.pts[1:]])
    mu, sd = posterior(engine, c, Xn)
    check_values("a point on a candidate", ei2(engine, c, pts, return_values=True)[4], c.truth(mu, sd, c.parts(Xn, pts)))
    Xn[[140, 11], [1, 0]] = np.nan
    posterior(engine, c, Xn)
    bi, bv, si, sv, ys = ei2(engine, c, pts, k_seeds=64, return_values=True)
    assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 140]]).all() and np.isfinite(np.delete(ys, [11, 140])).all()
    t = T.Case(*T.CASES["j16"], alpha=0.0)
    Xc = np.vstack([t.X, t.Xc[:33]])
    mu, sd = posterior(engine, t, Xc)
    engine.take_negative_variance_flag()
    assert (sd == 0).any() and not (sd == 0).all()
    ys, want = ei2(engine, t, return_values=True)[4], t.truth(mu, sd, t.parts(Xc))
    assert np.abs(-ys - want).max() <= 1e-6 * Y_STD
    check_values("alpha = 0", ys, want, (sd == 0) | (sd > 1e-3 * Y_STD))


def test_a_rows_bits_do_not_depend_on_where_it_sits(engine):
    c = T.Case(70, 3, 130, T.M25, 64, 32)
    out = []
    for Xc in (c.Xc, c.Xc[:70][::-1].copy(), c.Xc[3:]):
        mu, sd = posterior(engine, c, Xc)
        out.append((mu, sd, ei2(engine, c, return_values=True)[4]))
    for k, pick in ((1, np.arange(70)[::-1]), (2, np.arange(3, 130))):
        assert np.array_equal(out[k][0], out[0][0][pick]) and np.array_equal(out[k][1], out[0][1][pick]), "the posterior pass moved"
        assert np.array_equal(out[k][2], out[0][2][pick])


def test_reader_only(engine):
    eng, c = engine, T.Case(*T.CASES["j33"])
    mu0, sd0 = posterior(eng, c)
    eng.take_negative_variance_flag()
    ei2(eng, c, k_seeds=8, return_values=True)
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc) and eng.take_negative_variance_flag() is False
    mu1, sd1 = eng.posterior(0, Y_MEAN, Y_STD)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    x_new, yn2 = np.random.RandomState(5).uniform(size=(2, c.d)), np.concatenate([c.yn, [0.2, -0.4]])
    out = []
    for with_call in (False, True):
        posterior(eng, c)
        if with_call:
            ei2(eng, c, k_seeds=8)
        eng.fit_append(x_new, yn2)
        out.append(eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True))
    assert out[0][2] == 1 and out[1][2] == 1 and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


P, Z, W, O = np.full((5, 3), 0.5), np.array([-1.0, 0.0, 1.0]), np.array([0.25, 0.5, 0.25]), np.zeros(33)
bad = lambda x, at, v: np.where(np.arange(x.size).reshape(x.shape) == at, v, x)      # noqa: E731  (each call is wrong as matched AND in the next way)
REFUSALS = [(np.zeros((0, 3)), O, O, 4.0, {}, "n_points"), (np.zeros((65, 3)), O, O, 4.0, {}, "n_points"), (np.zeros((5, 65)), O, O, 4.0, {}, "n_nodes"),
            (np.zeros((5, 65)), Z, W, 4.0, {}, "d out of range"), (bad(P, 10, np.nan), bad(Z, 1, np.inf), W, 4.0, {}, "points must be finite"),
            (P, bad(Z, 1, np.inf), bad(W, 0, np.nan), 4.0, {}, "nodes"), (P, Z, bad(bad(W, 0, np.nan), 1, -1.0), 4.0, {}, "weights must be finite"),
            (P, Z, bad(W, 2, -0.25), np.nan, {}, "negative"), (P, Z, np.zeros(3), np.nan, {}, "all be zero"),
            (P, Z, W, np.inf, dict(k_seeds=65), "y_best"), (P, Z, W, 4.0, dict(k_seeds=-1, y_std=np.nan), "k_seeds"),
            (P, Z, W, 4.0, dict(y_std=0.0), "y_std"), (P, Z, W, 4.0, dict(y_mean=np.inf), "y_std"),
            (np.zeros((5, 4)), Z, W, 4.0, dict(y_std=0.5), "dimension"), (P, Z, W, 4.0, dict(y_std=0.5), "not the one")]


@pytest.mark.parametrize("points,nodes,weights,y_best,kw,match", REFUSALS)
def test_refusals_in_the_stated_order(engine, points, nodes, weights, y_best, kw, match):
    posterior(engine, T.Case(*T.CASES["j16"]))
    with pytest.raises(ValueError, match=match):
        engine.ei2_argbest(points, nodes, weights, y_best, **{**KW, **kw})


def test_refusals_of_pointers_and_state_at_their_place_in_the_order(engine):
    """NULL inputs before y_best, NULL outputs before y_std, a pending fit before the model's d, a missing pass before the recorded y_std"""
    eng, c = engine, T.Case(*T.CASES["j16"])
    posterior(eng, c)
    bi, bv, sv = np.empty(1, dtype=np.int64), np.empty(1), np.empty(4)
    p, z, w, out = dptr(P), dptr(Z), dptr(W), (iptr(bi), dptr(bv), None, None, None, None, None)
    def refused(exc, match, *a, on=eng):      # noqa: E306
        with pytest.raises(exc, match=match):
            on._check(on._lib.gpla_ei2_argbest(on._h, *a))
    for args in ((None, 5, 3, z, w), (p, 5, 3, None, w), (p, 5, 3, z, None)):
        refused(ValueError, "NULL points, nodes or weights", *args, 3, np.nan, Y_MEAN, Y_STD, 0, 0, *out)
    refused(ValueError, "NULL output", p, 5, 3, z, w, 3, 4.0, Y_MEAN, np.nan, 0, 0, None, *out[1:])
    refused(ValueError, "NULL output", p, 5, 3, z, w, 3, 4.0, Y_MEAN, np.nan, 4, 0, iptr(bi), dptr(bv), None, dptr(sv), None, None, None)
    assert eng._lib.gpla_ei2_argbest(eng._h, p, 5, 3, z, w, 3, 4.0, Y_MEAN, Y_STD, 0, 0, *out) == _lib.GPBO_OK
    eng.set_candidates(c.Xc[:50])
    refused(GpboError, "run gpbo_posterior for slot 0 first", p, 5, 3, z, w, 3, 4.0, Y_MEAN, 0.5, 0, 0, *out)
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, c.alpha)
        refused(GpboError, "pending gpbo_fit_begin", dptr(np.zeros((5, 4))), 5, 4, z, w, 3, 4.0, Y_MEAN, Y_STD, 0, 0, *out)
    with GpEngine(0) as fresh:
        refused(GpboError, "has not been fitted", p, 5, 3, z, w, 3, 4.0, Y_MEAN, Y_STD, 0, 0, *out, on=fresh)
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.ei2_argbest(object.__new__(GroupEngine), P, Z, W, 4.0)


def test_suggest_lookahead_end_to_end(engine):
    D, N, M = 2, 12, 2000
    bounds = np.array([[0.0, 1.0], [-1.0, 2.0]])
    rs = np.random.RandomState(77)
    X = bounds[:, 0] + rs.uniform(size=(N, D)) * (bounds[:, 1] - bounds[:, 0])
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) - 0.3 * (X[:, 0] - 0.5) ** 2
    drv, twin = (B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M) for _ in range(2))
    with pytest.raises(ValueError, match="n_nodes"):
        suggest_lookahead(drv, n_nodes=33)
    params, info = suggest_lookahead(drv, n_points=9, n_nodes=5, n_random=M, return_info=True)
    ym, ys_ = float(drv._gp._y_train_mean), float(drv._gp._y_train_std)
    assert np.array_equal(np.array(list(params.values())), engine.get_candidate_rows(np.array([info["index"]]), D)[0])
    assert info["value"] >= info["one_step"] - 1e-12 * ys_ and info["value"] > 0 and info["point_vars"].shape == (9,)
    neg_ei = engine.acq_argbest(EI, 0.0, y_max=float(y.max()), k_seeds=5, return_values=True)
    assert np.array_equal(info["points_index"][:5], neg_ei[2]) and info["one_step"] == -neg_ei[4][info["index"]]
    c5 = T.Case(1, D, 1, T.M25, 1, 5)
    bi, bv = engine.ei2_argbest(engine.get_candidate_rows(info["points_index"], D), c5.nodes, c5.weights, float(y.max()), y_mean=ym, y_std=ys_)[:2]
    assert bi == info["index"] and -bv == info["value"]
    Xt = rs.uniform(size=(7, D))
    mean, std = drv._gp.predict(Xt, return_std=True)
    S.fit_model(twin._gp, twin._space, "twin")      # the host replay of the fit and ONE candidate draw
    for t in range(D):
        twin._random_state.uniform(bounds[t, 0], bounds[t, 1], M)
    assert B.same_state(drv._random_state, twin._random_state)
    assert all(np.array_equal(a, b) for a, b in zip((mean, std), twin._gp.predict(Xt, return_std=True)))
