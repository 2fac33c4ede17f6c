"""CPU: the knowledge gradient's host side — the fp64 restatement (tests/kg_truth.py: `kg_values`) against the 50-digit mpmath truth
on the N = 40 fixture of tests/test_gpu_kg.py, the envelope's hand cases, and `suggest_kg` over an oracle-backed engine double: the
argument checks and their order, every gate refusal, the reference-point rule, the RandomState it leaves behind, the pick.  The
device's arithmetic is checked in tests/test_gpu_kg.py."""
import functools
import os
import re

import numpy as np
import pytest

import batch_truth as B
import kg_truth as T
import matern_family_truth as F
from bayesianoptimization_amd import _lib, suggest_kg
from conftest import ROOT


def small_case():
    """case a of tests/test_gpu_kg.py: N = 40, d = 3, Matern 2.5, noise 1e-2, length scale 0.15 sqrt(d) geomspace(0.75, 1.33, d)"""
    N, d = 40, 3
    X, y = F.data(N, d, seed=3 * N + d)
    ls = 0.15 * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
    Xc = np.random.RandomState(500 + N + d).uniform(size=(1000, d))[:257]
    return X, y, ls, 1e-2, Xc


def test_restatement_against_the_mpmath_truth():
    """Five candidates of the N = 40 fixture, J = 16 points by suggest_kg's rule: the fp64 restatement over an fp64 Cholesky
    covariance within 1e-9 scale of the truth whose solve, envelope and integral all run at 50 digits."""
    X, y, ls, noise, Xc = small_case()
    gp = F.fit_fixed_theta(F.MATERN25, X, y, ls, noise)
    yn = (y - gp.y_mean) / gp.y_std
    mu, sd = F.predict(gp, Xc)
    pts = Xc[T.reference_points(mu, 16)]
    mu_pts, _ = F.predict(gp, pts)
    rank = np.argsort(-T.kg_values(mu, sd, T.posterior_cov(F.MATERN25, X, ls, noise, Xc, pts), mu_pts, gp.y_std, noise, 0.0))
    pick = rank[[0, 1, 16, 64, 192]]                      # the two best, then down the ranking
    cov = T.posterior_cov(F.MATERN25, X, ls, noise, Xc[pick], pts)
    got, scale = T.kg_values(mu[pick], sd[pick], cov, mu_pts, gp.y_std, noise, 0.0, return_scale=True)
    want, wscale = T.kg_truth(F.MATERN25, X, yn, ls, noise, Xc[pick], pts, gp.y_mean, gp.y_std)
    err = np.abs(got - want) / wscale
    print(f"worst |error| / scale {err.max():.2e}; KG / scale {want / wscale}")
    assert (want >= 0).all() and want.max() > 1e-3 * wscale.max()
    assert err.max() <= T.BAR and np.abs(scale - wscale).max() <= 1e-9 * wscale.max()


def _closed(a1, b1, a2, b2):
    c = (a1 - a2) / (b2 - b1)
    return (b2 - b1) * T.f(-abs(c))


def test_envelope_hand_cases():
    rs = np.random.RandomState(4)
    # all slopes equal: the maximum is a constant line
    assert T.kg_lines([0.3, -1.0, 2.0], [0.7, 0.7, 0.7]) == 0.0
    assert T.kg_lines([1.5], [0.2]) == 0.0
    # two lines: the closed form, both orders of the intercepts
    for a1, b1, a2, b2 in ((0.0, 0.0, -0.5, 1.0), (0.2, -0.3, 0.9, 0.4), (1.0, 0.1, 1.0, 0.6)):
        assert T.kg_lines([a1, a2], [b1, b2]) == _closed(a1, b1, a2, b2)
        assert abs(T.kg_lines([a1, a2], [b1, b2]) - T.kg_lines_truth([a1, a2], [b1, b2])) <= 1e-15
    # a dominated line, duplicates and the order change nothing
    a, b = rs.standard_normal(12), rs.standard_normal(12)
    base = T.kg_lines(a, b)
    assert base >= 0.0 and abs(base - T.kg_lines_truth(a, b)) <= 1e-14 * np.abs(b).max()
    assert T.kg_lines(np.append(a, a.min() - 10.0), np.append(b, 0.5 * (b.min() + b.max()))) == base
    assert T.kg_lines(np.append(a, a[b.argmax()] - 1.0), np.append(b, b.max())) == base      # same slope, smaller intercept
    assert T.kg_lines(np.concatenate([a, a, a[:5]]), np.concatenate([b, b, b[:5]])) == base
    for _ in range(20):
        p = rs.permutation(12)
        assert T.kg_lines(a[p], b[p]) == base
    # KG >= 0, and adding a line never lowers it beyond rounding
    for n in (2, 3, 8, 65):
        a, b = rs.standard_normal(n), rs.standard_normal(n) * rs.uniform(0.01, 3.0)
        full = T.kg_lines(a, b)
        assert full >= 0.0
        assert abs(full - T.kg_lines_truth(a, b)) <= 1e-13 * np.abs(b).max()
        for k in range(1, n):
            assert T.kg_lines(a[:k + 1], b[:k + 1]) + (a[:k + 1].max() - a[:k].max()) >= T.kg_lines(a[:k], b[:k]) - 1e-14
    # non-finite entries
    assert np.isnan(T.kg_lines([0.0, np.nan], [0.0, 1.0])) and np.isnan(T.kg_lines([0.0, 1.0], [np.inf, 1.0]))
    # far breakpoints: f underflows to 0
    assert T.kg_lines([0.0, -1e3], [0.0, 1.0]) == 0.0 and T.kg_lines([0.0, -38.0], [0.0, 1.0]) > 0.0


def test_conventions():
    cov = np.array([[0.1, 0.05]] * 4)
    mu = np.array([0.3, np.nan, 0.3, 0.3])
    sd = np.array([0.0, 0.2, np.nan, 0.2])
    kg = T.kg_values(mu, sd, cov, [0.1, 0.2], 1.0, 0.0, 0.0)
    assert kg[0] == 0.0 and np.isnan(kg[1]) and np.isnan(kg[2]) and kg[3] > 0.0      # den == 0: nothing is learned
    assert T.kg_values(mu[3:], sd[3:], cov[3:], [0.1, 0.2], 1.0, 0.0, 0.0)[0] == kg[3]


# ---- suggest_kg over the engine double --------------------------------------------------------------------------------------------
D, N, M = 3, 30, 600
_driver = functools.partial(B.suggest_driver, T.KgFakeEngine, n_random=M)


@pytest.mark.parametrize("n_points", [1, 7, 32])
def test_pick_calls_randomstate_and_info(n_points):
    drv, eng, X, y = _driver()
    twin, teng, _, _ = _driver()
    fn = drv._acquisition_function
    before = (fn.i, fn.kappa)
    params, info = suggest_kg(drv, n_points, n_random=M, return_info=True)
    # the RandomState ends where the fit and ONE candidate draw leave it
    from bayesianoptimization_amd import _suggest as S

    S.fit_model(twin._gp, twin._space, "twin")
    teng.generate_candidates_like(M, B.SUGGEST_BOUNDS[:, 0], B.SUGGEST_BOUNDS[:, 1], twin._random_state)
    assert B.same_state(drv._random_state, twin._random_state) and np.array_equal(eng.Xc, teng.Xc)
    names = [c[0] for c in eng.calls]
    assert names.count("fit") == 1 and names.count("generate_candidates_like") == 1 and names.count("posterior") == 1
    assert [c for c in eng.calls if c[0] == "acq_argbest"] == [("acq_argbest", 0, (n_points + 1) // 2)]
    assert [c for c in eng.calls if c[0] == "kg_argbest"] == [("kg_argbest", n_points, 0)]
    assert names.index("fit") < names.index("generate_candidates_like") < names.index("posterior") < names.index("acq_argbest") \
        < names.index("kg_argbest")
    assert not {"posterior_refresh", "fit_append", "polish_seeds", "predict_grad", "set_candidates", "sample_paths"} & set(names)
    assert (fn.i, fn.kappa) == before
    # the reference points: the rule on the resident mean; info; the pick is the restatement's argmax
    mu, sd = eng.post[0]
    assert set(info) == {"points_index", "point_means", "value", "index"}
    assert np.array_equal(info["points_index"], T.reference_points(mu, n_points)) and len(set(info["points_index"])) == n_points
    assert np.array_equal(eng.points, eng.Xc[info["points_index"]]) and info["point_means"].shape == (n_points,)
    assert np.abs(info["point_means"] - mu[info["points_index"]]).max() <= 1e-9 * np.abs(mu).max()
    assert isinstance(info["index"], int) and isinstance(info["value"], float) and info["value"] > 0.0
    Xt, kind, ls, noise = eng.inputs[0]
    kg = T.kg_values(mu, sd, T.posterior_cov(kind, Xt, ls, noise, eng.Xc, eng.points), info["point_means"],
                     float(drv._gp._y_train_std), noise, 0.0)
    assert info["index"] == int(kg.argmax()) and info["value"] == kg.max()
    assert list(params) == drv._space.keys and np.array_equal(np.array(list(params.values())), eng.Xc[info["index"]])
    again, _, _, _ = _driver()
    assert suggest_kg(again, n_points, n_random=M) == params


def test_reference_point_rule():
    mu = np.array([0.1, 0.9, 0.9, 0.3, 0.9, 0.2, 0.0])
    assert T.reference_points(mu, 1).tolist() == [1]                        # ties to the lowest index
    assert T.reference_points(mu, 2).tolist() == [1, 0]
    assert T.reference_points(mu, 5).tolist() == [1, 2, 4, 0, 3]            # odd J: ceil(J / 2) by mean, floor(J / 2) first rows
    assert T.reference_points(mu, 7).tolist() == [1, 2, 4, 3, 0, 5, 6]

    class Stub:
        def acq_argbest(self, acq, param, k_seeds=0):
            ys = -mu
            order = np.lexsort((np.arange(len(ys)), ys))[:k_seeds]
            return int(order[0]), float(ys[order[0]]), order, ys[order], None

    from bayesianoptimization_amd.kg import reference_points

    for J in (1, 2, 5, 7):
        assert reference_points(Stub(), J, len(mu)).tolist() == T.reference_points(mu, J).tolist()


def test_refusals():
    drv, eng, X, y = _driver()
    for bad in (0, -1, 65, 1.5, True, None):
        with pytest.raises(ValueError, match="n_points"):
            suggest_kg(drv, bad)
    with pytest.raises(ValueError, match="n_random"):
        suggest_kg(drv, 8, n_random=7)
    assert not eng.calls
    # the caller's own checks come before the gate
    with pytest.raises(ValueError, match="n_points"):
        suggest_kg(type("Bare", (), {"_gp": object(), "_space": None})(), 0)
    group = B.check_shared_refusals(lambda d: suggest_kg(d, 4), _driver, "suggest_kg")
    with pytest.raises(NotImplementedError, match="device group"):
        type(group).kg_argbest(group, np.zeros((1, 3)))
    from helpers import FakeEngine

    drv, eng, X, y = _driver()
    drv._gp.engine = FakeEngine()
    with pytest.raises(NotImplementedError, match="kg_argbest"):
        suggest_kg(drv, 4)


def test_exported_and_header_limits():
    import bayesianoptimization_amd as pkg
    from bayesianoptimization_amd import kg

    assert "suggest_kg" in pkg.__all__ and pkg.suggest_kg is kg.suggest_kg
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    assert _lib.MAX_KG_POINTS == 64 and re.search(r"^#define GPBO_MAX_KG_POINTS 64\b", hdr, flags=re.M)
    m = re.search(r"^int gpbo_kg_argbest\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["gpbo_kg_argbest"][1]) == 14
    assert not [n for n in _lib.SIGNATURES if "kg" in n and n != "gpbo_kg_argbest"]      # no group / communicator form
