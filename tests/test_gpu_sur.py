"""GPU (-m gpu): gpls_sur_argbest — SUR for an excursion set over the resident candidates — against sur_truth (X, y, theta alone, in
np.longdouble behind SciPy's Cholesky, G by 40-node Gauss-Legendre in the theta form); a candidate's bits alone and among 257; every
refusal; suggest_levelset end to end.

Bar: the project's standing 1e-9 + 1e-9 |truth| on ys, p and the uncertainty.  Noise >= 1e-4 and integration points off the training
set keep s_j^2 from being a cancellation residue: tests/test_sur_host.py holds the truth's own fp64-versus-longdouble spread below
2.5e-10 on every case of CASES."""
import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import sur_truth as T
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_levelset
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import GroupEngine

pytestmark = pytest.mark.gpu

Y_MEAN, Y_STD = 3.5, 0.4
KW = dict(y_mean=Y_MEAN, y_std=Y_STD)
#        J,   N,   M,   d,  kind,       weighted, (c, w)
CASES = [(1, 5, 1, 1, F.RBF, False, None), (17, 33, 65, 5, F.MATERN25, True, None), (64, 64, 257, 17, F.MATERN15, False, None),
         (65, 65, 65, 5, F.MATERN05, True, None), (129, 300, 257, 5, F.RBF, True, None), (257, 33, 65, 1, F.MATERN25, False, None),
         (600, 65, 257, 5, F.MATERN15, True, None), (17, 5, 257, 17, F.MATERN05, False, None), (64, 300, 65, 1, F.MATERN25, True, None),
         (65, 33, 1, 17, F.RBF, False, None), (129, 64, 65, 1, F.MATERN15, True, None), (257, 65, 257, 17, F.MATERN25, True, None),
         (600, 5, 65, 17, F.RBF, False, None), (1, 300, 257, 5, F.MATERN05, True, None), (17, 64, 1, 5, F.MATERN15, False, None),
         (128, 33, 257, 5, F.MATERN05, False, None), (256, 64, 65, 5, F.RBF, True, None), (64, 65, 1, 5, F.MATERN25, False, None),
         (129, 5, 65, 5, F.MATERN05, True, None), (257, 300, 65, 17, F.MATERN15, False, None), (600, 33, 257, 1, F.RBF, True, None),
         (65, 64, 257, 5, F.MATERN25, True, (2.3, 0.05)), (17, 65, 65, 1, F.RBF, True, None), (1, 33, 65, 17, F.MATERN15, False, None)]


def inputs(J, N, M, d, kind, weighted, scaled):
    """The case's data: lengthscales that leave the points correlated with the candidates, a level inside the data's range, one
    integration point equal to a candidate, weights with zeros."""
    X, y = F.data(N, d, seed=3 * N + d)
    yn = (y - y.mean()) / y.std() if N > 1 else y
    ls = (0.35 if d > 1 else 0.05) * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
    Xc = np.random.RandomState(500 + N + d).uniform(size=(M, d))
    pts = np.random.RandomState(900 + J).uniform(size=(J, d))
    pts[J // 2] = Xc[M // 2]
    om = np.random.RandomState(7).uniform(0.5, 1.5, J) * (np.arange(J) % 5 != 3 if J > 4 else 1.0) if weighted else None
    c, w = scaled or (1.0, 0.0)
    return X, yn, ls, Xc, pts, om, c, w, Y_MEAN + 0.3 * Y_STD, 1e-3 if d > 1 else 0.05      # d = 1: a dense, noisy line


def run(eng, case, Xc=None):
    X, yn, ls, Xc0, pts, om, c, w, level, alpha = inputs(*case)
    eng.fit(X, yn, case[4], ls, alpha, **({"amplitude": c, "white": w} if case[6] else {}))
    eng.set_candidates(Xc0 if Xc is None else Xc)
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    return eng.sur_argbest(pts, level, om, k_seeds=min(4, len(Xc0 if Xc is None else Xc)), return_values=True, return_points=True, **KW)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "J{}-N{}-M{}-d{}-k{}".format(*c[:5]))
def test_values_against_the_truth(engine, case):
    X, yn, ls, Xc, pts, om, c, w, level, alpha = inputs(*case)
    bi, bv, si, sv, ys, p, unc = run(engine, case)
    J = case[0]
    want, want_p, want_unc = T.sur(case[4], X, yn, ls, alpha, Xc, pts, np.full(J, 1.0 / J) if om is None else om, level, Y_MEAN,
                                   Y_STD, c, w)
    err = [np.abs(-ys - want).max(), np.abs(p - want_p).max(), abs(unc - want_unc)]
    print(f"{case}: worst |error| ys {err[0]:.2e}, p {err[1]:.2e}, uncertainty {err[2]:.2e}; max SUR {want.max():.2e} of {want_unc:.2e}")
    assert want.max() >= 1e-3 * want_unc > 0, "the truth is (nearly) zero everywhere: this case checks nothing"
    assert (np.abs(-ys - want) <= 1e-9 + 1e-9 * np.abs(want)).all() and (ys <= 0).all()
    assert (np.abs(p - want_p) <= 1e-9 + 1e-9 * want_p).all() and abs(unc - want_unc) <= 1e-9 + 1e-9 * want_unc
    assert (-ys <= unc * (1 + 1e-9)).all()      # a reduction never exceeds the uncertainty itself
    order = np.argsort(ys, kind="stable")[:len(si)]
    assert bi == order[0] and bv == ys[order[0]] and np.array_equal(si, order) and np.array_equal(sv, ys[order])


def test_a_candidates_bits_alone_and_among_257(debug_engine, monkeypatch):
    # The posterior pass takes its GEMV path for one candidate and its MFMA path for 257, with other bits; the debug build's
    # GPBO_SMALL_MAX pins the GEMV path for both, as tests/test_gpu_pfes.py does.
    monkeypatch.setenv("GPBO_SMALL_MAX", "1024")
    case = CASES[6]
    Xc = inputs(*case)[3]
    ys = run(debug_engine, case)[4]
    for i in (0, 100, 256):
        assert run(debug_engine, case, Xc[i:i + 1])[4][0] == ys[i]


def test_nan_candidates_and_the_reader_contract(engine):
    case = CASES[1]
    Xc = inputs(*case)[3].copy()
    Xc[[40, 11], [1, 0]] = np.nan
    bi, bv, si, _sv, ys, _p, _unc = run(engine, case, Xc)
    assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 40]]).all() and np.isfinite(np.delete(ys, [11, 40])).all()
    assert not np.isin([11, 40], si).any() and np.array_equal(engine.get_candidate_rows(np.arange(65), 5), Xc, equal_nan=True)


BAD = [("n_points", dict(points=np.zeros((0, 5)))), ("n_points", dict(points=np.zeros((4097, 5)))), ("dimension", dict(points=np.zeros((3, 4)))),
       ("finite", dict(points=np.full((3, 5), np.inf))), ("weights", dict(weights=np.array([1.0, np.nan, 1.0]))),
       ("weights", dict(weights=np.array([1.0, -0.1, 1.0]))), ("sum", dict(weights=np.zeros(3))), ("weights", dict(weights=np.ones(4))),
       ("level", dict(level=np.nan)), ("level", dict(level=np.inf)), ("k_seeds", dict(k_seeds=65)), ("k_seeds", dict(k_seeds=-1)),
       ("y_std", dict(y_std=0.0)), ("y_std", dict(y_std=0.5)), ("y_std", dict(y_mean=np.nan))]


@pytest.mark.parametrize("match,bad", BAD)
def test_refusals(engine, match, bad):
    run(engine, CASES[1])
    kw = {"points": np.full((3, 5), 0.5), "level": 3.6, "weights": None, **KW, **bad}
    with pytest.raises(ValueError, match=match):
        engine.sur_argbest(kw.pop("points"), kw.pop("level"), kw.pop("weights"), **kw)


def test_state_refusals_and_null_outputs(engine):
    eng = engine
    run(eng, CASES[1])
    good, bi, bv = np.full((3, 5), 0.5), np.empty(1, dtype=np.int64), np.empty(1)
    call, g = eng._lib.gpls_sur_argbest, dptr(good)
    tail = (None, None, None, None, None)
    assert call(eng._h, None, None, 3, 5, 3.6, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), *tail) == _lib.ERR_INVALID
    assert call(eng._h, g, None, 3, 5, 3.6, Y_MEAN, Y_STD, 0, 0, None, dptr(bv), *tail) == _lib.ERR_INVALID
    assert call(eng._h, g, None, 3, 5, 3.6, Y_MEAN, Y_STD, 2, 0, iptr(bi), dptr(bv), *tail) == _lib.ERR_INVALID
    assert call(None, g, None, 3, 5, 3.6, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), *tail) == _lib.ERR_INVALID
    assert call(eng._h, g, None, 3, 5, 3.6, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), *tail) == _lib.GPBO_OK
    eng.set_candidates(np.full((10, 5), 0.25))
    with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
        eng.sur_argbest(good, 3.6, **KW)
    with eng.overlapped_fits():
        X, yn, ls = inputs(*CASES[1])[:3]
        eng.fit(X, yn, F.MATERN25, ls, 1e-3)
        assert call(eng._h, g, None, 3, 5, 3.6, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), *tail) == _lib.ERR_STATE
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.sur_argbest(object.__new__(GroupEngine), good, 3.6)


def levelset_problem():
    """f(x) = x0^2 + x1^2 on [-2, 2]^2, level 1: the unit circle; 40 observations.  On sur_truth alone (scikit-learn's fit of the same
    model, 2000 uniform candidates) the pick has P(f > level) = 0.39 and the corner (2, 2), f = 8, scores 0.12 % of the best."""
    rs = np.random.RandomState(5)
    X = rs.uniform(-2, 2, size=(40, 2))
    return X, (X ** 2).sum(1) + 0.01 * rs.standard_normal(40), np.array([[-2.0, 2.0], [-2.0, 2.0]]), 1.0


def test_suggest_levelset_probes_the_boundary(engine):
    X, y, bounds, level = levelset_problem()
    M, J = 2000, 300
    drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M)
    drv._gp.alpha = 1e-2
    params, info = suggest_levelset(drv, level, J, n_random=M, return_info=True)
    assert drv._acquisition_function.i == 0 and list(params) == drv._space.keys and info["points"].shape == (J, 2)
    x = np.array(list(params.values()))
    assert np.array_equal(x, engine.get_candidate_rows(np.array([info["index"]]), 2)[0])
    deep = np.array([[2.0, 2.0], x])      # the corner is deep inside {f > level}
    engine.set_candidates(deep)
    gp = drv._gp
    engine.posterior(0, float(gp._y_train_mean), float(gp._y_train_std), fetch=False)
    ys, p = engine.sur_argbest(np.vstack([info["points"], deep]), level, np.r_[np.full(J, 1.0 / J), 0.0, 0.0], y_mean=float(gp._y_train_mean),
                               y_std=float(gp._y_train_std), return_values=True, return_points=True)[4:6]
    print(f"pick {x}: |x|^2 = {x @ x:.3f}, P(f > level) = {p[-1]:.3f}; SUR {info['value']:.3e} of {info['uncertainty']:.3e}; corner {-ys[0]:.3e}")
    assert 0.1 < p[-1] < 0.9 and p[-2] > 1 - 1e-6
    assert abs(-ys[1] - info["value"]) <= 1e-9 and 0 <= -ys[0] < 0.01 * info["value"] and info["value"] < info["uncertainty"]
    assert abs(info["uncertainty"] - (info["p"] * (1 - info["p"])).mean()) <= 1e-12
    with pytest.raises(ValueError, match="level"):
        suggest_levelset(drv, np.nan)
    with pytest.raises(ValueError, match="n_points"):
        suggest_levelset(drv, level, 4097)
