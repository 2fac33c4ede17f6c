"""GPU (-m gpu): gpje_jes_argbest against jes_truth (the header in NumPy, r2 from mpmath, covariances from an fp64 Cholesky) on the
device's own fetched mu / sd; r2 alone; the conventions, the reader contract, every refusal, and suggest_jes end to end.
r2's bar is relative: the header's ranges restated in plain fp64 NumPy / SciPy miss mpmath by at most W = 1.77e-14 over R2_GRID (at
beta just above -2), and the device, with its own exp / erfcx / division, is held to 4 W = 7.1e-14; it measures 3.2e-15.
The values' bar is absolute, in nats: max(1e-9, 4 D), D the worst difference over case one between the truth with cov / m / p from an
fp64 Cholesky and from an np.longdouble one — the fp64 reference's own noise, 4.4e-16 on the host's mu / sd, so the bar is 1e-9.  The
truth itself is asserted to have at least 10 % of the candidates at a >= 1e-3: a test that passes on zeros checks nothing."""
import functools

import numpy as np
import pytest

import batch_truth as B
import jes_truth as T
import matern_family_truth as F
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_jes, suggest_mes
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import GroupEngine
from mes_truth import argbest

pytestmark = pytest.mark.gpu

NOISE, Y_MEAN, Y_STD = 1e-2, 3.5, 0.4
KW = dict(y_mean=Y_MEAN, y_std=Y_STD)
TS, BAR = np.array([2.0, 0.7, 0.0, -0.5]), []      # BAR: case one's, measured once
#        N, d, M, kind, f, S
CASES = {"s16": (40, 3, 257, F.MATERN25, 0.15, 16), "s17": (40, 3, 257, F.MATERN25, 0.15, 17), "s33": (130, 5, 300, F.MATERN25, 0.12, 33),
         "s64": (70, 2, 130, F.MATERN15, 0.15, 64), "s1": (40, 3, 130, F.RBF, 0.15, 1)}


class Case:
    def __init__(self, N, d, M, kind, f, S, c=1.0, w=0.0, alpha=NOISE):
        self.N, self.d, self.M, self.kind, self.S, self.c, self.w, self.alpha = N, d, M, kind, S, c, w, alpha
        self.X, y = F.data(N, d, seed=3 * N + d)
        self.yn = (y - y.mean()) / y.std()
        self.ls = f * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
        self.Xc = np.random.RandomState(500 + N + d).uniform(size=(1000, d))[:M]
        self.xs = np.random.RandomState(900 + S).uniform(size=(S, d))

    def parts(self, Xc=None, xs=None, dtype=np.float64):
        """(cov, m, p) in the slot's normalised units"""
        cov, m, p = T.parts(self.kind, self.X, self.yn, self.ls, (self.w + self.alpha) / self.c, self.Xc if Xc is None else Xc,
                            self.xs if xs is None else xs, dtype)
        return self.c * cov, m, self.c * p

    def f_star(self, m, p):
        return Y_STD * (m + np.resize(TS, len(m)) * np.sqrt(np.maximum(p, 0.0))) + Y_MEAN

    def posterior(self, eng, Xc=None):
        scaled = {} if (self.c, self.w) == (1.0, 0.0) else dict(amplitude=self.c, white=self.w)
        eng.fit(self.X, self.yn, self.kind, self.ls, self.alpha, **scaled)
        eng.set_candidates(self.Xc if Xc is None else Xc)
        return eng.posterior(0, Y_MEAN, Y_STD)

    def truth(self, mu, sd, f_star, parts):
        return T.jes(mu, sd, *parts, (f_star - Y_MEAN) / Y_STD, self.c, self.w, self.w + self.alpha, Y_MEAN, Y_STD)


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(*CASES[name])


def bar_of(c, mu, sd, f_star, xs=None, Xc=None, parts=None):
    """max(1e-9, 4 D): D = the fp64 truth against the same with the solves in np.longdouble"""
    p64, pld = parts or c.parts(Xc, xs), c.parts(Xc, xs, np.longdouble)
    if parts:
        pld = (pld[0],) + tuple(parts[1:])
    D = float(np.nanmax(np.abs(c.truth(mu, sd, f_star, p64) - c.truth(mu, sd, f_star, pld))))
    print(f"the fp64 reference's own noise D = {D:.2e}")
    return max(1e-9, 4.0 * D)


def check_values(what, ys, want, bar):
    assert np.array_equal(np.isnan(ys), np.isnan(want))
    worst = float(np.nanmax(np.abs(-ys - want)))
    print(f"{what}: worst |error| = {worst:.2e} nats (bar {bar:.1e}); share with a >= 1e-3: {np.nanmean(want >= 1e-3):.2f}")
    assert np.nanmean(want >= 1e-3) >= 0.10, "the truth is (nearly) zero everywhere: this fixture checks nothing"
    assert worst <= bar, f"{what}: {worst:.2e} over the bar"


def test_r2_on_the_device(debug_engine):
    got = debug_engine.debug_jes_r2(T.R2_GRID)
    want = np.array([T.r2(b) for b in T.R2_GRID])
    err = np.abs(got - want) / want
    print(f"worst relative error {err.max():.2e} at beta = {T.R2_GRID[err.argmax()]!r}")
    assert err.max() <= 4 * 1.77e-14 <= 1e-13
    assert debug_engine.debug_jes_r2([np.inf, -np.inf])[0] == 1.0 and np.isnan(debug_engine.debug_jes_r2([np.nan])[0])


SWEEP = {f"d{d}k{k}": (40, d, 130, k, 0.5, 20) for d in (3, 6, 11, 23, 47) for k in (F.RBF, F.MATERN25, F.MATERN15, F.MATERN05)}
CASES.update(SWEEP)                                               # row widths 4, 8, 16, 32, 64 x the four kernel kinds
CASES["scaled"] = CASES["s16"] + (2.5, 0.03, 1e-3)                # gpbo_fit_scaled: lambda = w + alpha, vl and vo leave w out


@pytest.mark.parametrize("name", list(CASES))
def test_values_and_selection(engine, name):
    c, one = case_of(name), case_of("s16")
    if not BAR:
        BAR.append(bar_of(one, *one.posterior(engine), one.f_star(*one.parts()[1:])))
    mu, sd = c.posterior(engine)
    parts = c.parts()
    f_star = c.f_star(*parts[1:])
    bi, bv, si, sv, ys, mu_star, var_star = engine.jes_argbest(c.xs, f_star, k_seeds=8, return_values=True, return_star=True, **KW)
    check_values(name, ys, c.truth(mu, sd, f_star, parts), BAR[0])
    assert np.abs(mu_star - (Y_STD * parts[1] + Y_MEAN)).max() <= 1e-9 * Y_STD
    assert np.abs(var_star - Y_STD ** 2 * parts[2]).max() <= 1e-9 * Y_STD ** 2
    wi, wv, wsi, wsv = argbest(ys, 8)
    assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv)
    if name in SWEEP:
        return
    oi, ov, osi, osv, _ = engine.jes_argbest(c.xs, f_star, k_seeds=8, index_offset=10_000_000_000, **KW)
    assert oi == bi + 10_000_000_000 and ov == bv and np.array_equal(osi, si + 10_000_000_000) and np.array_equal(osv, sv)


def test_conventions(engine):
    """A NaN coordinate wins; a sampled optimum ON a training point at alpha = 1e-10 (p_s tiny or <= 0) and candidates whose variance
    clips to 0 stay finite / follow IEEE as the truth does.  p_s there is the difference of two numbers next to 1, so the truth takes
    the device's own m_s / p_s (return_star) and the oracle's covariances; the bar is bar_of's on exactly these inputs."""
    c = case_of("s16")
    Xn = c.Xc.copy()
    Xn[[140, 11], [1, 0]] = np.nan
    c.posterior(engine, Xn)
    bi, bv, si, sv, ys = engine.jes_argbest(c.xs, c.f_star(*c.parts()[1:]), k_seeds=64, return_values=True, **KW)
    assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 140]]).all() and np.isfinite(np.delete(ys, [11, 140])).all()
    for alpha, Xc, on_train in ((1e-10, c.Xc[:130], True), (0.0, np.vstack([c.X, c.Xc[:33]]), False)):
        t = Case(*CASES["s16"], alpha=alpha)
        xs = np.vstack([t.X[5:6], t.xs[1:]]) if on_train else t.xs      # sample 0 ON a training point | as they are
        mu, sd = t.posterior(engine, Xc)
        engine.take_negative_variance_flag()
        assert on_train or ((sd == 0).any() and not (sd == 0).all())
        f_star = t.f_star(*t.parts(Xc, xs)[1:])
        ys, mu_star, var_star = engine.jes_argbest(xs, f_star, return_values=True, return_star=True, **KW)[4:]
        parts = (t.parts(Xc, xs)[0], (mu_star - Y_MEAN) / Y_STD, var_star / Y_STD ** 2)
        assert np.isfinite(ys[sd > 0]).all()
        check_values(f"alpha={alpha}", ys, t.truth(mu, sd, f_star, parts), bar_of(t, mu, sd, f_star, xs, Xc, parts))


def test_reader_only(engine):
    eng, c = engine, case_of("s33")
    f_star = c.f_star(*c.parts()[1:])
    mu0, sd0 = c.posterior(eng)
    eng.take_negative_variance_flag()
    before = eng.mes_argbest(f_star[:4], k_seeds=8, return_values=True)
    eng.jes_argbest(c.xs, f_star, k_seeds=8, return_values=True, **KW)
    after = eng.mes_argbest(f_star[:4], k_seeds=8, return_values=True)
    assert before[0] == after[0] and before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[2:], after[2:]))
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc) and eng.take_negative_variance_flag() is False
    mu1, sd1 = eng.posterior(0, Y_MEAN, Y_STD)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    x_new, yn2 = np.random.RandomState(5).uniform(size=(2, c.d)), np.concatenate([c.yn, [0.2, -0.4]])
    out = []
    for with_jes in (False, True):
        c.posterior(eng)
        if with_jes:
            eng.jes_argbest(c.xs, f_star, k_seeds=8, **KW)
        eng.fit_append(x_new, yn2)
        out.append(eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True))
    assert out[0][2] == 1 and out[1][2] == 1 and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


GOOD_X, GOOD_F = np.full((5, 3), 0.5), np.full(5, 4.0)
bad = lambda x, at, v: np.where(np.arange(x.size).reshape(x.shape) == at, v, x)      # noqa: E731  (flat index `at` set to v)
REFUSALS = [(np.zeros((0, 3)), np.zeros(0), {}, "n_samples"), (np.zeros((65, 3)), np.zeros(65), {}, "n_samples"),
            (np.zeros((5, 65)), GOOD_F, {}, "d out of range"), (bad(GOOD_X, 10, np.nan), GOOD_F, {}, "x_star must be finite"),
            (bad(GOOD_X, 10, np.inf), bad(GOOD_F, 2, np.nan), {}, "x_star must be finite"), (GOOD_X, bad(GOOD_F, 2, np.nan), {}, "f_star"),
            (GOOD_X, bad(GOOD_F, 2, -np.inf), dict(k_seeds=65), "f_star"), (GOOD_X, GOOD_F, dict(k_seeds=65), "k_seeds"),
            (GOOD_X, GOOD_F, dict(k_seeds=-1, y_std=np.nan), "k_seeds"), (GOOD_X, GOOD_F, dict(y_std=np.nan), "y_std"),
            (GOOD_X, GOOD_F, dict(y_std=0.0), "y_std"), (GOOD_X, GOOD_F, dict(y_mean=np.inf), "y_std"),
            (np.zeros((5, 4)), GOOD_F, dict(y_std=0.5), "dimension"), (GOOD_X, GOOD_F, dict(y_std=0.5), "not the one")]


@pytest.mark.parametrize("x_star,f_star,kw,match", REFUSALS)
def test_refusals_in_the_stated_order(engine, x_star, f_star, kw, match):
    case_of("s16").posterior(engine)
    with pytest.raises(ValueError, match=match):
        engine.jes_argbest(x_star, f_star, **{**KW, **kw})


def test_refusals_of_state_and_pointers(engine):
    eng, c = engine, case_of("s16")
    c.posterior(eng)
    bi, bv, sv = np.empty(1, dtype=np.int64), np.empty(1), np.empty(4)
    call, x, f = eng._lib.gpje_jes_argbest, dptr(GOOD_X), dptr(GOOD_F)
    assert call(eng._h, None, f, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, x, f, 5, 3, Y_MEAN, Y_STD, 0, 0, None, dptr(bv), None, None, None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, x, f, 5, 3, Y_MEAN, Y_STD, 4, 0, iptr(bi), dptr(bv), None, dptr(sv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, x, f, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None, None) == _lib.GPBO_OK
    eng.set_candidates(c.Xc[:100])
    with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
        eng.jes_argbest(GOOD_X, GOOD_F, **KW)
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        rc = call(eng._h, x, f, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None, None)
        assert rc == _lib.ERR_STATE
        with pytest.raises(GpboError, match="pending gpbo_fit_begin"):
            eng._check(rc)
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.jes_argbest(object.__new__(GroupEngine), GOOD_X, GOOD_F)


def test_suggest_jes_end_to_end(engine):
    D, N, M = 2, 12, 2000
    bounds = np.array([[0.0, 1.0], [-1.0, 2.0]])
    rs = np.random.RandomState(77)
    X = bounds[:, 0] + rs.uniform(size=(N, D)) * (bounds[:, 1] - bounds[:, 0])
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) - 0.3 * (X[:, 0] - 0.5) ** 2 + 0.05 * rs.standard_normal(N)

    def driver():
        drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M)
        drv._gp.alpha = 1e-2
        return drv

    twin = driver()
    suggest_mes(twin, n_samples=5, n_random=M, n_features=64)
    drv = driver()
    params, info = suggest_jes(drv, n_samples=5, n_random=M, n_features=64, return_info=True)
    assert B.same_state(drv._random_state, twin._random_state)
    x = np.array(list(params.values()))
    assert list(params) == drv._space.keys and (x >= bounds[:, 0]).all() and (x <= bounds[:, 1]).all()
    assert info["value"] >= 0 and info["x_star"].shape == (5, D) and np.isfinite(info["x_star"]).all()
    bi, bv = engine.jes_argbest(info["x_star"], info["f_star"], y_mean=float(drv._gp._y_train_mean), y_std=float(drv._gp._y_train_std))[:2]
    assert bi == info["index"] and -bv == info["value"] and np.array_equal(x, engine.get_candidate_rows(np.array([bi]), D)[0])
