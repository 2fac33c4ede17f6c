"""GPU (-m gpu): gpiv_ivr_argbest — integrated posterior variance reduction over the resident candidates and its selection —
against a dozen lines of NumPy on kg_truth.posterior_cov (fp64 Cholesky solve on the host) and the device's own fetched mu / sd;
the conventions, the reader contract, every refusal, and suggest_ivr end to end on the real engine.

Bar: |error| <= 2e-9 scale(x), scale(x) = y_std^2 (sum_j omega_j) max_j cov_j(x)^2 / den2(x): the project's 1e-9 on KG's slopes
b_j = y_std cov_j / den carried over — an error delta <= 1e-9 max|b| on each slope moves sum_j omega_j b_j^2 by at most
2 delta (sum omega) max|b|.  The truth itself is asserted to have at least 10 % of the candidates at IVR >= 1e-3 scale: a test
that passes on zeros checks nothing."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_ivr
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import GroupEngine
from kg_truth import posterior_cov
from mes_truth import argbest
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

BAR = 2e-9
NOISE = 1e-2
Y_MEAN, Y_STD = 3.5, 0.4
#        N, d, M, kind, f, J
CASES = {"a": (40, 3, 257, F.MATERN25, 0.15, 16), "b": (130, 5, 300, F.MATERN25, 0.12, 272), "c": (300, 17, 257, F.RBF, 0.15, 1040),
         "e": (70, 2, 130, F.MATERN15, 0.15, 4096)}
KW = dict(y_mean=Y_MEAN, y_std=Y_STD)


class Case:
    def __init__(self, N, d, M, kind, f, J):
        self.N, self.d, self.M, self.kind, self.J = N, d, M, kind, J
        self.X, y = F.data(N, d, seed=3 * N + d)
        self.yn = (y - y.mean()) / y.std()
        self.ls = f * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
        self.Xc = np.random.RandomState(500 + N + d).uniform(size=(1000, d))[:M]
        self.pts = np.random.RandomState(900 + J).uniform(size=(J, d))
        self.om = np.random.RandomState(7).uniform(0.5, 1.5, J)
        self.what = f"N={N} d={d} M={M} J={J} kind={kind}"

    def posterior(self, eng, Xc=None, **scaled):
        eng.fit(self.X, self.yn, self.kind, self.ls, scaled.pop("alpha", NOISE), **scaled)
        eng.set_candidates(self.Xc if Xc is None else Xc)
        return eng.posterior(0, Y_MEAN, Y_STD)

    def truth(self, mu, sd, pts, om, c=1.0, w=0.0, alpha=NOISE, Xc=None):
        """(IVR, scale) from the oracle's covariance and the device's mu / sd, with include/gpiv.h's conventions"""
        cov2 = (c * posterior_cov(self.kind, self.X, self.ls, (w + alpha) / c, self.Xc if Xc is None else Xc, pts)) ** 2
        den2 = ((sd / Y_STD) ** 2 + (w + alpha)) - w
        with np.errstate(all="ignore"):
            ivr = np.where(den2 == 0, 0.0, Y_STD ** 2 * (cov2 @ om) / den2)
            scale = Y_STD ** 2 * om.sum() * cov2.max(axis=1) / den2
        return np.where(np.isnan(mu) | np.isnan(sd), np.nan, ivr), scale


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(*CASES[name])


def check_values(what, ys, want, scale):
    err = np.abs(-ys - want) / scale
    worst = float(np.nanmax(err))
    print(f"{what}: worst |error| / scale = {worst:.2e} (bar {BAR:.0e}); share with IVR >= 1e-3 scale: {np.mean(want >= 1e-3 * scale):.2f}")
    assert np.mean(want >= 1e-3 * scale) >= 0.10, "the truth is (nearly) zero everywhere: this fixture checks nothing"
    assert np.array_equal(np.isnan(ys), np.isnan(want))
    assert worst <= BAR, f"{what}: {worst:.2e} over the bar"
    assert (ys[~np.isnan(ys)] <= 0).all()


@pytest.mark.parametrize("name,weighted", [("a", True), ("b", True), ("c", True), ("e", True), ("a", False), ("b", False)])
def test_values_and_selection(engine, name, weighted):
    c = case_of(name)
    mu, sd = c.posterior(engine)
    om = c.om if weighted else None
    bi, bv, si, sv, ys = engine.ivr_argbest(c.pts, om, k_seeds=8, return_values=True, **KW)
    want, scale = c.truth(mu, sd, c.pts, c.om if weighted else np.full(c.J, 1.0 / c.J))
    check_values(f"{c.what} weighted={weighted}", ys, want, scale)
    wi, wv, wsi, wsv = argbest(ys, 8)
    assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv)
    top = np.argsort(-want, kind="stable")[:9]
    assert (np.diff(-want[top]) > 2 * BAR * scale[top].max()).all(), "the truth's top nine are within the bar of each other"
    assert np.array_equal(si, top[:8]) and bi == top[0]
    oi, ov, osi, osv, _ = engine.ivr_argbest(c.pts, om, k_seeds=8, index_offset=10_000_000_000, **KW)
    assert oi == bi + 10_000_000_000 and ov == bv and np.array_equal(osi, si + 10_000_000_000) and np.array_equal(osv, sv)


@pytest.mark.parametrize("J", [1, 100])      # one point; the 128-column tile (the cases above take the 64- and 256-column ones)
def test_other_point_counts(engine, J):
    c = case_of("a")
    mu, sd = c.posterior(engine)
    pts, om = np.random.RandomState(900 + J).uniform(size=(J, c.d)), c.om[:1] if J == 1 else np.random.RandomState(7).uniform(0.5, 1.5, J)
    ys = engine.ivr_argbest(pts, om, return_values=True, **KW)[4]
    check_values(f"J={J} at {c.what}", ys, *c.truth(mu, sd, pts, om))


SWEEP = [(d, k) for d in (3, 6, 11, 23, 47) for k in (F.RBF, F.MATERN25, F.MATERN15, F.MATERN05)]     # row widths 4, 8, 16, 32, 64


@pytest.mark.parametrize("d,kind", SWEEP)
def test_every_width_and_kind(engine, d, kind):
    c = Case(40, d, 130, kind, 0.5, 40)
    mu, sd = c.posterior(engine)
    ys = engine.ivr_argbest(c.pts, c.om, return_values=True, **KW)[4]
    check_values(c.what, ys, *c.truth(mu, sd, c.pts, c.om))


def test_scaled_slot(engine):
    """case a through gpbo_fit_scaled: c = 2.3, w = 0.05, alpha = 1e-3; lambda = w + alpha, den2 leaves w out"""
    c = case_of("a")
    amp, white, alpha = 2.3, 0.05, 1e-3
    mu, sd = c.posterior(engine, alpha=alpha, amplitude=amp, white=white)
    ys = engine.ivr_argbest(c.pts, c.om, return_values=True, **KW)[4]
    check_values("scaled " + c.what, ys, *c.truth(mu, sd, c.pts, c.om, amp, white, alpha))


def test_conventions(engine):
    c = case_of("a")
    Xn = c.Xc.copy()
    Xn[[140, 11], [1, 0]] = np.nan
    c.posterior(engine, Xn)
    bi, bv, si, sv, ys = engine.ivr_argbest(c.pts, c.om, k_seeds=64, return_values=True, **KW)
    assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 140]]).all() and np.isfinite(np.delete(ys, [11, 140])).all()
    assert not np.isin([11, 140], si).any()
    # noise 0 and candidates ON the training points: the rows whose variance clips to 0 have den2 = 0 and score 0
    engine.fit(c.X, c.yn, c.kind, c.ls, 0.0)
    Xc = np.vstack([c.X, c.Xc[:33]])
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, Y_MEAN, Y_STD)
    clipped = sd == 0
    assert clipped.any() and not clipped.all()
    engine.take_negative_variance_flag()
    ys = engine.ivr_argbest(c.pts, c.om, return_values=True, **KW)[4]
    assert (ys[clipped] == 0).all() and np.isfinite(ys).all() and (ys <= 0).all() and (ys[~clipped] < 0).any()


def test_a_candidates_bits_do_not_depend_on_m(engine):
    small = case_of("a")
    big = Case(40, 3, 1000, F.MATERN25, 0.15, 16)
    assert np.array_equal(big.Xc[:257], small.Xc) and np.array_equal(big.pts, small.pts)
    mu_b, sd_b = big.posterior(engine)
    ys_b = engine.ivr_argbest(small.pts, small.om, return_values=True, **KW)[4]
    mu_s, sd_s = small.posterior(engine)
    ys_s = engine.ivr_argbest(small.pts, small.om, return_values=True, **KW)[4]
    same = (mu_b[:257] == mu_s) & (sd_b[:257] == sd_s)
    assert same.sum() >= 200, "the posterior's own bits differ between the two M: this test has nothing to compare"
    assert np.array_equal(ys_b[:257][same], ys_s[same])


def test_reader_only(engine):
    eng, c = engine, case_of("b")
    mu0, sd0 = c.posterior(eng)
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    eng.ivr_argbest(c.pts, c.om, k_seeds=8, return_values=True, **KW)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    assert before[0] == after[0] and before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[2:], after[2:]))
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc)
    assert eng.take_negative_variance_flag() is False
    mu1, sd1 = eng.posterior(0, Y_MEAN, Y_STD)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    x_new, yn2 = np.random.RandomState(5).uniform(size=(2, c.d)), np.concatenate([c.yn, [0.2, -0.4]])

    def arm(with_ivr):
        c.posterior(eng)
        if with_ivr:
            eng.ivr_argbest(c.pts, c.om, k_seeds=8, **KW)
        eng.fit_append(x_new, yn2)
        if with_ivr:
            with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
                eng.ivr_argbest(c.pts, c.om, **KW)
        return eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)

    mu_a, sd_a, route_a = arm(False)
    mu_b, sd_b, route_b = arm(True)
    assert route_a == 1 and route_b == 1 and np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)


def test_refusals(engine):
    eng, c = engine, case_of("a")
    c.posterior(eng)
    good, w5 = np.ascontiguousarray(c.pts[:5]), np.ascontiguousarray(c.om[:5])
    ref = eng.ivr_argbest(good, w5, k_seeds=4, return_values=True, **KW)
    for bad in (np.zeros((0, 3)), np.zeros((4097, 3))):
        with pytest.raises(ValueError, match="n_points"):
            eng.ivr_argbest(bad, **KW)
    with pytest.raises(ValueError, match="dimension"):
        eng.ivr_argbest(np.zeros((5, 4)), **KW)
    for bad_p, bad_w in ((np.nan, np.nan), (np.inf, np.inf), (-np.inf, -0.1)):
        p, w = good.copy(), w5.copy()
        p[3, 1], w[2] = bad_p, bad_w
        with pytest.raises(ValueError, match="finite"):
            eng.ivr_argbest(p, **KW)
        with pytest.raises(ValueError, match="weights"):
            eng.ivr_argbest(good, w, **KW)
    with pytest.raises(ValueError, match="sum"):
        eng.ivr_argbest(good, np.zeros(5), **KW)
    with pytest.raises(ValueError, match="weights"):
        eng.ivr_argbest(good, np.ones(4), **KW)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="k_seeds"):
            eng.ivr_argbest(good, k_seeds=bad, **KW)
    for bad in (np.nan, np.inf, 0.0, -0.4, 0.5):                           # 0.5: not the y_std the resident posterior was scaled with
        with pytest.raises(ValueError, match="y_std"):
            eng.ivr_argbest(good, y_mean=Y_MEAN, y_std=bad)
    bi, bv, sv = np.empty(1, dtype=np.int64), np.empty(1), np.empty(4)
    call, g, w = eng._lib.gpiv_ivr_argbest, dptr(good), dptr(w5)
    assert call(eng._h, None, w, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, w, 5, 3, Y_MEAN, Y_STD, 0, 0, None, dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, w, 5, 3, Y_MEAN, Y_STD, 4, 0, iptr(bi), dptr(bv), None, dptr(sv), None) == _lib.ERR_INVALID
    assert call(eng._h, g, w, 0, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, w, 4097, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(None, g, w, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, w, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.GPBO_OK
    assert bi[0] == ref[0] and bv[0] == ref[1]
    eng.set_candidates(c.Xc[:100])
    with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
        eng.ivr_argbest(good, **KW)
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE, slot=2)
    eng.posterior(2, Y_MEAN, Y_STD, fetch=False)
    with pytest.raises(GpboError, match="slot 0"):
        eng.ivr_argbest(good, **KW)
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        rc = call(eng._h, g, w, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None)
        assert rc == _lib.ERR_STATE
        with pytest.raises(GpboError, match="pending gpbo_fit_begin"):
            eng._check(rc)
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.ivr_argbest(object.__new__(GroupEngine), good)


def test_suggest_ivr_picks_the_restatements_maximiser(engine):
    D, N, M, J = 2, 25, 2000, 300
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    rs = np.random.RandomState(77)
    X = bounds[:, 0] + rs.uniform(size=(N, D)) * (bounds[:, 1] - bounds[:, 0])
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) - 0.3 * (X[:, 0] - 0.5) ** 2 + 0.05 * rs.standard_normal(N)
    drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M)
    drv._gp.alpha = 1e-2
    params, info = suggest_ivr(drv, J, n_random=M, return_info=True)
    gp, ys_ = drv._gp, float(drv._gp._y_train_std)
    assert drv._acquisition_function.i == 0 and list(params) == drv._space.keys and np.array_equal(info["points_index"], np.arange(J))
    Xc = engine.get_candidate_rows(np.arange(M), D)
    mu, sd = engine.posterior(0, float(gp._y_train_mean), ys_)
    ls = np.broadcast_to(np.exp(gp.kernel_.theta), (D,))
    cov2 = posterior_cov(F.MATERN25, X, ls, 1e-2, Xc, Xc[:J]) ** 2
    den2 = (sd / ys_) ** 2 + 1e-2
    ivr, scale = ys_ ** 2 * cov2.mean(axis=1) / den2, ys_ ** 2 * cov2.max(axis=1) / den2
    top = np.sort(ivr)[::-1][:2]
    assert top[0] - top[1] > 2 * BAR * scale.max(), "the restatement's best and second best are within the bar: pick another seed"
    assert info["index"] == int(ivr.argmax()) and abs(info["value"] - ivr.max()) <= BAR * scale.max() and info["value"] > 0
    assert np.array_equal(np.array(list(params.values())), Xc[info["index"]])
    from bayesianoptimization_amd import _suggest as S

    twin = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M)
    twin._gp.alpha = 1e-2
    S.fit_model(twin._gp, twin._space, "twin")
    for t in range(D):
        twin._random_state.uniform(bounds[t, 0], bounds[t, 1], M)
    assert B.same_state(drv._random_state, twin._random_state)
    for bad, what in ((0, "n_points"), (4097, "n_points"), (2.0, "n_points"), (J + 1, "n_random")):
        with pytest.raises(ValueError, match=what):
            suggest_ivr(drv, bad, n_random=J)
