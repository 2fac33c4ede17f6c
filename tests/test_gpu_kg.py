"""GPU (-m gpu): gpbo_kg_argbest — knowledge-gradient values over the resident candidates and their selection — against the fp64
restatement of tests/kg_truth.py evaluated on the device's own fetched mu / sd and the oracle's candidate x point covariance, the
50-digit mpmath truth at five candidates, the envelope alone through gpbo_debug_kg_lines, the conventions, the reader contract, every
refusal, and suggest_kg end to end on the real engine.

Bar: |error| <= 1e-9 scale(x), scale(x) = max_j |b_j| (the slopes' size: KG is a sum of slope differences times f <= 0.4).  The
fixtures use short length scales and noise 1e-2: with the suite's usual ones the median KG is 1e-127 and a test would pass on zeros;
here the truth itself is asserted to have at least 10 % of the candidates at KG >= 1e-3 scale.  The instance axis — every (padded width,
kernel kind) of kg_points_kernel and every (padded width, kernel kind, columns per pass) of kg_cov_kernel — is
tests/test_gpu_instances.py's."""
import functools

import numpy as np
import pytest

import batch_truth as B
import kg_truth as T
import matern_family_truth as F
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_kg
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import GpEngine, GroupEngine
from mes_truth import argbest
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NOISE = 1e-2
Y_MEAN, Y_STD = 3.5, 0.4
#        N, d, M, kind, f, J
CASES = {"a": (40, 3, 257, F.MATERN25, 0.15, 16), "b": (40, 3, 1000, F.MATERN25, 0.15, 64), "c": (130, 5, 257, F.MATERN25, 0.12, 33),
         "d": (300, 17, 257, F.RBF, 0.15, 40)}


class Case:
    """Data of one case (computed once, shared, never changed); the posterior is the device's own, fetched per test."""

    def __init__(self, N, d, M, kind, f, J):
        self.N, self.d, self.M, self.kind, self.J = N, d, M, kind, J
        self.X, y = F.data(N, d, seed=3 * N + d)
        self.yn = (y - y.mean()) / y.std()
        self.ls = f * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
        self.Xc = np.random.RandomState(500 + N + d).uniform(size=(1000, d))[:M]
        self.what = f"N={N} d={d} M={M} J={J}"

    def posterior(self, eng, Xc=None, **scaled):
        eng.fit(self.X, self.yn, self.kind, self.ls, scaled.pop("alpha", NOISE), **scaled)
        eng.set_candidates(self.Xc if Xc is None else Xc)
        return eng.posterior(0, Y_MEAN, Y_STD)

    def points(self, mu, J=None):
        return self.Xc[T.reference_points(mu, self.J if J is None else J)]

    def truth(self, mu, sd, pts, mu_pts, c=1.0, w=0.0, alpha=NOISE, Xc=None):
        """(KG, scale) of the restatement on the device's mu / sd / point means and the oracle's covariance"""
        cov = c * T.posterior_cov(self.kind, self.X, self.ls, (w + alpha) / c, self.Xc if Xc is None else Xc, pts)
        return T.kg_values(mu, sd, cov, mu_pts, Y_STD, w + alpha, w, return_scale=True)

    def mean_at(self, pts, eta=NOISE):
        gp = F.fit_fixed_theta(self.kind, self.X, self.yn, self.ls, eta, normalize_y=False)
        return Y_STD * (F.kernel_matrix(self.kind, pts, self.X, self.ls) @ gp.alpha) + Y_MEAN


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(*CASES[name])


def check_values(what, ys, want, scale):
    err = np.abs(-ys - want) / scale
    worst = float(np.nanmax(err))
    print(f"{what}: worst |error| / scale = {worst:.2e} (bar {T.BAR:.0e}); share with KG >= 1e-3 scale: {np.mean(want >= 1e-3 * scale):.2f}")
    assert np.array_equal(np.isnan(ys), np.isnan(want))
    assert worst <= T.BAR, f"{what}: {worst:.2e} over the bar"
    assert (ys[~np.isnan(ys)] <= 0).all()
    return worst


# ---- values and selection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_values_and_selection(engine, name):
    c = case_of(name)
    mu, sd = c.posterior(engine)
    pts = c.points(mu)
    bi, bv, si, sv, ys, mu_pts = engine.kg_argbest(pts, k_seeds=8, y_mean=Y_MEAN, y_std=Y_STD, return_values=True,
                                                   return_point_means=True)
    want_pts = c.mean_at(pts)
    print(f"{c.what}: point means off by {np.abs(mu_pts - want_pts).max():.2e}")
    assert np.abs(mu_pts - want_pts).max() <= T.BAR * max(1.0, np.abs(want_pts).max())
    want, scale = c.truth(mu, sd, pts, mu_pts)
    assert np.mean(want >= 1e-3 * scale) >= 0.10, "the truth is (nearly) zero everywhere: this fixture checks nothing"
    check_values(c.what, ys, want, scale)
    # the selection, exact against the returned values
    wi, wv, wsi, wsv = argbest(ys, 8)
    assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv)
    # ... and against the truth, whose nine best are further apart than the bar
    top = np.argsort(-want, kind="stable")[:9]
    assert (np.diff(-want[top]) > 2 * T.BAR * scale[top].max()).all(), "the truth's top nine are within the bar of each other"
    assert np.array_equal(si, top[:8]) and bi == top[0]
    # index_offset
    oi, ov, osi, osv, _ = engine.kg_argbest(pts, k_seeds=8, index_offset=10_000_000_000, y_mean=Y_MEAN, y_std=Y_STD)
    assert oi == bi + 10_000_000_000 and ov == bv and np.array_equal(osi, si + 10_000_000_000) and np.array_equal(osv, sv)


def test_mpmath_truth_at_five_candidates(engine):
    c = case_of("a")
    mu, sd = c.posterior(engine)
    pts = c.points(mu)
    ys = engine.kg_argbest(pts, y_mean=Y_MEAN, y_std=Y_STD, return_values=True)[4]
    pick = np.argsort(ys, kind="stable")[[0, 1, 16, 64, 192]]
    want, scale = T.kg_truth(c.kind, c.X, c.yn, c.ls, NOISE, c.Xc[pick], pts, Y_MEAN, Y_STD)
    err = np.abs(-ys[pick] - want) / scale
    print(f"against the 50-digit truth: |error| / scale = {err}")
    assert want.max() >= 1e-3 * scale.max() and err.max() <= T.BAR


def test_scaled_slot(engine):
    """case a through gpbo_fit_scaled: c = 2.3, w = 0.05, alpha = 1e-3; lambda = w + alpha, the candidate's own slope leaves w out"""
    c = case_of("a")
    amp, white, alpha = 2.3, 0.05, 1e-3
    mu, sd = c.posterior(engine, alpha=alpha, amplitude=amp, white=white)
    pts = c.points(mu)
    ys, mu_pts = engine.kg_argbest(pts, y_mean=Y_MEAN, y_std=Y_STD, return_values=True, return_point_means=True)[4:]
    want_pts = c.mean_at(pts, (white + alpha) / amp)
    assert np.abs(mu_pts - want_pts).max() <= T.BAR * max(1.0, np.abs(want_pts).max())
    want, scale = c.truth(mu, sd, pts, mu_pts, amp, white, alpha)
    assert np.mean(want >= 1e-3 * scale) >= 0.10
    check_values("scaled " + c.what, ys, want, scale)


# ---- the envelope alone ------------------------------------------------------------------------------------------------------------
def test_envelope_alone(debug_engine):
    rs = np.random.RandomState(4)
    sets = []

    def add(a, b):
        sets.append((np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))

    def run(n):
        group = [s for s in sets if len(s[0]) == n]
        got = debug_engine.debug_kg_lines(np.array([s[0] for s in group]), np.array([s[1] for s in group]))
        return group, got

    add([1.5], [0.2])
    add([0.0, -0.5], [0.0, 1.0]); add([0.2, 0.9], [-0.3, 0.4]); add([1.0, 1.0], [0.1, 0.6]); add([0.3, 0.3], [0.7, 0.7])
    add([0.5, 0.1], [0.7, 0.7])                                             # a slope tie with different intercepts
    for cc in (0.0, 1.0, 38.0, 1e3):                                         # breakpoints at |c| = 0, 1, 38, 1e3
        add([0.0, -cc], [0.0, 1.0]); add([-cc, 0.0], [0.0, 1.0])
    add([0.0, np.nan], [0.0, 1.0]); add([0.0, 1.0], [np.inf, 1.0]); add([-np.inf, 1.0], [0.0, 1.0]); add([0.0, 1.0], [0.0, np.nan])
    a12, b12 = rs.standard_normal(12), rs.standard_normal(12)
    add(a12, b12)
    for _ in range(6):
        p = rs.permutation(12)
        add(a12[p], b12[p])
    add(np.append(a12, a12.min() - 10.0), np.append(b12, 0.5 * (b12.min() + b12.max())))      # + a dominated line
    add(np.append(a12, a12[b12.argmax()] - 1.0), np.append(b12, b12.max()))                    # + a slope tie below
    add(np.concatenate([a12, a12]), np.concatenate([b12, b12]))                                # duplicates
    add(np.full(7, 0.25), np.full(7, -0.5))                                                    # all lines equal
    add(rs.standard_normal(7), np.full(7, 0.9))                                                # all slopes equal
    for _ in range(70):                                                                        # more than one workgroup of 65 lines
        add(rs.standard_normal(65), rs.standard_normal(65) * rs.uniform(0.01, 3.0))
    bad = sets[-3]
    bad[0][17] = np.nan                                                                        # a NaN set between good neighbours
    worst = 0.0
    for n in sorted({len(s[0]) for s in sets}):
        group, got = run(n)
        for (a, b), g in zip(group, got):
            w = T.kg_lines(a, b)
            if np.isnan(w):
                assert np.isnan(g), (a, b, g)
                continue
            assert g >= 0.0
            worst = max(worst, abs(g - w) / max(np.abs(b).max(), 1e-300))
    print(f"envelope alone: worst |error| / max|b| = {worst:.2e}")
    assert worst <= 1e-14
    g12 = run(12)[1]
    assert (g12 == g12[0]).all()                                           # the order of arrival changes nothing, to the bit
    assert run(13)[1][0] == g12[0] and run(13)[1][1] == g12[0] and run(24)[1][0] == g12[0]
    two = run(2)[1]
    assert two[3] == 0.0 and two[4] == 0.0                                   # equal slopes
    assert two[5] == two[6] and abs(two[5] - 1.0 / np.sqrt(2 * np.pi)) <= 1e-15      # c = 0: (b2 - b1) phi(0)
    assert two[11] == 0.0 and two[12] == 0.0 and two[9] > 0.0 and two[10] > 0.0      # |c| = 1e3: f is 0; |c| = 38: not yet
    assert np.isnan(two[13:17]).all()
    assert run(7)[1].tolist() == [0.0, 0.0] and run(1)[1].tolist() == [0.0]
    with pytest.raises(ValueError):
        debug_engine.debug_kg_lines(np.zeros((1, 66)), np.zeros((1, 66)))


# ---- conventions -----------------------------------------------------------------------------------------------------------------
def test_nothing_learned_scores_zero(engine):
    """Noise 0 and candidates ON the training points (case a's data: K stays well conditioned at its short length scales): the true
    variance there is 0, the computed one rounding alone, and the rows that clip to sd == 0 have den = 0 and score 0."""
    c = case_of("a")
    ym, ys_ = Y_MEAN, Y_STD
    engine.fit(c.X, c.yn, c.kind, c.ls, 0.0)
    Xc = np.vstack([c.X, c.Xc[:33]])
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys_)
    clipped = sd == 0
    print(f"{int(clipped.sum())} of {sd.shape[0]} candidates have a clipped variance")
    assert clipped.any() and not clipped.all()
    engine.take_negative_variance_flag()
    ys = engine.kg_argbest(Xc[T.reference_points(mu, 8)], y_mean=ym, y_std=ys_, return_values=True)[4]
    assert (ys[clipped] == 0).all() and np.isfinite(ys).all() and (ys <= 0).all()


def test_nan_row_wins(engine):
    c = case_of("a")
    Xn = c.Xc.copy()
    Xn[[140, 11], [1, 0]] = np.nan
    mu, sd = c.posterior(engine, Xn)
    pts = c.Xc[T.reference_points(np.nan_to_num(mu, nan=-np.inf), 16)]
    bi, bv, si, sv, ys = engine.kg_argbest(pts, k_seeds=64, y_mean=Y_MEAN, y_std=Y_STD, return_values=True)
    assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 140]]).all() and np.isfinite(np.delete(ys, [11, 140])).all()
    assert not np.isin([11, 140], si).any()


def test_a_candidates_bits_do_not_depend_on_m(engine):
    big, small = case_of("b"), case_of("a")
    assert np.array_equal(big.Xc[:257], small.Xc)
    mu_b, sd_b = big.posterior(engine)
    pts = big.points(mu_b, 16)
    ys_b = engine.kg_argbest(pts, y_mean=Y_MEAN, y_std=Y_STD, return_values=True)[4]
    mu_s, sd_s = small.posterior(engine)
    ys_s = engine.kg_argbest(pts, y_mean=Y_MEAN, y_std=Y_STD, return_values=True)[4]
    same = (mu_b[:257] == mu_s) & (sd_b[:257] == sd_s)
    print(f"{int(same.sum())} of 257 rows have the same posterior bits at both M")
    assert same.sum() >= 200, "the posterior's own bits differ between the two M: this test has nothing to compare"
    assert np.array_equal(ys_b[:257][same], ys_s[same])
    assert np.array_equal(engine.kg_argbest(pts, y_mean=Y_MEAN, y_std=Y_STD, return_values=True)[4], ys_s)


# ---- a reader --------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = case_of("d")
    mu0, sd0 = c.posterior(eng)
    eng.take_negative_variance_flag()
    pts = c.points(mu0)
    kw = dict(y_mean=Y_MEAN, y_std=Y_STD)
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    first = eng.kg_argbest(pts, k_seeds=8, return_values=True, **kw)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    assert before[0] == after[0] and before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[2:], after[2:]))
    again = eng.kg_argbest(pts, k_seeds=8, return_values=True, **kw)
    assert first[0] == again[0] and first[1] == again[1] and all(np.array_equal(a, b) for a, b in zip(first[2:], again[2:]))
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc)
    assert eng.take_negative_variance_flag() is False
    mu1, sd1 = eng.posterior(0, Y_MEAN, Y_STD)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    x_new = np.random.RandomState(5).uniform(size=(2, c.d))
    yn2 = np.concatenate([c.yn, [0.2, -0.4]])

    def arm(with_kg):
        c.posterior(eng)
        if with_kg:
            eng.kg_argbest(pts, k_seeds=8, **kw)
        eng.fit_append(x_new, yn2)
        if with_kg:
            with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
                eng.kg_argbest(pts, **kw)
        return eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)

    mu_a, sd_a, route_a = arm(False)
    mu_b, sd_b, route_b = arm(True)
    assert route_a == 1 and route_b == 1
    assert np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)
    assert eng.take_negative_variance_flag() is False


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = case_of("a")
    mu, sd = c.posterior(eng)
    good = np.ascontiguousarray(c.points(mu, 5))
    kw = dict(y_mean=Y_MEAN, y_std=Y_STD)
    ref = eng.kg_argbest(good, k_seeds=4, return_values=True, **kw)
    for bad in (np.zeros((0, 3)), np.zeros((65, 3))):
        with pytest.raises(ValueError, match="n_points"):
            eng.kg_argbest(bad, **kw)
    for bad in (np.zeros((5, 2)), np.zeros((5, 4))):
        with pytest.raises(ValueError, match="dimension"):
            eng.kg_argbest(bad, **kw)
    for bad in (np.nan, np.inf, -np.inf):
        p = good.copy()
        p[3, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            eng.kg_argbest(p, **kw)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="k_seeds"):
            eng.kg_argbest(good, k_seeds=bad, **kw)
    for bad in (np.nan, np.inf, 0.0, -0.4, 0.5):                           # 0.5: not the y_std the resident posterior was scaled with
        with pytest.raises(ValueError, match="y_std"):
            eng.kg_argbest(good, y_mean=Y_MEAN, y_std=bad)
    with pytest.raises(ValueError):
        eng.kg_argbest(np.zeros(3), **kw)
    bi, bv = np.empty(1, dtype=np.int64), np.empty(1)
    si, sv = np.empty(4, dtype=np.int64), np.empty(4)
    call = eng._lib.gpbo_kg_argbest
    g = dptr(good)
    assert call(eng._h, None, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, 5, 3, Y_MEAN, Y_STD, 0, 0, None, dptr(bv), None, None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), None, None, None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, 5, 3, Y_MEAN, Y_STD, 4, 0, iptr(bi), dptr(bv), None, dptr(sv), None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, 5, 3, Y_MEAN, Y_STD, 4, 0, iptr(bi), dptr(bv), iptr(si), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, 0, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None) == _lib.ERR_INVALID
    assert call(None, g, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, g, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None) == _lib.GPBO_OK
    assert bi[0] == ref[0] and bv[0] == ref[1]
    now = eng.kg_argbest(good, k_seeds=4, return_values=True, **kw)
    assert now[0] == ref[0] and all(np.array_equal(a, b) for a, b in zip(now[2:], ref[2:]))
    # missing state
    eng.set_candidates(c.Xc[:100])
    with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
        eng.kg_argbest(good, **kw)
    assert call(eng._h, g, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None) == _lib.ERR_STATE
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    eng.kg_argbest(good, **kw)
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
    with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
        eng.kg_argbest(good, **kw)
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE, slot=2)
    eng.posterior(2, Y_MEAN, Y_STD, fetch=False)
    with pytest.raises(GpboError, match="slot 0"):
        eng.kg_argbest(good, **kw)
    # a fit pending on slot 0 (the engine would wait for it: asked at the C boundary, and refused as such)
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        rc = call(eng._h, g, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None, None)
        assert rc == _lib.ERR_STATE
        with pytest.raises(GpboError, match="pending gpbo_fit_begin"):
            eng._check(rc)
    # ... and through the engine, which waits for the fit: the new fit has no posterior over the candidates
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
            eng.kg_argbest(good, **kw)
    eng.lml(c.X, c.yn, c.kind, c.ls, NOISE)
    with pytest.raises(GpboError):
        eng.kg_argbest(good, **kw)
    fresh = GpEngine(0)
    try:
        with pytest.raises(GpboError):
            fresh.kg_argbest(good, **kw)
        fresh.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        with pytest.raises(GpboError, match="slot 0"):
            fresh.kg_argbest(good, **kw)
        assert fresh._lib.gpbo_kg_argbest(fresh._h, g, 5, 3, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, None,
                                          None) == _lib.ERR_STATE
    finally:
        fresh.close()
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.kg_argbest(object.__new__(GroupEngine), good)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_suggest_kg_picks_the_restatements_maximiser(engine):
    """A driver built the way accelerate() leaves a BayesianOptimization (batch_truth.Driver: HipGPR on slot 0 of the real engine, an
    all-float space, the optimizer's RandomState) on a noisy 2-D target."""
    D, N, M, J = 2, 25, 2000, 9
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    rs = np.random.RandomState(77)
    X = bounds[:, 0] + rs.uniform(size=(N, D)) * (bounds[:, 1] - bounds[:, 0])
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) - 0.3 * (X[:, 0] - 0.5) ** 2 + 0.05 * rs.standard_normal(N)

    def run():
        drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M)
        drv._gp.alpha = 1e-2
        params, info = suggest_kg(drv, J, n_random=M, return_info=True)
        return drv, params, info

    drv, params, info = run()
    gp = drv._gp
    ym, ys_ = float(gp._y_train_mean), float(gp._y_train_std)
    assert drv._acquisition_function.i == 0 and gp.X_train_.shape[0] == N and list(params) == drv._space.keys
    Xc = engine.get_candidate_rows(np.arange(M), D)
    mu, sd = engine.posterior(0, ym, ys_)
    assert np.array_equal(info["points_index"], T.reference_points(mu, J))
    ls = np.broadcast_to(np.exp(gp.kernel_.theta), (D,))
    cov = T.posterior_cov(F.MATERN25, X, ls, 1e-2, Xc, Xc[info["points_index"]])
    kg, scale = T.kg_values(mu, sd, cov, info["point_means"], ys_, 1e-2, 0.0, return_scale=True)
    top = np.sort(kg)[::-1][:2]
    assert top[0] - top[1] > 2 * T.BAR * scale.max(), "the restatement's best and second best are within the bar: pick another seed"
    assert info["index"] == int(kg.argmax()) and abs(info["value"] - kg.max()) <= T.BAR * scale.max() and info["value"] > 0
    assert np.array_equal(np.array(list(params.values())), Xc[info["index"]])
    # the RandomState: the host replay of the fit and ONE candidate draw
    from bayesianoptimization_amd import _suggest as S

    twin = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M)
    twin._gp.alpha = 1e-2
    S.fit_model(twin._gp, twin._space, "twin")
    for t in range(D):
        twin._random_state.uniform(bounds[t, 0], bounds[t, 1], M)
    assert B.same_state(drv._random_state, twin._random_state)
    drv2, params2, info2 = run()
    assert params2 == params and info2["index"] == info["index"]
